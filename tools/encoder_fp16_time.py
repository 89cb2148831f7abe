"""forward_hidden of a 12-layer BERT-base (ffn 3072, random init) in the inference encoder's opt-in fp16 matmul mode, next to the default
path of this tree and of the PARENT commit, on one card in one call ("fp16 matrix products in the inference
encoder").  The baseline of any claim is the parent's library, not the code under test:

    git worktree add /some/dir HEAD~1 && (cd /some/dir && python -c "import __graft_entry__ as g; g.build()")
    python tools/encoder_fp16_time.py --parent-root /some/dir

Two worker processes hold the card, one per tree (a tree's Python package binds its own library: the parent's has no _prec entries);
this process does not touch the GPU and tells them, window by window, whose turn it is, so the three sides ALTERNATE in time:

    fp16      this tree, HipBertEncoder(model, matmul='fp16')
    default   this tree, HipBertEncoder(model)
    parent    the parent tree, HipBertEncoder(model)           (left out without --parent-root)

Per shape: the same weights and full-length inputs on every side, three warm-up forwards, then device events over windows of at least
--window-s seconds (0.5), --windows (5) windows per side; the median and the range of the per-forward times, the ratios to the parent's
median, and the mode's matrix-product rate (the four projections' 2 M N K flops per layer over the forward's whole time: a lower bound of
the GEMMs' own rate) against the 2.5 PFLOP/s fp16 peak.  One JSON line per shape.  Needs a GPU.

The kernels' own times: one side alone under rocprofv3 --kernel-trace --stats, with no counters, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/encoder_fp16_time.py --single fp16 --shapes 64x256
(tools/statsum.py prints the CSV by kernel; --single runs warm-up + one short window in this process.)
"""
import argparse
import json
import math
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_FP16 = 2.5e15


def projection_flops(rows, layers=12, ffn=3072):
    return layers * 2.0 * rows * (768 * 2304 + 768 * 768 + 2 * 768 * ffn)


# ---- a worker: one tree's package, one process on the card ---------------------------------------------------------------------------
def worker(root, layers):
    sys.path.insert(0, root)
    import torch
    from transformers import BertConfig, BertModel
    from aspire_amd.encoder import HipBertEncoder
    assert torch.cuda.is_available(), 'needs a GPU'
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=3000, hidden_size=768, num_hidden_layers=layers, num_attention_heads=12, intermediate_size=3072,
                     max_position_embeddings=512)
    model = BertModel(cfg, add_pooling_layer=False).eval()
    encs, state = {}, {}

    def encoder(side):
        if side not in encs:
            encs[side] = HipBertEncoder(model, matmul='fp16') if side == 'fp16' else HipBertEncoder(model)
            assert side != 'fp16' or encs[side].matmul == 'fp16'
        return encs[side]

    def forward(side):
        return encoder(side).forward_hidden(state['tok'], state['typ'], state['mask'], check_ids=False)

    def window(side, seconds):
        per = state['per'][side]
        calls = max(1, int(math.ceil(seconds * 1e3 / per)))
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            forward(side)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / calls

    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == 'quit':
            break
        if cmd[0] == 'shape':           # shape B L side [side ..]: inputs, warm-up, a first estimate of a forward's time
            b, l = int(cmd[1]), int(cmd[2])
            g = torch.Generator().manual_seed(b * 1000 + l)
            state['tok'] = torch.randint(5, 3000, (b, l), generator=g).cuda()
            state['typ'] = torch.zeros_like(state['tok'])
            state['mask'] = torch.ones_like(state['tok'])
            state['per'] = {}
            for side in cmd[3:]:
                for _ in range(3):
                    out = forward(side)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(out).all()), side
                state['per'][side] = 1.0
                state['per'][side] = window(side, 0.003)
            print('@@ready', flush=True)
        elif cmd[0] == 'window':        # window side seconds -> ms per forward
            print(f'@@{window(cmd[1], float(cmd[2])):.6f}', flush=True)


def start_worker(root, layers):
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', '--root', root, '--layers', str(layers)], stdin=subprocess.PIPE,
                            stdout=subprocess.PIPE, text=True, bufsize=1)


def ask(proc, line):
    proc.stdin.write(line + '\n')
    proc.stdin.flush()
    while True:                         # replies carry a marker: whatever else a library prints to stdout is passed over
        reply = proc.stdout.readline()
        if not reply:
            raise RuntimeError(f'a worker ended early (exit status {proc.poll()}) at: {line}')
        if reply.startswith('@@'):
            return reply[2:].strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-root', help="a checkout of the parent commit with its library built (its aspire_amd package is imported there)")
    ap.add_argument('--shapes', default='64x256,32x512,8x128')
    ap.add_argument('--layers', type=int, default=12)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-s', type=float, default=0.5)
    ap.add_argument('--single', choices=['fp16', 'default'], help='one side in this process, warm-up + one window (for a profiler)')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--root', default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.root, a.layers)
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes.split(',')]
    roots = {'this': HERE}
    sides = {'this': [a.single] if a.single else ['fp16', 'default']}
    if a.parent_root and not a.single:
        roots['parent'], sides['parent'] = os.path.abspath(a.parent_root), ['default']
    procs = {k: start_worker(r, a.layers) for k, r in roots.items()}
    names = {('this', 'fp16'): 'fp16', ('this', 'default'): 'default', ('parent', 'default'): 'parent'}
    try:
        for b, l in shapes:
            for k, p in procs.items():
                assert ask(p, f'shape {b} {l} ' + ' '.join(sides[k])) == 'ready'
            ms = {names[k, s]: [] for k in procs for s in sides[k]}
            for _ in range(1 if a.single else a.windows):
                for k, p in procs.items():             # the sides alternate window by window
                    for s in sides[k]:
                        ms[names[k, s]].append(float(ask(p, f'window {s} {0.05 if a.single else a.window_s}')))
            out = {'shape': f'{b}x{l}', 'rows': b * l, 'layers': a.layers, 'windows': len(next(iter(ms.values()))), 'window_s': a.window_s}
            for name, v in ms.items():
                v = sorted(v)
                out[name + '_ms'] = {'median': round(v[len(v) // 2], 4), 'min': round(v[0], 4), 'max': round(v[-1], 4)}
            base_name = next(n for n in ('parent', 'default', 'fp16') if n + '_ms' in out)
            base = out[base_name + '_ms']['median']
            out['baseline'] = base_name if base_name == 'parent' else base_name + ' (this tree: no parent side in this run)'
            for name in ms:
                out[name + '_over_baseline'] = round(out[name + '_ms']['median'] / base, 4)
            if 'fp16_ms' in out:
                rate = projection_flops(b * l, a.layers) / (out['fp16_ms']['median'] * 1e-3)
                out['fp16_projection_tflops_over_whole_forward'] = round(rate / 1e12, 1)
                out['fraction_of_2.5_pflops_fp16_peak'] = round(rate / PEAK_FP16, 4)
            print(json.dumps(out), flush=True)
    finally:
        for p in procs.values():
            try:
                p.stdin.write('quit\n')
                p.stdin.flush()
                p.wait(timeout=60)
            except Exception:
                p.kill()


if __name__ == '__main__':
    main()
