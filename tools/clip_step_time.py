"""Gradient clipping and AdamW inside the one-launch optimizer step, on BERT-base's parameter shapes (BertConfig(): 199 tensors, 109.5 M
elements, random values, nothing downloaded), in the manner of tools/optimizer_step_time.py:

  (a) hip_clip_fused     aspire_amd.grad_norm(params, 1.0) + HipAdam.step(grad_scale=coef)     two norm launches + the scaled step
      torch_clip_hip     torch.nn.utils.clip_grad_norm_(params, 1.0) + HipAdam.step()           the route a user had before
      hip_clip_inplace   aspire_amd.clip_grad_norm_(params, 1.0) + HipAdam.step()               recorded
      hip_norm           aspire_amd.grad_norm(params, 1.0) alone                                recorded
  (b) hip_adamw          HipAdamW(decay_groups).step()                                          recorded, not gated
      torch_adamw_fused  torch.optim.AdamW(fused=True).step()
  (c) plain_here         HipAdam.step() on this tree
      plain_parent       HipAdam.step() on another checkout (--parent ROOT, built); two processes per tree, started in the order
                         parent, here, here, parent, because a process's place among those on the card moves its step time

Every side has its own parameters and gradients, is warmed up, then timed with device events over windows of about 0.2 s, the sides of
a comparison alternating, five windows each.  One JSON line: medians, min-max, and the two gates -- (a) the fused route's median at or
under the torch route's highest window, (c) this tree's plain step at or under the parent's highest window (the plain path must not pay
for the new template arguments).  Needs a GPU; there is no CPU path.

    python tools/clip_step_time.py [--parent ROOT] [--windows 5] [--window-s 0.2]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def window(fn, calls):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls        # ms per call


def bert_base_tensors():
    import torch
    from transformers import BertConfig, BertModel
    torch.manual_seed(0)
    model = BertModel(BertConfig())
    names = [n for n, _ in model.named_parameters()]
    shapes = [tuple(p.shape) for p in model.parameters()]
    init = [0.02 * torch.randn(s, device='cuda') for s in shapes]
    grads = [1e-3 * torch.randn(s, device='cuda') for s in shapes]
    return names, init, grads


def fresh(init, grads):
    import torch
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    return ps


def calls_for(fn, window_s):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return max(int(window_s * 1e3 / window(fn, 3)), 2)


def serve(root):
    """the plain HipAdam.step() of the checkout at `root`, driven over stdin: 'calls SECONDS' -> the calls of a window, 'window N' ->
    ms per step over N steps, 'quit'"""
    sys.path.insert(0, root)
    import aspire_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(aspire_amd.__file__))) == os.path.abspath(root), aspire_amd.__file__
    _, init, grads = bert_base_tensors()
    opt = aspire_amd.HipAdam(fresh(init, grads), lr=2e-5)
    for line in sys.stdin:
        cmd, _, arg = line.strip().partition(' ')
        if cmd == 'quit':
            break
        out = calls_for(opt.step, float(arg)) if cmd == 'calls' else window(opt.step, int(arg))
        print(json.dumps(out), flush=True)


class Served:
    def __init__(self, root):
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--serve', root], stdin=subprocess.PIPE,
                                     stdout=subprocess.PIPE, text=True)

    def ask(self, line):
        self.proc.stdin.write(line + '\n')
        self.proc.stdin.flush()
        reply = self.proc.stdout.readline()
        if not reply:
            raise RuntimeError(f'the process serving {line!r} ended with status {self.proc.wait()}')
        return json.loads(reply)

    def close(self):
        if self.proc.poll() is None:
            self.proc.stdin.write('quit\n')
            self.proc.stdin.close()
            self.proc.wait(timeout=60)


def summarize(res, times, calls):
    import numpy as np
    for name, t in times.items():
        res[name + '_ms_median'] = round(float(np.median(t)), 4)
        res[name + '_ms_min_max'] = [round(min(t), 4), round(max(t), 4)]
        res[name + '_calls_per_window'] = calls[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help='root of a built checkout of the parent commit: comparison (c)')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-s', type=float, default=0.2)
    ap.add_argument('--serve', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.serve:
        return serve(a.serve)
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    import aspire_amd
    from aspire_amd import HipAdam, HipAdamW
    names, init, grads = bert_base_tensors()
    res = dict(tensors=len(init), elements=sum(t.numel() for t in init))

    # (a) and the recorded sides around it
    sets = {n: fresh(init, grads) for n in ('hip_clip_fused', 'torch_clip_hip', 'hip_clip_inplace', 'hip_norm')}
    opts = {n: HipAdam(ps, lr=2e-5) for n, ps in sets.items()}

    def fused():
        opts['hip_clip_fused'].step(grad_scale=aspire_amd.grad_norm(sets['hip_clip_fused'], 1.0)[1])

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(sets['torch_clip_hip'], 1.0)
        opts['torch_clip_hip'].step()

    def inplace():
        aspire_amd.clip_grad_norm_(sets['hip_clip_inplace'], 1.0)
        opts['hip_clip_inplace'].step()

    # the routes agree: one update from the same start (the fused route's norm is the double-precision one)
    fused(), torch_clip(), inplace()
    res['max_abs_diff_fused_vs_torch_clip'] = max(float((p.detach() - q.detach()).abs().max())
                                                  for p, q in zip(sets['hip_clip_fused'], sets['torch_clip_hip']))
    assert res['max_abs_diff_fused_vs_torch_clip'] < 1e-6, res
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(sets['hip_clip_fused'], sets['hip_clip_inplace']))
    sides = [('hip_clip_fused', fused), ('torch_clip_hip', torch_clip), ('hip_clip_inplace', inplace),
             ('hip_norm', lambda: aspire_amd.grad_norm(sets['hip_norm'], 1.0))]

    # (b)
    ps_w, ps_t = fresh(init, grads), fresh(init, grads)
    plain = {id(p) for n, p in zip(names, ps_w) if n.endswith('bias') or 'LayerNorm' in n}
    hip_w = HipAdamW([dict(params=[p for p in ps_w if id(p) not in plain], weight_decay=0.01),
                      dict(params=[p for p in ps_w if id(p) in plain], weight_decay=0.0)], lr=2e-5)
    plain_t = {id(q) for p, q in zip(ps_w, ps_t) if id(p) in plain}
    torch_w = torch.optim.AdamW([dict(params=[p for p in ps_t if id(p) not in plain_t], weight_decay=0.01),
                                 dict(params=[p for p in ps_t if id(p) in plain_t], weight_decay=0.0)], lr=2e-5, fused=True)
    hip_w.step(), torch_w.step()
    res['max_abs_diff_adamw_vs_torch_fused'] = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(ps_w, ps_t))
    assert res['max_abs_diff_adamw_vs_torch_fused'] < 1e-6, res
    sides += [('hip_adamw', hip_w.step), ('torch_adamw_fused', torch_w.step)]

    times, calls = {n: [] for n, _ in sides}, {}
    for name, fn in sides:
        calls[name] = calls_for(fn, a.window_s)
    for _ in range(a.windows):
        for name, fn in sides:
            times[name].append(window(fn, calls[name]))
    summarize(res, times, calls)
    res['norm_gbps'] = round(4 * res['elements'] / res['hip_norm_ms_median'] / 1e6, 1)
    res['gate_a_fused_median_at_or_under_torch_clip_max'] = bool(res['hip_clip_fused_ms_median'] <= res['torch_clip_hip_ms_min_max'][1])

    # (c): each tree in processes of its own, the windows alternating between them.  A process's step time depends on where it
    # stands among the processes on the card (its allocations land elsewhere): the same tree measured 0.52 and 0.61 ms in two
    # positions.  So each tree gets TWO processes, started in the order parent, here, here, parent, and a tree's windows are pooled.
    if a.parent:
        parent = os.path.abspath(a.parent)
        served = [('plain_parent', Served(parent)), ('plain_here', Served(HERE)), ('plain_here', Served(HERE)),
                  ('plain_parent', Served(parent))]
        try:
            per_call = [s.ask(f'calls {a.window_s}') for _, s in served]
            per_proc = [[] for _ in served]
            for _ in range(a.windows):
                for i, (_, s) in enumerate(served):
                    per_proc[i].append(s.ask(f'window {per_call[i]}'))
        finally:
            for _, s in served:
                s.close()
        times = {n: [t for (m, _), ts in zip(served, per_proc) if m == n for t in ts] for n in ('plain_here', 'plain_parent')}
        summarize(res, times, {n: [c for (m, _), c in zip(served, per_call) if m == n] for n in times})
        res['plain_process_medians_in_start_order'] = [[n, round(float(np.median(ts)), 4)] for (n, _), ts in zip(served, per_proc)]
        res['gate_c_plain_median_at_or_under_parent_max'] = bool(res['plain_here_ms_median'] <= res['plain_parent_ms_min_max'][1])
    res['peak_mem_gb'] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
