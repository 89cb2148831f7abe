"""One optimizer step on BERT-base's parameter shapes (BertConfig(): 199 tensors, 109.5 M elements, random values, nothing downloaded),
this library's multi-tensor kernel next to torch's two implementations on the same card:

    hip            aspire_amd.HipAdam(params).step()                      one launch of optim.hip per step
    torch_foreach  torch.optim.Adam(params).step()                        torch's default on the GPU
    torch_fused    torch.optim.Adam(params, fused=True).step()
    hip_entry      aspire_adam_step_f32 on a table built once             the kernel and its table copy without the Python around them

and the same for Adagrad (--rule adagrad).  All sides update their own copy of the parameters from one shared set of gradients, are warmed
up, then timed with device events over windows of about 0.2 s, the sides alternating, five windows each; medians and min-max of the
per-step times are printed as one JSON line, with the bytes a step must move (Adam: read p, g, m, v and write p, m, v = 7 passes x 4 B
x N; Adagrad: 5 passes) over the median as GB/s and as a fraction of the 6.29 TB/s a float4 copy sustains on an MI355X.  The results
are compared first.  Needs a GPU; there is no CPU path.

    python tools/optimizer_step_time.py [--rule adam|adagrad] [--windows 5] [--window-s 0.2]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY_TBPS = 6.29


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls        # ms per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rule', choices=['adam', 'adagrad'], default='adam')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-s', type=float, default=0.2, help='seconds of steps per timed window (small under a profiler)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from transformers import BertConfig, BertModel
    from aspire_amd import HipAdam, HipAdagrad, _lib, ops
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in BertModel(BertConfig()).parameters()]
    n_elem = sum(int(np.prod(s)) for s in shapes)
    init = [0.02 * torch.randn(s, device='cuda') for s in shapes]
    grads = [1e-3 * torch.randn(s, device='cuda') for s in shapes]

    def params():
        ps = [torch.nn.Parameter(t.clone()) for t in init]
        for p, g in zip(ps, grads):
            p.grad = g
        return ps

    lr, fused_refused = 2e-5, ''
    sets = {n: params() for n in ('hip', 'torch_foreach', 'torch_fused', 'hip_entry')}
    if a.rule == 'adam':
        opts = {'hip': HipAdam(sets['hip'], lr=lr), 'torch_foreach': torch.optim.Adam(sets['torch_foreach'], lr=lr),
                'torch_fused': torch.optim.Adam(sets['torch_fused'], lr=lr, fused=True)}
        passes, entry, mid = 7, _lib.lib.aspire_adam_step_f32, (0.9, 0.999, 1e-8)
    else:
        opts = {'hip': HipAdagrad(sets['hip'], lr=lr), 'torch_foreach': torch.optim.Adagrad(sets['torch_foreach'], lr=lr)}
        try:        # (a torch whose fused Adagrad is CPU-only refuses here or at its first step)
            opts['torch_fused'] = torch.optim.Adagrad(sets['torch_fused'], lr=lr, fused=True)
            opts['torch_fused'].step()
            for p, t in zip(sets['torch_fused'], init):
                p.data.copy_(t)
            opts['torch_fused'] = torch.optim.Adagrad(sets['torch_fused'], lr=lr, fused=True)
        except RuntimeError as e:
            opts.pop('torch_fused', None)
            fused_refused = str(e).splitlines()[0]
        passes, entry, mid = 5, _lib.lib.aspire_adagrad_step_f32, (0.0, 1e-10)
    # the bare entry: the table is built once (every step is "step 3" of its tensors: the arithmetic's cost does not depend on it)
    state = [[torch.zeros_like(p) for p in sets['hip_entry']] for _ in range(2)]
    table = (_lib.OptimTensor * len(shapes))(*[
        _lib.OptimTensor(p.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), p.numel(), 3, lr)
        for p, g, s1, s2 in zip(sets['hip_entry'], grads, *state)])
    ws = torch.empty(_lib.lib.aspire_optim_workspace_bytes(len(shapes)), device='cuda', dtype=torch.uint8)

    def bare():
        _lib.check(entry(table, len(shapes), *mid, ws.data_ptr(), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))

    sides = [(n, o.step) for n, o in opts.items()] + [('hip_entry', bare)]
    # the three optimizers agree after two steps (the bare entry runs other step numbers)
    for _ in range(2):
        for n in opts:
            opts[n].step()
    dev = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(sets['hip'], sets['torch_foreach']))
    res = dict(rule=a.rule, tensors=len(shapes), elements=n_elem, step_bytes=passes * 4 * n_elem, max_abs_diff_vs_foreach=dev)
    assert dev < 1e-6, dev
    if 'torch_fused' in opts:
        res['max_abs_diff_vs_fused'] = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(sets['hip'], sets['torch_fused']))
        assert res['max_abs_diff_vs_fused'] < 1e-6, res
    else:
        res['torch_fused'] = 'refused by this torch: ' + fused_refused
    times, calls = {n: [] for n, _ in sides}, {}
    for name, fn in sides:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(int(a.window_s * 1e3 / window(fn, 3)), 2)
    for _ in range(a.windows):
        for name, fn in sides:
            times[name].append(window(fn, calls[name]))
    for name, t in times.items():
        med = float(np.median(t))
        res[name + '_ms_median'] = round(med, 4)
        res[name + '_ms_min_max'] = [round(min(t), 4), round(max(t), 4)]
        res[name + '_steps_per_window'] = calls[name]
        if name.startswith('hip'):
            res[name + '_gbps'] = round(passes * 4 * n_elem / med / 1e6, 1)
            res[name + '_fraction_of_copy_rate'] = round(passes * 4 * n_elem / med / 1e6 / (COPY_TBPS * 1e3), 3)
    if 'torch_fused' in opts:
        res['aim_hip_median_at_or_under_fused_max'] = bool(res['hip_ms_median'] <= res['torch_fused_ms_min_max'][1])
    res['peak_mem_gb'] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
