"""The span mean pool's backward next to torch autograd through a torch restatement of the same pooling:
B = 32 documents of L = 256 tokens, S = 12 sentence slots in the reference's span layout ([CLS] title [SEP] sentence [SEP] ...).

    ours   ops.span_mean_pool_backward(grad_sent, grad_cls, ...)                       one launch of span_mean_pool_backward_kernel
    torch  autograd.grad of (sent, cls) = (index_add_ of the gathered token rows / counts, hidden[:, 0]) with respect to hidden

Each side is warmed up, then timed with device events over windows of about 0.2 s, the two sides alternating, five windows each; the
median and the spread of the per-call times are printed as one JSON line.  Both gradients are compared first (equal up to fp32
roundings of a row's few terms).  Needs a GPU; there is no CPU path.

    python tools/pool_backward_time.py [--B 32 --L 256 --S 12]

The kernels' own times: the same command under rocprofv3 --kernel-trace --stats with --windows 1 --window-s 0.02.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from aspire_amd import ops  # noqa: E402
from aspire_amd.batch_prep import spans_to_csr  # noqa: E402


def layout(rng, n_sents, seq_len):
    per = (seq_len - 4) // n_sents - 1          # tokens per sentence so that n_sents of them, each with its [SEP], fit
    spans, pos = [], 4
    for _ in range(n_sents):
        n = int(rng.randint(max(per // 2, 1), per + 1))
        spans.append(list(range(pos, pos + n)))
        pos += n + 1
    return spans


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / calls        # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=32)
    ap.add_argument('--L', type=int, default=256)
    ap.add_argument('--S', type=int, default=12)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-s', type=float, default=0.2, help='seconds of calls per timed window (small under a profiler)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    rng = np.random.RandomState(0)
    spans = [layout(rng, a.S if b == 0 else int(rng.randint(max(a.S // 2, 1), a.S + 1)), a.L) for b in range(a.B)]     # ragged
    tok_idx, span_off = (t.cuda() for t in spans_to_csr(spans, a.S))
    g = torch.Generator('cuda').manual_seed(0)
    gs = torch.randn(a.B, a.S, 768, device='cuda', generator=g)
    gc = torch.randn(a.B, 768, device='cuda', generator=g)
    out = torch.empty(a.B, a.L, 768, device='cuda')

    def ours():
        return ops.span_mean_pool_backward(gs, gc, tok_idx, span_off, a.B, a.L, a.S, out=out)

    # the torch restatement: one gather of the listed token rows, a segment sum by index_add_, the division by the counts
    counts = (span_off[1:] - span_off[:-1]).to(torch.int64)
    seg = torch.repeat_interleave(torch.arange(a.B * a.S, device='cuda'), counts)
    flat = (seg // a.S) * a.L + tok_idx.to(torch.int64)
    hidden = torch.randn(a.B, a.L, 768, device='cuda', generator=g, requires_grad=True)
    rows = hidden.view(-1, 768)[flat]
    sent = torch.zeros(a.B * a.S, 768, device='cuda').index_add_(0, seg, rows) / counts.clamp(min=1).unsqueeze(1)
    cls = hidden[:, 0]

    def theirs():
        return torch.autograd.grad((sent, cls), hidden, (gs.view(-1, 768), gc), retain_graph=True)[0]

    dev = float((ours() - theirs()).abs().max())
    assert dev <= 4 * 2.0 ** -23 * float(gs.abs().max() + gc.abs().max()), dev
    times = {'ours': [], 'torch': []}
    calls = {}
    for name, fn in (('ours', ours), ('torch', theirs)):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(int(a.window_s * 1e6 / window(fn, 200)), 20)
    for _ in range(a.windows):
        for name, fn in (('ours', ours), ('torch', theirs)):
            times[name].append(window(fn, calls[name]))
    res = dict(B=a.B, L=a.L, S=a.S, span_tokens=int(tok_idx.numel()), grad_hidden_mb=round(a.B * a.L * 768 * 4 / 1e6, 2), max_abs_diff=dev)
    for name, t in times.items():
        res[name + '_us_median'] = round(float(np.median(t)), 2)
        res[name + '_us_min_max'] = [round(min(t), 2), round(max(t), 2)]
        res[name + '_calls_per_window'] = calls[name]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
