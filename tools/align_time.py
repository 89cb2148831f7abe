"""The alignment step of the co-citation data path: aspire_amd.align.align_cocited (three ops.dot_argmax calls for the whole list)
against the reference's own loop -- three np.matmul + argmax per example on the host (pre_proc_cocits.py:487-494) -- on the same
machine and the same rows.

    python tools/align_time.py                 # 100 000 examples, five windows; one JSON line
    python tools/align_time.py 20000 3         # examples, windows

100 000 examples over 5 000 abstracts of 3 .. 20 rows and 5 000 co-cited sets of 1 .. 10 context rows, unit-norm rows; every example
names a set and two distinct papers at random, so a paper sits in about 40 examples and is stored once.  A window is one whole
align_cocited call between two device events (the host's index tables, six small uploads, three launches and the copy back of the
picks all fall inside it); `kernels_ms` is the three launches alone on device tables that are already there.  `host_tables_ms` is
align_cocited on the host clock with a stand-in that returns zeros in the place of the launches -- the passes over the example
tuples, the id numbering, the gathers and the pair lists alone -- and `np_unique_ms` np.unique(..., return_inverse=True) over the
same 200 000 ids (here ints), the numpy-only way to number them, for comparison with that whole host part.  The numpy loop is timed
once per window on the host clock.  The figures are recorded in DESIGN.md section 7; nothing is gated on them."""
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aspire_amd import ops  # noqa: E402
from aspire_amd.align import align_cocited, device_view  # noqa: E402

N_PAPERS, N_SETS, WARMUPS = 5000, 5000, 1


def _unit_docs(rng, lens):
    rows = rng.standard_normal((int(lens.sum()), 768)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    return rows, (np.cumsum(lens) - lens).astype(np.int64)


def _event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def _numpy_loop(abs_rows, a_start, a_len, ctx_rows, c_start, c_len, examples):
    cc, ab = [], []
    for s, a, p in examples:
        q = abs_rows[a_start[a]:a_start[a] + a_len[a]]
        pos = abs_rows[a_start[p]:a_start[p] + a_len[p]]
        ctx = ctx_rows[c_start[s]:c_start[s] + c_len[s]]
        a2c = np.matmul(q, ctx.T)
        i0 = np.unravel_index(a2c.argmax(), a2c.shape)
        p2c = np.matmul(pos, ctx.T)
        i1 = np.unravel_index(p2c.argmax(), p2c.shape)
        a2p = np.matmul(q, pos.T)
        i2 = np.unravel_index(a2p.argmax(), a2p.shape)
        cc.append((int(i0[0]), int(i1[0])))
        ab.append((int(i2[0]), int(i2[1])))
    return cc, ab


def bench(n_examples, windows):
    rng = np.random.default_rng(9)
    a_len, c_len = rng.integers(3, 21, N_PAPERS), rng.integers(1, 11, N_SETS)
    abs_rows, a_start = _unit_docs(rng, a_len)
    ctx_rows, c_start = _unit_docs(rng, c_len)
    papers = np.stack([rng.choice(N_PAPERS, 2, replace=False) for _ in range(n_examples)])
    sets = rng.integers(0, N_SETS, n_examples)
    examples = list(zip(sets.tolist(), papers[:, 0].tolist(), papers[:, 1].tolist()))
    dev_abs, dev_ctx = torch.from_numpy(abs_rows).cuda(), torch.from_numpy(ctx_rows).cuda()
    abs_store = types.SimpleNamespace(_dev_rows=dev_abs, _dev_index={k: (int(s), int(n)) for k, (s, n) in enumerate(zip(a_start, a_len))})
    ctx_set = device_view(dev_ctx, c_start, c_len)

    anchor = device_view(dev_abs, a_start[papers[:, 0]], a_len[papers[:, 0]])
    positive = device_view(dev_abs, a_start[papers[:, 1]], a_len[papers[:, 1]])
    contexts = device_view(dev_ctx, c_start[sets], c_len[sets])
    outs = [(torch.empty(n_examples, 2, dtype=torch.int32, device='cuda'), None) for _ in range(3)]

    def kernels():
        ops.dot_argmax(anchor, contexts, want_best=False, out=outs[0])
        ops.dot_argmax(positive, contexts, want_best=False, out=outs[1])
        ops.dot_argmax(anchor, positive, want_best=False, out=outs[2])

    for _ in range(WARMUPS):
        got = align_cocited(abs_store, ctx_set, examples)
        kernels()
    torch.cuda.synchronize()
    call_ms, kernel_ms, loop_ms, moved = [], [], [], None
    for _ in range(windows):
        ms, got = _event_ms(lambda: align_cocited(abs_store, ctx_set, examples))
        call_ms.append(ms)
        kernel_ms.append(_event_ms(kernels)[0])
        t = time.perf_counter()
        want = _numpy_loop(abs_rows, a_start, a_len, ctx_rows, c_start, c_len, examples)
        loop_ms.append(1e3 * (time.perf_counter() - t))
        moved = sum(g != w for g, w in zip(got[0] + got[1], want[0] + want[1]))
    zeros = lambda q, c: np.zeros((len(q.start), 2), np.int32)
    host_view = types.SimpleNamespace(rows=None, start=c_start, len=c_len)
    host_ms, unique_ms = [], []
    for _ in range(windows):
        t = time.perf_counter()
        align_cocited(abs_store, host_view, examples, dot_argmax=zeros)
        host_ms.append(1e3 * (time.perf_counter() - t))
        ids = [e[1] for e in examples] + [e[2] for e in examples]
        t = time.perf_counter()
        np.unique(np.array(ids), return_inverse=True)
        unique_ms.append(1e3 * (time.perf_counter() - t))
    rng_of = lambda v: [round(min(v), 1), round(max(v), 1)]
    med = lambda v: round(float(np.median(v)), 1)
    print(json.dumps({'examples': n_examples, 'windows': windows, 'abstract_rows': int(a_len.sum()), 'context_rows': int(c_len.sum()),
                      'align_cocited_ms': med(call_ms), 'align_cocited_ms_range': rng_of(call_ms),
                      'kernels_ms': round(float(np.median(kernel_ms)), 3), 'kernels_ms_range': [round(min(kernel_ms), 3), round(max(kernel_ms), 3)],
                      'host_tables_ms': med(host_ms), 'host_tables_ms_range': rng_of(host_ms),
                      'np_unique_ms': med(unique_ms), 'np_unique_ms_range': rng_of(unique_ms),
                      'numpy_loop_ms': med(loop_ms), 'numpy_loop_ms_range': rng_of(loop_ms),
                      'speedup': round(float(np.median(loop_ms)) / float(np.median(call_ms)), 1),
                      'pairs_that_differ_from_numpy': moved}), flush=True)


if __name__ == '__main__':
    ops.require_gpu()
    bench(int(sys.argv[1]) if len(sys.argv) > 1 else 100000, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
