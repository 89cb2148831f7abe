"""'l2top2' / 'l2attention' over batched jobs: ONE scorer.rank_pools call (aspire_l2agg_rank_batch_f32: one upload of the queries, one
scoring launch, one rank launch, two downloads) against the route these two aggregations had before it, a loop of scorer.rank_pool
per query (per query: an upload, aspire_l2agg_scores_f32, aspire_topk_desc_f32, two downloads).  Both routes run in this tree, so
one process alternates them.

    python tools/l2aggbench.py                    # both shapes, both methods, three rounds; one JSON line per (shape, method)
    python tools/l2aggbench.py csf 1 5            # one shape ('csf' / 'pool'), rounds, timed windows per round (a profiler run)

  csf   config 4's shape: 50 jobs x ~125 candidates (100 .. 150), documents and queries of 3 .. 20 rows
  pool  20 jobs x 1000 candidates x 8 rows
The pools are index lists into one resident row matrix (RepStore.to_device's layout); the queries are host arrays, uploaded by
either route.  A figure is the median over `windows` (>= 20) device-event windows of >= 0.3 s each, after 3 warm-up calls; the two
routes alternate round by round, and the spread is the range of the rounds' medians."""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aspire_amd import ops, scorer  # noqa: E402

WINDOW_S, WARMUPS = 0.3, 3
METHODS = (('l2top2', None), ('l2attention', {'cdatt_sm_temp': 0.5}))


def _window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / calls           # us per call


def _median_us(fn, windows):
    for _ in range(WARMUPS):
        fn()
    torch.cuda.synchronize()
    calls = max(1, math.ceil(WINDOW_S * 1e6 / _window(fn, 1)))
    return float(np.median([_window(fn, calls) for _ in range(windows)])), calls


def _jobs(sizes, c_rows, q_rows, seed):
    """J pools over one resident row matrix + the J queries as host arrays"""
    rng = np.random.RandomState(seed)
    gen = torch.Generator(device='cuda').manual_seed(seed)
    c_len = rng.randint(c_rows[0], c_rows[1] + 1, int(sum(sizes))).astype(np.int32)
    c_start = (np.cumsum(c_len) - c_len).astype(np.int32)
    rows = torch.randn(int(c_len.sum()), 768, device='cuda', generator=gen)
    start, lens = torch.from_numpy(c_start).cuda(), torch.from_numpy(c_len).cuda()
    pools, lo = [], 0
    for n in sizes:
        rs = ops.DeviceRepSet(rows, start[lo:lo + n].contiguous(), lens[lo:lo + n].contiguous(), ext=0, max_len=int(c_len[lo:lo + n].max()),
                              lens_host=c_len[lo:lo + n].tolist())
        pools.append(scorer.CandidatePool.from_repset(rs))
        lo += n
    queries = [rng.standard_normal((int(n), 768)).astype(np.float32) for n in rng.randint(q_rows[0], q_rows[1] + 1, len(sizes))]
    return queries, pools


def shapes():
    rng = np.random.RandomState(4)
    return {'csf': ('50 x ~125 x 3..20 rows', lambda: _jobs(rng.randint(100, 151, 50).tolist(), (3, 20), (3, 20), 4)),
            'pool': ('20 x 1000 x 8 rows', lambda: _jobs([1000] * 20, (8, 8), (8, 8), 20))}


def bench(name, rounds, windows):
    label, make = shapes()[name]
    queries, pools = make()
    for method, hparams in METHODS:
        routes = {'batched': lambda: scorer.rank_pools(queries, pools, method=method, hparams=hparams),
                  'per_query': lambda: [scorer.rank_pool([q], p, method=method, hparams=hparams) for q, p in zip(queries, pools)]}
        # the two routes rank the same pools: the same order wherever their scores differ by more than rounding
        a, b = routes['batched'](), [r[0] for r in routes['per_query']()]
        diff = max(abs(x[1] - y[1]) for ra, rb in zip(a, b) for x, y in zip(ra, rb))
        moved = sum(x[0] != y[0] for ra, rb in zip(a, b) for x, y in zip(ra, rb))
        us = {k: [] for k in routes}
        calls = {}
        for _ in range(rounds):
            for k, fn in routes.items():
                t, calls[k] = _median_us(fn, windows)
                us[k].append(t)
        out = {'shape': label, 'method': method, 'pairs': sum(len(p) for p in pools), 'windows': windows, 'calls_per_window': calls,
               'max_score_diff': diff, 'list_positions_that_differ': moved}
        for k, v in us.items():
            out[f'{k}_us'] = [round(t, 1) for t in v]
            out[f'{k}_us_median'] = round(float(np.median(v)), 1)
        out['speedup'] = round(float(np.median(us['per_query'])) / float(np.median(us['batched'])), 2)
        out['speedup_worst_round_pairing'] = round(min(us['per_query']) / max(us['batched']), 2)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    ops.require_gpu()
    which = sys.argv[1] if len(sys.argv) > 1 else 'both'
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    windows = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    for name in ('csf', 'pool'):
        if which in (name, 'both'):
            bench(name, rounds, windows)
