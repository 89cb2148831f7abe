"""The precomputed-embedding rankers' score + rank: ops.dense_rank_batch (aspire_dense_rank_batch_f32: row-index lists into one
resident matrix) against the only route there was before it, ops.l2max_rank_batch over one-row CSR documents with the same pools
MATERIALISED (every pool's rows copied out of the matrix, a start / len entry per candidate).  Both routes run in this tree, so one
process alternates them.

    python tools/densebench.py                    # both shapes, three rounds; one JSON line per shape
    python tools/densebench.py deep 1 5           # one shape ('csf' / 'deep'), rounds, timed windows per round

  csf   CSFCube-like: 50 jobs x ~125 candidates (100 .. 150) drawn from 5 000 rows
  deep  50 jobs x 5 000 candidates drawn from 20 000 rows (every row sits in about 12 pools)
Both rank every pool in full (k = the longest pool, what nearest.rank_pool asks for); `scores_only` is the same call with k = 0.
A figure is the median over `windows` device-event windows of >= 0.3 s each, after 3 warm-up calls; the routes alternate round by
round.  hbm_fraction = C * 3072 B / time over the 6.29 TB/s a float4 copy reaches on this chip -- an algorithmic rate: the matrices
here fit the Infinity Cache and rows shared by pools are served from it."""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aspire_amd import _lib, ops  # noqa: E402

WINDOW_S, WARMUPS, COPY_TBS = 0.3, 3, 6.29


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
    return float(np.median([_window(fn, calls) for _ in range(windows)]))


SHAPES = {'csf': ('50 x ~125 of 5000 rows', 5000, lambda rng: rng.integers(100, 151, 50).tolist()),
          'deep': ('50 x 5000 of 20000 rows', 20000, lambda rng: [5000] * 50)}


def bench(name, rounds, windows):
    label, n_rows, sizes_of = SHAPES[name]
    rng = np.random.default_rng(5)
    sizes = sizes_of(rng)
    J, C, max_job = len(sizes), int(sum(sizes)), max(sizes)
    rows = torch.randn(n_rows, 768, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))
    q_host = rng.choice(n_rows, J, replace=False)
    c_host = np.concatenate([rng.choice(n_rows, n, replace=False) for n in sizes])
    q_idx = torch.from_numpy(q_host.astype(np.int32)).cuda()
    cand_idx = torch.from_numpy(c_host.astype(np.int32)).cuda()
    job_off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).cuda()
    # the old route's inputs: the pools copied out, one-row documents
    ones = lambda n: torch.ones(n, dtype=torch.int32, device='cuda')
    q_set = ops.DeviceRepSet(rows[q_idx.long()].contiguous(), torch.arange(J, dtype=torch.int32, device='cuda'), ones(J), 0, 1, lens_host=[1] * J)
    c_set = ops.DeviceRepSet(rows[cand_idx.long()].contiguous(), torch.arange(C, dtype=torch.int32, device='cuda'), ones(C), 0, 1,
                             lens_host=[1] * C)
    routes = {}
    for tag, k in (('rank', max_job), ('scores_only', 0)):
        out_d = ops.dense_rank_batch(rows, q_idx, cand_idx, job_off, max_job, k)
        out_l = ops.l2max_rank_batch(q_set, c_set, job_off, max_job, k)
        ws_d = torch.empty(max(_lib.lib.aspire_dense_rank_batch_workspace_bytes(J, C, max_job, k), 16), device='cuda', dtype=torch.uint8)
        ws_l = torch.empty(max(ops.rank_batch_workspace_bytes('l2max', q_set, c_set, max_job, k), 16), device='cuda', dtype=torch.uint8)
        routes[f'dense_{tag}'] = lambda k=k, o=out_d, w=ws_d: ops.dense_rank_batch(rows, q_idx, cand_idx, job_off, max_job, k, out=o, workspace=w)
        routes[f'l2max_csr_{tag}'] = lambda k=k, o=out_l, w=ws_l: ops.l2max_rank_batch(q_set, c_set, job_off, max_job, k, out=o, workspace=w)
        if k:
            diff = float((out_d[0] - out_l[0]).abs().max())
            moved = int((out_d[2] != out_l[2]).sum())
    us = {r: [] for r in routes}
    for _ in range(rounds):
        for r, fn in routes.items():
            us[r].append(_median_us(fn, windows))
    out = {'shape': label, 'jobs': J, 'candidates': C, 'k': max_job, 'windows': windows, 'max_score_diff_between_routes': diff,
           'list_positions_that_differ': moved, 'pool_copy_bytes_old_route': C * 3072 + 8 * C}
    for r, v in us.items():
        med = float(np.median(v))
        out[f'{r}_us'] = [round(t, 1) for t in v]
        out[f'{r}_us_median'] = round(med, 1)
        if r.startswith('dense'):
            out[f'{r}_TBs'] = round(C * 3072 / med / 1e6, 3)
            out[f'{r}_hbm_fraction'] = round(C * 3072 / med / 1e6 / COPY_TBS, 3)
    for tag in ('rank', 'scores_only'):
        out[f'speedup_{tag}'] = round(float(np.median(us[f'l2max_csr_{tag}'])) / float(np.median(us[f'dense_{tag}'])), 2)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    ops.require_gpu()
    which = sys.argv[1] if len(sys.argv) > 1 else 'both'
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    windows = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    for name in SHAPES:
        if which in (name, 'both'):
            bench(name, rounds, windows)
