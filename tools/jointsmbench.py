"""jointsm against its yardstick: aspire_jointsm_* and aspire_dotmax_* (ASPIRE_SIM_DOT) on identical inputs -- the same matrix
products, jointsm adds one exp and a rescale per block entry.

    python tools/jointsmbench.py                  # both shapes, one JSON line each
    python tools/jointsmbench.py rank 200         # only the batched rank, 200 timed calls per entry (for a profiler run)

  rank   config 4's shape: 50 jobs x 125 candidates, documents of 3..20 rows (one wave per pair + the segmented rank)
  cross  32 queries x 50 000 candidates x 8 rows (the CROSS kernels that keep candidate rows in LDS)
Times are device-event times per call over `reps` calls after a warm-up, the two entries alternating in blocks of 10 calls."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aspire_amd import _lib, ops  # noqa: E402


def _timed(fns, reps, block=10):
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    total = {k: 0.0 for k in fns}
    for _ in range(max(1, reps // block)):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(block):
                fn()
            t1.record()
            t1.synchronize()
            total[k] += t0.elapsed_time(t1)
    n = max(1, reps // block) * block
    return {k: 1e3 * v / n for k, v in total.items()}           # us per call


def _rows(gen, n):
    return 0.6 * torch.randn(n, 768, device='cuda', generator=gen) + 0.5 * torch.randn(768, device='cuda', generator=gen)


def rank(reps):
    gen = torch.Generator(device='cuda').manual_seed(4)
    rng = np.random.RandomState(4)
    J, per = 50, 125
    clen, qlen = rng.randint(3, 21, J * per).astype(np.int32), rng.randint(3, 21, J).astype(np.int32)
    sets = []
    for lens in (qlen, clen):
        start = (np.cumsum(lens) - lens).astype(np.int32)
        sets.append(ops.DeviceRepSet(_rows(gen, int(lens.sum())), torch.from_numpy(start).cuda(), torch.from_numpy(lens).cuda(), 0, 20,
                                     lens_host=lens.tolist()))
    q, c = sets
    job_off = torch.arange(J + 1, dtype=torch.int32, device='cuda') * per
    outs = {k: (torch.empty(c.n, device='cuda'), torch.empty(J, per, device='cuda'), torch.empty(J, per, device='cuda', dtype=torch.int64))
            for k in ('jointsm', 'dotmax')}
    ws = torch.empty(16, device='cuda', dtype=torch.uint8)
    us = _timed({'jointsm': lambda: ops.jointsm_rank_batch(q, c, job_off, per, per, out=outs['jointsm'], workspace=ws),
                 'dotmax': lambda: ops.dotmax_rank_batch(q, c, job_off, per, per, sim=_lib.SIM_DOT, out=outs['dotmax'], workspace=ws)}, reps)
    return {'shape': 'rank 50 x 125 x 3..20 rows', 'jointsm_us': us['jointsm'], 'dotmax_us': us['dotmax'], 'ratio': us['jointsm'] / us['dotmax']}


def cross(reps):
    gen = torch.Generator(device='cuda').manual_seed(3)
    Q, C, S = 32, 50000, 8
    sets = []
    for n in (Q, C):
        lens = torch.full((n,), S, dtype=torch.int32, device='cuda')
        sets.append(ops.DeviceRepSet(_rows(gen, n * S), torch.arange(n, dtype=torch.int32, device='cuda') * S, lens, 0, S, lens_host=[S] * n))
    q, c = sets
    us = _timed({'jointsm': lambda: ops.jointsm_scores(q, c, _lib.PAIR_CROSS),
                 'dotmax': lambda: ops.dotmax_scores(q, c, _lib.PAIR_CROSS, sim=_lib.SIM_DOT)}, reps)
    return {'shape': 'cross 32 x 50000 x 8 rows', 'jointsm_us': us['jointsm'], 'dotmax_us': us['dotmax'], 'ratio': us['jointsm'] / us['dotmax']}


if __name__ == '__main__':
    ops.require_gpu()
    which = sys.argv[1] if len(sys.argv) > 1 else 'both'
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 400
    for name, fn in (('rank', rank), ('cross', cross)):
        if which in (name, 'both'):
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in fn(reps).items()}))
