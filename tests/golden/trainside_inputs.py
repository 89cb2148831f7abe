"""Inputs and float64 yardsticks of the train-side fixture (tests/golden/trainside.npz): the backward of the joint soft-max alignment
score and the supervised-alignment distances l2sup / l2sup_weighted, forward and backward.  Shared by make_golden_trainside.py (which
runs the reference on these inputs and records its own fp32 error against the yardsticks) and by the tests (which hold the kernels to
a bound made of that error).  The jointsm inputs are jointsm_inputs.CASES, regenerated from their seeds by case_inputs."""
import math

import numpy as np
import torch

from jointsm_inputs import CASES, D, OFFSET, case_inputs  # noqa: F401  (re-exported)

STORE_JOINTSM_GRADS = ('one', 'nb', 's8pk')         # cases whose reference fp32 gradients the fixture holds
STORE_L2SUP_GRADS = ('e8', 'e8co')

_E8 = dict(shape=(4, 8, 8), qlens=[1, 3, 8, 5], clens=[1, 8, 2, 5], scale=0.6)
# name: seed, (B, Sq, Sc), lens, alignment (query row, candidate row) per pair, pairs whose aligned candidate row is a copy of the query row
L2SUP_CASES = {
    'e8':     dict(_E8, seed=301, align=[[0, 0], [1, 5], [6, 1], [2, 3]], same=[]),             # indices in range
    'e8last': dict(_E8, seed=302, align=[[0, 0], [2, 7], [7, 1], [4, 4]], same=[]),             # at the last valid row
    'e8clip': dict(_E8, seed=302, align=[[3, 5], [7, 8], [9, 2], [5, 100]], same=[]),           # beyond the length: clipped to e8last's
    'e8co':   dict(_E8, seed=303, align=[[0, 0], [1, 5], [6, 1], [2, 3]], same=[1, 3]),         # coincident aligned rows: d == 0
    'e40':    dict(seed=304, shape=(1, 40, 40), qlens=[33], clens=[40], scale=0.6, align=[[17, 39]], same=[]),
    'full':   dict(seed=305, shape=(1, 128, 128), qlens=[128], clens=[128], scale=0.6, align=[[127, 64]], same=[]),
}


def jointsm_upstream(name, spec):
    """gs [B] float32 = dLoss / dscore of a jointsm case: seeded; s8 holds one zero and one negative entry."""
    gs = np.random.RandomState(int(spec['seed']) + 1000).standard_normal(int(spec['shape'][0])).astype(np.float32)
    if name == 's8':
        gs[1] = 0.0
        gs[2] = -abs(gs[2]) - 0.25
    return gs


def l2sup_inputs(spec):
    """-> q [B, Sq, 768], c [B, Sc, 768] float32 with zero pad rows, qlens, clens, align (list of [int, int]), gs [B] float32."""
    rng = np.random.RandomState(int(spec['seed']))
    b, sq, sc = (int(x) for x in spec['shape'])
    qlens, clens = [int(x) for x in spec['qlens']], [int(x) for x in spec['clens']]
    off = OFFSET * rng.standard_normal(D)
    q = (float(spec['scale']) * rng.standard_normal((b, sq, D)) + off).astype(np.float32)
    c = (float(spec['scale']) * rng.standard_normal((b, sc, D)) + off).astype(np.float32)
    gs = rng.standard_normal(b).astype(np.float32)
    align = [[int(a0), int(a1)] for a0, a1 in spec['align']]
    for p in spec['same']:
        c[p, min(align[p][1], clens[p] - 1)] = q[p, min(align[p][0], qlens[p] - 1)]
    for i in range(b):
        q[i, qlens[i]:] = 0.0
        c[i, clens[i]:] = 0.0
    return q, c, qlens, clens, align, gs


def jointsm_sims(qt, ct, qlens, clens):
    """The closed form S = 2 sum_ij p_ij d_ij of every pair on torch tensors [B, S, 768], in their dtype, differentiable -> [B]."""
    sims = []
    for b, (ql, cl) in enumerate(zip(qlens, clens)):
        d = (qt[b, :ql] @ ct[b, :cl].T).reshape(-1)
        sims.append(2.0 * (torch.softmax(d / math.sqrt(float(D)), dim=0) * d).sum())
    return torch.stack(sims)


def jointsm_grad64(q, c, qlens, clens, gs):
    """float64 autograd over the closed form, loss = sum_b gs[b] S_b -> grad_q [B, Sq, 768], grad_c [B, Sc, 768] float64 (pad rows 0)."""
    qt = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    ct = torch.tensor(c, dtype=torch.float64, requires_grad=True)
    (jointsm_sims(qt, ct, qlens, clens) * torch.tensor(gs, dtype=torch.float64)).sum().backward()
    return qt.grad.numpy(), ct.grad.numpy()


def l2sup_dists(qt, ct, qlens, clens, align, weighted):
    """The distance ||q_i - c_j|| (/ (q_len c_len)) of every pair's clipped alignment on torch tensors [B, S, 768], in their dtype,
    differentiable through torch.cdist (whose rule gives 0 for coincident rows) -> [B]."""
    dist = []
    for b, (ql, cl) in enumerate(zip(qlens, clens)):
        i, j = min(align[b][0], ql - 1), min(align[b][1], cl - 1)
        d = torch.cdist(qt[b, i:i + 1], ct[b, j:j + 1])[0, 0]
        dist.append(d / float(ql * cl) if weighted else d)
    return torch.stack(dist)


def l2sup_ref64(q, c, qlens, clens, align, weighted, gs):
    """float64: l2sup_dists and, by autograd, the gradient of loss = sum_b gs[b] * (-distance_b)
    -> dist [B], grad_q [B, Sq, 768], grad_c [B, Sc, 768]."""
    qt = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    ct = torch.tensor(c, dtype=torch.float64, requires_grad=True)
    dist = l2sup_dists(qt, ct, qlens, clens, align, weighted)
    (-dist * torch.tensor(gs, dtype=torch.float64)).sum().backward()
    return dist.detach().numpy(), qt.grad.numpy(), ct.grad.numpy()


def bound(ref_err, max_grad):
    """What a kernel may deviate from the float64 yardstick: four times the reference's own fp32 error (the margin for another
    summation order), and never less than four fp32 roundings of the largest entry."""
    return max(4.0 * float(ref_err), 4.0 * 2.0 ** -23 * float(max_grad))
