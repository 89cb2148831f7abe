"""Inputs of the jointsm fixture (tests/golden/jointsm.npz), regenerated from seeds, and the float64 closed form they are checked
against.  Shared by make_golden_jointsm.py (which writes each case's seed, shapes and lens into the fixture beside the reference's
outputs) and by tests/test_jointsm_cpu.py / tests/test_gpu_jointsm.py (which read them back from the fixture: `spec_of`)."""
import numpy as np

D = 768
OFFSET = 0.5            # every row = scale * N(0, 1) + OFFSET * (one N(0, 1) vector per case): the common component of sentence embeddings
POOL_SWAP_CAP = 0.05    # share of a pool's adjacent candidate pairs that may be closer than the parity bound (end-to-end ranking test)

# name: seed, batch, (Sq, Sc), query lens, candidate lens, row scale, index of a pair of identical documents (or -1)
CASES = {
    'one':   dict(seed=101, shape=(3, 1, 1), qlens=[1, 1, 1], clens=[1, 1, 1], scale=1.0, dup=-1),
    's8':    dict(seed=102, shape=(6, 8, 8), qlens=[8, 8, 5, 1, 8, 3], clens=[8, 5, 8, 8, 1, 2], scale=0.6, dup=0),
    's8pk':  dict(seed=103, shape=(4, 8, 8), qlens=[8, 7, 8, 2], clens=[8, 8, 6, 8], scale=1.0, dup=2),
    'nb':    dict(seed=104, shape=(4, 7, 6), qlens=[7, 3, 1, 7], clens=[6, 6, 4, 1], scale=0.3, dup=-1),
    'mid':   dict(seed=105, shape=(4, 20, 30), qlens=[20, 17, 1, 16], clens=[30, 1, 30, 23], scale=0.6, dup=-1),
    'long':  dict(seed=106, shape=(3, 100, 128), qlens=[100, 33, 97], clens=[128, 128, 65], scale=0.3, dup=-1),
    'full':  dict(seed=107, shape=(3, 128, 128), qlens=[128, 128, 113], clens=[128, 127, 128], scale=1.0, dup=0),
    'fullf': dict(seed=108, shape=(2, 128, 128), qlens=[128, 64], clens=[128, 128], scale=0.3, dup=-1),
}
# WordSentAlignPolyEnc.score: one query against a pool of ragged candidates
POOLS = {
    'pool':  dict(seed=201, qlen=7, clens=[int(n) for n in np.random.RandomState(1).randint(1, 21, size=150)], scale=0.6,
                  keep_pair_scores=[0, 1, 149]),
    'poolf': dict(seed=202, qlen=12, clens=[int(n) for n in np.random.RandomState(2).randint(3, 31, size=130)], scale=0.3,
                  keep_pair_scores=[0]),
}


def case_inputs(spec):
    """-> q [B, Sq, 768], c [B, Sc, 768] float32 with zero pad rows, qlens, clens."""
    rng = np.random.RandomState(int(spec['seed']))
    b, sq, sc = (int(x) for x in spec['shape'])
    qlens, clens = [int(x) for x in spec['qlens']], [int(x) for x in spec['clens']]
    off = OFFSET * rng.standard_normal(D)
    q = (float(spec['scale']) * rng.standard_normal((b, sq, D)) + off).astype(np.float32)
    c = (float(spec['scale']) * rng.standard_normal((b, sc, D)) + off).astype(np.float32)
    dup = int(spec['dup'])
    if dup >= 0:
        assert sq == sc
        c[dup] = q[dup]
        clens[dup] = qlens[dup]
    for i in range(b):
        q[i, qlens[i]:] = 0.0
        c[i, clens[i]:] = 0.0
    return q, c, qlens, clens


def pool_inputs(spec):
    """-> query [qlen, 768], list of candidates [clen_i, 768], float32."""
    rng = np.random.RandomState(int(spec['seed']))
    off = OFFSET * rng.standard_normal(D)
    query = (float(spec['scale']) * rng.standard_normal((int(spec['qlen']), D)) + off).astype(np.float32)
    return query, [(float(spec['scale']) * rng.standard_normal((int(n), D)) + off).astype(np.float32) for n in spec['clens']]


def closed_form(q, c, qlens, clens):
    """float64: per pair 2 sum_ij p_ij d_ij with p = softmax over the valid block of d / sqrt(768); -> scores [B], p [B, Sq, Sc]
    (0 outside the valid block)."""
    scores, soft = np.zeros(len(qlens)), np.zeros((len(qlens), q.shape[1], c.shape[1]))
    for b, (ql, cl) in enumerate(zip(qlens, clens)):
        d = q[b, :ql].astype(np.float64) @ c[b, :cl].astype(np.float64).T
        e = np.exp((d - d.max()) / np.sqrt(float(D)))
        soft[b, :ql, :cl] = e / e.sum()
        scores[b] = 2.0 * (soft[b, :ql, :cl] * d).sum()
    return scores, soft


def spec_of(fixture, name):
    """The case or pool `name` as the fixture records it."""
    keys = ('seed', 'shape', 'qlens', 'clens', 'scale', 'dup') if f'{name}_shape' in fixture else ('seed', 'qlen', 'clens', 'scale')
    return {k: fixture[f'{name}_{k}'] for k in keys}
