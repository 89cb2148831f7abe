"""A candidate that shares a sentence with its query, on rows that carry a common vector (tools/fuzz_parity.py seeds
111 / 114 of round 4).  geomloss's cost is sqrt(clamp_min(|x|^2 - 2 x.y + |y|^2, 1e-8)) (pair_distances.py:48-56 via geomloss 0.2.4's
`distances`): for two EQUAL rows the bracket is rounding noise of |x|^2 -- in float64 ~1e-13, clamped, cost 1e-4; in fp32 a few ulps of
|x|^2, so the reference's own fp32 path returns sqrt(noise), anything between 1e-4 and ~5e-2 by rounding luck.  The HIP kernels are held
to the FLOAT64 oracle at 1e-4 in every kernel family; the fp32 oracle's own distance from float64 is printed beside it."""
import numpy as np
import pytest
import torch

from oracle import aspire_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope='module')
def amd():
    from aspire_amd import ops, scorer, _lib
    assert torch.cuda.is_available()
    return type('NS', (), dict(ops=ops, scorer=scorer, lib=_lib, pinned=_lib.pinned))


def _case(seed, sigma, nq, nc, qlen, clen, near=0.0):
    g = torch.Generator().manual_seed(seed)
    common = sigma * torch.randn(768, generator=g)
    q = [torch.randn(qlen, 768, generator=g) + common for _ in range(nq)]
    c = [torch.randn(int(n), 768, generator=g) + common for n in torch.randint(max(1, clen - 3), clen + 1, (nc,), generator=g)]
    delta = near * torch.randn(768, generator=g) if near else 0.0    # near > 0: the shared rows are NEARLY equal (drawn last: q and c are the equal-rows case's)
    shared = []
    for k, j in enumerate(range(1, nc, max(1, nc // 12))):          # a dozen candidates repeat one of the first query's sentences
        row = k % qlen
        c[j] = c[j].clone()
        c[j][k % len(c[j])] = q[0][row] + delta
        shared.append(j)
    c[0] = q[0][:1] + delta                                          # and a one-sentence candidate that IS a query sentence
    shared.append(0)
    return q, c, shared


def _sim64(x, y):
    return orc.get_similarity(x.double(), y.double())


FAMILIES = [
    # name, pins, queries, candidates, query rows, candidate rows, planes
    ('fused', dict(OT_FORM='fused'), 1, 4200, 8, 8, False),
    ('small', dict(OT_FORM='small'), 2, 60, 8, 8, False),
    ('one wave per pair', dict(OT_FORM='one'), 2, 900, 8, 8, False),
    ('tile16', dict(), 1, 2600, 12, 14, False),
    ('gram bf16x3', dict(COST_PATH='mfma'), 24, 300, 8, 8, False),
    ('plane tiles', dict(COST_PATH='mfma'), 24, 2100, 8, 8, True),
    # documents beyond 25 rows: torch.cdist's matmul formula for -cdist (the reference's own max-sim there is sqrt(noise): 5e-2 bar), geomloss's cost
    # still from the exact sum where it cancels (round 6: tools/fuzz_parity.py 24 412 planes found the plane tiles deriving it from the noisy -cdist)
    ('small, 30 rows', dict(OT_FORM='small'), 2, 60, 28, 30, False),
    ('tile16 records, 32 rows', dict(), 1, 2600, 30, 32, False),
    ('generic, 40 rows', dict(), 1, 40, 40, 40, False),
    ('gram bf16x3, 32 rows', dict(COST_PATH='mfma'), 24, 300, 30, 32, False),
    ('plane tiles, 32 rows', dict(COST_PATH='mfma'), 2, 2300, 30, 32, True),
]


@pytest.mark.parametrize('sigma', [0.0, 1.0, 3.0])
@pytest.mark.parametrize('family', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_shared_sentence_against_float64(amd, family, sigma):
    name, pins, nq, nc, qlen, clen, planes = family
    q, c, shared = _case(1000 + int(10 * sigma), sigma, nq, nc, qlen, clen)
    pool = amd.scorer.CandidatePool(c)
    if planes:
        pool.prepare_planes()
    with amd.pinned(**pins):
        ot = amd.scorer.score_pool(q, pool, method='ot', schedule='pair').cpu().numpy()
        l2 = amd.scorer.score_pool(q, pool, method='l2max').cpu().numpy()
    assert np.isfinite(ot).all() and np.isfinite(l2).all()
    rng = np.random.RandomState(3)
    others = rng.choice(nc, size=6, replace=False).tolist()
    worst, ref_gap = 0.0, 0.0
    for j in shared + others:
        w64 = _sim64(q[0], c[j])
        w32 = orc.get_similarity(q[0], c[j])
        e = abs(float(ot[0, j]) - w64)
        worst, ref_gap = max(worst, e), max(ref_gap, abs(w32 - w64))
        assert e < TOL, (name, sigma, j, j in shared, float(ot[0, j]), w64, w32)
        l64 = -torch.cdist(q[0].double(), c[j].double()).min().item()
        # max-sim of a shared sentence: the best match is the pair of equal rows, -cdist = -0 exactly in float64; torch.cdist's
        # fp32 direct formula gives exactly 0 too (<= 25 rows), and so must the kernels' redo of cancelling entries
        tol_l2 = 5e-2 if (j in shared and max(qlen, len(c[j])) > 25) else TOL      # beyond 25 rows the reference's own -cdist of equal rows is sqrt(noise)
        assert abs(float(l2[0, j]) - l64) < tol_l2, (name, sigma, j, float(l2[0, j]), l64)
    print(f'{name:12s} sigma {sigma}: max |HIP - float64 oracle| {worst:.2e}; the fp32 oracle itself is {ref_gap:.2e} from float64')


def _rel(got, want):
    return abs(got - want) / abs(want)


def _expansion_max_sim(x, y):
    """-min of the fp32 expansion |x|^2 - 2 x.y + |y|^2 with torch CPU ops: what a kernel gives when its redo did NOT run."""
    sq = (x * x).sum(1)[:, None] - 2.0 * (x @ y.t()) + (y * y).sum(1)[None, :]
    return -sq.clamp_min(0).sqrt().min().item()


# |delta| = 0.0125 sqrt(768) = 0.35: d^2 = 0.12 against a threshold of 1e-4 (2 * 768)^2 = 236 at sigma = 0, more beyond.  (0.05 left the
# expansion of single pairs within the bar by rounding luck -- 7e-7 against 2.6e-6 in 'fused' at sigma 0; at 0.05 / 4 every pair's misses
# it tenfold or more.)
NEAR = 0.0125


@pytest.mark.parametrize('sigma', [0.0, 1.0, 3.0])
@pytest.mark.parametrize('family', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_nearly_shared_sentence_exact_sum(amd, family, sigma):
    """The arithmetic of the exact sums (the equal-rows test above only checks that the right rows are addressed: their exact sum is 0
    over any coordinates in any order).  The shared rows differ by delta = NEAR randn(768): the rule fires in every family, the exact
    sum is non-zero and depends on every coordinate.  otAspire: the file's TOL against float64.  Max-sim of a shared candidate = -|delta|:
    relative error against float64 under max(4 e_ref, 1e-6), e_ref = the relative error of torch.cdist's own fp32 direct formula (CPU,
    <= 25 rows) on the same inputs, 4 = the margin test_gpu_baselines.py gives another summation order; beyond 25 rows the 5e-2 of the
    test above.  The fp32 EXPANSION of the same pairs has to miss that bar, or the test could not tell a redo that ran from none."""
    name, pins, nq, nc, qlen, clen, planes = family
    q, c, shared = _case(1000 + int(10 * sigma), sigma, nq, nc, qlen, clen, near=NEAR)
    direct = max(qlen, clen) <= 25
    l64 = {j: -torch.cdist(q[0].double(), c[j].double()).min().item() for j in shared}
    e_ref = max(_rel(-torch.cdist(q[0], c[j]).min().item(), l64[j]) for j in shared) if direct else float('nan')
    bar = max(4 * e_ref, 1e-6) if direct else float('nan')
    if direct:
        e_exp = min(_rel(_expansion_max_sim(q[0], c[j]), l64[j]) for j in shared)
        assert e_exp > bar, (name, sigma, e_exp, bar)        # every shared pair's expansion misses the bar
    pool = amd.scorer.CandidatePool(c)
    if planes:
        pool.prepare_planes()
    with amd.pinned(**pins):
        ot = amd.scorer.score_pool(q, pool, method='ot', schedule='pair').cpu().numpy()
        l2 = amd.scorer.score_pool(q, pool, method='l2max').cpu().numpy()
    assert np.isfinite(ot).all() and np.isfinite(l2).all()
    others = np.random.RandomState(3).choice(nc, size=6, replace=False).tolist()
    worst_ot = max(abs(float(ot[0, j]) - _sim64(q[0], c[j])) for j in shared + others)
    e_hip = max(_rel(float(l2[0, j]), l64[j]) for j in shared)
    e_abs = max(abs(float(l2[0, j]) - l64[j]) for j in shared)
    print(f'{name:12s} sigma {sigma}: otAspire max |HIP - float64| {worst_ot:.2e}; shared max-sim: HIP rel {e_hip:.3e} (abs {e_abs:.2e}), '
          f'torch fp32 direct e_ref {e_ref:.3e}, ratio {e_hip / e_ref:.2f}, bar {bar:.2e}')
    for j in shared + others:
        assert abs(float(ot[0, j]) - _sim64(q[0], c[j])) < TOL, (name, sigma, j, j in shared, float(ot[0, j]), _sim64(q[0], c[j]))
    for j in shared:
        if direct:
            assert _rel(float(l2[0, j]), l64[j]) <= bar, (name, sigma, j, float(l2[0, j]), l64[j], e_ref, bar)
        else:
            assert abs(float(l2[0, j]) - l64[j]) < 5e-2, (name, sigma, j, float(l2[0, j]), l64[j])
    for j in others:
        assert abs(float(l2[0, j]) - (-torch.cdist(q[0].double(), c[j].double()).min().item())) < TOL, (name, sigma, j, float(l2[0, j]))
