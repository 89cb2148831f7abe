"""GPU: the pair arg-max kernel (aspire_amd/csrc/dot_argmax.hip: aspire_dot_argmax_f32) through ops.dot_argmax and
torch.ops.aspire.dot_argmax -- where np.unravel_index(np.matmul(q, c.T).argmax(), ...) lands, per pair, in one launch.

The yardstick is float64 with the reference's own fp32 error as the bar: for a pair's block s64,
    tol = max(4 x max|np.float32 matmul - s64|, 4 x 2^-23 x max|s64|)      (factor 4: another summation order)
the kernel's pick must satisfy s64[pick] >= s64.max() - tol, and where float64's top two entries are more than tol apart the
pick must BE float64's argmax.  Pairs whose gap is within tol are excused from the second check; at most 2 % may be.
Documents of {1, 2, 15, 16, 17, 31, 33, 128} rows on both sides (every combination once, and random draws for P in
{1, 3, 4, 5, 9} around the four waves of a workgroup), shared between pairs and stored out of order in the row matrix.

Observed on an MI355X (printed by test_picks_against_float64): 172 pairs, largest tol / gap 0.075, excused 0 (0.00 %).  The random
pairs take two different documents: a document of unit rows against itself has a diagonal of ones, ties by construction (drawn with
repeats, 2 of 172 pairs were such self pairs, tol / gap 2322, and were excused: 1.16 %).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 768
SIZES = (1, 2, 15, 16, 17, 31, 33, 128)
PS = (1, 3, 4, 5, 9)
KINDS = ('normal', 'common')
SENTINEL_ARG, SENTINEL_BEST = -7, 123.0


def _docs(kind, rng, lens):
    if kind == 'normal':
        return [rng.standard_normal((n, D)).astype(np.float32) for n in lens]
    common = rng.standard_normal(D)
    out = []
    for n in lens:
        x = common + 0.15 * rng.standard_normal((n, D))
        out.append((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
    return out


def _store(docs, rng):
    """the documents in one row matrix in a shuffled order: (rows tensor on the GPU, start [n], len [n]) in document order"""
    order = rng.permutation(len(docs))
    start = np.zeros(len(docs), np.int64)
    at = 0
    for k in order:
        start[k] = at
        at += docs[k].shape[0]
    rows = np.zeros((at, D), np.float32)
    for k, d in enumerate(docs):
        rows[start[k]:start[k] + d.shape[0]] = d
    return torch.from_numpy(rows).cuda(), start, np.array([d.shape[0] for d in docs], np.int64)


def _view(rows, start, lens, ids, max_len=None):
    from aspire_amd import ops
    ids = np.asarray(ids)
    to = lambda a: torch.from_numpy(a[ids].astype(np.int32)).cuda()
    return ops.DeviceRepSet(rows, to(start), to(lens), ext=0, max_len=int(lens[ids].max()) if max_len is None else max_len,
                            lens_host=lens[ids].tolist())


class Run:
    """one dot_argmax call over pairs of documents drawn from one store, with dotmax's scores of the same pairs"""

    def __init__(self, kind, pairs_of, seed):
        from aspire_amd import _lib, ops
        rng = np.random.default_rng(seed)
        # every size twice: a pair may meet a document of its own size, and documents are shared between the pairs
        self.docs = _docs(kind, rng, SIZES + SIZES)
        rows, start, lens = _store(self.docs, rng)
        self.pairs = pairs_of(rng, len(self.docs))
        self.q = _view(rows, start, lens, [a for a, _ in self.pairs])
        self.c = _view(rows, start, lens, [b for _, b in self.pairs])
        arg, best = ops.dot_argmax(self.q, self.c)
        self.arg, self.best = arg.cpu().numpy(), best.cpu().numpy()
        self.dotmax = ops.dotmax_scores(self.q, self.c, pairing=_lib.PAIR_PAIRED, sim=_lib.SIM_DOT).cpu().numpy()
        self.kind = kind


@pytest.fixture(scope='module')
def runs():
    out = []
    for k, kind in enumerate(KINDS):
        every = lambda rng, n: [(a, 8 + b) for a in range(8) for b in range(8)]       # all 64 size combinations
        out.append(Run(kind, every, seed=10 + k))
        for P in PS:
            # two different documents per pair (a unit-row document against itself has a diagonal of ones: ties by construction)
            out.append(Run(kind, lambda rng, n, P=P: [tuple(rng.choice(n, 2, replace=False)) for _ in range(P)], seed=100 * P + k))
    return out


def test_picks_against_float64(runs):
    n_pairs = excused = 0
    worst = 0.0
    for run in runs:
        assert run.arg.shape == (len(run.pairs), 2) and run.arg.dtype == np.int32
        for p, (a, b) in enumerate(run.pairs):
            q, c = run.docs[a], run.docs[b]
            s64 = q.astype(np.float64) @ c.astype(np.float64).T
            s32 = np.matmul(q, c.T)
            tol = max(4 * np.abs(s32 - s64).max(), 4 * 2.0 ** -23 * np.abs(s64).max())
            i, j = (int(x) for x in run.arg[p])
            assert 0 <= i < q.shape[0] and 0 <= j < c.shape[0], (run.kind, p, (i, j), s64.shape)
            assert s64[i, j] >= s64.max() - tol, (run.kind, p, (i, j), s64[i, j], s64.max(), tol)
            top = np.sort(s64, axis=None)[::-1]
            gap = top[0] - top[1] if top.size > 1 else np.inf
            n_pairs += 1
            worst = max(worst, tol / gap)
            if gap > tol:
                assert (i, j) == np.unravel_index(s64.argmax(), s64.shape), (run.kind, p, (i, j), gap, tol)
            else:
                excused += 1
            # best is the dot product at the pick, to the same bar
            assert abs(float(run.best[p]) - s64[i, j]) <= tol
    print(f'[dot_argmax] {n_pairs} pairs: largest tol / gap {worst:.3f}, excused {excused} ({100.0 * excused / n_pairs:.2f} %)')
    assert n_pairs == 2 * (64 + sum(PS))
    assert excused <= 0.02 * n_pairs


def test_best_has_dotmax_bits(runs):
    for run in runs:
        assert np.isfinite(run.best).all()
        assert run.best.tobytes() == run.dotmax.tobytes(), (run.kind, len(run.pairs))


def _one_pair(q, c):
    from aspire_amd import ops
    arg, best = ops.dot_argmax(ops.DeviceRepSet.from_list([q]), ops.DeviceRepSet.from_list([c]))
    return tuple(arg.cpu().numpy()[0].tolist()), float(best.cpu().numpy()[0])


def _numpy_pick(q, c):
    with np.errstate(all='ignore'):
        s = np.matmul(q, c.T)
    return tuple(int(x) for x in np.unravel_index(s.argmax(), s.shape)), s


def test_equal_maxima_in_four_tiles_give_the_first_in_row_major_order():
    rng = np.random.default_rng(3)
    u = rng.standard_normal(D).astype(np.float32)
    q = 0.1 * rng.standard_normal((21, D)).astype(np.float32)
    c = 0.1 * rng.standard_normal((23, D)).astype(np.float32)
    q[2] = q[18] = 3 * u
    c[3] = c[20] = 3 * u
    pick, s = _numpy_pick(q, c)
    assert s[2, 3] == s[2, 20] == s[18, 3] == s[18, 20] == s.max() and pick == (2, 3)
    got, best = _one_pair(q, c)
    assert got == (2, 3)
    # the other way round too (candidate tiles are the outer loop: the walk meets (18, 3) before (2, 20))
    got, _ = _one_pair(c, q)
    assert got == (3, 2)


def test_zeros_of_both_signs_tie():
    """Zero rows of both signs against generic rows: every product is a zero and the pick is numpy's.  This does NOT tell a kernel
    with the key's -0 -> +0 step from one without it: the accumulators start at +0.0 and (+0) + (-0) = +0, so the kernel only ever
    forms +0.0 here and no input reaches a -0.0 product through this arithmetic.  The step is kept as the key's definition (a -0.0
    would otherwise rank below +0.0); what the test pins is the result on zero blocks, not that step."""
    rng = np.random.default_rng(4)
    q = np.where(rng.random((5, D)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    c = rng.standard_normal((19, D)).astype(np.float32)
    assert np.signbit(q).any() and not np.signbit(q).all()
    assert _numpy_pick(q, c)[0] == (0, 0)
    assert _one_pair(q, c)[0] == (0, 0) and _one_pair(c, q)[0] == (0, 0)
    # behind a row of negative products the first zero wins, whatever its sign
    q[0] = -np.abs(rng.standard_normal(D)).astype(np.float32)
    c = np.abs(c)
    pick, s = _numpy_pick(q, c)
    assert (s[0] < 0).all() and (s[1:] == 0).all() and pick == (1, 0)
    got, best = _one_pair(q, c)
    assert got == (1, 0) and best == 0.0


def test_all_minus_inf_gives_the_first_entry():
    q = np.zeros((18, D), np.float32)
    c = np.zeros((17, D), np.float32)
    q[:, 0] = np.inf               # one infinite coordinate of one sign per row, finite non-zero partners: no inf - inf, no inf x 0
    c[:, 0] = -np.arange(1, 18)
    pick, s = _numpy_pick(q, c)
    assert np.isneginf(s).all() and pick == (0, 0)
    got, best = _one_pair(q, c)
    assert got == (0, 0) and best == -np.inf
    # rows of -inf against positive candidates: the same block from the other sign
    got, best = _one_pair(-q, -c)
    assert got == (0, 0) and best == -np.inf


def test_the_first_nan_wins_over_a_larger_finite_entry_before_it():
    rng = np.random.default_rng(6)
    q = rng.standard_normal((23, D)).astype(np.float32)
    c = rng.standard_normal((19, D)).astype(np.float32)
    q[:, 5] = q[:, 6] = 0.0
    c[:, 5] = c[:, 6] = 1.0
    q[17, 5] = np.inf              # row 17: +inf everywhere but NaN (inf x 0) at candidate 1
    c[1, 5] = 0.0
    q[20, 6] = np.inf              # row 20: NaN at candidate 0
    c[0, 6] = 0.0
    q[3] = 50 * c[4]               # a large finite entry earlier in row-major order
    q[3, 5] = q[3, 6] = 0.0
    pick, s = _numpy_pick(q, c)
    assert np.isnan(s[17, 1]) and np.isnan(s[20, 0]) and np.isnan(s).sum() == 2 and s[3, 4] > 1000 and pick == (17, 1)
    got, best = _one_pair(q, c)
    assert got == (17, 1) and np.isnan(best)


def test_buffers_are_written_for_P_pairs_only_and_runs_repeat(runs):
    from aspire_amd import ops
    run = runs[1 + PS.index(5)]           # P = 5: two workgroups, the second with one live wave
    P = len(run.pairs)
    assert P == 5
    arg = torch.full((P + 3, 2), SENTINEL_ARG, dtype=torch.int32, device='cuda')
    best = torch.full((P + 3,), SENTINEL_BEST, dtype=torch.float32, device='cuda')
    ops.dot_argmax(run.q, run.c, out=(arg, best))
    arg, best = arg.cpu().numpy(), best.cpu().numpy()
    assert (arg[P:] == SENTINEL_ARG).all() and (best[P:] == SENTINEL_BEST).all()
    assert arg[:P].tobytes() == run.arg.tobytes() and best[:P].tobytes() == run.best.tobytes()      # the same bits as the first run
    assert (arg[:P] >= 0).all()
    # best = NULL
    only_arg, none = ops.dot_argmax(run.q, run.c, want_best=False)
    assert none is None and only_arg.cpu().numpy().tobytes() == run.arg.tobytes()


def test_a_document_longer_than_its_bound_is_poisoned():
    from aspire_amd import ops
    rng = np.random.default_rng(8)
    docs = _docs('normal', rng, (3, 6, 4, 2))
    rows, start, lens = _store(docs, rng)
    q = _view(rows, start, lens, [0, 1, 2], max_len=4)          # document 1 has 6 rows: beyond the bound the host gave
    c = _view(rows, start, lens, [3, 3, 1], max_len=6)
    arg, best = ops.dot_argmax(q, c)
    arg, best = arg.cpu().numpy(), best.cpu().numpy()
    assert arg[1].tolist() == [-1, -1] and np.isnan(best[1])
    for p, (a, b) in ((0, (0, 3)), (2, (2, 1))):
        assert tuple(arg[p].tolist()) == _numpy_pick(docs[a], docs[b])[0] and np.isfinite(best[p])


def test_torch_op(runs):
    import aspire_amd.torch_ops  # noqa: F401  (registers the operators)
    run = runs[1 + PS.index(4)]
    args = (run.q.rows, run.q.start, run.q.len, run.c.rows, run.c.start, run.c.len, run.q.max_len, run.c.max_len)
    torch.library.opcheck(torch.ops.aspire.dot_argmax, args, test_utils=('test_schema', 'test_faketensor'))
    arg, best = torch.ops.aspire.dot_argmax(*args)
    assert arg.dtype == torch.int32 and arg.cpu().numpy().tobytes() == run.arg.tobytes()
    assert best.cpu().numpy().tobytes() == run.best.tobytes()
