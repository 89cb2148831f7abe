"""GPU: the frame the one-wave-per-pair forward kernels share (aspire_amd/csrc/pair_fwd.h: dotmax_pair_kernel, jointsm_pair_kernel,
l2agg_pair_kernel) -- the pair index of the CROSS / PAIRED / MAPPED forms, the job lookup with empty jobs, the last workgroup's idle
wave, the tile walk over one-row documents, exact tile edges and one row past an edge, and the poisoned pair with its pair_softmax
block.  A pair's bits depend on its two documents only: every form and every call size must give the same ones.

Seven documents per side, rows Q_ROWS x C_ROWS (P = 7: two workgroups, the second with one idle wave), drawn as
tests/test_gpu_jointsm.py draws them.  References and bars are the kernels' own: test_gpu_dotmax_forms.py's float64 bars, test_gpu_jointsm.py's
SHORT_BAR / LONG_BAR / SM_BAR, test_gpu_l2agg_batch.py's TOL against float64 numpy.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from test_gpu_jointsm import LONG_BAR, SHORT_BAR, SM_BAR, OFFSET, D, _docs, _rel, _want, closed_form
from test_gpu_jointsm import _scores as _jsm_scores
from test_gpu_l2agg_batch import AGGS, TOL, _agg_id
from test_gpu_dotmax_forms import check_cos, check_dot, cos_refs, dot_refs
from test_gpu_sentenc import _f64_cos_max

pytestmark = pytest.mark.gpu

Q_ROWS = (1, 16, 17, 3, 33, 8, 2)
C_ROWS = (17, 1, 16, 33, 5, 2, 8)
JOB_OFF = (0, 0, 3, 3, 7, 7)            # five jobs: empty ones first, in the middle and last
JOB_OF = (1, 1, 1, 3, 3, 3, 3)          # the job of candidate p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope='module')
def docs():
    rng = np.random.RandomState(4483)
    off = OFFSET * rng.standard_normal(D)
    return _docs(rng, Q_ROWS, 0.6, off), _docs(rng, C_ROWS, 0.6, off)


def _csr(d):
    from aspire_amd import ops
    return ops.DeviceRepSet.from_list(d)


def _dot_want(x, y, cosine):
    return _f64_cos_max(x, y, dot=not cosine)


def _dot_ok(got, x, y, cosine):
    """test_gpu_dotmax_forms.py's own checks, both references of each (they raise where a bar is missed)"""
    (check_cos if cosine else check_dot)(got, *(cos_refs if cosine else dot_refs)(x, y))
    return True


def _forms(docs, paired_call, cross_call, batch_call, ok, want, name):
    """PAIRED over the seven pairs; each pair alone; CROSS 7 x 7 (a bound of 33: the pair kernel); the batched entry over JOB_OFF"""
    q_docs, c_docs = docs
    n = len(q_docs)
    paired = paired_call(q_docs, c_docs)
    assert paired.shape == (n,) and np.isfinite(paired).all()
    for p in range(n):
        alone = paired_call([q_docs[p]], [c_docs[p]])
        assert alone.shape == (1,) and _bits(alone)[0] == _bits(paired)[p], (name, 'alone', p)
    cross = cross_call(q_docs, c_docs).reshape(n, n)
    assert np.array_equal(_bits(cross.diagonal()), _bits(paired)), (name, 'cross diagonal')
    worst = 0.0
    for i in range(n):
        for j in range(n):
            w = want(q_docs[i], c_docs[j])
            worst = max(worst, abs(float(cross[i, j]) - w) / max(abs(w), 1.0))
            assert ok(float(cross[i, j]), w, q_docs[i], c_docs[j]), (name, i, j, cross[i, j], w)
    print(f'FRAME {name}: worst err of the 49 CROSS scores {worst:.3e} (relative to max(|score|, 1))')
    per_cand = paired_call([q_docs[j] for j in JOB_OF], c_docs)
    for k in (0, max(JOB_OFF[j + 1] - JOB_OFF[j] for j in range(5))):            # scores only; the full lists
        got = batch_call(q_docs[:5], c_docs, k)
        assert np.array_equal(_bits(got), _bits(per_cand)), (name, 'batched', k)


@pytest.mark.parametrize('sim', ['cosine', 'dot'])
def test_dotmax_forms_give_a_pair_the_same_bits(docs, sim):
    from aspire_amd import _lib, ops
    cosine = sim == 'cosine'
    sim_id = _lib.SIM_COSINE if cosine else _lib.SIM_DOT
    job_off = torch.tensor(JOB_OFF, dtype=torch.int32, device='cuda')
    _forms(docs,
           lambda q, c: ops.dotmax_scores(_csr(q), _csr(c), pairing=_lib.PAIR_PAIRED, sim=sim_id).cpu().numpy(),
           lambda q, c: ops.dotmax_scores(_csr(q), _csr(c), pairing=_lib.PAIR_CROSS, sim=sim_id).cpu().numpy(),
           lambda q, c, k: ops.dotmax_rank_batch(_csr(q), _csr(c), job_off, 4, k, sim=sim_id)[0].cpu().numpy(),
           lambda got, w, x, y: _dot_ok(got, x, y, cosine), lambda x, y: _dot_want(x, y, cosine), f'dotmax {sim}')


def test_jointsm_forms_give_a_pair_the_same_bits(docs):
    from aspire_amd import _lib, ops
    job_off = torch.tensor(JOB_OFF, dtype=torch.int32, device='cuda')

    def ok(got, w, x, y):
        return _rel(got, w) <= (SHORT_BAR if max(len(x), len(y)) <= 16 else LONG_BAR)

    _forms(docs,
           lambda q, c: _jsm_scores(_csr(q), _csr(c), _lib.PAIR_PAIRED)[0],
           lambda q, c: _jsm_scores(_csr(q), _csr(c), _lib.PAIR_CROSS)[0],
           lambda q, c, k: ops.jointsm_rank_batch(_csr(q), _csr(c), job_off, 4, k)[0].cpu().numpy(),
           ok, _want, 'jointsm')


def _l2agg_want(x, y, agg, temp):
    """float64 numpy on the fp32 inputs (test_gpu_l2agg_batch.py: test_shared_sentence_against_float64)"""
    d = np.sqrt(((x.astype(np.float64)[:, None, :] - y.astype(np.float64)[None, :, :]) ** 2).sum(-1))
    s = -d.ravel()
    if agg == 'top2':
        return float(np.sort(s)[-2:].sum())
    w = np.exp((s - s.max()) / temp)
    return float((w * s).sum() / w.sum())


@pytest.mark.parametrize('agg,temp', AGGS)
def test_l2agg_jobs_give_a_pair_the_same_bits(docs, agg, temp):
    from aspire_amd import ops
    q_docs, c_docs = docs
    assert all(len(q_docs[j]) * len(c) > 1 for j, c in zip(JOB_OF, c_docs))        # (no 1 x 1 pair: TOP2's -10e8 is not float64's)
    job_off = torch.tensor(JOB_OFF, dtype=torch.int32, device='cuda')
    one = torch.tensor([0, 1], dtype=torch.int32, device='cuda')
    got = ops.l2agg_rank_batch(_csr(q_docs[:5]), _csr(c_docs), job_off, 4, 0, _agg_id(agg), temp=temp)[0].cpu().numpy()
    assert got.shape == (7,) and np.isfinite(got).all()
    worst = 0.0
    for p, j in enumerate(JOB_OF):
        alone = ops.l2agg_rank_batch(_csr([q_docs[j]]), _csr([c_docs[p]]), one, 1, 0, _agg_id(agg), temp=temp)[0].cpu().numpy()
        assert alone.shape == (1,) and _bits(alone)[0] == _bits(got)[p], (agg, temp, p)
        worst = max(worst, abs(float(got[p]) - _l2agg_want(q_docs[j], c_docs[p], agg, temp)))
    print(f'FRAME l2agg {agg} temp={temp}: worst err {worst:.3e} (TOL {TOL:.0e})')
    assert worst <= TOL


def test_jointsm_pair_softmax_blocks_and_the_poisoned_pair():
    """padded sets with extents 20 x 18: a 1 x 1 pair, tile edges, the full extents, and a pair whose q.len = 21 exceeds the extent"""
    from aspire_amd import _lib, ops
    qext, cext = 20, 18
    lens = ((1, 1), (16, 17), (20, 18), (17, 3), (21, 5))
    rng = np.random.RandomState(2018)
    off = OFFSET * rng.standard_normal(D)
    q = (0.6 * rng.standard_normal((5, qext, D)) + off).astype(np.float32)
    c = (0.6 * rng.standard_normal((5, cext, D)) + off).astype(np.float32)
    qlens, clens = [a for a, _ in lens], [b for _, b in lens]
    qs = ops.DeviceRepSet.from_padded(torch.from_numpy(q), [min(n, qext) for n in qlens])
    cs = ops.DeviceRepSet.from_padded(torch.from_numpy(c), clens)
    qs.len.copy_(torch.tensor(qlens, dtype=torch.int32))
    got, sm = _jsm_scores(qs, cs, _lib.PAIR_PAIRED, soft=True)
    plain, _ = _jsm_scores(qs, cs, _lib.PAIR_PAIRED)
    assert sm.shape == (5, qext, cext)
    assert np.isnan(got[4]) and np.isnan(sm[4]).all() and np.isnan(plain[4])
    assert np.array_equal(_bits(got[:4]), _bits(plain[:4]))
    want, want_sm = closed_form(q[:4], c[:4], qlens[:4], clens[:4])
    for i in range(4):
        ql, cl = lens[i]
        assert np.all(_bits(sm[i, ql:, :]) == 0) and np.all(_bits(sm[i, :, cl:]) == 0), i          # exactly +0.0
        total = float(sm[i, :ql, :cl].astype(np.float64).sum())
        err_sm = float(np.abs(sm[i].astype(np.float64) - want_sm[i]).max())
        err = float(_rel(got[i], want[i]))
        print(f'SOFTMAX pair {i} ({ql} x {cl}): sum {total:.8f}, entries err {err_sm:.3e} (bar {SM_BAR:.3e}), score err {err:.3e}')
        assert abs(total - 1.0) <= 1e-5, (i, total)
        assert err_sm <= SM_BAR, (i, err_sm)
        assert err <= (SHORT_BAR if max(ql, cl) <= 16 else LONG_BAR), (i, err)
