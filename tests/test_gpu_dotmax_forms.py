"""Every form of the dot-product max-sim kernels (aspire_amd/csrc/dotmax.hip): every pair of row-slot widths of
dotmax_cross_kernel (documents padded to 1, 2, 4, 8 or 16 slots on either side, each width with its own reduction and its own
set of writing lanes), both similarities, both layouts, dotmax_pair_kernel on the same pairs, the batched call with the raw
dot, with documents of 33..128 rows and with empty jobs, the NaN of a document longer than the host bound, and rep sets whose
CSR `start` is an index list into a shared row matrix.

References and bars are those of tests/test_gpu_sentenc.py: sklearn's float32 cosine_similarity + np.max (SK_TOL), float64
numpy (F64_TOL); for the raw dot numpy's float32 matmul and float64, at the two bounds of test_dot_form_matches_matmul.  Every
pair of every case is checked; none is left out (the references agree with each other within the bars for these seeds)."""
import ctypes

import numpy as np
import pytest
import torch
from sklearn.metrics.pairwise import cosine_similarity

from test_gpu_sentenc import SK_TOL, F64_TOL, _f64_cos_max, _rows

pytestmark = pytest.mark.gpu

BOUNDS = (1, 2, 3, 4, 5, 8, 9, 16)
# documents per side by bound: Q * Wq is not a multiple of 16 wherever Wq < 16 allows it, C * Wc never a multiple of 32;
# bound 5 (8 slots) x 17 queries = 8.5 chunks of 16 slots and bound 16 x 9 queries = 9 chunks: a wave takes a third chunk, and the
# last chunk of the first lies partly beyond Q
N_QUERIES = {1: 21, 2: 11, 3: 7, 4: 7, 5: 17, 8: 5, 9: 3, 16: 9}
N_CANDS = {1: 45, 2: 37, 3: 19, 4: 19, 5: 13, 8: 13, 9: 7, 16: 5}


def _slots(b):
    w = 1
    while w < b:
        w *= 2
    return w


for _b in BOUNDS:          # the geometry the comment above promises (checked wherever this module is imported, no GPU needed)
    assert (N_QUERIES[_b] * _slots(_b)) % 16 != 0 or _slots(_b) == 16
    assert (N_CANDS[_b] * _slots(_b)) % 32 != 0
assert N_QUERIES[5] * _slots(5) > 128 and (N_QUERIES[5] * _slots(5)) % 16 != 0 and N_QUERIES[16] * 16 > 128


def sweep_kind(bq, bc):
    return 'aniso' if (BOUNDS.index(bq) + BOUNDS.index(bc)) % 2 else 'normal'


def sweep_docs(bq, bc, kind):
    """Q query and C candidate documents with lengths from 1..bound, at least one of exactly the bound on each side; the
    lengths depend on the bounds alone, the values on `kind` too: 'normal', 'aniso' (tests/test_gpu_sentenc.py: _rows) or
    'signed' = 'aniso' with every other query document negated (CPU only)"""
    rng = np.random.default_rng(1000 + 17 * bq + bc)
    ql = rng.integers(1, bq + 1, N_QUERIES[bq])
    cl = rng.integers(1, bc + 1, N_CANDS[bc])
    ql[int(rng.integers(0, len(ql)))] = bq
    ql[-1] = bq                                           # ... and the last query, whose chunk may end beyond Q
    cl[int(rng.integers(0, len(cl)))] = bc
    rng = np.random.default_rng(5000 + 17 * bq + bc + (0 if kind == 'normal' else 500))
    rows_kind = 'normal' if kind == 'normal' else 'aniso'
    q_docs, c_docs = [_rows(rng, int(n), rows_kind) for n in ql], [_rows(rng, int(n), rows_kind) for n in cl]
    if kind == 'signed':                                  # every other query negated: all its dots are ~ -6900, a masked slot
        q_docs = [-x if i % 2 else x for i, x in enumerate(q_docs)]      # that leaked 0 into the max would win
    return q_docs, c_docs


def cos_refs(x, y):
    """(sklearn float32, float64) max cosine of one pair"""
    return float(np.max(cosine_similarity(x, y))), _f64_cos_max(x, y)


def dot_refs(x, y):
    """(numpy float32 matmul, float64) max dot of one pair"""
    return float(np.matmul(x, y.T).max()), float(np.matmul(x.astype(np.float64), y.T.astype(np.float64)).max())


def check_cos(got, want_sk, want_64, where=None):
    assert abs(got - want_sk) <= SK_TOL, (where, got, want_sk)
    assert abs(got - want_64) <= F64_TOL, (where, got, want_64)


def check_dot(got, want, want64, where=None):
    assert abs(got - want) <= 1e-6 * max(1.0, abs(want64)) * 4, (where, got, want)
    assert abs(got - want64) <= 1e-6 * abs(want64) + 1e-5, (where, got, want64)


_REFS = {}


def _sweep_refs(bq, bc, sim):
    """[Q, C, 2] reference values: the cosine on rows of sweep_kind (isotropic rows, and for every other pair of bounds a
    sentence-embedding-like space with a mean cosine of ~0.9), the raw dot on the latter only, half of the queries negated (dots
    of ~ +6900 and ~ -6900) -- the bounds of the raw dot scale with the result, and between isotropic rows it is a small
    remainder of large terms, on which numpy's own float32 matmul is up to 7 x the float32 bound away from float64: no kernel
    could meet both references there"""
    if (bq, bc, sim) not in _REFS:
        q_docs, c_docs = sweep_docs(bq, bc, sweep_kind(bq, bc) if sim == 'cosine' else 'signed')
        refs = cos_refs if sim == 'cosine' else dot_refs
        _REFS[bq, bc, sim] = np.array([[refs(x, y) for y in c_docs] for x in q_docs])
    return _REFS[bq, bc, sim]


def _repset(docs, layout, ext=None):
    from aspire_amd import ops
    if layout == 'csr':
        return ops.DeviceRepSet.from_list(docs)
    s = ext if ext is not None else max(len(d) for d in docs)
    pad = np.full((len(docs), s, 768), 1e3, np.float32)                # padding rows must not be read
    for i, d in enumerate(docs):
        pad[i, :len(d)] = d
    return ops.DeviceRepSet.from_padded(torch.from_numpy(pad), [len(d) for d in docs])


def _scores(q, c, pairing, sim):
    from aspire_amd import ops
    return ops.dotmax_scores(q, c, pairing=pairing, sim=sim).cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('layout', ['csr', 'padded'])
@pytest.mark.parametrize('bc', BOUNDS)
@pytest.mark.parametrize('bq', BOUNDS)
def test_cross_widths_both_similarities_and_the_pair_kernel(bq, bc, layout):
    from aspire_amd import _lib
    for sim, sim_id, check in (('cosine', _lib.SIM_COSINE, check_cos), ('dot', _lib.SIM_DOT, check_dot)):
        q_docs, c_docs = sweep_docs(bq, bc, sweep_kind(bq, bc) if sim == 'cosine' else 'signed')
        assert max(len(d) for d in q_docs) == bq and max(len(d) for d in c_docs) == bc
        Q, C = len(q_docs), len(c_docs)
        refs = _sweep_refs(bq, bc, sim)
        q, c = _repset(q_docs, layout), _repset(c_docs, layout)
        assert (q.ext if layout == 'padded' else q.max_len) == bq and (c.ext if layout == 'padded' else c.max_len) == bc
        cross = _scores(q, c, _lib.PAIR_CROSS, sim_id).reshape(Q, C)
        assert np.isfinite(cross).all()
        for qi in range(Q):
            for ci in range(C):
                check(float(cross[qi, ci]), refs[qi, ci, 0], refs[qi, ci, 1], (sim, qi, ci, len(q_docs[qi]), len(c_docs[ci])))
        # the same pairs one wave each (dotmax_pair_kernel), pair p = (p // C, p % C): the same bits
        pq = _repset([q_docs[p // C] for p in range(Q * C)], layout)
        pc = _repset([c_docs[p % C] for p in range(Q * C)], layout)
        paired = _scores(pq, pc, _lib.PAIR_PAIRED, sim_id)
        assert np.array_equal(_bits(paired), _bits(cross.reshape(-1))), sim


@pytest.mark.parametrize('bc', BOUNDS)
@pytest.mark.parametrize('bq', BOUNDS)
def test_appending_a_longer_document_moves_no_other_score(bq, bc):
    """one more document of another width (and one of 17 rows: the whole call moves to dotmax_pair_kernel) on either side:
    every other pair keeps its bits"""
    from aspire_amd import _lib
    q_docs, c_docs = sweep_docs(bq, bc, sweep_kind(bq, bc))
    Q, C = len(q_docs), len(c_docs)
    rng = np.random.default_rng(5)
    q, c = _repset(q_docs, 'csr'), _repset(c_docs, 'csr')
    for sim in (_lib.SIM_COSINE, _lib.SIM_DOT):
        base = _scores(q, c, _lib.PAIR_CROSS, sim).reshape(Q, C)
        for side, b in (('q', bq), ('c', bc)):
            longer = ([2 * _slots(b)] if _slots(b) < 16 else []) + [17]      # the next width's bound; beyond the cross kernel
            for rows in longer:
                extra = _rows(rng, rows, 'normal')
                if side == 'q':
                    got = _scores(_repset(q_docs + [extra], 'csr'), c, _lib.PAIR_CROSS, sim).reshape(Q + 1, C)[:Q]
                else:
                    got = _scores(q, _repset(c_docs + [extra], 'csr'), _lib.PAIR_CROSS, sim).reshape(Q, C + 1)[:, :C]
                assert np.array_equal(_bits(got), _bits(base)), (sim, side, rows)


def _job_data(sizes, seed, q_rows, bank_rows, n_bank, sim):
    """queries, a bank of documents and every job's pool as indices into it; for the cosine isotropic and anisotropic rows
    mixed, for the raw dot anisotropic rows only, every other query negated (see _sweep_refs)"""
    rng = np.random.default_rng(seed)
    mixed = sim == 'cosine'
    queries = [_rows(rng, int(n), 'normal' if mixed and j % 2 == 0 else 'aniso') for j, n in enumerate(q_rows)]
    if not mixed:
        queries = [-x if j % 2 else x for j, x in enumerate(queries)]      # negative dots too (see sweep_docs, 'signed')
    bank = [_rows(rng, int(n), 'normal' if mixed and i % 3 == 0 else 'aniso') for i, n in enumerate(rng.choice(bank_rows, n_bank))]
    pools = []
    for n in sizes:
        idx = [int(i) for i in rng.integers(0, len(bank), n)]
        if n >= 7:
            idx[3] = idx[1]                                # a duplicated candidate: equal scores, pool order kept
        pools.append(idx)
    return queries, bank, pools


def _rank_batch(queries, flat, sizes, k, sim):
    from aspire_amd import ops
    from test_gpu_rank_tail import _check_lists
    q, c = ops.DeviceRepSet.from_list(queries), ops.DeviceRepSet.from_list(flat)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    job_off = torch.from_numpy(off.astype(np.int32)).cuda()
    scores, top_s, top_i = (t.cpu().numpy() for t in ops.dotmax_rank_batch(q, c, job_off, max(sizes), k, sim=sim))
    _check_lists(sizes, off, scores, top_s, top_i, k, np.zeros(len(sizes), np.int64))
    return scores, off


@pytest.mark.parametrize('sim', ['cosine', 'dot'])
@pytest.mark.parametrize('rows', ['short', 'long'])
def test_rank_batch_raw_dot_and_long_documents(sim, rows):
    """aspire_dotmax_rank_batch_f32 with ASPIRE_SIM_DOT, and with documents of 33..128 rows on both sides: every candidate's
    score against both references, every list the stable descending sort of its job's scores"""
    from aspire_amd import _lib
    sizes = [1, 7, 300, 0, 64, 3]
    if rows == 'short':
        q_rows, bank_rows = [1, 19, 8, 4, 16, 2], np.arange(1, 33)
    else:
        q_rows, bank_rows = [33, 128, 1, 77, 64, 100], np.concatenate([np.arange(33, 129), [1, 16, 128, 33]])
    queries, bank, pools = _job_data(sizes, 21 if rows == 'short' else 22, q_rows, bank_rows, 90, sim)
    flat = [bank[i] for p in pools for i in p]
    sim_id, refs, check = (_lib.SIM_COSINE, cos_refs, check_cos) if sim == 'cosine' else (_lib.SIM_DOT, dot_refs, check_dot)
    scores, off = _rank_batch(queries, flat, sizes, 50, sim_id)
    assert np.isfinite(scores).all()
    for j, p in enumerate(pools):
        mine = scores[off[j]:off[j + 1]]
        for t, i in enumerate(p):
            check(float(mine[t]), *refs(queries[j], bank[i]), where=(j, t))
        if len(p) >= 7:
            assert mine[3] == mine[1]


@pytest.mark.parametrize('sim', ['cosine', 'dot'])
def test_rank_batch_with_empty_jobs(sim):
    """empty jobs in front, in a row, in the middle and at the end: candidate p is scored against the query of the job that
    job_off puts it in -- the PAIRED score of that pair, bit for bit (both are dotmax_pair_kernel)"""
    from aspire_amd import _lib, ops
    sim_id = _lib.SIM_COSINE if sim == 'cosine' else _lib.SIM_DOT
    sizes = [0, 0, 5, 0, 1, 700, 0]
    queries, bank, pools = _job_data(sizes, 31, [3, 9, 5, 12, 1, 8, 6], np.arange(1, 21), 200, sim)
    flat = [bank[i] for p in pools for i in p]
    scores, off = _rank_batch(queries, flat, sizes, 10, sim_id)
    job_of = np.repeat(np.arange(len(sizes)), sizes)                  # the host's answer: [2] * 5 + [4] + [5] * 700
    assert len(job_of) == len(flat) and job_of[0] == 2 and job_of[5] == 4 and job_of[6] == 5 and job_of[-1] == 5
    pq = ops.DeviceRepSet.from_list([queries[j] for j in job_of])
    paired = _scores(pq, ops.DeviceRepSet.from_list(flat), _lib.PAIR_PAIRED, sim_id)
    assert np.array_equal(_bits(scores), _bits(paired))
    # (the queries differ in every row, so a candidate scored against a neighbouring job's query cannot pass)
    other = _scores(ops.DeviceRepSet.from_list([queries[j - 1] for j in job_of]), ops.DeviceRepSet.from_list(flat), _lib.PAIR_PAIRED, sim_id)
    assert (other != paired).mean() > 0.99


def _scores_with_bounds(q, c, pairing, sim, q_max_len=None, c_max_len=None):
    """aspire_dotmax_scores_f32 through ctypes with the rep sets' host bound (max_len) overridden on the structs"""
    from aspire_amd import _lib, ops
    qs, cs = q.struct(), c.struct()
    if q_max_len is not None:
        qs.max_len = q_max_len
    if c_max_len is not None:
        cs.max_len = c_max_len
    n = q.n if pairing == _lib.PAIR_PAIRED else q.n * c.n
    out = torch.full((n,), 7.0, device='cuda', dtype=torch.float32)
    _lib.check(_lib.lib.aspire_dotmax_scores_f32(ctypes.byref(qs), ctypes.byref(cs), ops.D, pairing, sim, ops._ptr(out), ops._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('sim', ['cosine', 'dot'])
@pytest.mark.parametrize('longest', [2, 3, 8, 9, 13, 16, 17, 40, 128])
def test_a_document_longer_than_the_host_bound_scores_nan(longest, sim):
    """include/aspire_hip.h, aspire_repset.max_len: "A document longer than the bound yields a NaN score".  One document per
    side has `longest` rows, max_len says longest - 1 (a power of two and not: the cross kernel's row slots end beyond a bound
    of 7, 12 or 15): CROSS (dotmax_cross_kernel up to 16 rows, dotmax_pair_kernel beyond) and PAIRED (dotmax_pair_kernel); that
    document's pairs are NaN, every other pair has the bits of the call with the true bound"""
    from aspire_amd import _lib, ops
    sim_id = _lib.SIM_COSINE if sim == 'cosine' else _lib.SIM_DOT
    rng = np.random.default_rng(longest)
    lens = [int(n) for n in rng.integers(1, longest, 11)]             # 1 .. longest - 1
    q_docs = [_rows(rng, n, 'normal') for n in lens]
    c_docs = [_rows(rng, n, 'aniso') for n in lens[::-1]]
    q_docs[4] = _rows(rng, longest, 'normal')
    c_docs[9] = _rows(rng, longest, 'aniso')
    q_docs[0] = _rows(rng, longest - 1, 'normal')                     # a document of exactly the bound is not too long
    c_docs[0] = _rows(rng, longest - 1, 'aniso')
    q, c = ops.DeviceRepSet.from_list(q_docs), ops.DeviceRepSet.from_list(c_docs)
    n = len(q_docs)
    for pairing, shape, q_bad, c_bad in ((_lib.PAIR_CROSS, (n, n), np.s_[4, :], np.s_[:, 9]), (_lib.PAIR_PAIRED, (n,), np.s_[4], np.s_[9])):
        true = _scores_with_bounds(q, c, pairing, sim_id).reshape(shape)
        assert np.isfinite(true).all() and (true != 7.0).all()            # every pair written over the pre-fill
        for qb, cb in ((longest - 1, None), (None, longest - 1), (longest - 1, longest - 1)):
            got = _scores_with_bounds(q, c, pairing, sim_id, qb, cb).reshape(shape)
            bad = np.zeros(shape, bool)
            if qb is not None:
                bad[q_bad] = True
            if cb is not None:
                bad[c_bad] = True
            assert np.isnan(got[bad]).all(), (pairing, qb, cb, got[bad])
            assert np.array_equal(_bits(got[~bad]), _bits(true[~bad])), (pairing, qb, cb)


@pytest.mark.parametrize('sim', ['cosine', 'dot'])
@pytest.mark.parametrize('max_rows', [4, 16, 50])
def test_csr_start_as_an_index_list_into_shared_rows(max_rows, sim):
    """a pool as an index list into one row matrix: `start` neither ascending nor disjoint (documents in any order, two that
    share rows, one that is a prefix of another) -- the scores of the copied-out documents, bit for bit, from both kernels"""
    from aspire_amd import _lib, ops
    sim_id = _lib.SIM_COSINE if sim == 'cosine' else _lib.SIM_DOT
    rng = np.random.default_rng(40 + max_rows)
    rows = _rows(rng, 400, 'aniso')
    n = 23
    lens = rng.integers(1, max_rows + 1, n)
    lens[2] = lens[7] = max_rows
    start = rng.integers(0, 400 - max_rows, n)                        # any order, overlaps by chance ...
    start[7] = start[2] + max_rows // 2                               # ... and by construction: the second half of 2 opens 7
    start[11], lens[11] = start[2], max(1, max_rows // 2)             # a prefix of document 2
    start[12], lens[12] = start[5], lens[5]                           # the same document twice
    assert (np.diff(start) < 0).any() and start.max() + max_rows <= 400
    dev_rows = torch.from_numpy(rows).cuda()

    def shared(order):
        return ops.DeviceRepSet(dev_rows, torch.from_numpy(start[order].astype(np.int32)).cuda(),
                                torch.from_numpy(lens[order].astype(np.int32)).cuda(), 0, max_rows, lens_host=lens[order].tolist())

    def copied(order):
        return ops.DeviceRepSet.from_list([rows[start[i]:start[i] + lens[i]].copy() for i in order])

    qo, co = np.arange(n)[::-1][:9].copy(), np.arange(n)
    cross_shared = _scores(shared(qo), shared(co), _lib.PAIR_CROSS, sim_id)
    cross_copied = _scores(copied(qo), copied(co), _lib.PAIR_CROSS, sim_id)
    assert np.isfinite(cross_copied).all() and np.array_equal(_bits(cross_shared), _bits(cross_copied))
    po = rng.permutation(n)
    pair_shared = _scores(shared(po), shared(co), _lib.PAIR_PAIRED, sim_id)
    pair_copied = _scores(copied(po), copied(co), _lib.PAIR_PAIRED, sim_id)
    assert np.array_equal(_bits(pair_shared), _bits(pair_copied))
