"""GPU: the batched score + rank entry of the sibling aggregations 'l2top2' / 'l2attention' (aspire_amd/csrc/l2agg_pair.hip,
aspire_l2agg_rank_batch_f32) -- parity with the oracle per pair on tile boundaries, the rank contract, one kernel form at every call
size, the SHARED SENTENCES rule against float64, the public layer (rank_pools, InFlightRanker, evaluate.score) and the host bound.

The bar.  TOL = 1e-4 absolute: the bar tests/test_gpu_siblings.py holds these two aggregations to against the same oracle.  Rows are
torch.randn in 768-d with fixed seeds (distances of about 39; at temp = 0.2 the soft-max is sharp but finite).  Every figure is
printed before it is asserted (run with -s to see them)."""
import json

import numpy as np
import pytest
import torch

from oracle import aspire_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-4
D = 768
AGGS = (('top2', 1.0), ('att', 1.0), ('att', 0.2))          # (aggregation, temp)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _agg_id(agg):
    from aspire_amd import _lib
    return _lib.AGG_TOP2 if agg == 'top2' else _lib.AGG_ATTENTION


def _oracle(x, y, agg, temp):
    """the reference's own function restated (oracle/), one un-padded B = 1 pair, negated to the similarity"""
    qt, ct = orc.RepLen(x[None].permute(0, 2, 1), [len(x)]), orc.RepLen(y[None].permute(0, 2, 1), [len(y)])
    if agg == 'top2':
        return -orc.allpair_masked_dist_l2topk(qt, ct).item()
    return -orc.AllPairMaskedAttention({'cdatt_sm_temp': temp}).compute_distance(qt, ct).item()


def _call(queries, pools, agg, temp=1.0, k=None, **kw):
    """ops.l2agg_rank_batch on J (query, pool) jobs; k None: the largest pool"""
    from aspire_amd import ops
    sizes = [len(p) for p in pools]
    q = ops.DeviceRepSet.from_list(queries)
    c = ops.DeviceRepSet.from_list([d for p in pools for d in p])
    job_off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device='cuda')
    out = ops.l2agg_rank_batch(q, c, job_off, max(sizes), max(sizes) if k is None else k, _agg_id(agg), temp=temp, **kw)
    torch.cuda.synchronize()
    return out


# ---- cases 1 and 2 share one set of jobs ---------------------------------------------------------------------------------------
Q_LENS = (1, 8, 17, 128)
POOL_LENS = ((1, 2, 15, 16, 17, 32, 33), (), (128, 16, 1, 33, 16), (128, 17, 2, 15, 32, 1))      # 7 + 0 + 5 + 6 = 18 candidates
DUP = (2, 1, 4)          # pool 2: candidate 4 IS candidate 1


@pytest.fixture(scope='module')
def boundary_jobs():
    assert {n for p in POOL_LENS for n in p} == {1, 2, 15, 16, 17, 32, 33, 128} and sum(len(p) for p in POOL_LENS) % 4 != 0
    g = torch.Generator().manual_seed(1729)
    queries = [torch.randn(n, D, generator=g) for n in Q_LENS]
    pools = [[torch.randn(n, D, generator=g) for n in lens] for lens in POOL_LENS]
    pools[DUP[0]][DUP[2]] = pools[DUP[0]][DUP[1]]
    want = {}
    for agg, temp in AGGS:
        want[agg, temp] = [[None if (agg == 'top2' and len(x) * len(y) == 1) else _oracle(x, y, agg, temp) for y in pool]
                           for x, pool in zip(queries, pools)]
    got = {(agg, temp): tuple(t.cpu().numpy() for t in _call(queries, pools, agg, temp)) for agg, temp in AGGS}
    return queries, pools, want, got


@pytest.mark.parametrize('agg,temp', AGGS)
def test_parity_on_tile_boundaries(boundary_jobs, agg, temp):
    """queries of 1, 8, 17, 128 rows against pools of 7, 0, 5, 6 candidates of 1 .. 128 rows (18 pairs: not a multiple of the four
    waves of a workgroup): every pair within TOL of the oracle; a 1 x 1 pair under TOP2, where the oracle's topk raises, is the
    documented -d - 10e8 that aspire_l2agg_scores_f32 gives (one ulp there is 64: rtol 1e-7)"""
    from aspire_amd import _lib, ops
    queries, pools, want, got = boundary_jobs
    scores = got[agg, temp][0]
    flat = [(j, i) for j, pool in enumerate(pools) for i in range(len(pool))]
    assert scores.shape == (len(flat),) and np.isfinite(scores).all()
    worst, n_single = 0.0, 0
    for p, (j, i) in enumerate(flat):
        w = want[agg, temp][j][i]
        if w is None:
            single = ops.l2agg_scores(ops.DeviceRepSet.from_list([queries[j]]), ops.DeviceRepSet.from_list([pools[j][i]]), _lib.AGG_TOP2,
                                      pairing=_lib.PAIR_PAIRED).cpu().numpy()
            print(f'1x1 top2: batched {scores[p]!r} paired entry {single[0]!r}')
            np.testing.assert_allclose(scores[p], single[0], rtol=1e-7, atol=0)
            assert scores[p] < -9.9e8
            n_single += 1
            continue
        err = abs(float(scores[p]) - w)
        print(f'{agg} temp={temp} job {j} ({len(queries[j])} rows) cand {i} ({len(pools[j][i])} rows): got {scores[p]:.6f} want {w:.6f} err {err:.2e}')
        worst = max(worst, err)
    print(f'PARITY {agg} temp={temp}: worst err {worst:.3e} (TOL {TOL:.0e})')
    assert n_single == (1 if agg == 'top2' else 0)
    assert worst <= TOL


def _check_lists(scores, ts, ti, sizes, k, base=None):
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert ts.shape == ti.shape == (len(sizes), k)
    for j, n in enumerate(sizes):
        seg = scores[off[j]:off[j + 1]].tolist()
        order = sorted(range(n), key=lambda i: seg[i], reverse=True)[:k]          # Python's stable sort: ties in pool order
        assert ti[j, :len(order)].tolist() == [i + (int(base[j]) if base is not None else 0) for i in order], j
        assert np.array_equal(_bits(ts[j, :len(order)]), _bits(np.array([seg[i] for i in order], np.float32))), j
        assert (ti[j, len(order):] == -1).all() and np.isneginf(ts[j, len(order):]).all(), j


@pytest.mark.parametrize('agg,temp', AGGS)
def test_rank_contract(boundary_jobs, agg, temp):
    """per job the stable descending sort of its slice of `scores` (the bits, ties in pool order, index = position in the pool,
    (-inf, -1) beyond the pool's size, the empty pool's row all padding); a document that sits twice in a pool scores the same bits
    and ranks in pool order; the key form + job_base decodes to the same lists; k = 0 returns scores only"""
    from aspire_amd import ops
    queries, pools, _, got = boundary_jobs
    sizes = [len(p) for p in pools]
    scores, ts, ti = got[agg, temp]
    k = max(sizes)
    assert k == 7
    _check_lists(scores, ts, ti, sizes, k)
    assert (ti[1] == -1).all() and np.isneginf(ts[1]).all()
    off = np.concatenate([[0], np.cumsum(sizes)])
    a, b = off[DUP[0]] + DUP[1], off[DUP[0]] + DUP[2]
    assert _bits(scores[a:a + 1])[0] == _bits(scores[b:b + 1])[0]
    row = ti[DUP[0]].tolist()
    assert row.index(DUP[1]) + 1 == row.index(DUP[2])
    # keys + job_base
    base = np.array([(j + 1) * 100003 for j in range(len(sizes))], dtype=np.int32)
    s2, keys = _call(queries, pools, agg, temp, key_form=True, job_base=torch.from_numpy(base).cuda())
    assert np.array_equal(_bits(s2.cpu().numpy()), _bits(scores))
    keys_np = keys.cpu().numpy()
    for j, n in enumerate(sizes):
        idx = 0xFFFFFFFF - (keys_np[j, :n].astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)      # the low word is ~(global index)
        assert np.array_equal(idx, ti[j, :n] + base[j]), j
        assert (keys_np[j, n:] == 0).all(), j
    m_s, m_i = ops.topk_merge_keys(keys.view(1, len(sizes), k).contiguous(), k)
    _check_lists(scores, m_s.cpu().numpy().reshape(len(sizes), k), m_i.cpu().numpy().reshape(len(sizes), k), sizes, k, base)
    # a k below the pools' sizes, and k = 0
    _, ts3, ti3 = _call(queries, pools, agg, temp, k=3)
    _check_lists(scores, ts3.cpu().numpy(), ti3.cpu().numpy(), sizes, 3)
    s0, none_s, none_i = _call(queries, pools, agg, temp, k=0)
    assert none_s is None and none_i is None and np.array_equal(_bits(s0.cpu().numpy()), _bits(scores))


# ---- case 3 ----------------------------------------------------------------------------------------------------------------------
def test_one_form_whatever_the_size_of_the_call():
    """the same (query, candidate) pair in a call of one job with one candidate and in a call of 40 jobs (pools of 1 .. 9 short
    documents, about 200 pairs): the same bits, both aggregations"""
    g = torch.Generator().manual_seed(40)
    sizes = [1 + (7 * j) % 9 for j in range(40)]
    queries = [torch.randn(int(n), D, generator=g) for n in torch.randint(1, 9, (40,), generator=g)]
    pools = [[torch.randn(int(n), D, generator=g) for n in torch.randint(1, 9, (size,), generator=g)] for size in sizes]
    assert 180 <= sum(sizes) <= 220
    off = np.concatenate([[0], np.cumsum(sizes)])
    for agg, temp in AGGS:
        big = _call(queries, pools, agg, temp)[0].cpu().numpy()
        for j, i in ((5, 0), (0, sizes[0] - 1), (13, sizes[13] - 1), (26, sizes[26] - 1), (39, sizes[39] - 1)):
            alone = _call([queries[j]], [[pools[j][i]]], agg, temp)[0].cpu().numpy()
            assert alone.shape == (1,)
            if not (agg == 'top2' and len(queries[j]) * len(pools[j][i]) == 1):
                assert abs(float(alone[0]) - _oracle(queries[j], pools[j][i], agg, temp)) <= TOL
            assert _bits(alone)[0] == _bits(big[off[j] + i:off[j] + i + 1])[0], (agg, temp, j, i)


# ---- case 4 ----------------------------------------------------------------------------------------------------------------------
def test_shared_sentence_against_float64():
    """a candidate that holds one of its query's rows exactly and another at 1e-3 relative perturbation: the expansion
    |q|^2 + |c|^2 - 2 q.c cancels there and the fp32 reference returns the square root of rounding noise (include/aspire_hip.h, SHARED
    SENTENCES), so the expectation is float64 numpy on the fp32 inputs -- the pattern of tests/test_gpu_coincident.py"""
    g = torch.Generator().manual_seed(77)
    worst = 0.0
    for q_rows, c_rows in ((6, 4), (20, 33)):
        query, cand = torch.randn(q_rows, D, generator=g), torch.randn(c_rows, D, generator=g)
        cand[1] = query[2]
        cand[c_rows - 1] = query[4] * (1.0 + 1e-3 * torch.randn(D, generator=g))
        d = np.sqrt(((query.numpy().astype(np.float64)[:, None, :] - cand.numpy().astype(np.float64)[None, :, :]) ** 2).sum(-1))
        assert d[2, 1] == 0.0 and 0.01 < d[4, c_rows - 1] < 0.1 and np.sort(d.ravel())[2] > 30
        s = -d.ravel()
        for agg, temp in AGGS:
            if agg == 'top2':
                want = float(np.sort(s)[-2:].sum())
            else:
                w = np.exp((s - s.max()) / temp)
                want = float((w * s).sum() / w.sum())
            got = float(_call([query], [[cand]], agg, temp)[0].cpu().numpy()[0])
            print(f'SHARED {q_rows}x{c_rows} {agg} temp={temp}: got {got:.6e} want {want:.6e} err {abs(got - want):.2e}')
            worst = max(worst, abs(got - want))
    print(f'SHARED worst err {worst:.3e} (TOL {TOL:.0e})')
    assert worst <= TOL


# ---- case 5 ----------------------------------------------------------------------------------------------------------------------
PUBLIC = (('l2top2', 'top2', None), ('l2attention', 'att', {'cdatt_sm_temp': 0.5}))


def _well_separated(want):
    s = sorted(want, reverse=True)
    return all(a - b > 2 * TOL for a, b in zip(s[:-1], s[1:]))


@pytest.fixture(scope='module')
def public_jobs():
    g = torch.Generator().manual_seed(5)
    queries = [torch.randn(int(n), D, generator=g) for n in (2, 20, 7, 16, 11)]
    sizes = (3, 12, 5, 9, 8)
    pools = [[torch.randn(int(n), D, generator=g) for n in torch.randint(1, 21, (size,), generator=g)] for size in sizes]
    want = {method: [[_oracle(x, y, agg, (hp or {}).get('cdatt_sm_temp', 1.0)) for y in pool] for x, pool in zip(queries, pools)]
            for method, agg, hp in PUBLIC}
    return queries, pools, want


@pytest.mark.parametrize('method,agg,hparams', PUBLIC)
def test_rank_pools_and_in_flight_ranker(public_jobs, method, agg, hparams):
    """scorer.rank_pools on 5 queries with pools of 3 .. 12 documents of 1 .. 20 rows: the oracle's per-pair values, sorted (the seed
    keeps neighbouring oracle scores more than 2 TOL apart, asserted here); InFlightRanker returns the same lists; deterministic=True
    is refused as rank_pool refuses it"""
    from aspire_amd import scorer
    queries, pools, want = public_jobs
    assert all(_well_separated(w) for w in want[method])
    cpools = [scorer.CandidatePool(p, [f'd{j}_{i}' for i in range(len(p))]) for j, p in enumerate(pools)]
    ranked = scorer.rank_pools(queries, cpools, method=method, hparams=hparams)
    worst = 0.0
    for j, (r, w) in enumerate(zip(ranked, want[method])):
        order = orc.rank_descending(w)
        assert [pid for pid, _ in r] == [f'd{j}_{i}' for i in order], j
        worst = max(worst, max(abs(s - w[i]) for (_, s), i in zip(r, order)))
    print(f'PUBLIC {method}: worst err {worst:.3e} (TOL {TOL:.0e})')
    assert worst <= TOL
    ranker = scorer.InFlightRanker(method=method, hparams=hparams)
    tickets = [ranker.submit(queries, cpools), ranker.submit(queries[:2], cpools[:2])]
    assert ranker.result(tickets[0]) == ranked and ranker.result(tickets[1]) == ranked[:2]
    top3 = scorer.rank_pools(queries, cpools, k=3, method=method, hparams=hparams)
    assert top3 == [r[:3] for r in ranked]
    with pytest.raises(ValueError, match="deterministic=True is built for method 'ot'"):
        scorer.rank_pools(queries, cpools, method=method, hparams=hparams, deterministic=True)


def test_evaluate_score_takes_the_batched_branch(tmp_path):
    """evaluate.score(method='l2attention') on a small RepStore, resident and not, with queries_per_call 32 (the batched branch, new
    with this entry) and 1 (one rank_pool per query, as before): the written scores agree within TOL with the oracle and with each
    other, and the pid order is the oracle's (its neighbouring scores are more than 2 TOL apart, asserted)"""
    from aspire_amd import evaluate
    from aspire_amd.repstore import RepStore
    g = torch.Generator().manual_seed(21)
    pids = [f'p{i}' for i in range(24)]
    reps = {p: torch.randn(int(n), D, generator=g) for p, n in zip(pids, torch.randint(1, 15, (24,), generator=g))}
    store = RepStore({p: r.numpy() for p, r in reps.items()})
    test_pool = {'p0': {'cands': pids[4:13]}, 'p1': {'cands': pids[8:24]}, 'p2': {'cands': []}, 'p3': {'cands': pids[10:14]}}
    hp = {'cdatt_sm_temp': 0.5}
    want = {qid: [_oracle(reps[qid], reps[c], 'att', 0.5) for c in pool['cands']] for qid, pool in test_pool.items()}
    assert all(_well_separated(w) for w in want.values())
    results = {}
    for resident in (False, True):          # (not resident first: to_device keeps the store resident afterwards)
        for per_call in (32, 1):
            out = tmp_path / f'r{int(resident)}_{per_call}'
            got = evaluate.score(str(out), test_pool, store, method='l2attention', hparams=hp, queries_per_call=per_call, resident=resident)
            assert json.load(open(evaluate.get_scores_filename(str(out), None))) == {k: [list(t) for t in v] for k, v in got.items()}
            results[resident, per_call] = got
    worst = 0.0
    for key, got in results.items():
        assert list(got) == list(test_pool)
        for qid, pool in test_pool.items():
            order = orc.rank_descending(want[qid])
            assert [pid for pid, _ in got[qid]] == [pool['cands'][i] for i in order], (key, qid)
            worst = max([worst] + [abs(-s - want[qid][i]) for (_, s), i in zip(got[qid], order)])      # evaluate.py:77 stores -similarity
    print(f'EVALUATE l2attention: worst err {worst:.3e} (TOL {TOL:.0e})')
    assert worst <= TOL
    for resident in (False, True):
        for qid in test_pool:
            a, b = results[resident, 32][qid], results[resident, 1][qid]
            assert [p for p, _ in a] == [p for p, _ in b] and all(abs(x - y) <= TOL for (_, x), (_, y) in zip(a, b))
    assert results[False, 32] == results[True, 32]          # one form: the same bits from uploaded and from resident pools


# ---- case 6 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('agg,temp', AGGS[:2])
def test_a_document_longer_than_the_host_bound_scores_nan(agg, temp):
    """a candidate (a query) whose len exceeds its set's max_len comes back NaN; its neighbours keep their bits"""
    from aspire_amd import ops
    g = torch.Generator().manual_seed(6)
    queries = [torch.randn(n, D, generator=g) for n in (4, 9, 3)]
    sizes = [3, 4, 2]
    c_lens = [5, 2, 7, 3, 19, 8, 6, 4, 2]
    cands = [torch.randn(n, D, generator=g) for n in c_lens]
    q, c = ops.DeviceRepSet.from_list(queries), ops.DeviceRepSet.from_list(cands)
    job_off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device='cuda')
    run = lambda qs, cs: ops.l2agg_rank_batch(qs, cs, job_off, 4, 0, _agg_id(agg), temp=temp)[0].cpu().numpy()
    true = run(q, c)
    assert np.isfinite(true).all()
    short_c = ops.DeviceRepSet(c.rows, c.start, c.len, 0, 8)          # candidate 4 has 19 rows
    got = run(q, short_c)
    assert np.isnan(got[4]) and np.array_equal(_bits(np.delete(got, 4)), _bits(np.delete(true, 4)))
    short_q = ops.DeviceRepSet(q.rows, q.start, q.len, 0, 4)          # query 1 has 9 rows: its whole job
    got = run(short_q, c)
    assert np.isnan(got[3:7]).all() and np.array_equal(_bits(np.delete(got, np.s_[3:7])), _bits(np.delete(true, np.s_[3:7])))
