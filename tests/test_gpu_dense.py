"""GPU: the dense gather-and-rank entry (aspire_amd/csrc/dense.hip: aspire_dense_rank_batch_f32) through ops.dense_rank_batch, the
torch op and nearest.rank_pool, against float64 numpy computed here.

Shape: N = 70 rows of N(0, 1), D = 768; J = 4 jobs with pools of 1, 5, 64 and 67 candidates (one candidate, less than a wave's
slice of 8, a whole number of slices, a remainder -- and slices that cross every job boundary).  The pools overlap; pool 1 holds
row 12 twice (an exact tie: pool order decides) and its own query row 10 (L2 exactly -0.0); pool 3 holds a second copy of one of
its rows and its own query row too.
Bar: the project's 1e-4 absolute parity bar.  The L2 distances here are about 39 (one ulp: 3.8e-6) and the cosines below 1; the
largest number formed is the dot product of a row with itself, about 768, one ulp of which is 6.1e-5.
Worst |error| per metric: printed by test_scores_and_ranking_against_float64; DESIGN.md section 6 keeps what was measured."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BAR = 1e-4
SWAP_CAP = 0.05                  # at most this share of the adjacent pairs of the float64 ranking may be closer than the window
# Near-tie window of the ranking check: candidates whose float64 scores are closer than this may swap.  Twice the bar for the L2
# distance and the dot product.  The cosines of 70 N(0, 1) rows in 768 dimensions all lie within +-0.12 (sigma = 768 ** -0.5 =
# 0.036): a pool of 67 packs them about 2e-3 apart, so about one adjacent pair in ten is closer than 2e-4 whatever the seed, and
# the 5 % condition on the float64 reference cannot hold with that window.  A cosine is at most 1 and comes from 12-term chains,
# six butterfly additions, two square roots and two divisions in fp32 (2 ** -24 each): its error stays below 2e-6, so the cosine
# ranking is held to a window ten times NARROWER, 2e-5 -- a stricter check, under which the reference has 3 near-ties in 133.
WINDOW = {'l2': 2 * BAR, 'dot': 2 * BAR, 'cosine': 2e-5}
N, D = 70, 768
Q_ROWS = [3, 10, 20, 33]
GUARD = 256                      # guard elements (bytes for the workspace) on either side of every buffer
F32_SENTINEL = 12345.5
I64_SENTINEL = 0x5A5A5A5A5A5A5A5A
U8_SENTINEL = 0xA5
METRICS = ('l2', 'cosine', 'dot')


def _pools():
    rng = np.random.default_rng(7)
    p2 = rng.permutation(N)[:64].tolist()
    p3 = rng.permutation(N)[:67].tolist()
    if 33 not in p3:
        p3[11] = 33
    p3[40] = p3[5]                                       # a second copy of a row, 35 places behind the first
    return [[7], [7, 12, 10, 12, 50], p2, p3]


def _want(x64, q, pool, metric):
    c, qv = x64[pool], x64[q]
    if metric == 'l2':
        return -np.sqrt(((c - qv) ** 2).sum(1))
    if metric == 'dot':
        return c @ qv
    return c @ qv / np.linalg.norm(qv) / np.linalg.norm(c, axis=1)


class _Data:
    def __init__(self):
        from aspire_amd import _lib
        self.code = {'l2': _lib.DENSE_L2, 'cosine': _lib.DENSE_COSINE, 'dot': _lib.DENSE_DOT}
        self.x = np.random.default_rng(0).standard_normal((N, D)).astype(np.float32)
        self.x64 = self.x.astype(np.float64)
        self.pools = _pools()
        self.sizes = [len(p) for p in self.pools]
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.rows = torch.from_numpy(self.x).cuda()
        self.q_idx = torch.tensor(Q_ROWS, dtype=torch.int32).cuda()
        self.cand_idx = torch.tensor(sum(self.pools, []), dtype=torch.int32).cuda()
        self.job_off = torch.from_numpy(self.off.astype(np.int32)).cuda()
        self.max_job = max(self.sizes)
        self.want = {m: [_want(self.x64, q, p, m) for q, p in zip(Q_ROWS, self.pools)] for m in METRICS}     # float64, never changed
        self.got = {}

    def call(self, metric):
        """the 4-job call, full lists (k = max_job), once per metric -> (scores, top_scores, top_idx) on the host"""
        from aspire_amd import ops
        if metric not in self.got:
            out = ops.dense_rank_batch(self.rows, self.q_idx, self.cand_idx, self.job_off, self.max_job, self.max_job,
                                       metric=self.code[metric])
            self.got[metric] = tuple(t.cpu().numpy() for t in out)
        return self.got[metric]


@pytest.fixture(scope='module')
def data():
    return _Data()


def _bits(a):
    a = np.asarray(a, dtype=np.float32)
    return a.view(np.uint32) if a.ndim == 0 else np.ascontiguousarray(a).view(np.uint32)


def test_the_float64_reference_has_few_near_ties(data):
    """the ranking rule below lets candidates closer than WINDOW swap: on this seed the float64 reference alone must keep
    those to at most 5 % of the adjacent pairs (the copies of a row are among them)"""
    for m in METRICS:
        close = total = 0
        for w in data.want[m]:
            s = np.sort(w)[::-1]
            close += int((np.abs(np.diff(s)) < WINDOW[m]).sum())
            total += len(s) - 1
        assert total == sum(data.sizes) - len(data.sizes)
        assert 2 <= close <= SWAP_CAP * total, (m, close, total)          # (2: the two copies)


@pytest.mark.parametrize('metric', METRICS)
def test_scores_and_ranking_against_float64(data, metric):
    scores, top_s, top_i = data.call(metric)
    assert scores.shape == (sum(data.sizes),) and top_s.shape == top_i.shape == (4, data.max_job)
    worst = 0.0
    for j, (pool, want) in enumerate(zip(data.pools, data.want[metric])):
        n = len(pool)
        mine = scores[data.off[j]:data.off[j + 1]]
        err = np.abs(mine.astype(np.float64) - want)
        worst = max(worst, float(err.max()))
        # the ranking: a permutation of the pool that is the float64 stable ranking, except between candidates whose float64
        # scores are closer than the window (twice the bar; narrower for the cosine); exact float64 ties (copies of a row) keep
        # pool order
        order = top_i[j, :n]
        assert sorted(order.tolist()) == list(range(n)), j
        assert np.array_equal(_bits(top_s[j, :n]), _bits(mine[order] + np.float32(0))), j     # (the rank hands -0.0 out as +0.0)
        assert (top_i[j, n:] == -1).all() and np.isneginf(top_s[j, n:]).all(), j
        for a, b in zip(order[:-1], order[1:]):
            if want[a] == want[b]:
                assert a < b and _bits(mine[a]) == _bits(mine[b]), (j, a, b)
            else:
                assert want[a] > want[b] or abs(want[a] - want[b]) < WINDOW[metric], (j, a, b, want[a], want[b])
    print(f'DENSE {metric}: worst |error| vs float64 {worst:.3e} (bar {BAR:.0e})')
    assert worst <= BAR, (metric, worst)


def test_ties_and_the_query_in_its_own_pool(data):
    s_l2, _, i_l2 = data.call('l2')
    s_cos = data.call('cosine')[0]
    # pool 1 = [7, 12, 10, 12, 50] against row 10: the query itself first, at exactly -0.0; the two copies of row 12 in pool order
    l2 = s_l2[data.off[1]:data.off[2]]
    assert l2[2] == 0 and np.signbit(l2[2]) and _bits(l2[2]) == 0x80000000
    assert i_l2[1, 0] == 2
    for m in METRICS:
        s, _, order = data.call(m)
        mine = s[data.off[1]:data.off[2]]
        assert _bits(mine[1]) == _bits(mine[3])
        o = order[1, :5].tolist()
        assert o.index(3) == o.index(1) + 1, (m, o)
        p3 = data.pools[3]
        mine3, o3 = s[data.off[3]:data.off[4]], order[3, :67].tolist()
        assert p3[40] == p3[5] and _bits(mine3[40]) == _bits(mine3[5]) and o3.index(40) == o3.index(5) + 1, m
    assert abs(float(s_cos[data.off[1] + 2]) - 1.0) <= BAR
    own3 = data.pools[3].index(33)
    assert _bits(s_l2[data.off[3] + own3]) == 0x80000000 and abs(float(s_cos[data.off[3] + own3]) - 1.0) <= BAR
    # the same row against the same query scores the same bits in every pool it sits in (row 7 is in pools 0 and 1 under
    # different queries; rows shared by pools 2 and 3 likewise: only the pair counts)
    for m in METRICS:
        seen = {}
        s = data.call(m)[0]
        for j, pool in enumerate(data.pools):
            for i, r in enumerate(pool):
                key = (Q_ROWS[j], r)
                bits = int(_bits(s[data.off[j] + i]))
                assert seen.setdefault(key, bits) == bits, (m, key)


@pytest.mark.parametrize('metric', METRICS)
def test_a_pair_scores_the_same_bits_in_a_one_job_call(data, metric):
    from aspire_amd import ops
    whole = data.call(metric)[0]
    for j, pool in enumerate(data.pools):
        s1, ts1, ti1 = ops.dense_rank_batch(data.rows, data.q_idx[j:j + 1].contiguous(), torch.tensor(pool, dtype=torch.int32).cuda(),
                                            torch.tensor([0, len(pool)], dtype=torch.int32).cuda(), len(pool), len(pool),
                                            metric=data.code[metric])
        assert np.array_equal(_bits(s1.cpu().numpy()), _bits(whole[data.off[j]:data.off[j + 1]])), (metric, j)
        assert np.array_equal(ti1.cpu().numpy()[0], data.call(metric)[2][j, :len(pool)])


def _guarded(n, dtype, sentinel):
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device='cuda')
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n, sentinel):
    return bool((whole[:GUARD] == sentinel).all()) and bool((whole[GUARD + n:] == sentinel).all())


def _call_guarded(rows, q_idx, cand_idx, job_off, max_job, k, metric, job_base=None, key_form=False):
    """one call with every output and the workspace (at exactly its documented size) inside sentinel guards; results on the host"""
    from aspire_amd import _lib, ops
    J, C = q_idx.numel(), cand_idx.numel()
    need = int(_lib.lib.aspire_dense_rank_batch_workspace_bytes(J, C, max_job, k))
    assert need % 16 == 0 and need == _lib.lib.aspire_topk_workspace_bytes(J, max_job, k) * (k > 0) and (need > 0) == (max_job > 4096 and k > 0)
    ws_whole, ws = _guarded(need, torch.uint8, U8_SENTINEL)
    assert (ws_whole.data_ptr() + GUARD) % 16 == 0
    sc_whole, scores = _guarded(C, torch.float32, F32_SENTINEL)
    bufs = [(sc_whole, C, F32_SENTINEL), (ws_whole, need, U8_SENTINEL)]
    if key_form:
        k_whole, keys = _guarded(J * k, torch.int64, I64_SENTINEL)
        out = (scores, keys.view(J, k))
        bufs.append((k_whole, J * k, I64_SENTINEL))
    else:
        s_whole, top_s = _guarded(J * k, torch.float32, F32_SENTINEL)
        i_whole, top_i = _guarded(J * k, torch.int64, I64_SENTINEL)
        out = (scores, top_s.view(J, k), top_i.view(J, k))
        bufs += [(s_whole, J * k, F32_SENTINEL), (i_whole, J * k, I64_SENTINEL)]
    got = ops.dense_rank_batch(rows, q_idx, cand_idx, job_off, max_job, k, metric=metric, out=out, workspace=ws, job_base=job_base,
                               key_form=key_form)
    torch.cuda.synchronize()
    for whole, n, sentinel in bufs:
        assert _guards_intact(whole, n, sentinel), (k, key_form, whole.dtype, n)
    if k == 0:                   # scores only: the lists' (empty) views and the workspace are not written
        assert bool((ws_whole == U8_SENTINEL).all())
    return tuple(t.cpu().numpy() for t in got)


def _check_lists(sizes, off, scores, top_s, top_i, k, base):
    for j, n in enumerate(sizes):
        mine = scores[off[j]:off[j + 1]]
        order = np.argsort(-mine.astype(np.float64), kind='stable')[:k]
        kk = min(k, n)
        assert np.array_equal(top_i[j, :kk], base[j] + order), j
        assert np.array_equal(_bits(top_s[j, :kk]), _bits(mine[order] + np.float32(0))), j    # (+-0.0 are one rank key: listed as +0.0)
        assert (top_i[j, kk:] == -1).all() and np.isneginf(top_s[j, kk:]).all(), j


@pytest.mark.parametrize('k', [0, 3, 67, 80])
def test_rank_contract(data, k):
    """k = 0 (scores only), k below the pools' sizes, k = max_job and k beyond every pool ((-inf, -1) padding); job_base; keys"""
    from aspire_amd import _lib, ops
    ref = data.call('l2')[0]
    base = np.array([0, 1000, 123456, 2 ** 31 - 1 - 67], dtype=np.int64)
    job_base = torch.from_numpy(base.astype(np.int32)).cuda()
    args = (data.rows, data.q_idx, data.cand_idx, data.job_off, data.max_job, k, _lib.DENSE_L2)
    scores, top_s, top_i = _call_guarded(*args)
    assert np.array_equal(_bits(scores), _bits(ref))
    assert top_s.shape == top_i.shape == (4, k)
    _check_lists(data.sizes, data.off, scores, top_s, top_i, k, np.zeros(4, np.int64))
    if k == 0:
        return
    scores_b, top_s_b, top_i_b = _call_guarded(*args, job_base=job_base)
    assert np.array_equal(_bits(scores_b), _bits(ref)) and np.array_equal(_bits(top_s_b), _bits(top_s))
    _check_lists(data.sizes, data.off, scores_b, top_s_b, top_i_b, k, base)
    scores_k, keys = _call_guarded(*args, job_base=job_base, key_form=True)
    assert np.array_equal(_bits(scores_k), _bits(ref))
    for j, n in enumerate(data.sizes):
        kk = min(k, n)
        mine = torch.from_numpy(scores[data.off[j]:data.off[j + 1]].copy()).cuda()
        assert np.array_equal(keys[j], ops.topk_keys(mine[None], k, idx_base=int(base[j]))[0].cpu().numpy()), j
        idx = 0xFFFFFFFF - (keys[j, :kk].astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert np.array_equal(idx, top_i_b[j, :kk]) and (keys[j, kk:] == 0).all(), j


@pytest.mark.parametrize('k', [100, 4097])
def test_a_pool_beyond_one_rank_chunk_takes_the_workspace(data, k):
    """a pool of 4097 candidates (row indices repeating over the 70 rows: 58 or 59 exact ties per row, pool order decides) beside
    a pool of 5: the rank's multi-pass routes (chunk winners for k = 100, the full sort for k = 4097) and their scratch"""
    from aspire_amd import _lib
    rng = np.random.default_rng(11)
    long_pool = rng.integers(0, N, 4097).tolist()
    sizes = [5, 4097]
    off = np.array([0, 5, 4102], dtype=np.int64)
    q_idx = torch.tensor([10, 41], dtype=torch.int32).cuda()
    cand_idx = torch.tensor(data.pools[1] + long_pool, dtype=torch.int32).cuda()
    job_off = torch.from_numpy(off.astype(np.int32)).cuda()
    scores, top_s, top_i = _call_guarded(data.rows, q_idx, cand_idx, job_off, 4097, k, _lib.DENSE_L2)
    want = np.concatenate([data.want['l2'][1], _want(data.x64, 41, long_pool, 'l2')])
    assert float(np.abs(scores.astype(np.float64) - want).max()) <= BAR
    assert np.array_equal(_bits(scores[:5]), _bits(data.call('l2')[0][data.off[1]:data.off[2]]))
    by_row = {}
    for i, r in enumerate(long_pool):                   # every copy of a row scores its bits
        assert by_row.setdefault(r, int(_bits(scores[5 + i]))) == int(_bits(scores[5 + i]))
    _check_lists(sizes, off, scores, top_s, top_i, k, np.zeros(2, np.int64))


def test_out_of_range_indices_score_nan_and_nothing_else_changes(data):
    """one bad row index in cand_idx and one in q_idx: NaN for exactly the pairs they touch, the bits of the clean call elsewhere.
    The kernel's guard replaces the loads of such a row by zeros -- nothing is read for it.  The matrix handed in is the middle of
    a larger allocation and the bad indices stay within that margin, so this test cannot become a stray read whatever it finds."""
    from aspire_amd import _lib, ops
    margin = 8
    big = torch.zeros(N + 2 * margin, D, device='cuda')
    big[margin:margin + N] = data.rows
    rows = big[margin:margin + N]
    assert rows.is_contiguous() and rows.data_ptr() % 16 == 0
    for metric in METRICS:
        clean = data.call(metric)[0]
        for bad in (N, N + 3, -1, -4):
            cand = data.cand_idx.clone()
            hit = int(data.off[2]) + 9                   # in the middle of a slice of pool 2
            cand[hit] = bad
            s = ops.dense_rank_batch(rows, data.q_idx, cand, data.job_off, data.max_job, 0, metric=data.code[metric])[0].cpu().numpy()
            assert np.isnan(s[hit]) and np.isnan(s).sum() == 1
            keep = np.arange(len(s)) != hit
            assert np.array_equal(_bits(s[keep]), _bits(clean[keep])), (metric, bad)
            q = data.q_idx.clone()
            q[1] = bad                                   # job 1: candidates 1 .. 5, inside the slices of jobs 0 and 2
            s = ops.dense_rank_batch(rows, q, data.cand_idx, data.job_off, data.max_job, 0, metric=data.code[metric])[0].cpu().numpy()
            in_job = (np.arange(len(s)) >= data.off[1]) & (np.arange(len(s)) < data.off[2])
            assert np.isnan(s[in_job]).all() and not np.isnan(s[~in_job]).any()
            assert np.array_equal(_bits(s[~in_job]), _bits(clean[~in_job])), (metric, bad)
    torch.cuda.synchronize()
    assert bool((big[:margin] == 0).all()) and bool((big[margin + N:] == 0).all())


def test_torch_op_opcheck(data):
    import aspire_amd.torch_ops  # noqa: F401
    from aspire_amd import _lib
    for metric in METRICS:
        args = (data.rows, data.q_idx, data.cand_idx, data.job_off, data.max_job, 9, data.code[metric])
        torch.library.opcheck(torch.ops.aspire.dense_rank_batch, args, test_utils=('test_schema', 'test_faketensor'))
        s, ts, ti = torch.ops.aspire.dense_rank_batch(*args)
        ref = data.call(metric)
        assert np.array_equal(_bits(s.cpu().numpy()), _bits(ref[0]))
        assert np.array_equal(ti.cpu().numpy()[:, :5], ref[2][:, :5]) and ti.dtype == torch.int64 and tuple(ts.shape) == (4, 9)
    assert _lib.DENSE_L2 == 0


def test_rank_pool_end_to_end(data):
    """nearest.rank_pool / rank_pool_faceted on the same data against the numpy ranking: ascending positive distances at the bar,
    the float64 order except between near-ties, the query left out of its own list, copies in pool order"""
    from aspire_amd import nearest
    reps = nearest.DenseReps(data.x, {f'p{i}': i for i in range(N)})
    assert reps.rows.is_cuda and tuple(reps.rows.shape) == (N, D)
    qpid2pool = {f'p{q}': {'cands': [f'p{r}' for r in pool] + (['gone'] if j == 2 else [])}
                 for j, (q, pool) in enumerate(zip(Q_ROWS, data.pools))}
    out = nearest.rank_pool(reps, qpid2pool)
    assert list(out) == [f'p{q}' for q in Q_ROWS]
    for j, (q, pool) in enumerate(zip(Q_ROWS, data.pools)):
        want = -data.want['l2'][j]                       # float64 distances by pool position
        ranked = out[f'p{q}']
        assert len(ranked) == len(pool) - pool.count(q)
        assert all(pid != f'p{q}' for pid, _ in ranked)
        dists = [d for _, d in ranked]
        assert dists == sorted(dists) and all(type(d) is float and d > 0 for d in dists)
        want_of = {f'p{r}': w for r, w in zip(pool, want)}
        keep = [i for i in np.argsort(want, kind='stable') if pool[i] != q]
        for (pid, d), i in zip(ranked, keep):
            assert abs(d - want[i]) <= BAR, (j, pid)
            assert pid == f'p{pool[i]}' or abs(want_of[pid] - want[i]) < WINDOW['l2'], (j, pid, pool[i])
    faceted = nearest.rank_pool_faceted(reps, {k: v for k, v in qpid2pool.items() if k != 'p20'})
    assert faceted == {k: v for k, v in out.items() if k != 'p20'}
    with pytest.raises(KeyError):
        nearest.rank_pool_faceted(reps, qpid2pool)
    cos = nearest.rank_pool(reps, {'p33': qpid2pool['p33']}, metric='cosine')['p33']
    want = 1.0 - data.want['cosine'][3]
    first = [i for i in np.argsort(want, kind='stable') if data.pools[3][i] != 33][:5]
    assert np.diff(want[first]).min() > WINDOW['cosine']
    assert [pid for pid, _ in cos][:5] == [f'p{data.pools[3][i]}' for i in first]
    assert all(abs(d - want[i]) <= BAR for (_, d), i in zip(cos, first))
