"""The segmented rank that ends every batched scoring call (aspire_amd/csrc/batch_host.h: BatchRank::rank -> topk_run with
seg_off = job_off, seg_base = job_base), once, through all three entry points: ops.ot_rank_batch, ops.l2max_rank_batch and
ops.dotmax_rank_batch.  The job-size lists put ragged segments (empty jobs, one-candidate jobs, a short job beside a long one)
into every route of topk_run: the select kernels on 1024-, 2048- and 4096-key chunks, the one-chunk sort pass, the multi-pass
winners route and the full sort beyond one chunk.

The rank's reference is the call's own `scores` output, which the scoring kernels write and the rank only reads: numpy's
stable argsort of it, exact.  The scores themselves are checked on a fixed sample against the oracle at the bars of the suites
of each entry point (tests/test_gpu_batch.py, tests/test_gpu_sentenc.py).  Every output and the workspace are views into larger
buffers filled with a sentinel, the workspace at exactly the bytes its *_workspace_bytes function returns; the sentinel around
them must survive the call."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import aspire_oracle as orc
from test_gpu_sentenc import _check_pair

pytestmark = pytest.mark.gpu
TOL = 1e-4                       # otAspire / tsAspire against the oracle (tests/test_gpu_batch.py, smoke())
GUARD = 256                      # guard elements (bytes for the workspace) on either side of every buffer
F32_SENTINEL = 12345.5
I64_SENTINEL = 0x5A5A5A5A5A5A5A5A
U8_SENTINEL = 0xA5

REGIMES = {
    'select': [0, 300, 0, 0, 1, 1024, 257, 0],          # one chunk of 1024 keys, select + 256-key sort
    'select2048': [1500, 3, 2048, 0, 1025],             # the 2048-key select chunk
    'sortpass': [900, 4096, 0, 17],                     # one 4096-key chunk; k > 128 takes the sort pass
    'winners': [9001, 5, 0, 4097, 4096],                # max_job > 4096, k < 1024: chunk winners, then further passes
    'fullsort': [9001, 5, 0, 4097, 12289],              # max_job > 4096, k >= 1024: sorted chunks + merge passes + emit
}
# (regime, k); 'max' = max_job, 'max+7' = beyond every pool
CASES = [('select', 10), ('select', 128), ('select2048', 100), ('sortpass', 129), ('sortpass', 1000), ('sortpass', 'max'),
         ('winners', 100), ('winners', 1023), ('fullsort', 1024), ('fullsort', 5000), ('fullsort', 'max'), ('fullsort', 'max+7')]
# entry point + pinned switches: otAspire on its default form, on the small-batch kernels, and on the fused kernel behind the
# tables launch (FUSED_NOSELF: not the in-wave tables that <= 64 jobs take by themselves)
VARIANTS = [('ot', {}, c) for c in CASES] + [('l2max', {}, c) for c in CASES] + [('dotmax', {}, c) for c in CASES] + \
    [('ot', {'OT_FORM': 'small'}, c) for c in (('select', 10), ('select2048', 100), ('sortpass', 129))] + \
    [('ot', {'OT_FORM': 'fused', 'FUSED_NOSELF': 1}, c) for c in (('winners', 100), ('fullsort', 1024))]


def _id(v):
    entry, pins, (regime, k) = v
    return '-'.join([entry] + [str(x).lower() for x in pins.values()] + [regime, f'k{k}'])


class _Jobs:
    """queries [J] and every job's candidates back to back: ragged documents of 1..8 rows, formed on the device; a few
    candidates of every job of >= 7 are copies of another one of the same job (exact ties, pool order decides), in the long
    jobs also across the 4096-key chunk boundaries"""

    def __init__(self, name):
        from aspire_amd import ops
        self.sizes = sizes = REGIMES[name]
        seed = sorted(REGIMES).index(name)
        rng = np.random.default_rng(100 + seed)
        self.off = off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        C, J = int(off[-1]), len(sizes)
        lens = rng.integers(1, 9, C)
        lens[off[:-1][np.array(sizes) > 0]] = 8                      # the first candidate of every job has all 8 rows
        self.dups = []                                               # (job, dst, src): candidate dst is a copy of src
        for j, n in enumerate(sizes):
            dsts, srcs = set(), set()
            want = []
            for b in range(4096, n, 4096):                           # both sides of every chunk boundary inside the job
                want += [(b, b - 1), (b - 2, 5), (b + 1, b - 3)]
            if n >= 7:
                want += [(3, 1), (n - 2, 2)]
            for dst, src in want:                                    # a copy is nobody's original, an original nobody's copy
                if dst < n and dst not in dsts and dst not in srcs and src not in dsts:
                    dsts.add(dst)
                    srcs.add(src)
                    self.dups.append((j, dst, src))
        for j, dst, src in self.dups:
            lens[off[j] + dst] = lens[off[j] + src]
        start = np.cumsum(lens) - lens
        self.start, self.lens = start, lens
        g = torch.Generator(device='cuda').manual_seed(1000 + seed)
        rows = torch.randn(int(lens.sum()), 768, device='cuda', generator=g)
        for j, dst, src in self.dups:
            d, s = off[j] + dst, off[j] + src
            rows[start[d]:start[d] + lens[d]] = rows[start[s]:start[s] + lens[s]]
        self.c = ops.DeviceRepSet(rows, torch.from_numpy(start.astype(np.int32)).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda(),
                                  0, 8, lens_host=lens.tolist())
        qlens = rng.integers(1, 9, J)
        qlens[0] = 8
        self.queries = [torch.randn(int(n), 768, generator=torch.Generator().manual_seed(2000 + 10 * seed + j))
                        for j, n in enumerate(qlens)]
        self.q = ops.DeviceRepSet.from_list(self.queries)
        self.job_off = torch.from_numpy(off.astype(np.int32)).cuda()
        self.max_job = max(sizes)
        # distinct per job: small values, 0 for one job, and for the longest job the largest base whose indices still fit int32
        base = np.array([(j + 1) * 100003 for j in range(J)], dtype=np.int64)
        self.long_job = int(np.argmax(sizes))
        base[self.long_job] = 2 ** 31 - 1 - self.max_job
        base[1 if self.long_job == 0 else 0] = 0
        assert len(set(base.tolist())) == J
        self.base = base
        self.job_base = torch.from_numpy(base.astype(np.int32)).cuda()
        # the fixed sample the oracle sees: the first and the last two candidates of every job (both neighbours of every
        # job_off boundary), two in the middle, and every copy
        sample = set()
        for j, n in enumerate(sizes):
            sample |= {(j, i) for i in (0, 1, n // 3, n // 2, n - 2, n - 1) if 0 <= i < n}
        sample |= {(j, d) for j, d, _ in self.dups[:6]}
        self.sample = sorted(sample)
        self.want = {}                                               # entry -> oracle values of the sample

    def doc(self, j, i):
        p = int(self.off[j] + i)
        s, n = int(self.start[p]), int(self.lens[p])
        return self.c.rows[s:s + n].cpu()


@pytest.fixture(scope='module')
def jobs_of():
    """regime name -> its _Jobs, formed once and kept (with its device row matrices) until this module is done"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Jobs(name)
        return cache[name]
    yield get
    cache.clear()


def _oracle(entry, qd, cd):
    if entry == 'ot':
        return float(orc.get_similarity(qd, cd))
    assert entry == 'l2max'
    return -orc.allpair_masked_dist_l2max(orc.RepLen(qd[None].permute(0, 2, 1), [len(qd)]),
                                          orc.RepLen(cd[None].permute(0, 2, 1), [len(cd)])).item()


def _guarded(n, dtype, sentinel):
    """a contiguous [n] view in the middle of a larger buffer, all of it (the view too) filled with `sentinel`"""
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device='cuda')
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n, sentinel):
    return bool((whole[:GUARD] == sentinel).all()) and bool((whole[GUARD + n:] == sentinel).all())


def _call(entry, q, c, job_off, max_job, k, job_base, key_form):
    """one batched call with every output and the workspace inside sentinel guards -> (scores, top_s, top_i) or (scores, keys),
    on the host"""
    from aspire_amd import _lib, ops
    fn = {'ot': ops.ot_rank_batch, 'l2max': ops.l2max_rank_batch, 'dotmax': ops.dotmax_rank_batch}[entry]
    ws_fn = {'ot': _lib.lib.aspire_ot_rank_batch_workspace_bytes, 'l2max': _lib.lib.aspire_l2max_rank_batch_workspace_bytes,
             'dotmax': _lib.lib.aspire_dotmax_rank_batch_workspace_bytes}[entry]
    J, C = q.n, c.n
    qs, cs = q.struct(), c.struct()
    need = int(ws_fn(ctypes.byref(qs), ctypes.byref(cs), max_job, k))
    assert need % 16 == 0
    if entry == 'dotmax':                                 # its workspace is the rank's multi-pass scratch and nothing else
        assert need == _lib.lib.aspire_topk_workspace_bytes(J, max_job, k) and (need > 0) == (max_job > 4096)
    ws_whole, ws = _guarded(need, torch.uint8, U8_SENTINEL)
    assert ws.numel() == need and (ws_whole.data_ptr() + GUARD) % 16 == 0
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
    got = fn(q, c, job_off, max_job, k, out=out, workspace=ws, job_base=job_base, key_form=key_form)
    torch.cuda.synchronize()
    for whole, n, sentinel in bufs:
        assert _guards_intact(whole, n, sentinel), (entry, k, key_form, whole.dtype, n)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, out))
    return tuple(t.cpu().numpy() for t in got)


def _check_scores(entry, jobs, scores):
    """the fixed sample against the oracle; copies score what their originals score"""
    assert np.isfinite(scores).all()                     # (also: no element of `scores` kept the sentinel's place unwritten
    assert not (scores == np.float32(F32_SENTINEL)).any()         # -- no similarity here is anywhere near it)
    if entry == 'dotmax':
        for j, i in jobs.sample:
            _check_pair(float(scores[jobs.off[j] + i]), jobs.queries[j].numpy(), jobs.doc(j, i).numpy())
    else:
        if entry not in jobs.want:
            jobs.want[entry] = np.array([_oracle(entry, jobs.queries[j], jobs.doc(j, i)) for j, i in jobs.sample])
        got = np.array([scores[jobs.off[j] + i] for j, i in jobs.sample], dtype=np.float64)
        err = np.abs(got - jobs.want[entry])
        assert err.max() <= TOL, (jobs.sample[int(err.argmax())], float(err.max()))
    for j, dst, src in jobs.dups:
        assert scores[jobs.off[j] + dst] == scores[jobs.off[j] + src], (j, dst, src)


def _expected(scores_j, k):
    return np.argsort(-scores_j.astype(np.float64), kind='stable')[:k]


def _check_lists(sizes, off, scores, top_s, top_i, k, base):
    for j, n in enumerate(sizes):
        mine = scores[off[j]:off[j + 1]]
        order = _expected(mine, k)
        kk = min(k, n)
        assert len(order) == kk
        assert np.array_equal(top_i[j, :kk], base[j] + order), j
        assert np.array_equal(top_s[j, :kk].view(np.uint32), mine[order].view(np.uint32)), j
        assert (top_i[j, kk:] == -1).all() and np.isneginf(top_s[j, kk:]).all(), j


@pytest.mark.parametrize('variant', VARIANTS, ids=_id)
def test_segmented_rank_contract(variant, jobs_of):
    from aspire_amd import _lib, ops
    entry, pins, (regime, k) = variant
    jobs = jobs_of(regime)
    sizes, off, J = jobs.sizes, jobs.off, len(jobs.sizes)
    k = jobs.max_job if k == 'max' else jobs.max_job + 7 if k == 'max+7' else k
    zero = np.zeros(J, np.int64)
    with _lib.pinned(**pins):
        scores, top_s, top_i = _call(entry, jobs.q, jobs.c, jobs.job_off, jobs.max_job, k, None, False)
        scores_b, top_s_b, top_i_b = _call(entry, jobs.q, jobs.c, jobs.job_off, jobs.max_job, k, jobs.job_base, False)
        scores_k, keys = _call(entry, jobs.q, jobs.c, jobs.job_off, jobs.max_job, k, jobs.job_base, True)
    _check_scores(entry, jobs, scores)
    # job_base = NULL: positions inside the job's own pool
    _check_lists(sizes, off, scores, top_s, top_i, k, zero)
    # job_base: the same scores, the same lists, every index moved by exactly job_base[j]
    assert np.array_equal(scores_b.view(np.uint32), scores.view(np.uint32))
    assert np.array_equal(top_s_b.view(np.uint32), top_s.view(np.uint32))
    _check_lists(sizes, off, scores_b, top_s_b, top_i_b, k, jobs.base)
    for j, n in enumerate(sizes):
        kk = min(k, n)
        assert np.array_equal(top_i_b[j, :kk] - top_i[j, :kk], np.full(kk, jobs.base[j])), j
    assert int(top_i_b.max()) == 2 ** 31 - 2 or k < jobs.max_job      # (the longest job's last candidate, when it is listed)
    # key form: the single-pool key entry on the job's own scores with idx_base = job_base[j]; padding keys are 0
    assert np.array_equal(scores_k.view(np.uint32), scores.view(np.uint32))
    for j, n in enumerate(sizes):
        kk = min(k, n)
        if n:
            mine = torch.from_numpy(scores[off[j]:off[j + 1]].copy()).cuda()
            want = ops.topk_keys(mine[None], k, idx_base=int(jobs.base[j]))[0].cpu().numpy()
            assert np.array_equal(keys[j], want), j
            assert (keys[j, :kk] != 0).all()
            # ... and read directly: the low word is ~(global index)
            idx = 0xFFFFFFFF - (keys[j, :kk].astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
            assert np.array_equal(idx, top_i_b[j, :kk]), j
        assert (keys[j, kk:] == 0).all(), j
    if k <= 4096:
        m_s, m_i = ops.topk_merge_keys(torch.from_numpy(keys[None].copy()).cuda(), k)
        assert np.array_equal(m_i.cpu().numpy(), top_i_b)
        assert np.array_equal(m_s.cpu().numpy().view(np.uint32), top_s_b.view(np.uint32))


@pytest.mark.parametrize('entry', ['ot', 'l2max', 'dotmax'])
@pytest.mark.parametrize('regime,k', [('select2048', 100), ('winners', 100), ('fullsort', 5000), ('fullsort', 'max')])
def test_two_shards_of_a_long_job_merge_by_one_key_sort(entry, regime, k, jobs_of):
    """section 8(e) through the batched calls: the longest job's pool as two contiguous blocks, each ranked by a call of its own
    with job_base = [0] and [split]; one unsigned descending sort of the two key lists is the order of the whole pool"""
    from aspire_amd import ops
    jobs = jobs_of(regime)
    j, n = jobs.long_job, jobs.max_job
    k = n if k == 'max' else k
    lo = int(jobs.off[j])
    split = n // 2 + 3                                   # not a multiple of a chunk: the second block starts mid-chunk
    q1 = ops.DeviceRepSet.from_list([jobs.queries[j]])
    shard_scores, shard_keys = [], []
    for a, b in ((0, split), (split, n)):
        c1 = jobs.c.slice(lo + a, lo + b)
        job_off = torch.tensor([0, b - a], dtype=torch.int32).cuda()
        s, keys = _call(entry, q1, c1, job_off, b - a, k, torch.tensor([a], dtype=torch.int32).cuda(), True)
        shard_scores.append(s)
        shard_keys.append(keys[0])
    whole = np.concatenate(shard_scores)
    merged = np.sort(np.concatenate(shard_keys).astype(np.uint64))[::-1][:min(k, n)]
    assert (merged != 0).all()
    idx = (0xFFFFFFFF - (merged & np.uint64(0xFFFFFFFF))).astype(np.int64)
    assert np.array_equal(idx, _expected(whole, k))
    # the un-sharded call: the same candidates against the same query.  dotmax scores every pair with one kernel, one wave per
    # pair, so its bits do not depend on the batch; otAspire / tsAspire may take another kernel form for another batch size
    full = _call(entry, jobs.q, jobs.c, jobs.job_off, n, k, None, False)
    mine = full[0][lo:lo + n]
    if entry == 'dotmax':
        assert np.array_equal(mine.view(np.uint32), whole.view(np.uint32))
        assert np.array_equal(full[2][j, :min(k, n)], idx)
    else:
        np.testing.assert_allclose(mine, whole, atol=TOL, rtol=0)
