"""The fused otAspire kernel's Solve16 form (fused.hip: a wave streams a super-item of sixteen candidates and solves the
sixteen pairs in the four-lanes-per-pair layout of fused_solve.h) against the sixteen-lanes-per-pair form it stands beside:
the same batch under pinned(FUSED_SOLVE16=1) and pinned(FUSED_SOLVE16=0), bit for bit -- scores, top-k scores, indices.  Every
call checks, by the library's count of Solve16 launches, that the pinned form is the one that ran."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
K = 10
MIN_GROUPS = 512        # score.hip: kStreamMinGroupsBatch -- batches below it never reach the fused kernel


@pytest.fixture(scope='module')
def amd():
    from aspire_amd import ops, _lib
    assert torch.cuda.is_available()
    return type('NS', (), dict(ops=ops, lib=_lib, pinned=_lib.pinned))


def _launches(amd):
    buf = ctypes.create_string_buffer(64)
    amd.lib.check(amd.lib.lib.aspire_debug_get(b'FUSED_SOLVE16_LAUNCHES', buf, len(buf)))
    return int(buf.value)


def _sets(amd, queries, pools, scaling=0.9, **_):
    sizes = [len(p) for p in pools]
    # fused.hip, fused_self_ok: <= 64 jobs and scaling >= 0.25; score.hip: enough groups of four for the fused kernel
    assert len(pools) <= 64 and scaling >= 0.25 and len(pools) * ((max(sizes) + 3) // 4) >= MIN_GROUPS, 'the batch would not take the fused SELF form'
    q = amd.ops.DeviceRepSet.from_list(queries)
    c = amd.ops.DeviceRepSet.from_list([d for p in pools for d in p])
    job_off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32).cuda()
    return q, c, job_off, max(sizes)


def _run(amd, form, queries, pools, pins=None, **kw):
    q, c, job_off, max_job = _sets(amd, queries, pools, **kw)
    before = _launches(amd)
    with amd.pinned(FUSED_SOLVE16=form, **(pins or {})):
        s, ts, ti = amd.ops.ot_rank_batch(q, c, job_off, max_job, K, **kw)
        torch.cuda.synchronize()
    assert _launches(amd) - before == form, 'the pinned form did not run'
    return s, ts, ti


def _same(amd, queries, pools, **kw):
    old = _run(amd, 0, queries, pools, **kw)
    new = _run(amd, 1, queries, pools, **kw)
    for o, n, what in zip(old, new, ('scores', 'top scores', 'top indices')):
        assert torch.equal(o, n), (what, int((o != n).sum()), o.numel())
    return new


def _docs(g, n, smin=1, smax=8):
    return [torch.randn(int(l), 768, generator=g) for l in torch.randint(smin, smax + 1, (n,), generator=g)]


def _uniform(seed, jobs=33, n=64):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(8, 768, generator=g) for _ in range(jobs)], [[torch.randn(8, 768, generator=g) for _ in range(n)] for _ in range(jobs)]


def test_uniform_pools(amd):
    """33 jobs x 64 candidates, 8 rows on both sides, the bench's hyper-parameters: four full super-items per job"""
    s, _, _ = _same(amd, *_uniform(1), blur=0.05, scaling=0.9, sent_sm_temp=1.0)
    assert torch.isfinite(s).all() and (s < 0).all()


def test_partial_and_tiny_super_items(amd):
    """pool sizes around the super-item's sixteen and the sub-item's four, empty pools among them"""
    g = torch.Generator().manual_seed(2)
    sizes = [1, 5, 15, 16, 17, 31, 33, 100] * 5
    sizes[3], sizes[20], sizes[39] = 0, 0, 0
    queries = _docs(g, len(sizes), 8, 8)
    pools = [_docs(g, n, 8, 8) for n in sizes]
    s, _, ti = _same(amd, queries, pools)
    assert torch.isfinite(s).all() and torch.all(ti[3] == -1)


def test_ragged_rows(amd):
    """documents of 1 .. 8 rows on both sides; a 1-row query meets a 1-row candidate inside one super-item"""
    g = torch.Generator().manual_seed(3)
    sizes = [61, 64, 70] * 11
    queries = _docs(g, len(sizes))
    pools = [_docs(g, n) for n in sizes]
    queries[4] = torch.randn(1, 768, generator=g)
    pools[4][18] = torch.randn(1, 768, generator=g)
    pools[4][19] = torch.randn(8, 768, generator=g)
    s, _, _ = _same(amd, queries, pools)
    assert torch.isfinite(s).all()


@pytest.mark.parametrize('scale', [1.0, 3.0])
def test_shared_sentence(amd, scale):
    """a copy of the query and a candidate sharing one sentence with it (the cancelling-entry redo), at super-item positions 0, 7
    and 15; on 3 x N(0, 1) vectors the zero cost takes the shifted sums out of range and the pair is solved again in the wave"""
    queries, pools = _uniform(4)
    queries = [scale * x for x in queries]
    pools = [[scale * d for d in p] for p in pools]
    g = torch.Generator().manual_seed(40)
    for job, pos in ((0, 0), (5, 16 + 7), (32, 48 + 15)):
        pools[job][pos] = queries[job].clone()
        other = (pos + 16) % 64
        pools[job][other] = torch.cat([queries[job][2:3], scale * torch.randn(4, 768, generator=g)])
    s, _, _ = _same(amd, queries, pools)
    assert torch.isfinite(s).all()


def test_mixed_schedule_lengths_in_one_wave(amd):
    """candidates scaled by 0.05 and by 20 beside plain ones: diameters, and with them step counts, differ widely inside a super-item"""
    queries, pools = _uniform(5)
    for p in pools:
        for i in range(0, 64, 3):
            p[i] = 0.05 * p[i]
        for i in range(1, 64, 5):
            p[i] = 20.0 * p[i]
    s, _, _ = _same(amd, queries, pools)
    assert torch.isfinite(s).all()


@pytest.mark.parametrize('hp', [dict(blur=0.01, scaling=0.5), dict(blur=0.5, scaling=0.95)])
def test_hyper_parameters(amd, hp):
    g = torch.Generator().manual_seed(6)
    sizes = [64] * 33
    s, _, _ = _same(amd, _docs(g, 33), [_docs(g, n) for n in sizes], **hp)
    assert torch.isfinite(s).all()


def _eq_nan(x, y):
    return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0))


def test_poisoned_pairs_reach_the_re_solve(amd):
    """The issue's 'NaN follow-up' case.  The setting that test_gpu_fused uses for it (scaling = 0.01) is outside the SELF form
    (fused_self_ok: scaling >= 0.25), so neither pin would reach the kernels compared here; inside it the shifted sums leave fp32
    range for a candidate that shares a sentence with its query on 3 x N(0, 1) vectors (test_gpu_fused.
    test_fused_kernel_overflowed_pairs_are_resolved), and the wave that finds such a pair solves it again in the max-shifted form
    (solve_safe / solve16_safe; no launch behind the kernel in this tree).  With that re-solve switched off (FUSED_NOREPAIR) the
    poisoned pairs show: there are some, they are the same pairs with the same raw scores under either form, and with the re-solve on
    both forms give them the same finite scores."""
    queries, pools = _uniform(7)
    queries = [3.0 * x for x in queries]
    pools = [[3.0 * d for d in p] for p in pools]
    g = torch.Generator().manual_seed(70)
    for job, pos in ((0, 0), (1, 5), (5, 16 + 7), (17, 33), (32, 48 + 15)):
        pools[job][pos] = torch.cat([queries[job][:1], 3.0 * torch.randn(pos % 7 + 1, 768, generator=g)])
    old, new = _run(amd, 0, queries, pools), _run(amd, 1, queries, pools)
    raw_old = _run(amd, 0, queries, pools, pins=dict(FUSED_NOREPAIR=1))
    raw_new = _run(amd, 1, queries, pools, pins=dict(FUSED_NOREPAIR=1))
    hit_old = ~torch.isfinite(raw_old[0]) | (raw_old[0] != old[0])
    hit_new = ~torch.isfinite(raw_new[0]) | (raw_new[0] != new[0])
    print('poisoned pairs:', int(hit_old.sum()), int(hit_new.sum()))
    assert int(hit_old.sum()) >= 1 and torch.equal(hit_old, hit_new)
    assert _eq_nan(raw_old[0], raw_new[0])
    assert torch.isfinite(new[0]).all()
    for o, n in zip(old, new):
        assert torch.equal(o, n)


@pytest.mark.parametrize('want', ['DISTANCE', 'PLAN_SIM'])
def test_other_outputs(amd, want):
    """the transport cost itself and the plan-weighted similarity: solve16_output's other two forms"""
    g = torch.Generator().manual_seed(10)
    s, _, _ = _same(amd, _docs(g, 33), [_docs(g, 64) for _ in range(33)], want=getattr(amd.lib, 'OT_' + want))
    assert torch.isfinite(s).all()


def test_centred_rows(amd):
    """ASPIRE_OT_FLAG_CENTER: the staged rows move by the query's mean inside the stage loop, under either form"""
    g = torch.Generator().manual_seed(11)
    queries = [d + 5.0 for d in _docs(g, 33)]
    pools = [[d + 5.0 for d in _docs(g, 64)] for _ in range(33)]
    amd.ops.set_center_hint(True)
    try:
        s, _, _ = _same(amd, queries, pools)
    finally:
        amd.ops.set_center_hint(None)
    assert torch.isfinite(s).all()


def test_unpinned_form_follows_the_streams(amd):
    """unpinned, a launch takes Solve16 when its stream differs from the previous launch's (fused.hip, solve16_wanted): calls that
    rotate over two streams take it, calls that stay on one do not; the scores are the same bits whichever ran"""
    queries, pools = _uniform(12)
    q, c, job_off, max_job = _sets(amd, queries, pools)
    want = _run(amd, 0, queries, pools)[0]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with amd.pinned(FUSED_SOLVE16=''):
        def call(stream):
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                s = amd.ops.ot_rank_batch(q, c, job_off, max_job, K)[0]
            stream.synchronize()
            assert torch.equal(s, want)
        call(s1)
        n0 = _launches(amd)
        for st in (s2, s1, s2):
            call(st)
        assert _launches(amd) - n0 == 3
        for st in (s2, s2, s2):
            call(st)
        assert _launches(amd) - n0 == 3


def test_permutation_invariance(amd):
    """reversing the jobs reverses the outputs: a job's bits do not depend on its place in the batch"""
    g = torch.Generator().manual_seed(8)
    sizes = [64, 17, 100, 33] * 6
    queries = _docs(g, len(sizes))
    pools = [_docs(g, n) for n in sizes]
    s, ts, ti = _run(amd, 1, queries, pools)
    s2, ts2, ti2 = _run(amd, 1, queries[::-1], pools[::-1])
    off = np.concatenate([[0], np.cumsum(sizes)])
    off2 = np.concatenate([[0], np.cumsum(sizes[::-1])])
    J = len(sizes)
    for j in range(J):
        assert torch.equal(s[off[j]:off[j + 1]], s2[off2[J - 1 - j]:off2[J - j]]), j
    assert torch.equal(ts, ts2.flip(0)) and torch.equal(ti, ti2.flip(0))


def test_stage_entry_point(amd):
    """stages 1, 6 and 8 of aspire_debug_ot_rank_batch_stages_f32, one after the other on one workspace and as one mask, give the full
    call's outputs"""
    queries, pools = _uniform(9)
    q, c, job_off, max_job = _sets(amd, queries, pools)
    lib = amd.lib.lib
    qs, cs = q.struct(), c.struct()
    prm = amd.ops._ot_params(c, 0.05, 0.9, 1.0, amd.lib.CDIST_AUTO, False)
    ws = torch.empty(max(lib.aspire_ot_rank_batch_workspace_bytes(ctypes.byref(qs), ctypes.byref(cs), max_job, K), 16), dtype=torch.uint8,
                     device='cuda')
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    with amd.pinned(FUSED_SOLVE16=1):
        want = amd.ops.ot_rank_batch(q, c, job_off, max_job, K, workspace=ws)
        want = [t.clone() for t in want]
        s = torch.full_like(want[0], float('nan'))
        ts = torch.full_like(want[1], float('nan'))
        ti = torch.full_like(want[2], -7)
        for masks in ((1, 6, 8), (1 | 6 | 8,)):
            s.fill_(float('nan'))
            ts.fill_(float('nan'))
            ti.fill_(-7)
            before = _launches(amd)
            for stages in masks:
                amd.lib.check(lib.aspire_debug_ot_rank_batch_stages_f32(
                    ctypes.byref(qs), ctypes.byref(cs), 768, ptr(job_off), max_job, ctypes.byref(prm), amd.lib.OT_SIMILARITY, ptr(s), K,
                    ptr(ts), ptr(ti), ptr(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), stages))
            torch.cuda.synchronize()
            assert _launches(amd) - before == 1
            assert torch.equal(s, want[0]) and torch.equal(ts, want[1]) and torch.equal(ti, want[2]), masks
