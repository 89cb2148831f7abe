"""GPU: the jointsm scorer (aspire_amd/csrc/jointsm.hip) -- parity with the float64 closed form at twice the reference's own fp32
error on every fixture case (tests/golden/jointsm.npz: seeds + the reference's outputs and its own error), the kernel forms against
each other, the batched rank, the entry's contracts, and the polyenc host layer end to end.

The bar.  Per fixture case the reference's own error against the float64 closed form 2 sum_ij p_ij d_ij is stored (relative to
max(|score|, 1) for scores, absolute for pair_sm); the kernels are held to TWICE that: the working precision is the reference's,
the summation order is not bmm's.  Inputs that are not fixture cases (the width and length sweeps, the rank jobs' sample) are built
the way the fixture's are and are held to twice the LARGEST stored error among the fixture cases of their shape class: SHORT_BAR for
documents of <= 16 rows, LONG_BAR beyond.  Every figure is printed before it is asserted (run with -s to see them)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from jointsm_inputs import D, OFFSET, POOL_SWAP_CAP, case_inputs, closed_form, pool_inputs, spec_of  # noqa: E402
from test_gpu_dotmax_forms import BOUNDS, N_CANDS, N_QUERIES  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jointsm.npz'))
CASE_NAMES = [str(n) for n in FIXTURE['cases']]
_short = [n for n in CASE_NAMES if max(int(x) for x in FIXTURE[f'{n}_shape'][1:]) <= 16]
SHORT_BAR = 2 * max(float(FIXTURE[f'{n}_ref_err']) for n in _short)
LONG_BAR = 2 * max(float(FIXTURE[f'{n}_ref_err']) for n in CASE_NAMES)
SM_BAR = 2 * max(float(FIXTURE[f'{n}_ref_err_sm']) for n in CASE_NAMES)
GUARD = 256
F32_SENTINEL, I64_SENTINEL, U8_SENTINEL = 12345.5, 0x5A5A5A5A5A5A5A5A, 0xA5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rel(got, want):
    return np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), 1.0)


def _docs(rng, lens, scale, off):
    return [(scale * rng.standard_normal((int(n), D)) + off).astype(np.float32) for n in lens]


def _want(qd, cd):
    return closed_form(qd[None], cd[None], [len(qd)], [len(cd)])[0][0]


def _scores(q, c, pairing, soft=False, q_max_len=None, c_max_len=None, stream=None):
    """aspire_jointsm_scores_f32 through ctypes (optionally with the host bounds overridden): scores, pair_softmax or None"""
    from aspire_amd import _lib, ops
    qs, cs = q.struct(), c.struct()
    if q_max_len is not None:
        qs.max_len = q_max_len
    if c_max_len is not None:
        cs.max_len = c_max_len
    n = q.n if pairing == _lib.PAIR_PAIRED else q.n * c.n
    out = torch.full((n,), 7.0, device='cuda', dtype=torch.float32)
    sm = torch.full((n, q.ext, c.ext), 7.0, device='cuda', dtype=torch.float32) if soft else None
    _lib.check(_lib.lib.aspire_jointsm_scores_f32(ctypes.byref(qs), ctypes.byref(cs), ops.D, pairing, ops._ptr(out), ops._ptr(sm),
                                                  stream if stream is not None else ops._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), (sm.cpu().numpy() if soft else None)


# ---- parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASE_NAMES)
def test_parity_with_float64_at_twice_the_reference_error(name):
    """every fixture case through the C ABI, PAIRED and CROSS (the case's pairs are the diagonal), CSR and padded; pair_softmax
    from the padded forms.  Measured worst values: DESIGN.md section 6."""
    from aspire_amd import _lib, ops
    q, c, qlens, clens = case_inputs(spec_of(FIXTURE, name))
    b = len(qlens)
    want, want_sm = closed_form(q, c, qlens, clens)
    bar, bar_sm = 2 * float(FIXTURE[f'{name}_ref_err']), 2 * float(FIXTURE[f'{name}_ref_err_sm'])
    sets = {'padded': (ops.DeviceRepSet.from_padded(torch.from_numpy(q), qlens), ops.DeviceRepSet.from_padded(torch.from_numpy(c), clens)),
            'csr': (ops.DeviceRepSet.from_list([q[i, :n] for i, n in enumerate(qlens)]),
                    ops.DeviceRepSet.from_list([c[i, :n] for i, n in enumerate(clens)]))}
    worst, worst_sm = 0.0, 0.0
    for layout, (qs, cs) in sets.items():
        for pairing in (_lib.PAIR_PAIRED, _lib.PAIR_CROSS):
            for soft in ((False, True) if layout == 'padded' else (False,)):
                got, sm = _scores(qs, cs, pairing, soft)
                if pairing == _lib.PAIR_CROSS:
                    got = got.reshape(b, b).diagonal()
                    sm = sm.reshape(b, b, *sm.shape[1:])[np.arange(b), np.arange(b)] if soft else None
                err = float(_rel(got, want).max())
                print(f'{name} {layout} pairing={pairing} soft={soft}: score err {err:.3e} (bar {bar:.3e})')
                worst = max(worst, err)
                if soft:
                    err_sm = float(np.abs(sm.astype(np.float64) - want_sm).max())
                    print(f'{name} {layout} pairing={pairing}: pair_softmax err {err_sm:.3e} (bar {bar_sm:.3e})')
                    worst_sm = max(worst_sm, err_sm)
                    for i, (ql, cl) in enumerate(zip(qlens, clens)):
                        assert np.all(_bits(sm[i, ql:, :]) == 0) and np.all(_bits(sm[i, :, cl:]) == 0), (name, i)     # exactly +0.0
    print(f'PARITY {name}: worst score err {worst:.3e} / bar {bar:.3e}; worst pair_softmax err {worst_sm:.3e} / bar {bar_sm:.3e}')
    assert worst <= bar, (name, worst, bar)
    assert worst_sm <= bar_sm, (name, worst_sm, bar_sm)


# ---- forms ------------------------------------------------------------------------------------------------------------
def _sweep_docs(bq, bc, nq, nc, seed):
    rng = np.random.RandomState(seed)
    ql, cl = rng.randint(1, bq + 1, nq), rng.randint(1, bc + 1, nc)
    ql[-1], cl[int(rng.randint(0, nc))] = bq, bc
    off = OFFSET * rng.standard_normal(D)
    scale = (0.3, 0.6, 1.0)[seed % 3]
    return _docs(rng, ql, scale, off), _docs(rng, cl, scale, off)


@pytest.mark.parametrize('bc', BOUNDS)
@pytest.mark.parametrize('bq', BOUNDS)
def test_cross_widths_against_the_pair_kernel(bq, bc):
    """all 64 pairs of row-slot widths of jointsm_cross_kernel: against float64 and against jointsm_pair_kernel (the same pairs
    PAIRED).  The two kernels form the same dot products and sum the soft-max in different orders: the same bar, not the same bits."""
    from aspire_amd import _lib, ops
    q_docs, c_docs = _sweep_docs(bq, bc, N_QUERIES[bq], N_CANDS[bc], 1000 + 17 * bq + bc)
    q, c = ops.DeviceRepSet.from_list(q_docs), ops.DeviceRepSet.from_list(c_docs)
    cross = _scores(q, c, _lib.PAIR_CROSS)[0].reshape(len(q_docs), len(c_docs))
    assert (cross != 7.0).all() and np.isfinite(cross).all()
    pairs = [(i, j) for i in range(len(q_docs)) for j in range(len(c_docs))]
    paired = _scores(ops.DeviceRepSet.from_list([q_docs[i] for i, _ in pairs]), ops.DeviceRepSet.from_list([c_docs[j] for _, j in pairs]),
                     _lib.PAIR_PAIRED)[0].reshape(cross.shape)
    want = np.array([_want(q_docs[i], c_docs[j]) for i, j in pairs]).reshape(cross.shape)
    e_cross, e_pair, e_forms = float(_rel(cross, want).max()), float(_rel(paired, want).max()), float(_rel(cross, paired.astype(np.float64)).max())
    print(f'WIDTHS {bq}x{bc}: cross {e_cross:.3e} pair {e_pair:.3e} cross-vs-pair {e_forms:.3e} (bar {SHORT_BAR:.3e})')
    assert max(e_cross, e_pair, e_forms) <= SHORT_BAR, (bq, bc, e_cross, e_pair, e_forms)


@pytest.mark.parametrize('rows', [17, 31, 32, 33, 48, 64, 65, 100, 127, 128])
def test_lengths_beyond_the_cross_kernel(rows):
    """documents of 17 .. 128 rows on either side (CROSS goes to jointsm_pair_kernel): CROSS and PAIRED give the same bits, both
    meet the bar"""
    from aspire_amd import _lib, ops
    rng = np.random.RandomState(rows)
    off = OFFSET * rng.standard_normal(D)
    scale = (0.3, 0.6, 1.0)[rows % 3]
    q_docs = _docs(rng, [rows, 3, max(1, rows - 16), 16], scale, off)
    c_docs = _docs(rng, [1, rows, rows - 1, 17, 9], scale, off)
    cross = _scores(ops.DeviceRepSet.from_list(q_docs), ops.DeviceRepSet.from_list(c_docs), _lib.PAIR_CROSS)[0].reshape(4, 5)
    pairs = [(i, j) for i in range(4) for j in range(5)]
    paired = _scores(ops.DeviceRepSet.from_list([q_docs[i] for i, _ in pairs]), ops.DeviceRepSet.from_list([c_docs[j] for _, j in pairs]),
                     _lib.PAIR_PAIRED)[0].reshape(4, 5)
    want = np.array([_want(q_docs[i], c_docs[j]) for i, j in pairs]).reshape(4, 5)
    err = float(_rel(cross, want).max())
    print(f'LENGTHS {rows}: err {err:.3e} (bar {LONG_BAR:.3e})')
    assert np.array_equal(_bits(cross), _bits(paired))            # one kernel, one order: equality
    assert err <= LONG_BAR, (rows, err)


# ---- batched rank -------------------------------------------------------------------------------------------------------
def _guarded(n, dtype, sentinel):
    buf = torch.full((n + 2 * GUARD,), sentinel, device='cuda', dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, sentinel):
    return bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all())


@pytest.mark.parametrize('sizes,k', [([0, 37, 1, 0, 300, 5], 10), ([0, 37, 1, 0, 300, 5], 300), ([4200, 0, 9, 4097], 50), ([4200, 0, 9, 4097], 4200)])
def test_rank_batch_bits_order_and_guards(sizes, k):
    """ragged jobs with empty ones (and a pool above one 4096-key chunk): scores = the bits of jointsm_scores PAIRED on the same
    pairs; top_scores / top_idx = Python's stable sorted(..., reverse=True) over them, + job_base; the key form decodes to the same
    lists; nothing is written outside the outputs or the workspace."""
    from aspire_amd import _lib, ops
    rng = np.random.RandomState(len(sizes) * 1000 + k)
    J, C, max_job = len(sizes), sum(sizes), max(sizes)
    off = OFFSET * rng.standard_normal(D)
    lens = rng.randint(1, 9, C)
    c_docs = _docs(rng, lens, 0.6, off)
    job_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    for j, n in enumerate(sizes):           # exact ties: copies inside a job, also across the 4096-key boundary
        for dst, src in ((3, 1), (n - 2, 2), (4096, 4095), (4098, 7)):
            if 0 <= src < dst < n:
                c_docs[job_off[j] + dst] = c_docs[job_off[j] + src]
    queries = _docs(rng, rng.randint(1, 9, J), 0.6, off)
    q, c = ops.DeviceRepSet.from_list(queries), ops.DeviceRepSet.from_list(c_docs)
    job_of = np.repeat(np.arange(J), sizes)
    idx = torch.from_numpy(job_of).cuda()
    q_per_cand = ops.DeviceRepSet(q.rows, q.start[idx].contiguous(), q.len[idx].contiguous(), 0, q.max_len)
    paired = _scores(q_per_cand, c, _lib.PAIR_PAIRED)[0]
    base = np.array([(j + 1) * 100003 for j in range(J)], dtype=np.int32)
    need = ops.rank_batch_workspace_bytes('jointsm', q, c, max_job, k)
    assert (need > 0) == (max_job > 4096)
    for key_form in (False, True):
        sbuf, scores = _guarded(C, torch.float32, F32_SENTINEL)
        wbuf, ws = _guarded(max(need, 16), torch.uint8, U8_SENTINEL)
        if key_form:
            kbuf, keys = _guarded(J * k, torch.int64, I64_SENTINEL)
            out = (scores, keys.view(J, k))
        else:
            tsbuf, top_s = _guarded(J * k, torch.float32, F32_SENTINEL)
            tibuf, top_i = _guarded(J * k, torch.int64, I64_SENTINEL)
            out = (scores, top_s.view(J, k), top_i.view(J, k))
        ret = ops.jointsm_rank_batch(q, c, torch.from_numpy(job_off).cuda(), max_job, k, out=out, workspace=ws[:max(need, 16)],
                                     job_base=torch.from_numpy(base).cuda(), key_form=key_form)
        torch.cuda.synchronize()
        assert _guards_intact(sbuf, C, F32_SENTINEL) and _guards_intact(wbuf, max(need, 16), U8_SENTINEL)
        got = scores.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(paired))
        if key_form:
            assert _guards_intact(kbuf, J * k, I64_SENTINEL)
            ts, ti = ops.topk_merge_keys(ret[1].view(1, J, k).contiguous(), k) if k <= 4096 else (None, None)
            if ts is None:
                continue
        else:
            assert _guards_intact(tsbuf, J * k, F32_SENTINEL) and _guards_intact(tibuf, J * k, I64_SENTINEL)
            ts, ti = ret[1], ret[2]
        ts, ti = ts.cpu().numpy(), ti.cpu().numpy()
        for j, n in enumerate(sizes):
            seg = got[job_off[j]:job_off[j + 1]].tolist()
            order = sorted(range(n), key=lambda i: seg[i], reverse=True)[:k]
            assert ti[j, :len(order)].tolist() == [i + int(base[j]) for i in order], (j, key_form)
            assert np.array_equal(_bits(ts[j, :len(order)]), _bits(np.array([seg[i] for i in order], np.float32))), (j, key_form)
            assert (ti[j, len(order):] == -1).all() and np.isneginf(ts[j, len(order):]).all()
    # a sample of the scores against float64
    sample = [p for p in (0, 1, C // 3, C // 2, C - 2, C - 1) if 0 <= p < C]
    err = max(float(_rel(paired[p], _want(queries[job_of[p]], c_docs[p]))) for p in sample)
    print(f'RANK {sizes} k={k}: sample err {err:.3e} (bar {SHORT_BAR:.3e})')
    assert err <= SHORT_BAR


# ---- contracts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('longest', [2, 3, 8, 9, 13, 16, 17, 40, 128])
def test_a_document_longer_than_the_host_bound_scores_nan(longest):
    """one document per side has `longest` rows, max_len says longest - 1 (a power of two and not): that document's pairs are NaN
    in CROSS (both kernels) and PAIRED; every other pair keeps its value (its bits, unless the smaller bound moved the call
    from one kernel to the other: 17 -> 16)"""
    from aspire_amd import _lib, ops
    rng = np.random.RandomState(longest)
    off = OFFSET * rng.standard_normal(D)
    lens = [int(n) for n in rng.randint(1, longest, 11)]
    q_docs, c_docs = _docs(rng, lens, 0.6, off), _docs(rng, lens[::-1], 0.6, off)
    q_docs[4], c_docs[9] = _docs(rng, [longest, longest], 0.6, off)
    q_docs[0], c_docs[0] = _docs(rng, [longest - 1, longest - 1], 0.6, off)       # exactly the bound: not too long
    q, c = ops.DeviceRepSet.from_list(q_docs), ops.DeviceRepSet.from_list(c_docs)
    n = len(q_docs)
    for pairing, shape, q_bad, c_bad in ((_lib.PAIR_CROSS, (n, n), np.s_[4, :], np.s_[:, 9]), (_lib.PAIR_PAIRED, (n,), np.s_[4], np.s_[9])):
        true = _scores(q, c, pairing)[0].reshape(shape)
        assert np.isfinite(true).all() and (true != 7.0).all()
        for qb, cb in ((longest - 1, None), (None, longest - 1), (longest - 1, longest - 1)):
            got = _scores(q, c, pairing, q_max_len=qb, c_max_len=cb)[0].reshape(shape)
            bad = np.zeros(shape, bool)
            if qb is not None:
                bad[q_bad] = True
            if cb is not None:
                bad[c_bad] = True
            assert np.isnan(got[bad]).all(), (pairing, qb, cb, got[bad])
            same_kernel = pairing == _lib.PAIR_PAIRED or longest != 17 or (qb is None) != (cb is None)
            if same_kernel:
                assert np.array_equal(_bits(got[~bad]), _bits(true[~bad])), (pairing, qb, cb)
            else:
                assert float(_rel(got[~bad], true[~bad].astype(np.float64)).max()) <= SHORT_BAR, (pairing, qb, cb)
    # padded sets: ext is the bound; pair_softmax of such a pair is NaN throughout
    qp = ops.DeviceRepSet.from_padded(torch.zeros(2, max(longest - 1, 1), D), [1, 1])
    qp.len.copy_(torch.tensor([longest, 1], dtype=torch.int32))
    got, sm = _scores(qp, qp, _lib.PAIR_PAIRED, soft=True)
    assert np.isnan(got[0]) and np.isnan(sm[0]).all() and np.isfinite(got[1]) and np.isfinite(sm[1]).all()


def test_large_logits_stay_finite():
    """logits d / sqrt(768) of about +-70 (rows scaled up, every other query document negated): finite scores at the bar, in
    both kernels; a soft-max without the max shift overflows exp() at 88.7"""
    from aspire_amd import _lib, ops
    rng = np.random.RandomState(7)
    off = 1.55 * rng.standard_normal(D)
    q_docs, c_docs = _docs(rng, [8, 3, 16, 1, 20, 40], 0.5, off), _docs(rng, [8, 16, 2, 33, 5], 0.5, off)
    q_docs = [-x if i % 2 else x for i, x in enumerate(q_docs)]
    logits = np.array([[(qd.astype(np.float64) @ cd.astype(np.float64).T).max() for cd in c_docs] for qd in q_docs]) / np.sqrt(768.0)
    print(f'LOGITS {logits.min():.1f} .. {logits.max():.1f}')
    assert logits.max() > 60 and logits.min() < -40
    want = np.array([[_want(qd, cd) for cd in c_docs] for qd in q_docs])
    for qs, cs in ((q_docs, c_docs), (q_docs[:4], c_docs[:3])):            # the pair kernel (long documents present), the cross kernel
        got = _scores(ops.DeviceRepSet.from_list(qs), ops.DeviceRepSet.from_list(cs), _lib.PAIR_CROSS)[0].reshape(len(qs), len(cs))
        err = float(_rel(got, want[:len(qs), :len(cs)]).max())
        print(f'LOGITS err {err:.3e} (bar {LONG_BAR:.3e})')
        assert np.isfinite(got).all() and err <= LONG_BAR


def test_two_streams_with_their_own_outputs_do_not_interfere():
    from aspire_amd import _lib, ops
    rng = np.random.RandomState(3)
    off = OFFSET * rng.standard_normal(D)
    sets = [(ops.DeviceRepSet.from_list(_docs(rng, rng.randint(1, 17, 40), 0.6, off)), ops.DeviceRepSet.from_list(_docs(rng, rng.randint(1, 17, 900), 0.6, off)))
            for _ in range(2)]
    alone = [_scores(q, c, _lib.PAIR_CROSS)[0] for q, c in sets]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[torch.full((q.n * c.n,), 7.0, device='cuda') for _ in range(6)] for q, c in sets]
    torch.cuda.synchronize()
    for rep in range(6):
        for (q, c), st, out in zip(sets, streams, outs):
            with torch.cuda.stream(st):
                qs, cs = q.struct(), c.struct()
                _lib.check(_lib.lib.aspire_jointsm_scores_f32(ctypes.byref(qs), ctypes.byref(cs), ops.D, _lib.PAIR_CROSS, ops._ptr(out[rep]), None,
                                                              ops._stream()))
    torch.cuda.synchronize()
    for want, out in zip(alone, outs):
        for o in out:
            assert np.array_equal(_bits(o.cpu().numpy()), _bits(want))


# ---- the host layer, end to end -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [str(n) for n in FIXTURE['pools']])
def test_trained_scoring_model_against_the_reference_pool(name):
    """polyenc.TrainedScoringModel.predict / rank on the fixture's pools against WordSentAlignPolyEnc.score's stored outputs: scores
    at the bar; the ranking is the float64 ranking except between candidates whose float64 scores are closer than the bar, and at most
    POOL_SWAP_CAP of the adjacent pairs are that close (the generator checks the reference's own fp32 ranking the same way)."""
    from aspire_amd import polyenc, scorer
    spec = spec_of(FIXTURE, name)
    query, cands = pool_inputs(spec)
    pids = [f'p{i}' for i in range(len(cands))]
    model = polyenc.TrainedScoringModel('miswordpolyenc')
    pred = model.predict(query=query, cands=cands)
    want = np.array([_want(query, cd) for cd in cands])
    bar = 2 * float(FIXTURE[f'{name}_ref_err'])
    err, err_ref = float(_rel(pred['cand_scores'], want).max()), float(_rel(pred['cand_scores'], FIXTURE[f'{name}_scores'].astype(np.float64)).max())
    print(f'POOL {name}: err vs float64 {err:.3e} (bar {bar:.3e}); vs the reference fp32 {err_ref:.3e}')
    assert err <= bar and err_ref <= 1.5 * bar          # (the reference sits within bar / 2 of float64 itself)
    for i, p in enumerate(pred['pair_scores']):
        assert p.shape == (len(query), len(cands[i]))
        sm64 = closed_form(query[None], cands[i][None], [len(query)], [len(cands[i])])[1][0]
        assert float(np.abs(p - sm64).max()) <= SM_BAR, (i, float(np.abs(p - sm64).max()))
        key = f'{name}_pair_scores_{i}'
        if key in FIXTURE:
            assert float(np.abs(p - FIXTURE[key]).max()) <= 1.5 * SM_BAR
    ranked = model.rank(query, cands, pids)
    assert [s for _, s in ranked] == sorted(-s for s in pred['cand_scores'])
    close = lambda a, b: abs(want[a] - want[b]) < bar * max(abs(want[a]), 1.0)
    order = [int(p[1:]) for p, _ in ranked]
    order64 = sorted(range(len(want)), key=lambda i: want[i], reverse=True)
    assert sum(close(a, b) for a, b in zip(order64[:-1], order64[1:])) <= POOL_SWAP_CAP * (len(want) - 1)
    for a, b in zip(order[:-1], order[1:]):
        assert want[a] >= want[b] or close(a, b), (a, b)
    # the scorer's routes rank the same pool: rank_pool (cross entry + top-k), rank_pools (batched entry), deterministic
    by_batch = scorer.rank_pools([query], [scorer.CandidatePool(cands, pids)], method='jointsm')[0]
    by_pool = scorer.rank_pool([query], scorer.CandidatePool(cands, pids), method='jointsm', deterministic=True)[0]
    assert [p for p, _ in by_batch] == [p for p, _ in by_pool] and np.array_equal(_bits([s for _, s in by_batch]), _bits([s for _, s in by_pool]))
    assert float(_rel([s for _, s in by_batch], np.array([want[int(p[1:])] for p, _ in by_batch])).max()) <= bar
    sp = scorer.score_pool([query], cands, method='jointsm', schedule='batch', score_batch_size=7).cpu().numpy()[0]      # schedule: ignored
    assert float(_rel(sp, want).max()) <= bar


def test_pair_distances_and_torch_op():
    from aspire_amd import _lib, ops, allpair_joint_sm_negscore, rep_len_tup
    import aspire_amd.torch_ops  # noqa: F401
    q, c, qlens, clens = case_inputs(spec_of(FIXTURE, 's8'))
    want, want_sm = closed_form(q, c, qlens, clens)
    bar, bar_sm = 2 * float(FIXTURE['s8_ref_err']), 2 * float(FIXTURE['s8_ref_err_sm'])
    qt = rep_len_tup(embed=torch.from_numpy(q).permute(0, 2, 1), abs_lens=qlens)
    ct = rep_len_tup(embed=torch.from_numpy(c).permute(0, 2, 1), abs_lens=clens)
    dist = allpair_joint_sm_negscore(qt, ct)
    dist2, pair_sm = allpair_joint_sm_negscore(qt, ct, return_pair_sims=True)
    assert dist.device.type == 'cpu' and torch.equal(dist, dist2) and pair_sm.shape == (len(qlens), 8, 8)
    assert float(_rel(-dist.numpy(), want).max()) <= bar and float(np.abs(pair_sm.numpy() - want_sm).max()) <= bar_sm
    assert np.array_equal(_bits(-dist.numpy()), _bits(FIXTURE['s8_scores'])) or float(_rel(-dist.numpy(), FIXTURE['s8_scores'].astype(np.float64)).max()) <= 1.5 * bar
    qd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    ql, cl = torch.tensor(qlens, dtype=torch.int32).cuda(), torch.tensor(clens, dtype=torch.int32).cuda()
    for paired in (True, False):
        got = torch.ops.aspire.jointsm_scores(qd, ql, cd, cl, paired)
        same = ops.jointsm_scores(ops.DeviceRepSet.from_padded(qd, qlens), ops.DeviceRepSet.from_padded(cd, clens),
                                  pairing=_lib.PAIR_PAIRED if paired else _lib.PAIR_CROSS)
        assert torch.equal(got, same)
        torch.library.opcheck(torch.ops.aspire.jointsm_scores, (qd, ql, cd, cl, paired), test_utils=('test_schema', 'test_faketensor'))
