"""The 16-row streaming kernels (tile16.hip: pair_tile16_kernel, CROSS / MAPPED / REC, otAspire and max-sim) and the tiled cost kernel
for documents of <= 8 rows (cost_valu.hip: pair_tile_kernel) with SEVERAL items per wave.  A wave of these kernels is persistent:
`for (item = first; item < n_items; item += n_waves)` with the next item's context fetched one item ahead, accumulators zeroed per
item, a per-wave stage buffer that doubles as the norm table between items, the hybrid form's `continue` past items the fused kernel
has scored, and (REC) the roles wide / crow0 / qrow0 changing from item to item.  The launches take min(items bound, 2048) waves, so
at the sizes of the other suites a wave gets one or two items and an REC wave never a second one.  TILE_WAVES caps these launches at
4 .. 20 waves (the frame of tests/test_gpu_fused_wave_runs.py, whose helpers this file borrows), which puts 3 .. 500 items through
every wave.

Two properties per case:
 (a) wave-count invariance, bit for bit: the same call under TILE_WAVES = 4, 8, 12, 20 and unpinned gives torch.equal scores (the
     batched entries: top-k scores and indices too), for SIMILARITY, DISTANCE and PLAN_SIM where the entry takes `want`;
 (b) parity in the few-waves regime: the TILE_WAVES = 4 run against oracle.aspire_oracle.get_similarity at the project's 1e-4
     absolute, on >= 100 pairs per case (every pair where there are fewer) that hold the first and last item
     of every wave's run at four waves, the first and last real candidate of every job and every candidate of a tail item; max-sim
     against float64 -cdist from direct differences, maximum over the valid block, EVERY pair.  PLAN_SIM is held by (a) alone.
     Every otAspire case holds one candidate that shares a sentence with its query (the whole-wave direct-formula redo then runs
     between two items of a wave): the fp32 reference returns the square root of rounding noise for it (1.5e-2 .. 5.4e-2 from its
     own float64 value), so that pair is held to the FLOAT64 oracle, at the same 1e-4.
     Caller-supplied diameters: the oracle is given the same diameter (compute_distance(diameter=...)).

Every case works out on the host which items each wave receives from the launch rules (_all_runs: `bound` is the launcher's
items_bound) and asserts >= 3 items per wave at four waves and <= 1 unpinned, and that the route it names ran: differing bits
against OT_FORM = small (the per-pair kernels) is the handle.  Outputs and workspaces are views inside sentinel-filled buffers: the
guards survive and every output element is written.

Shapes that differ from a plain reading of the kernels' thresholds (the form rules of score.hip stay as they are):
 * CROSS max-sim takes tile16 from 4 096 candidates of ONE query, whatever the pins: 4 097 candidates are 2 049 items on the
   unpinned launch's 2 048 waves, so ONE unpinned wave gets two items there (asserted as <= 2).
 * the hybrid (few long pairs) needs J * ceil(max_job / 4) >= 2048 groups besides C >= 6000, and a batch whose queries all have
   <= 8 rows takes the CHUNK form instead: 8 jobs of 1024, 5 x 900, 541 and 20 candidates (6 085), the 20-candidate job's query of
   12 rows (every pair of that job is long), ~20 documents of 9 .. 16 rows scattered over the other jobs.  Its launches have more
   items (3 044) than unpinned waves: TILE_WAVES = 64 and 256 against unpinned (<= 2 items per wave), and want = PLAN_SIM is left
   out (the hybrid rule excludes it).
 * REC items are laid out by atomics (chunk16_prep_kernel): which candidates share an item, and the items' order, vary from run to
   run; the host model counts them (query halves * (wide + ceil(narrow / 2)) per job) and the oracle sees every pair."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import aspire_oracle as orc
from test_gpu_fused_wave_runs import (BOUNDS, F32_SENTINEL, K, TOL, U8_SENTINEL, WANTS, WAVES, _assert_same, _call_batch, _ends_of_jobs,
                                      _guarded, _guards_intact, _l2max_ref, _one_thread, _runs)

pytestmark = pytest.mark.gpu
CAP = 256 * 8                    # tile16.hip / launch_cost_stage: the launch's waves without a pin
SAMPLE = 100
JOBS16 = [7, 1, 0, 18, 2, 33, 0, 5, 3, 12, 16]       # MAPPED tile16: a one-candidate job (an item with both slots past its end), empty jobs
JOBS_REC = [9, 1, 0, 14, 5]
HYBRID = [1024, 900, 900, 900, 900, 900, 541, 20]


@pytest.fixture(scope='module')
def amd():
    from aspire_amd import ops, _lib
    assert torch.cuda.is_available()
    ops.set_center_hint(False)          # one arithmetic for every call of the module (no sampling of the rows)
    yield type('NS', (), dict(ops=ops, lib=_lib, pinned=_lib.pinned))
    ops.set_center_hint(None)


# ---- the launch rules, on the host ---------------------------------------------------------------------------------------------
def _launch_waves(bound, cap):
    """tile16.hip, launch_cost_stage: min(items bound, cap) waves, rounded up to whole workgroups of four"""
    return 4 * ((min(bound, cap or CAP) + 3) // 4)


def _all_runs(n_items, bound, label, caps=WAVES, unpinned_max=1):
    """wave -> its items (every n_waves-th one) per wave count; asserted: >= 3 items per wave at the pins' fewest waves (four), and
    at most `unpinned_max` (one) unpinned"""
    runs = {cap: _runs(n_items, _launch_waves(bound, cap), 'stride') for cap in tuple(caps) + (None,)}
    said = []
    for cap, r in runs.items():
        counts = [len(x) for x in r]
        assert sorted(u for x in r for u in x) == list(range(n_items))
        said.append(f'{cap or "unpinned"}: {min(counts)}..{max(counts)} on {len(r)}')
    print(f'{label}: {n_items} items; per wave at TILE_WAVES ' + ', '.join(said))
    few = min(caps)
    assert len(runs[few]) == few and min(len(x) for x in runs[few]) >= 3, 'the fewest waves no longer get three items each'
    assert max(len(x) for x in runs[None]) <= unpinned_max, 'unpinned, a wave gets more items than expected'
    return runs


def _cross_items(nq, c_lo, c_hi, per):
    """one CROSS launch over the candidates [c_lo, c_hi): items = (group of `per` candidates, query), group-major -> per item its real
    (query, candidate) pairs"""
    n = c_hi - c_lo
    return [[(qi, c_lo + i) for i in range(per * cg, min(per * cg + per, n))] for cg in range((n + per - 1) // per) for qi in range(nq)]


def _mapped_items(sizes, per):
    """MAPPED: the job tables' groups of four, job after job; per = 4: a group is an item (pair_tile_kernel), per = 2: each half of a
    group is one (tile16) -> per item its real (job, candidate) pairs: none where both slots lie past the job's end"""
    return [[(j, i) for i in range(4 * g + per * h, min(4 * g + per * h + per, n))]
            for j, n in enumerate(sizes) for g in range((n + 3) // 4) for h in range(4 // per)]


def _rec_items(q_lens, pools):
    """chunk16_prep_kernel: per job (one classification block up to 384 candidates) query halves * (wide + ceil(narrow / 2)) items;
    -> the count, and whether some job has an odd number of narrow candidates (an item whose second slot repeats the first)"""
    total, odd = 0, False
    for ql, pool in zip(q_lens, pools):
        assert len(pool) <= 384
        wide = sum(len(d) > 16 for d in pool)
        narrow = len(pool) - wide
        total += (2 if ql > 16 else 1) * (wide + (narrow + 1) // 2)
        odd |= bool(narrow & 1)
    return total, odd


def _chunk_items_bound(J, C, max_job):
    """batch_prep.hip: chunk_items_bound (one part per job at these sizes)"""
    assert max_job <= 384
    return max(C + 3 * J, (J if J <= 64 else 0) * max(1, max_job))


def _must(items, runs_few, sizes, per):
    """the pairs the oracle must see: the first and last item of every wave's run, the ends of every job, every pair of a tail item"""
    must = set(_ends_of_jobs(sizes))
    for run in runs_few:
        if run:
            must |= set(items[run[0]]) | set(items[run[-1]])
    for it in items:
        if len(it) < per:
            must |= set(it)
    return must


def _sample(pair_count, must, seed, n=SAMPLE):
    """`must` + a seeded prefix of ONE order of all pairs up to n (every pair where there are fewer)"""
    every = [(j, i) for j, m in enumerate(pair_count) for i in range(m)]
    order = np.random.default_rng(seed).permutation(len(every))
    picked = set(must)
    assert picked <= set(every)
    for t in order:
        if len(picked) >= min(n, len(every)):
            break
        picked.add(every[t])
    return sorted(picked)


# ---- references ----------------------------------------------------------------------------------------------------------------
def _oracle(x, y, diameter=None):
    if diameter is None:
        return float(orc.get_similarity(x, y))
    xt = orc.RepLen(embed=x[None, :].permute(0, 2, 1), abs_lens=[len(x)])
    yt = orc.RepLen(embed=y[None, :].permute(0, 2, 1), abs_lens=[len(y)])
    return -orc.AllPairMaskedWasserstein({}).compute_distance(query=xt, cand=yt, diameter=diameter).item()


def _check_oracle(cache, doc_pair, scores, flat, sample, sign, label, planted=(), diameter=None):
    """scores[flat(j, i)] of the sample against sign * the oracle (float64 for the planted pairs: a shared sentence); prints the worst
    error before it asserts"""
    with _one_thread():
        for key in sample:
            if key not in cache:
                x, y = doc_pair(*key)
                if key in planted:
                    x, y = x.double(), y.double()
                cache[key] = _oracle(x, y, None if diameter is None else diameter(*key))
    got = np.array([scores[flat(j, i)] for j, i in sample], dtype=np.float64)
    err = np.abs(sign * got - np.array([cache[k] for k in sample]))
    print(f'{label}: worst oracle error {err.max():.3e} over {len(sample)} pairs (at {sample[int(err.argmax())]})')
    assert np.isfinite(got).all() and err.max() <= TOL, (label, sample[int(err.argmax())], float(err.max()))


def _check_l2max(got, queries, pools, label):
    want = np.array([_l2max_ref(queries[j], d) for j, p in enumerate(pools) for d in p])
    err = np.abs(got.astype(np.float64) - want)
    print(f'{label}: worst error against float64 {err.max():.3e} over {len(want)} pairs')
    assert np.isfinite(got).all() and err.max() <= TOL, (label, int(err.argmax()), float(err.max()))


# ---- documents -----------------------------------------------------------------------------------------------------------------
def _docs(g, n, smin, smax, longest_at=None):
    lens = torch.randint(smin, smax + 1, (n,), generator=g).tolist()
    if longest_at is not None:
        lens[longest_at] = smax
    return [torch.randn(l, 768, generator=g) for l in lens]


def _plant(query, cand, row):
    """`cand` with its first row replaced by the query's row `row`: a shared sentence, the length kept"""
    return torch.cat([query[row:row + 1], cand[1:]])


class _Jobs:
    """J jobs for the batched entries, in the shape tests/test_gpu_fused_wave_runs.py's _call_batch takes"""

    def __init__(self, amd, queries, pools):
        self.queries, self.pools = queries, pools
        self.sizes = [len(p) for p in pools]
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.q = amd.ops.DeviceRepSet.from_list(queries)
        self.c = amd.ops.DeviceRepSet.from_list([d for p in pools for d in p])
        self.job_off = torch.tensor(self.off, dtype=torch.int32).cuda()
        self.max_job = max(self.sizes)
        self.oracle = {}

    def flat(self, j, i):
        return int(self.off[j]) + i

    def pair(self, j, i):
        return self.queries[j], self.pools[j][i]


def _pins(form, cap):
    return dict(OT_FORM=form, TILE_WAVES=cap if cap else '')


# ---- one pool (CROSS) ------------------------------------------------------------------------------------------------------------
def _call_cross(amd, q, c, form, cap, want='SIMILARITY', diameter=None, diam_group=0, ws_bytes=None, entry='ot'):
    """one single-pool call, the scores and the workspace inside sentinel guards -> a clone of the scores [nq, C]"""
    nq, C = q.n, c.n
    out = _guarded(nq * C, torch.float32, F32_SENTINEL)
    qs, cs = q.struct(), c.struct()
    ws = None
    with amd.pinned(**_pins(form, cap)):
        if entry == 'ot':
            need = ws_bytes or int(amd.lib.lib.aspire_ot_workspace_bytes(ctypes.byref(qs), ctypes.byref(cs), amd.lib.PAIR_CROSS))
            ws = _guarded(need, torch.uint8, U8_SENTINEL)
            assert ws[1].data_ptr() % 16 == 0
            amd.ops.ot_sinkhorn(q, c, want=getattr(amd.lib, 'OT_' + want), diameter=diameter, diam_group=diam_group, out=out[1],
                                workspace=ws[1])
        else:       # ops.l2max_scores makes its own output: the same entry point on a guarded buffer
            amd.lib.check(amd.lib.lib.aspire_l2max_scores_f32(ctypes.byref(qs), ctypes.byref(cs), 768, amd.lib.PAIR_CROSS, amd.lib.CDIST_AUTO,
                                                              amd.ops._ptr(out[1]), None, amd.ops._stream()))
        torch.cuda.synchronize()
    assert _guards_intact(out) and (ws is None or _guards_intact(ws)), ('written outside its bounds', form, cap)
    assert not bool((out[1] == F32_SENTINEL).any()), ('scores left unwritten', int((out[1] == F32_SENTINEL).sum()), form, cap)
    return out[1].view(nq, C).clone()


def _cross_case(amd, queries, cands, per, label, seed, planted=(), diam_group=0, chunk=None, wants=WANTS):
    """queries x one pool through ops.ot_sinkhorn under OT_FORM = tile: (a) for every want, (b) for SIMILARITY and DISTANCE.  per: the
    candidates of an item (2: tile16, 4: pair_tile_kernel); chunk: candidates per launch where the workspace is short of the pool"""
    nq, C = len(queries), len(cands)
    q, c = amd.ops.DeviceRepSet.from_list(queries), amd.ops.DeviceRepSet.from_list(cands)
    launches = [(lo, min(lo + chunk, C)) for lo in range(0, C, chunk)] if chunk else [(0, C)]
    items, runs_few = [], []
    for lo, hi in launches:           # every launch has its own items and its own waves
        mine = _cross_items(nq, lo, hi, per)
        runs = _all_runs(len(mine), len(mine), f'{label} [candidates {lo} .. {hi}]')
        runs_few += [[len(items) + u for u in run] for run in runs[4]]
        items += mine
    # a wave at four waves meets a short query (<= 8 rows) between two long ones where the case has both
    q_long = [len(x) > 8 for x in queries]
    if per == 2 and any(q_long) and not all(q_long):
        assert any(q_long[items[u][0][0]] and not q_long[items[v][0][0]] and q_long[items[w][0][0]]
                   for run in runs_few for u, v, w in zip(run, run[1:], run[2:]))
    ws_bytes = None
    if chunk:
        per_cand = ((2 * 64 * 4 + 1) * 4 if per == 2 else (2 * 64 + 1) * 4) * nq          # score.hip: slot_bytes, per_cand_bytes
        ws_bytes = chunk * per_cand + nq * 2 * 768 * 4 + 48
        assert ((ws_bytes - nq * 2 * 768 * 4) // 16 * 16 - 32) // per_cand == chunk
    diameter = amd.ops.group_diameter(q, c, amd.lib.PAIR_CROSS, diam_group) if diam_group else None
    at4 = {}
    for want in wants:
        ref = _call_cross(amd, q, c, 'tile', None, want, diameter, diam_group, ws_bytes)
        assert torch.isfinite(ref).all()
        for cap in WAVES:
            got = _call_cross(amd, q, c, 'tile', cap, want, diameter, diam_group, ws_bytes)
            assert torch.equal(ref, got), (label, want, cap, int((ref != got).sum()), ref.numel())
            if cap == 4:
                at4[want] = got
        if chunk:       # candidate chunks do not change a bit
            assert torch.equal(ref, _call_cross(amd, q, c, 'tile', None, want, diameter, diam_group)), (label, want, 'chunks')
    # the route: the per-pair kernels of OT_FORM = small sum in another order
    small = _call_cross(amd, q, c, 'small', None, 'SIMILARITY', diameter, diam_group)
    n_diff = int((small != at4['SIMILARITY']).sum())
    print(f'{label}: {n_diff} of {small.numel()} scores differ in bits from OT_FORM = small')
    assert n_diff > 0, 'OT_FORM = tile ran the kernels of OT_FORM = small'
    must = _must(items, runs_few, [C] * nq, per) | set(planted)
    sample = _sample([C] * nq, must, seed)
    cache = {}
    diam_host = diameter.cpu().numpy() if diam_group else None
    n_groups = (C + diam_group - 1) // diam_group if diam_group else 0
    for want, sign in (('SIMILARITY', 1.0), ('DISTANCE', -1.0)):
        _check_oracle(cache, lambda j, i: (queries[j], cands[i]), at4[want].cpu().numpy().reshape(-1), lambda j, i: j * C + i, sample, sign,
                      f'{label} [{want}]', planted,
                      (lambda j, i: float(diam_host[j * n_groups + i // diam_group])) if diam_group else None)


@pytest.fixture(scope='module')
def cross16():
    """queries of 16, 9 and 5 rows against 41 candidates of 1 .. 16 rows (one of 16; an odd count: every query's last item is a tail
    item); candidate 22 shares a sentence with query 0 (item 33: the middle of wave 1's run at four waves)"""
    g = torch.Generator().manual_seed(41)
    queries = [torch.randn(l, 768, generator=g) for l in (16, 9, 5)]
    cands = _docs(g, 41, 1, 16, longest_at=17)
    cands[22] = _plant(queries[0], cands[22], 3)
    return queries, cands, {(0, 22)}


def test_tile16_cross_several_queries(amd, cross16):
    """consecutive items of a wave change query (16, 9, 5 rows: the short-query MFMA branch between long-query items) and candidates"""
    queries, cands, planted = cross16
    _cross_case(amd, queries, cands, 2, 'tile16 cross', 41, planted)


def test_tile16_cross_one_query(amd):
    """nq == 1: the index path without the division; 83 candidates, a tail item at the end of wave 1's run"""
    g = torch.Generator().manual_seed(42)
    queries = [torch.randn(13, 768, generator=g)]
    cands = _docs(g, 83, 1, 16, longest_at=5)
    cands[40] = _plant(queries[0], cands[40], 12)
    _cross_case(amd, queries, cands, 2, 'tile16 one query', 42, {(0, 40)})


def test_tile16_cross_caller_diameters(amd, cross16):
    """own_diam false: the query-box loads read the candidate's rows instead and the box term is unused; one diameter per (query,
    group of 64 candidates) from ops.group_diameter, which the oracle is given too"""
    queries, cands, planted = cross16
    _cross_case(amd, queries, cands, 2, 'tile16 caller diameters', 43, planted, diam_group=64)


def test_tile16_cross_centred_rows(amd, cross16):
    """ASPIRE_OT_FLAG_CENTER (set_center_hint(True)) on rows with a common component of 2.0: the staged rows and the query box move by
    the mean of the sixteen staged query rows, stage after stage, item after item"""
    queries, cands, planted = cross16
    amd.ops.set_center_hint(True)
    try:
        _cross_case(amd, [x + 2.0 for x in queries], [x + 2.0 for x in cands], 2, 'tile16 centred', 44, planted)
    finally:
        amd.ops.set_center_hint(False)


def test_tile16_cross_candidate_chunks(amd, cross16):
    """a workspace for 14 of the 41 candidates: launches over the candidates 0 .. 14, 14 .. 28 and 28 .. 41 (cand0 > 0, slots relative
    to the chunk, the last launch with a tail item), each with its own waves"""
    queries, cands, planted = cross16
    _cross_case(amd, queries, cands, 2, 'tile16 chunks', 45, planted, chunk=14)


def test_tile16_cross_max_sim(amd):
    """ops.l2max_scores takes tile16 from 4 096 candidates of one query (score.hip), whatever the pins: 4 097 candidates of 1 .. 16
    rows, 2 049 items -- 512 or 513 per wave at four waves, and two on ONE of the unpinned launch's 2 048 waves"""
    g = torch.Generator().manual_seed(46)
    query = torch.randn(13, 768, generator=g)
    cands = _docs(g, 4097, 1, 16, longest_at=9)
    cands[2048] = _plant(query, cands[2048], 0)
    q, c = amd.ops.DeviceRepSet.from_list([query]), amd.ops.DeviceRepSet.from_list(cands)
    n_items = (4097 + 1) // 2
    _all_runs(n_items, n_items, 'tile16 cross max-sim', unpinned_max=2)
    ref = _call_cross(amd, q, c, '', None, entry='l2max')
    for cap in WAVES:
        got = _call_cross(amd, q, c, '', cap, entry='l2max')
        assert torch.equal(ref, got), (cap, int((ref != got).sum()))
        if cap == 4:
            at4 = got
    small = _call_cross(amd, q, c, 'small', None, entry='l2max')           # the Gram tiles / the per-candidate kernel
    print('tile16 cross max-sim:', int((small != at4).sum()), 'of 4097 scores differ in bits from OT_FORM = small')
    assert not torch.equal(small, at4), 'the streaming kernel did not run'
    assert float(at4[0, 2048]) == 0.0                                   # a shared sentence: exactly 0 from the direct formula
    _check_l2max(at4.cpu().numpy().reshape(-1), [query], [cands], 'tile16 cross max-sim')


# ---- batched jobs (MAPPED) -------------------------------------------------------------------------------------------------------
def _batched_case(amd, b, form, items, bound, per, label, seed, planted=(), wants=WANTS, caps=WAVES, unpinned_max=1, sample=None,
                  small_form='small'):
    """ops.ot_rank_batch on the jobs `b` under OT_FORM = form: (a) for every want, scores and lists; (b) for SIMILARITY and DISTANCE.
    items: per item its real pairs (a host model of the launch), or their count where the order is the device's (REC)"""
    n_items = items if isinstance(items, int) else len(items)
    runs = _all_runs(n_items, bound, label, caps, unpinned_max)
    few = min(caps)
    at_few = {}
    for want in wants:
        ref = _call_batch(amd, b, _pins(form, None), 0, want)
        assert torch.isfinite(ref[0]).all()
        for cap in caps:
            got = _call_batch(amd, b, _pins(form, cap), 0, want)
            _assert_same(ref, got, (label, want, cap))
            if cap == few:
                at_few[want] = got
    if small_form is not None:
        small = _call_batch(amd, b, _pins(small_form, None), 0, 'SIMILARITY')[0]
        n_diff = int((small != at_few['SIMILARITY'][0]).sum())
        print(f'{label}: {n_diff} of {small.numel()} scores differ in bits from OT_FORM = {small_form}')
        assert n_diff > 0, f'OT_FORM = {form or "default"} ran the kernels of OT_FORM = {small_form}'
    if sample is None:
        must = set(planted) | (set(_ends_of_jobs(b.sizes)) if isinstance(items, int) else _must(items, runs[few], b.sizes, per))
        sample = _sample(b.sizes, must, seed)
    for want, sign in (('SIMILARITY', 1.0), ('DISTANCE', -1.0)):
        _check_oracle(b.oracle, b.pair, at_few[want][0].cpu().numpy(), b.flat, sample, sign, f'{label} [{want}]', planted)
    return runs, at_few


def _l2max_case(amd, b, form, n_items, bound, label, caps=WAVES, unpinned_max=1, small_form='small'):
    """ops.l2max_rank_batch on the same frame: (a) scores and lists, (b) every pair against float64"""
    _all_runs(n_items, bound, label, caps, unpinned_max)
    ref = _call_batch(amd, b, _pins(form, None), 0, entry='l2max')
    for cap in caps:
        got = _call_batch(amd, b, _pins(form, cap), 0, entry='l2max')
        _assert_same(ref, got, (label, cap))
        if cap == min(caps):
            at_few = got[0]
    if small_form is not None:
        small = _call_batch(amd, b, _pins(small_form, None), 0, entry='l2max')[0]
        n_diff = int((small != at_few).sum())
        print(f'{label}: {n_diff} of {small.numel()} scores differ in bits from OT_FORM = {small_form}')
        assert n_diff > 0, f'OT_FORM = {form or "default"} ran the kernels of OT_FORM = {small_form}'
    _check_l2max(at_few.cpu().numpy(), b.queries, b.pools, label)
    return at_few


@pytest.fixture(scope='module')
def jobs16(amd):
    """JOBS16 with queries of 3 .. 16 rows (six of them longer than 8: the query branch changes from item to item) and candidates of
    1 .. 16; candidate 13 of job 5 shares a sentence with its query"""
    g = torch.Generator().manual_seed(51)
    queries = [torch.randn(l, 768, generator=g) for l in (16, 5, 9, 3, 12, 8, 4, 16, 7, 10, 14)]
    pools = [_docs(g, n, 1, 16) for n in JOBS16]
    pools[3][0] = torch.randn(16, 768, generator=g)
    pools[5][13] = _plant(queries[5], pools[5][13], 2)
    return _Jobs(amd, queries, pools)


def test_tile16_mapped(amd, jobs16):
    """items = halves of the job tables' groups of four: 2 * sum ceil(n_j / 4); 97 pairs, all of them to the oracle"""
    items = _mapped_items(JOBS16, 2)
    assert len(items) == 2 * sum((n + 3) // 4 for n in JOBS16) and any(len(it) == 0 for it in items) and any(len(it) == 1 for it in items)
    bound = 2 * len(JOBS16) * ((max(JOBS16) + 3) // 4)          # launch_cost_stage: 2 * jobs * max_job_groups
    _batched_case(amd, jobs16, 'tile', items, bound, 2, 'tile16 mapped', 51, {(5, 13)})


def test_tile16_mapped_max_sim(amd, jobs16):
    n_items = 2 * sum((n + 3) // 4 for n in JOBS16)
    bound = 2 * len(JOBS16) * ((max(JOBS16) + 3) // 4)          # aspire_l2max_rank_batch_f32: 2 * groups_bound
    at4 = _l2max_case(amd, jobs16, 'tile', n_items, bound, 'tile16 mapped max-sim')
    assert float(at4[jobs16.flat(5, 13)]) == 0.0


@pytest.fixture(scope='module')
def hybrid(amd):
    """HYBRID: documents of 1 .. 8 rows, up to 23 of 9 .. 16 rows scattered over jobs 0 .. 6, and job 7 (20 candidates) with a query of 12
    rows: at most 43 long pairs of 6 085 (the census' limit: C / 24 = 253)"""
    g = torch.Generator().manual_seed(61)
    queries = [torch.randn(l, 768, generator=g) for l in (8, 3, 5, 8, 1, 6, 7, 12)]
    pools = [_docs(g, n, 1, 8) for n in HYBRID]
    long_at = [(0, 0), (2, 124), (0, 1023), (6, 540)]       # (items 0 and 1024: both on wave 0 at 64 and at 256 waves)
    long_at += [(int(j), int(i)) for j, i in zip(torch.randint(0, 7, (18,), generator=g),
                                                                                 torch.randint(1, 540, (18,), generator=g))]
    for t, (j, i) in enumerate(long_at):
        pools[j][i] = torch.randn(9 + t % 8, 768, generator=g)
    pools[3][77] = _plant(queries[3], torch.randn(11, 768, generator=g), 4)       # a long pair that shares a sentence
    b = _Jobs(amd, queries, pools)
    b.long = sorted({(j, i) for j, p in enumerate(pools) for i, d in enumerate(p) if len(d) > 8 or len(queries[j]) > 8})
    return b


def _hybrid_model(b, label):
    """the hybrid's tile16 launch: 3 044 items on min(4096, TILE_WAVES) waves; an item is worked on where it holds a long pair"""
    J, C = len(HYBRID), sum(HYBRID)
    groups_bound = J * ((max(HYBRID) + 3) // 4)
    assert groups_bound >= 2048 and C >= 6000 and max(len(x) for x in b.queries) > 8 and len(b.long) <= C // 24      # score.hip: hybrid, gate_limit
    items = _mapped_items(HYBRID, 2)
    runs = _all_runs(len(items), 2 * groups_bound, label, caps=(64, 256), unpinned_max=2)
    long = set(b.long)
    work = [any(p in long for p in it) for it in items]
    for cap in (64, 256):
        # some wave works on an item, skips some, and works on one again; most of what a wave meets is skipped
        assert any(work[u] and not work[v] and any(work[w] for w in run[t + 2:]) for run in runs[cap]
                   for t, (u, v) in enumerate(zip(run, run[1:])))
        print(f'{label}: at TILE_WAVES {cap}, {sum(work)} of {len(items)} items hold a long pair; '
              f'{sum(1 for run in runs[cap] if any(work[u] for u in run))} of {len(runs[cap])} waves work on one')
    assert sum(work) * 20 < len(items)
    return len(items), 2 * groups_bound


def test_hybrid_few_long_pairs(amd, hybrid):
    """default form: the fused kernel scores the short pairs, tile16 (selective) walks every item and `continue`s past those without
    a long pair -- after `next` has been advanced.  Oracle: every long pair and 60 short ones"""
    b = hybrid
    n_items, bound = _hybrid_model(b, 'hybrid')
    short = [p for p in _sample(b.sizes, set(), 61, n=400) if p not in set(b.long)][:60]
    assert len(short) == 60
    _, at_few = _batched_case(amd, b, '', n_items, bound, 2, 'hybrid', 61, {(3, 77)}, wants=('SIMILARITY', 'DISTANCE'), caps=(64, 256),
                              unpinned_max=2, sample=sorted(set(b.long) | set(short)), small_form='tile')


def test_hybrid_few_long_pairs_max_sim(amd, hybrid):
    b = hybrid
    n_items, bound = _hybrid_model(b, 'hybrid max-sim')
    # (the fused max-sim kernel and tile16 may agree in every bit on short pairs: the route is the rule's conditions, _hybrid_model)
    at_few = _l2max_case(amd, b, '', n_items, bound, 'hybrid max-sim', caps=(64, 256), unpinned_max=2, small_form=None)
    assert float(at_few[b.flat(3, 77)]) == 0.0


# ---- record items (REC) ----------------------------------------------------------------------------------------------------------
def _rec_jobs(amd, seed, q_lens, cmax, plant):
    g = torch.Generator().manual_seed(seed)
    queries = [torch.randn(l, 768, generator=g) for l in q_lens]
    pools = [_docs(g, n, 1, cmax) for n in JOBS_REC]
    pools[0][0] = torch.randn(cmax, 768, generator=g)             # the longest document is present
    j, i = plant
    pools[j][i] = _plant(queries[j], pools[j][i], 1)
    if sum(len(d) <= 16 for d in pools[0]) % 2 == 0:                # job 0 gets an odd number of narrow candidates
        pools[0][1] = torch.randn(cmax - 1 if len(pools[0][1]) <= 16 else 7, 768, generator=g)
    return _Jobs(amd, queries, pools)


def _rec_model(b, both_halves):
    n_items, odd = _rec_items([len(x) for x in b.queries], b.pools)
    lens = [len(d) for p in b.pools for d in p]
    assert odd and any(l > 16 for l in lens) and any(l <= 16 for l in lens)
    assert not both_halves or (any(len(x) > 16 for x in b.queries) and any(len(x) <= 16 for x in b.queries))
    return n_items, 2 * _chunk_items_bound(len(JOBS_REC), sum(JOBS_REC), max(JOBS_REC))


@pytest.mark.parametrize('tw,q_lens', [(3, (12, 20, 5, 24, 16)), (4, (16, 32, 7, 20, 9))])
def test_rec_items(amd, tw, q_lens):
    """whole abstracts of up to 8 * tw rows on both sides: queries of <= 16 rows (one half) and of more (two), narrow candidates in
    pairs, wide ones over both slots of a wave, an odd narrow count -- wide / crow0 / qrow0 change from item to item"""
    b = _rec_jobs(amd, 70 + tw, q_lens, 8 * tw, (3, 6))
    assert max(max(len(x) for x in b.queries), max(len(d) for p in b.pools for d in p)) == 8 * tw
    n_items, bound = _rec_model(b, True)
    _batched_case(amd, b, 'chunk', n_items, bound, 2, f'rec tw {tw}', 70 + tw, {(3, 6)})


def test_rec_items_max_sim(amd):
    """queries of 9 .. 16 rows against candidates of up to 32 (a query of more than 16 keeps the per-candidate kernel)"""
    b = _rec_jobs(amd, 75, (9, 16, 12, 13, 10), 32, (3, 6))
    n_items, bound = _rec_model(b, False)
    at4 = _l2max_case(amd, b, 'chunk', n_items, bound, 'rec max-sim')
    assert float(at4[b.flat(3, 6)]) == 0.0


# ---- documents of <= 8 rows: pair_tile_kernel --------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cross8():
    g = torch.Generator().manual_seed(81)
    queries = [torch.randn(l, 768, generator=g) for l in (8, 3, 1)]
    cands = _docs(g, 50, 1, 8, longest_at=11)
    cands[26] = _plant(queries[0], cands[26], 5)
    return queries, cands, {(0, 26)}


def test_pair_tile_cross_several_queries(amd, cross8):
    """3 queries x 50 candidates of 1 .. 8 rows: 39 items of four candidates, the last group of two"""
    queries, cands, planted = cross8
    _cross_case(amd, queries, cands, 4, 'pair_tile cross', 81, planted)


def test_pair_tile_cross_one_query(amd):
    g = torch.Generator().manual_seed(82)
    queries = [torch.randn(6, 768, generator=g)]
    cands = _docs(g, 70, 1, 8, longest_at=3)
    cands[33] = _plant(queries[0], cands[33], 0)
    _cross_case(amd, queries, cands, 4, 'pair_tile one query', 82, {(0, 33)})


def test_pair_tile_cross_caller_diameters(amd, cross8):
    queries, cands, planted = cross8
    _cross_case(amd, queries, cands, 4, 'pair_tile caller diameters', 83, planted, diam_group=64)


def test_pair_tile_mapped(amd):
    """the BOUNDS job sizes of tests/test_gpu_fused_wave_runs.py: a wave's run crosses job boundaries, empty jobs and tail groups"""
    g = torch.Generator().manual_seed(84)
    queries = _docs(g, len(BOUNDS), 1, 8)
    pools = [_docs(g, n, 1, 8) for n in BOUNDS]
    pools[4][30] = _plant(queries[4], pools[4][30], 0)
    b = _Jobs(amd, queries, pools)
    items = _mapped_items(BOUNDS, 4)
    bound = len(BOUNDS) * ((max(BOUNDS) + 3) // 4)              # launch_cost_stage: jobs * max_job_groups
    _batched_case(amd, b, 'tile', items, bound, 4, 'pair_tile mapped', 84, {(4, 30)})
