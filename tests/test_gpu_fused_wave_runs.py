"""The fused otAspire kernels (fused.hip, fused_kernel_body.h, fused_solve.h) with SEVERAL units per wave.  A wave of these kernels
is persistent and carries state from one item into the next -- the context fetched one item ahead, the previous item's solve
sliced through the current item's stages, the cached query box, Solve16's stash of three sub-items, the stage buffer that
Solve16 borrows -- and at the sizes of the other suites nearly every wave gets one item, so none of that carry-over runs.  Here
FUSED_WAVES caps the launch at 4 .. 20 waves, which puts tens of items through each wave, across job boundaries.

Two properties, for every kernel form:
 (a) wave-count invariance, bit for bit: the same call under FUSED_WAVES = 4, 8, 12, 20 and unpinned (at least one wave per unit
     at these sizes) gives torch.equal scores, top-k scores and top-k indices, for SIMILARITY, DISTANCE and PLAN_SIM;
 (b) parity with the oracle in the few-waves regime: the FUSED_WAVES = 4 run against oracle.aspire_oracle.get_similarity at the
     suite's 1e-4 absolute (tests/test_gpu_batch.py: TOL), on a seeded sample of >= 300 pairs (every pair
     where a case has fewer) that holds the first and last real candidate of every job and the first and last item of every
     wave's run; the max-sim forms against float64 -cdist from direct differences, maximum over the valid block, every pair.
     PLAN_SIM is held by (a) alone (its own bar: tests/plan_sim_floor.py).

Every test works out on the host how many units (items of four candidates, Solve16 super-items of sixteen, CHUNK items) each
wave receives, from the sizes and the launch rules of fused.hip / fused_kernel_body.h, and asserts that at four waves every wave
gets at least three; by the library's count of Solve16 launches it checks that the pinned form is the one that ran.  Every
batched call writes into views of sentinel-filled buffers (outputs and workspace): the guards must survive and every output
element must have been written."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from oracle import aspire_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-4                       # otAspire / tsAspire against the oracle (tests/test_gpu_batch.py)
K = 10
WAVES = (4, 8, 12, 20)           # FUSED_WAVES pins; None = unpinned
CAP = 256 * 8                    # fused.hip: the launch's waves without a pin
SAMPLE = 300
GUARD = 256                      # guard elements (bytes for the workspace) on either side of every buffer
F32_SENTINEL = 12345.5
I64_SENTINEL = 0x5A5A5A5A5A5A5A5A
U8_SENTINEL = 0xA5
WANTS = ('SIMILARITY', 'DISTANCE', 'PLAN_SIM')
BOUNDS = [16, 1, 0, 33, 64, 17, 0, 0, 5, 48, 100, 15, 31, 4, 3]      # job sizes: boundaries, empty jobs, partial super-items

# batched forms: pins beside OT_FORM = fused, Solve16 launches per call, candidates per unit, how a wave's units are chosen
FORMS = {
    'self16': (dict(FUSED_SOLVE16=0), 0, 4, 'run'),                   # SELF, sixteen lanes per pair: a run of consecutive items
    'solve16': (dict(FUSED_SOLVE16=1), 1, 16, 'run'),                 # SELF, Solve16: a run of consecutive super-items
    'tables': (dict(FUSED_SOLVE16=0, FUSED_NOSELF=1), 0, 4, 'stride'),      # tables launch + table-driven kernel: every n-th item
}


@pytest.fixture(scope='module')
def amd():
    from aspire_amd import ops, _lib
    assert torch.cuda.is_available()
    ops.set_center_hint(False)          # one arithmetic for every call of the module (no sampling of the rows)
    yield type('NS', (), dict(ops=ops, lib=_lib, pinned=_lib.pinned))
    ops.set_center_hint(None)


# ---- the launch rules, on the host ---------------------------------------------------------------------------------------------
def _launch_waves(bound, cap):
    """fused.hip: min(bound, cap) waves, rounded up to whole workgroups of four"""
    return 4 * ((min(bound, cap or CAP) + 3) // 4)


def _runs(n_units, n_waves, split):
    """wave -> the units it receives, in its order.  'run' (fused_kernel_body.h, the SELF split): wave w takes base + (w < rem)
    consecutive units; 'stride': every n_waves-th unit"""
    if split == 'stride':
        return [list(range(w, n_units, n_waves)) for w in range(n_waves)]
    base, rem = divmod(n_units, n_waves)
    return [list(range(w * base + min(w, rem), w * base + min(w, rem) + base + (1 if w < rem else 0))) for w in range(n_waves)]


def _all_runs(n_units, bound, split, label):
    """runs per wave count; the suite's reason to exist, asserted: >= 3 units per wave at four waves, <= 1 unpinned"""
    runs = {cap: _runs(n_units, _launch_waves(bound, cap), split) for cap in WAVES + (None,)}
    said = []
    for cap, r in runs.items():
        counts = [len(x) for x in r]
        assert sorted(u for x in r for u in x) == list(range(n_units))
        said.append(f'{cap or "unpinned"}: {min(counts)}..{max(counts)} on {len(r)}')
    print(f'{label}: {n_units} units; per wave at FUSED_WAVES ' + ', '.join(said))
    assert len(runs[4]) == 4 and min(len(x) for x in runs[4]) >= 3, 'four waves no longer get three units each'
    assert max(len(x) for x in runs[None]) <= 1, 'unpinned, a wave gets more than one unit'
    return runs


def _chunk_items(lens):
    """items chunk_prep_kernel (batch_prep.hip) makes of one job's candidates: [4], [3, 1], [2, 2], one [2, 1, 1], [1, 1, 1, 1]"""
    n = [0, 0, 0, 0]
    for l in lens:
        n[min(4, max(1, (l + 7) >> 3)) - 1] += 1
    n1, n2, n3, n4 = n
    s3 = min(n1, n3)
    odd2 = n2 & 1
    s2 = min(n1 - s3, 2) if odd2 else 0
    return n4 + n3 + (n2 >> 1) + odd2 + ((n1 - s3 - s2 + 3) >> 2)


# ---- calls ---------------------------------------------------------------------------------------------------------------------
def _launches(amd):
    buf = ctypes.create_string_buffer(64)
    amd.lib.check(amd.lib.lib.aspire_debug_get(b'FUSED_SOLVE16_LAUNCHES', buf, len(buf)))
    return int(buf.value)


def _guarded(n, dtype, sentinel):
    """a contiguous [n] view in the middle of a larger buffer, all of it (the view too) filled with `sentinel`"""
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device='cuda')
    return whole, whole[GUARD:GUARD + n], sentinel


def _guards_intact(buf):
    whole, view, sentinel = buf
    n = view.numel()
    return bool((whole[:GUARD] == sentinel).all()) and bool((whole[GUARD + n:] == sentinel).all())


class _Batch:
    """J jobs: queries [J], pools [J][n_j]; `oracle` caches reference values per (job, candidate) -- a batch made of another one's
    jobs (prefix) shares it: a pair's reference does not depend on its batch"""

    def __init__(self, amd, queries, pools, oracle=None):
        self.queries, self.pools = queries, pools
        self.sizes = [len(p) for p in pools]
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.q = amd.ops.DeviceRepSet.from_list(queries)
        self.c = amd.ops.DeviceRepSet.from_list([d for p in pools for d in p])
        self.job_off = torch.tensor(self.off, dtype=torch.int32).cuda()
        self.max_job = max(self.sizes)
        self.oracle = {} if oracle is None else oracle
        assert len(pools) <= 64 and self.c.n <= 1600

    def prefix(self, amd, jobs):
        return _Batch(amd, self.queries[:jobs], self.pools[:jobs], self.oracle)

    def units(self, per):
        """the launch's units in the kernel's order: (job, first candidate, end) -- whole jobs one after the other"""
        return [(j, lo, min(lo + per, n)) for j, n in enumerate(self.sizes) for lo in range(0, n, per)]

    def bound(self, form):
        groups = len(self.sizes) * ((self.max_job + 3) // 4)        # score.hip: groups_bound
        return (groups + 3) // 4 + len(self.sizes) if form == 'solve16' else groups     # fused.hip: supers


def _call_batch(amd, b, pins, launches, want='SIMILARITY', entry='ot'):
    """one batched call, every output and the workspace inside sentinel guards -> clones of (scores, top scores, top indices)"""
    lib = amd.lib.lib
    J, C = b.q.n, b.c.n
    qs, cs = b.q.struct(), b.c.struct()
    ws_fn = lib.aspire_ot_rank_batch_workspace_bytes if entry == 'ot' else lib.aspire_l2max_rank_batch_workspace_bytes
    need = int(ws_fn(ctypes.byref(qs), ctypes.byref(cs), b.max_job, K))
    bufs = [_guarded(C, torch.float32, F32_SENTINEL), _guarded(J * K, torch.float32, F32_SENTINEL),
            _guarded(J * K, torch.int64, I64_SENTINEL), _guarded(need, torch.uint8, U8_SENTINEL)]
    s, ts, ti, ws = bufs[0][1], bufs[1][1].view(J, K), bufs[2][1].view(J, K), bufs[3][1]
    assert ws.data_ptr() % 16 == 0
    before = _launches(amd)
    with amd.pinned(**pins):
        if entry == 'ot':
            amd.ops.ot_rank_batch(b.q, b.c, b.job_off, b.max_job, K, want=getattr(amd.lib, 'OT_' + want), out=(s, ts, ti), workspace=ws)
        else:
            amd.ops.l2max_rank_batch(b.q, b.c, b.job_off, b.max_job, K, out=(s, ts, ti), workspace=ws)
        torch.cuda.synchronize()
    assert _launches(amd) - before == launches, 'the pinned form did not run'
    for buf, what in zip(bufs, ('scores', 'top scores', 'top indices', 'workspace')):
        assert _guards_intact(buf), (what, 'written outside its bounds', pins)
    # every candidate's score and every list entry written (no similarity, distance or index is anywhere near the sentinels)
    assert not bool((s == F32_SENTINEL).any()), ('scores left unwritten', int((s == F32_SENTINEL).sum()), pins)
    assert not bool((ts == F32_SENTINEL).any()) and not bool((ti == I64_SENTINEL).any()), ('lists left unwritten', pins)
    return s.clone(), ts.clone(), ti.clone()


def _pins(form_pins, cap, ot_form='fused', **more):
    return dict(OT_FORM=ot_form, FUSED_WAVES=cap if cap else '', **form_pins, **more)


def _eq_nan(x, y):
    return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0))


def _assert_same(ref, got, label, nan_ok=False):
    """bit for bit; nan_ok: a NaN equals a NaN in the same place (the re-solve case's PLAN_SIM alone)"""
    for r, g, what in zip(ref, got, ('scores', 'top scores', 'top indices')):
        same = _eq_nan(r, g) if nan_ok and r.is_floating_point() else torch.equal(r, g)
        assert same, (label, what, int((r != g).sum()), r.numel())


# ---- references ----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _one_thread():
    """the oracle is a few thousand tiny tensor operations per pair: one thread runs them three times as fast as a pool"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _sample(pair_count, must, seed):
    """`must` + seeded further pairs up to SAMPLE (every pair where there are fewer); pair_count: per job (or query), its candidates.
    The further pairs are a prefix of ONE seeded order of all pairs, so that forms sharing a batch share most of their sample."""
    every = [(j, i) for j, n in enumerate(pair_count) for i in range(n)]
    order = np.random.default_rng(seed).permutation(len(every))
    picked = set(must)
    assert picked <= set(every)
    for t in order:
        if len(picked) >= min(SAMPLE, len(every)):
            break
        picked.add(every[t])
    return sorted(picked)


def _ends_of_jobs(sizes):
    return {(j, i) for j, n in enumerate(sizes) if n for i in (0, n - 1)}


def _ends_of_runs(runs, cands_of_unit):
    """the candidates of the first and the last ITEM (of four) of every wave's run; cands_of_unit(u) -> [(job, candidate)] in order"""
    must = set()
    for run in runs:
        if run:
            must |= set(cands_of_unit(run[0])[:4])
            last = cands_of_unit(run[-1])
            must |= set(last[4 * ((len(last) - 1) // 4):])
    return must


def _check_oracle(cache, doc_pair, scores, flat, sample, sign, label):
    """scores[flat(j, i)] of the sample against sign * get_similarity; prints the worst error before it asserts"""
    with _one_thread():
        for key in sample:
            if key not in cache:
                cache[key] = float(orc.get_similarity(*doc_pair(*key)))
    got = np.array([scores[flat(j, i)] for j, i in sample], dtype=np.float64)
    err = np.abs(sign * got - np.array([cache[k] for k in sample]))
    print(f'{label}: worst oracle error {err.max():.3e} over {len(sample)} pairs (at {sample[int(err.argmax())]})')
    assert np.isfinite(got).all() and err.max() <= TOL, (label, sample[int(err.argmax())], float(err.max()))


def _l2max_ref(q, c):
    """-cdist from direct differences in float64, maximum over the valid block"""
    d = (q.double()[:, None, :] - c.double()[None, :, :]).pow(2).sum(-1).sqrt()
    return -float(d.min())


# ---- batches -------------------------------------------------------------------------------------------------------------------
def _docs(g, n, smin=1, smax=8, scale=1.0):
    return [scale * torch.randn(int(l), 768, generator=g) for l in torch.randint(smin, smax + 1, (n,), generator=g)]


def _make(amd, name):
    if name == 'bounds':
        # a wave's run crosses job boundaries, steps over empty jobs and meets partial super-items (1, 3, 4, 5, 15, 17 candidates)
        # between full ones; 352 items / 108 super-items: multiples of 4 and 8 / of 4 and 12 waves, not of the other counts
        g = torch.Generator().manual_seed(1)
        sizes = BOUNDS * 4
        return _Batch(amd, _docs(g, len(sizes)), [_docs(g, n) for n in sizes])
    if name == 'neighbours':
        # consecutive jobs differ in everything a wave could carry over: query lengths 1, 8, 3, 8, 1, 5, ragged candidates, and
        # the whole job scaled by 0.05, 1, 20 (diameters and with them step counts change from one item to the next).  The base rows
        # are N(0, 1 / 768) -- unit length, as sentence embeddings are: the x 20 jobs then have the distances (~28) of the N(0, 1)
        # rows for which the suite's 1e-4 absolute bar was set; on N(0, 1) rows x 20 one fp32 ulp of a score is 6e-5
        g = torch.Generator().manual_seed(2)
        sizes = [37, 16, 5, 64, 1, 23] * 5
        qlens = [1, 8, 3, 8, 1, 5] * 5
        scales = [(0.05, 1.0, 20.0)[j % 3] / 768 ** 0.5 for j in range(len(sizes))]
        queries = [s * torch.randn(l, 768, generator=g) for l, s in zip(qlens, scales)]
        return _Batch(amd, queries, [_docs(g, n, scale=s) for n, s in zip(sizes, scales)])
    if name == 'box':
        # both halves of the box cache: a job long enough that a wave stays inside it for several units (box from the cache), then
        # a one-candidate job (box formed afresh on the next unit)
        g = torch.Generator().manual_seed(3)
        sizes = [120, 1, 64, 1, 90, 1, 33, 1]
        return _Batch(amd, _docs(g, len(sizes)), [_docs(g, n) for n in sizes])
    if name == 'centred':
        # rows with a large common component (tests/test_gpu_round3.py): ASPIRE_OT_FLAG_CENTER moves the staged rows by the query's mean
        g = torch.Generator().manual_seed(4)
        base = 2.0 * torch.randn(768, generator=g)
        sizes = BOUNDS * 2
        return _Batch(amd, [d + base for d in _docs(g, len(sizes))], [[d + base for d in _docs(g, n)] for n in sizes])
    if name in ('resolve', 'resolve-plain'):
        # tests/test_gpu_fused_solve16.py, test_poisoned_pairs_reach_the_re_solve: 3 x N(0, 1) rows; a candidate that shares a sentence
        # with its query takes the shifted sums out of fp32 range and is solved again in the wave.  12 jobs x 48: at four waves a
        # wave's run is three whole jobs under either form; planted in the first, a middle and the last unit of a run
        g = torch.Generator().manual_seed(5)
        queries = [3.0 * torch.randn(8, 768, generator=g) for _ in range(12)]
        pools = [[3.0 * torch.randn(8, 768, generator=g) for _ in range(48)] for _ in range(12)]
        if name == 'resolve':
            g2 = torch.Generator().manual_seed(50)
            for job, pos in RESOLVE_PLANTED:
                pools[job][pos] = torch.cat([queries[job][:1], 3.0 * torch.randn(pos % 7 + 1, 768, generator=g2)])
        return _Batch(amd, queries, pools)
    raise KeyError(name)


RESOLVE_PLANTED = [(0, 0), (3, 1), (4, 21), (5, 46), (11, 47)]


@pytest.fixture(scope='module')
def batches(amd):
    """name -> its _Batch, formed once and kept (device rows and oracle values) until this module is done"""
    cache = {}

    def get(name):
        if name not in cache:
            if name == 'bounds-2':                  # the same jobs without the last two: unit counts that four waves do not divide
                cache[name] = get('bounds').prefix(amd, len(BOUNDS) * 4 - 2)
            else:
                cache[name] = _make(amd, name)
        return cache[name]
    yield get
    cache.clear()


def _batched_case(amd, b, form, label, wants=WANTS, oracle=True, nan_ok=()):
    """(a) for every want, (b) for SIMILARITY and DISTANCE, of batch `b` on batched form `form`; returns the runs per wave count and
    the four-wave outputs per want"""
    form_pins, launches, per, split = FORMS[form]
    units = b.units(per)
    runs = _all_runs(len(units), b.bound(form), split, f'{label} [{form}]')
    at4 = {}
    for want in wants:
        ref = _call_batch(amd, b, _pins(form_pins, None), launches, want)
        for cap in WAVES:
            got = _call_batch(amd, b, _pins(form_pins, cap), launches, want)
            _assert_same(ref, got, (label, form, want, cap), want in nan_ok)
            if cap == 4:
                at4[want] = got
    if oracle:
        def cands(u):
            j, lo, hi = units[u]
            return [(j, i) for i in range(lo, hi)]
        sample = _sample(b.sizes, _ends_of_jobs(b.sizes) | _ends_of_runs(runs[4], cands), 7)
        for want, sign in (('SIMILARITY', 1.0), ('DISTANCE', -1.0)):
            if want in at4:
                _check_oracle(b.oracle, lambda j, i: (b.queries[j], b.pools[j][i]), at4[want][0].cpu().numpy(),
                              lambda j, i: int(b.off[j]) + i, sample, sign, f'{label} [{form}, {want}]')
    return runs, at4


# ---- batched forms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['bounds', 'bounds-2'])
@pytest.mark.parametrize('form', list(FORMS))
def test_job_boundaries_inside_a_run(amd, batches, form, name):
    """BOUNDS x 4: runs that cross several job boundaries and empty jobs; 'bounds' has unit counts that four waves divide
    (rem == 0 in the SELF split), 'bounds-2' has not, and the other wave counts give both as well"""
    b = batches(name)
    runs, _ = _batched_case(amd, b, form, name)
    if FORMS[form][3] == 'run':
        n_units = sum(len(r) for r in runs[4])
        assert (n_units % 4 == 0) == (name == 'bounds')
        assert name != 'bounds' or {n_units % len(runs[cap]) == 0 for cap in WAVES} == {True, False}
        # a run at four waves crosses job boundaries and empty jobs
        units = b.units(FORMS[form][2])
        for run in runs[4]:
            jobs = sorted({units[u][0] for u in run})
            assert len(jobs) >= 5 and any(b.sizes[j] == 0 for j in range(jobs[0], jobs[-1]))


@pytest.mark.parametrize('form', list(FORMS))
def test_neighbours_that_differ(amd, batches, form):
    """a stale q_len, query box, stash entry, step count or slice from the previous job changes a score by far more than the bar"""
    _batched_case(amd, batches('neighbours'), form, 'neighbours')


@pytest.mark.parametrize('form', ['self16', 'solve16'])
def test_both_halves_of_the_box_cache(amd, batches, form):
    b = batches('box')
    runs, _ = _batched_case(amd, b, form, 'box')
    units = b.units(FORMS[form][2])
    # some wave meets at least three units of one long job in a row and then a one-candidate job
    assert any(units[u][0] == units[v][0] == units[w][0] and b.sizes[units[x][0]] == 1
               for run in runs[4] for u, v, w, x in zip(run, run[1:], run[2:], run[3:]))


@pytest.mark.parametrize('form', list(FORMS))
def test_centred_rows(amd, batches, form):
    """ASPIRE_OT_FLAG_CENTER (set_center_hint(True)): the staged rows move by the query's mean, item after item"""
    amd.ops.set_center_hint(True)
    try:
        _batched_case(amd, batches('centred'), form, 'centred')
    finally:
        amd.ops.set_center_hint(False)


@pytest.mark.parametrize('form', ['self16', 'solve16'])
def test_re_solve_inside_a_run(amd, batches, form):
    """Poisoned pairs in the first, a middle and the last unit of a wave's run.  With the re-solve off (FUSED_NOREPAIR) the same pairs
    are hit, with the same raw scores, at every wave count; with it on every score is finite and the same bits at every wave count
    (_batched_case); and every OTHER pair has the bits it has in the batch where plain candidates stand in for the planted ones:
    a re-solve leaves nothing behind for the units after it.  PLAN_SIM of a planted pair is NaN -- as it is in the fp32 reference
    (exp((f + g - d) / blur) leaves fp32 range; float64 gives -1e-46): there a NaN must meet a NaN, at the planted pairs alone."""
    b, plain = batches('resolve'), batches('resolve-plain')
    form_pins, launches, per, split = FORMS[form]
    runs, at4 = _batched_case(amd, b, form, 'resolve', oracle=False, nan_ok=('PLAN_SIM',))
    units = b.units(per)
    place = set()
    for job, pos in RESOLVE_PLANTED:
        u = next(t for t, (j, lo, hi) in enumerate(units) if j == job and lo <= pos < hi)
        run = next(r for r in runs[4] if u in r)
        place.add('first' if u == run[0] else 'last' if u == run[-1] else 'middle')
    assert place == {'first', 'middle', 'last'}
    fixed = at4['SIMILARITY'][0]
    assert torch.isfinite(fixed).all()
    hits = {}
    for cap in (None,) + WAVES:
        raw = _call_batch(amd, b, _pins(form_pins, cap, FUSED_NOREPAIR=1), launches)[0]
        hits[cap] = (~torch.isfinite(raw) | (raw != fixed), raw)
    print(f'resolve [{form}]: poisoned pairs', int(hits[None][0].sum()))
    assert int(hits[None][0].sum()) >= 1
    for cap in WAVES:
        assert torch.equal(hits[cap][0], hits[None][0]) and _eq_nan(hits[cap][1], hits[None][1]), cap
    other = torch.ones(b.c.n, dtype=torch.bool, device='cuda')
    for job, pos in RESOLVE_PLANTED:
        other[int(b.off[job]) + pos] = False
    assert not bool((hits[None][0] & other).any())          # only planted pairs are poisoned
    assert torch.isfinite(at4['DISTANCE'][0]).all() and torch.isfinite(at4['PLAN_SIM'][0][other]).all()
    for cap in (4, 12, None):
        s_plain = _call_batch(amd, plain, _pins(form_pins, cap), launches)[0]
        assert torch.isfinite(s_plain).all()
        assert torch.equal(s_plain[other], fixed[other]), (cap, int((s_plain[other] != fixed[other]).sum()))


@pytest.mark.parametrize('form', list(FORMS))
def test_idle_waves_write_nothing(amd, batches, form):
    """FUSED_WAVES above the unit count, and a value that is no multiple of four (the grid rounds up): waves without a unit, or
    beyond the pinned count, write nothing -- the guards of _call_batch -- and the units' bits stay what they are"""
    b = batches('bounds')
    form_pins, launches, per, split = FORMS[form]
    n_units = len(b.units(per))
    ref = _call_batch(amd, b, _pins(form_pins, None), launches)
    for cap in (401, 10):
        n_waves = _launch_waves(b.bound(form), cap)
        counts = [len(r) for r in _runs(n_units, n_waves, split)]
        print(f'idle [{form}]: FUSED_WAVES={cap}: {n_units} units on {n_waves} waves, {counts.count(0)} idle')
        assert n_waves % 4 == 0 and n_waves >= cap and (cap != 401 or (n_waves > n_units and counts.count(0) >= 40))
        _assert_same(ref, _call_batch(amd, b, _pins(form_pins, cap), launches), (form, cap))


# ---- max-sim -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['self', 'tables'])
@pytest.mark.parametrize('name', ['bounds', 'neighbours'])
def test_l2max_forms(amd, batches, form, name):
    """tsAspire on the same streaming phase (launch_pair_fused_l2max honours FUSED_WAVES): SELF runs and table-driven strides"""
    b = batches(name)
    form_pins, split = (dict(), 'run') if form == 'self' else (dict(FUSED_NOSELF=1), 'stride')
    n_units = len(b.units(4))
    _all_runs(n_units, b.bound('self16'), split, f'l2max {name} [{form}]')
    ref = _call_batch(amd, b, _pins(form_pins, None), 0, entry='l2max')
    for cap in WAVES + (401, 10):
        got = _call_batch(amd, b, _pins(form_pins, cap), 0, entry='l2max')
        _assert_same(ref, got, (name, form, cap))
        if cap == 4:
            at4 = got[0].cpu().numpy().astype(np.float64)
    want = np.array([_l2max_ref(b.queries[j], d) for j, p in enumerate(b.pools) for d in p])
    err = np.abs(at4 - want)
    print(f'l2max {name} [{form}]: worst error against float64 {err.max():.3e} over {len(want)} pairs')
    assert err.max() <= TOL


# ---- one pool: QBOX, CROSS with several queries, caller-supplied diameters ------------------------------------------------------
def _pool_case(amd, queries, cands, label, seed, diam_group=0, oracle=True, wants=WANTS):
    """queries x one pool through ops.ot_rank on the fused kernel: items = (candidate group, query), group-major, every n-th one"""
    nq, C = len(queries), len(cands)
    q, c = amd.ops.DeviceRepSet.from_list(queries), amd.ops.DeviceRepSet.from_list(cands)
    n_items = (C + 3) // 4 * nq
    runs = _all_runs(n_items, n_items, 'stride', label)           # score.hip: groups4_all
    diameter = amd.ops.group_diameter(q, c, amd.lib.PAIR_CROSS, diam_group) if diam_group else None

    def call(cap, want):
        before = _launches(amd)
        with amd.pinned(**_pins({}, cap)):
            out = amd.ops.ot_rank(q, c, K, want=getattr(amd.lib, 'OT_' + want), diameter=diameter, diam_group=diam_group)
            torch.cuda.synchronize()
        assert _launches(amd) == before
        return out
    at4 = {}
    for want in wants:
        ref = call(None, want)
        assert torch.isfinite(ref[0]).all()
        for cap in WAVES:
            got = call(cap, want)
            _assert_same(ref, got, (label, want, cap))
            if cap == 4:
                at4[want] = got
        # the scores alone into a guarded buffer, at a wave count that is no multiple of four
        buf = _guarded(nq * C, torch.float32, F32_SENTINEL)
        with amd.pinned(**_pins({}, 10)):
            amd.ops.ot_sinkhorn(q, c, want=getattr(amd.lib, 'OT_' + want), diameter=diameter, diam_group=diam_group, out=buf[1])
            torch.cuda.synchronize()
        assert _guards_intact(buf) and torch.equal(buf[1].view(nq, C), ref[0]), (label, want)
    if oracle:
        def cands_of(item):
            cg, qi = divmod(item, nq)
            return [(qi, i) for i in range(4 * cg, min(4 * cg + 4, C))]
        cache = {}
        sample = _sample([C] * nq, _ends_of_jobs([C] * nq) | _ends_of_runs(runs[4], cands_of), seed)
        for want, sign in (('SIMILARITY', 1.0), ('DISTANCE', -1.0)):
            _check_oracle(cache, lambda j, i: (queries[j], cands[i]), at4[want][0].cpu().numpy().reshape(-1),
                          lambda j, i: j * C + i, sample, sign, f'{label} [{want}]')


def test_one_query_in_wave_box(amd):
    """QBOX: the box is formed during a wave's first item and read from the LDS cache for every later one; a tail group of three"""
    g = torch.Generator().manual_seed(21)
    _pool_case(amd, _docs(g, 1, 5, 5), _docs(g, 1203), 'qbox', 21)


def test_several_queries_one_pool(amd):
    """CROSS, strided and group-major: consecutive items of a wave change query (1, 8 and 3 rows) and candidate group"""
    g = torch.Generator().manual_seed(22)
    queries = [torch.randn(l, 768, generator=g) for l in (1, 8, 3)]
    _pool_case(amd, queries, _docs(g, 403), 'cross', 22)


def test_caller_supplied_diameters(amd):
    """caching_score's pattern: one diameter per (query, group of 64 candidates) from the caller (own_diam false in the kernel);
    invariance alone -- the per-pair oracle has another schedule"""
    g = torch.Generator().manual_seed(23)
    queries = [torch.randn(l, 768, generator=g) for l in (6, 2)]
    _pool_case(amd, queries, _docs(g, 603), 'diameters', 23, diam_group=64, oracle=False)


# ---- CHUNK ---------------------------------------------------------------------------------------------------------------------
def test_chunk_items(amd):
    """queries of <= 8 rows against candidates of 9 .. 32 (a quarter of them shorter): items of every make-up -- [4], [3, 1], [2, 2],
    [2, 1, 1], [1, 1, 1, 1] -- strided over the waves; which candidates share an item is the preparation kernel's choice, so the
    oracle sees every pair (fewer than 300)"""
    g = torch.Generator().manual_seed(31)
    sizes = [70, 1, 0, 90, 33, 100]
    queries = [torch.randn(l, 768, generator=g) for l in (8, 3, 1, 5, 8, 2)]
    pools = []
    for n in sizes:
        lens = [int(l) if int(t) else int(l) % 8 + 1 for l, t in zip(torch.randint(9, 33, (n,), generator=g), torch.randint(0, 4, (n,), generator=g))]
        pools.append([torch.randn(l, 768, generator=g) for l in lens])
    b = _Batch(amd, queries, pools)
    assert b.c.n < SAMPLE
    J, C = len(sizes), b.c.n
    n_items = sum(_chunk_items([len(d) for d in p]) for p in pools)
    bound = max(C + 3 * J, J * b.max_job)                        # batch_prep.hip: chunk_items_bound, one part and one region per job
    _all_runs(n_items, bound, 'stride', 'chunk')
    at4 = {}
    for want in WANTS:
        ref = _call_batch(amd, b, _pins({}, None, ot_form='chunk'), 0, want)
        for cap in WAVES + (10,):
            got = _call_batch(amd, b, _pins({}, cap, ot_form='chunk'), 0, want)
            _assert_same(ref, got, ('chunk', want, cap))
            if cap == 4:
                at4[want] = got
    sample = _sample(sizes, set(), 31)
    assert len(sample) == C
    for want, sign in (('SIMILARITY', 1.0), ('DISTANCE', -1.0)):
        _check_oracle(b.oracle, lambda j, i: (queries[j], pools[j][i]), at4[want][0].cpu().numpy(), lambda j, i: int(b.off[j]) + i,
                      sample, sign, f'chunk [{want}]')
