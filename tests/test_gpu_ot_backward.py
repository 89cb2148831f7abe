"""GPU: the backward of the otAspire distance (aspire_ot_backward_f32, ops.ot_backward, torch.ops.aspire.ot_pair_scores /
ot_pair_backward, AllPairMaskedWasserstein.compute_distance of aspire_amd.pair_distances) against float64 torch autograd on the CPU
over a restatement of the reference plus geomloss with geomloss's detach pattern (tests/ot_backward_ref.py; geomloss itself is not
available: the gradient is a restatement, as the Sinkhorn oracle is).

Tolerance, per case: the same restatement run in fp32 on the CPU with distances from direct differences is compared with the float64
gradient (geomloss's matmul cost formula); the kernel gets 4 x its largest absolute deviation over the case's pairs (the kernel's
summation orders differ from torch's: 4 is margin for that and nothing else), floored at 1e-6; the fp32 restatement's deviation is
itself asserted to stay below 1e-4.  Rows are 0.3 N(0, 1), pad rows zero.  Measured on the CPU (valid rows):

    case                          CPU fp32 deviation   bound      largest |gradient|   kernel on an MI355X
    (a) 4 pairs, 8 x 8            2.8e-07              1.1e-06    8.0e-02              4.4e-08
    (b) 2 pairs, 40 x 33          1.0e-07              1.0e-06    1.7e-02              3.3e-08
    (c) 1 pair, 128 x 128         1.4e-08              1.0e-06    2.4e-03              5.4e-09
    (d) (a) with coincident rows  2.8e-07              1.1e-06    9.8e-02              4.0e-08
    (f) (a), temp 0.2, blur 0.1   6.2e-07              2.5e-06    2.2e-01              1.6e-07

The kernel's column is one run on an MI355X (NOTES.md, "The backward of the OT distance"; (e), the CSR call, has (a)'s bits: 4.4e-08;
the own-box call 5.4e-08, the triplet loss 7.6e-08 / 5.3e-08 / 6.3e-08 on query / pos / neg).  Solver settings, row scales, diameter
groups and the schedule's discontinuities are in tests/test_gpu_ot_backward_edges.py.  The kernel's solve and the forward's
kernel family differ by rounding; a flip of an arg-max pick j*(i) / i*(j) cannot hide behind the bound: from the reference alone
(float64, CPU) the best and second-best entry of every row and column differ by more than 1e-4 in every case.

Every comparison prints an `OTBWD ...` line before it asserts (pytest -s shows them)."""
import functools

import pytest
import torch

import ot_backward_ref as ref

pytestmark = pytest.mark.gpu
D = 768
# name -> (padded extents (Sq, Sc), [(q_len, c_len)], solver keywords)
CASES = {
    'a': ((8, 8), [(8, 8), (3, 8), (1, 2), (5, 1)], {}),
    'b': ((40, 33), [(40, 33), (17, 9)], {}),                    # crosses the 32-row family boundary of the forward
    'c': ((128, 128), [(128, 128)], {}),                         # the limit
    'd': ((8, 8), [(8, 8), (3, 8), (1, 2), (5, 1)], {}),         # (a) with an equal and a nearly equal row
    'f': ((8, 8), [(8, 8), (3, 8), (1, 2), (5, 1)], dict(temp=0.2, blur=0.1)),
}
SEEDS = {'a': 4100, 'b': 4101, 'c': 4102, 'd': 4100, 'f': 4100}
GS = {'a': [0.9, -1.3, 0.0, 0.6], 'b': [-0.7, 1.2], 'c': [1.1]}          # dLoss / dscore: mixed signs, a zero
GS['d'] = GS['f'] = GS['a']


@pytest.fixture(scope='module')
def amd():
    from aspire_amd import ops, pair_distances, _lib
    import aspire_amd.torch_ops as torch_ops
    assert torch.cuda.is_available()
    return type('NS', (), dict(ops=ops, pd=pair_distances, lib=_lib, to=torch_ops))


def _padded(exts, lens, gen):
    """(x, y) [B, Sq, 768], [B, Sc, 768] fp32: 0.3 N(0, 1) valid rows, zero pad rows"""
    x, y = torch.zeros(len(lens), exts[0], D), torch.zeros(len(lens), exts[1], D)
    for b, (ql, cl) in enumerate(lens):
        x[b, :ql] = 0.3 * torch.randn(ql, D, generator=gen)
        y[b, :cl] = 0.3 * torch.randn(cl, D, generator=gen)
    return x, y


@functools.lru_cache(maxsize=None)
def _inputs(case):
    exts, lens, kw = CASES[case]
    gen = torch.Generator().manual_seed(SEEDS[case])
    x, y = _padded(exts, lens, gen)
    if case == 'd':
        y[0, 0] = x[0, 0]                                                       # d = 0 exactly
        y[0, 1] = x[0, 2] * (1.0 + 3e-4 * torch.randn(D, generator=gen))        # 3e-4 relative noise
    return x, y, [l[0] for l in lens], [l[1] for l in lens], torch.tensor(GS[case]), kw


@functools.lru_cache(maxsize=None)
def _yardstick(case):
    """(float64 grad_x, grad_y, the bound) -- computed once per case, never changed"""
    x, y, ql, cl, gs, kw = _inputs(case)
    # the picks are far from flipping (from the reference alone); in (d) the two built entries ARE the picks, by a wide margin
    gap = ref.pick_margins(x, y, ql, cl)
    assert gap > 1e-4, (case, gap)
    if case == 'd':
        d = torch.cdist(x[0].double(), y[0].double())
        for i, j in ((0, 0), (2, 1)):
            others_row = torch.cat([d[i, :j], d[i, j + 1:]]).min().item()
            others_col = torch.cat([d[:i, j], d[i + 1:, j]]).min().item()
            assert d[i, j] < 1e-2 and others_row > 1.0 and others_col > 1.0, (i, j, d[i, j], others_row, others_col)
    g64 = ref.autograd_grads(x, y, ql, cl, gs, torch.float64, direct=False, **kw)
    g32 = ref.autograd_grads(x, y, ql, cl, gs, torch.float32, direct=True, **kw)
    dev32 = ref.valid_dev(*g32, *g64, ql, cl)
    # fp32 rounding of these gradients is far below this; beyond it the fp32 restatement itself would have gone another way (a
    # pick, a schedule length), and the bound must not grow from that unnoticed
    assert dev32 < 1e-4, (case, dev32)
    tol = max(4.0 * dev32, 1e-6)
    scale = max(g64[0].abs().max().item(), g64[1].abs().max().item())
    print(f'OTBWD yardstick ({case}) pick gap {gap:.3e}, CPU fp32 restatement deviation {dev32:.3e} -> bound {tol:.3e}, '
          f'largest |gradient| {scale:.3e}')
    return g64[0], g64[1], tol


def _nan_like(t):
    return torch.full_like(t, float('nan'))


def _sets(amd, x, y, ql, cl):
    return amd.ops.DeviceRepSet.from_padded(x, ql), amd.ops.DeviceRepSet.from_padded(y, cl)


def _backward(amd, qs, cs, gs, kw, diam=None, want=None, n=None):
    """ops.ot_backward into NaN-filled buffers (a row the kernel does not write shows), with ONE epsilon schedule for the batch as
    AllPairMaskedWasserstein.compute_distance has it (group = batch size); diam: the diameter tensor to use instead"""
    n = qs.n if n is None else n
    if diam is None:
        diam = amd.ops.group_diameter(qs, cs, amd.lib.PAIR_PAIRED, n)
    return amd.ops.ot_backward(qs, cs, gs.cuda(), blur=kw.get('blur', 0.05), scaling=kw.get('scaling', 0.9),
                               sent_sm_temp=kw.get('temp', 1.0), diameter=diam, diam_group=n,
                               want=amd.lib.OT_DISTANCE if want is None else want, out=(_nan_like(qs.rows), _nan_like(cs.rows)))


@pytest.mark.parametrize('case', list(CASES))
def test_padded_backward_matches_float64_autograd(amd, case):
    """(a) (b) (c) (d) (f); (h): pad rows are exactly 0.0; in (d) the gradient on the coincident entry is finite"""
    x, y, ql, cl, gs, kw = _inputs(case)
    g64x, g64y, tol = _yardstick(case)
    qs, cs = _sets(amd, x, y, ql, cl)
    gq, gc = _backward(amd, qs, cs, gs, kw)
    gq, gc = gq.view(x.shape).cpu(), gc.view(y.shape).cpu()
    err = ref.valid_dev(gq, gc, g64x, g64y, ql, cl)
    print(f'OTBWD padded ({case}) kernel |error| {err:.3e}, bound {tol:.3e}')
    assert torch.isfinite(gq).all() and torch.isfinite(gc).all()
    for b in range(len(ql)):
        assert torch.count_nonzero(gq[b, ql[b]:]) == 0 and torch.count_nonzero(gc[b, cl[b]:]) == 0, 'pad rows must be exact zeros'
    assert torch.count_nonzero(gq[2]) == 0 and torch.count_nonzero(gc[2]) == 0 if case in 'adf' else True      # grad_scores[2] == 0
    assert err <= tol


def test_csr_sets_give_the_padded_bits(amd):
    """(e) CSR sets of (a)'s documents, the same diameter: the bits of the padded call on the valid rows, and the yardstick's values"""
    x, y, ql, cl, gs, kw = _inputs('a')
    g64x, g64y, tol = _yardstick('a')
    ps, pc = _sets(amd, x, y, ql, cl)
    diam = amd.ops.group_diameter(ps, pc, amd.lib.PAIR_PAIRED, len(ql))
    pq, pcand = _backward(amd, ps, pc, gs, kw, diam=diam)
    pq, pcand = pq.view(x.shape), pcand.view(y.shape)
    qs = amd.ops.DeviceRepSet.from_list([x[b, :n] for b, n in enumerate(ql)])
    cs = amd.ops.DeviceRepSet.from_list([y[b, :n] for b, n in enumerate(cl)])
    gq, gc = _backward(amd, qs, cs, gs, kw, diam=diam)
    assert torch.equal(gq, torch.cat([pq[b, :n] for b, n in enumerate(ql)]))          # (a row left unwritten is NaN: it fails here)
    assert torch.equal(gc, torch.cat([pcand[b, :n] for b, n in enumerate(cl)]))
    want_q, want_c = torch.cat([g64x[b, :n] for b, n in enumerate(ql)]), torch.cat([g64y[b, :n] for b, n in enumerate(cl)])
    err = max((gq.cpu().double() - want_q).abs().max().item(), (gc.cpu().double() - want_c).abs().max().item())
    print(f'OTBWD csr (a) kernel |error| {err:.3e}, bound {tol:.3e}')
    assert err <= tol


def test_similarity_is_minus_distance_and_runs_repeat(amd):
    """(g) ASPIRE_OT_SIMILARITY = minus the DISTANCE gradient, bit for bit; (i) two runs give equal bits; pad rows are not read"""
    x, y, ql, cl, gs, kw = _inputs('a')
    qs, cs = _sets(amd, x, y, ql, cl)
    diam = amd.ops.group_diameter(qs, cs, amd.lib.PAIR_PAIRED, len(ql))
    first = _backward(amd, qs, cs, gs, kw, diam=diam)
    again = _backward(amd, *_sets(amd, x, y, ql, cl), gs, kw, diam=diam)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    sim = _backward(amd, qs, cs, gs, kw, diam=diam, want=amd.lib.OT_SIMILARITY)
    assert torch.equal(sim[0], -first[0]) and torch.equal(sim[1], -first[1])
    x2, y2 = x.clone(), y.clone()
    for b in range(len(ql)):            # other values in the pad rows, the same diameter: nothing moves
        x2[b, ql[b]:] = 7.0
        y2[b, cl[b]:] = -3.0
    other = _backward(amd, *_sets(amd, x2, y2, ql, cl), gs, kw, diam=diam)
    assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])


def test_own_box_diameter_matches_the_forward_reading(amd):
    """diameter None: every pair's schedule from the box of its own valid rows (the forward's B = 1 reading); against the restatement
    called pair by pair on the unpadded documents, bound by the same recipe on these calls"""
    x, y, ql, cl, gs, kw = _inputs('a')
    qs, cs = _sets(amd, x, y, ql, cl)
    gq, gc = amd.ops.ot_backward(qs, cs, gs.cuda(), out=(_nan_like(qs.rows), _nan_like(cs.rows)))
    gq, gc = gq.view(x.shape).cpu(), gc.view(y.shape).cpu()
    err = dev32 = 0.0
    for b in range(len(ql)):
        xb, yb = x[b:b + 1, :ql[b]], y[b:b + 1, :cl[b]]
        g64 = ref.autograd_grads(xb, yb, ql[b:b + 1], cl[b:b + 1], gs[b:b + 1], torch.float64, direct=False)
        g32 = ref.autograd_grads(xb, yb, ql[b:b + 1], cl[b:b + 1], gs[b:b + 1], torch.float32, direct=True)
        dev32 = max(dev32, ref.valid_dev(*g32, *g64, ql[b:b + 1], cl[b:b + 1]))
        err = max(err, ref.valid_dev(gq[b:b + 1], gc[b:b + 1], *g64, ql[b:b + 1], cl[b:b + 1]))
    assert dev32 < 1e-4
    tol = max(4.0 * dev32, 1e-6)
    print(f'OTBWD own-box (a) kernel |error| {err:.3e}, CPU fp32 restatement deviation {dev32:.3e} -> bound {tol:.3e}')
    assert err <= tol


def test_unsupported_forms_say_so(amd):
    """(j) CROSS, PLAN_SIM and 129 rows raise NotImplementedError"""
    import ctypes
    x, y, ql, cl, gs, kw = _inputs('a')
    qs, cs = _sets(amd, x, y, ql, cl)
    with pytest.raises(NotImplementedError, match='PLAN_SIM'):
        amd.ops.ot_backward(qs, cs, gs.cuda(), want=amd.lib.OT_PLAN_SIM)
    gq, gc = torch.zeros_like(qs.rows), torch.zeros_like(cs.rows)
    prm = amd.lib.OtParams(0.05, 0.9, 1.0, 0, 0)
    a, b = qs.struct(), cs.struct()
    with pytest.raises(NotImplementedError, match='ASPIRE_PAIR_PAIRED'):
        amd.lib.check(amd.lib.lib.aspire_ot_backward_f32(ctypes.byref(a), ctypes.byref(b), D, amd.lib.PAIR_CROSS, ctypes.byref(prm), None, 0,
                                                         amd.lib.OT_DISTANCE, gs.cuda().data_ptr(), gq.data_ptr(), gc.data_ptr(), None))
    long_q = amd.ops.DeviceRepSet.from_padded(torch.zeros(1, 129, D), [129])
    one_c = amd.ops.DeviceRepSet.from_padded(torch.zeros(1, 4, D), [4])
    with pytest.raises(NotImplementedError, match='more than 128 sentence rows'):
        amd.ops.ot_backward(long_q, one_c, torch.ones(1).cuda())
    with pytest.raises(NotImplementedError, match='more than 128 sentence rows'):
        amd.ops.ot_backward(one_c, long_q, torch.ones(1).cuda())


def _lens(ql, cl):
    return torch.tensor(ql, dtype=torch.int32).cuda(), torch.tensor(cl, dtype=torch.int32).cuda()


@pytest.mark.parametrize('case', ['a', 'b'])
def test_differentiable_forward_is_todays_forward(amd, case):
    """(l) ot_pair_scores: the bits of ot_sinkhorn_scores(paired=True), attached to the graph; its backward is the kernel's result"""
    x, y, ql, cl, gs, kw = _inputs(case)
    lq, lc = _lens(ql, cl)
    prm = (kw.get('blur', 0.05), kw.get('scaling', 0.9), kw.get('temp', 1.0), len(ql))
    xg, yg = x.cuda().requires_grad_(), y.cuda().requires_grad_()
    for want in (amd.lib.OT_DISTANCE, amd.lib.OT_SIMILARITY):
        scores = torch.ops.aspire.ot_pair_scores(xg, lq, yg, lc, *prm, want)
        assert scores.grad_fn is not None and scores.shape == (len(ql),)
        today = torch.ops.aspire.ot_sinkhorn_scores(x.cuda(), lq, y.cuda(), lc, *prm, want, True, False)[0]
        assert torch.equal(scores.detach(), today)
    xg.grad = yg.grad = None
    (torch.ops.aspire.ot_pair_scores(xg, lq, yg, lc, *prm, amd.lib.OT_DISTANCE) * gs.cuda()).sum().backward()
    gq, gc = _backward(amd, *_sets(amd, x, y, ql, cl), gs, kw)
    assert torch.equal(xg.grad, gq.view(x.shape)) and torch.equal(yg.grad, gc.view(y.shape))


def test_opcheck_both_operators(amd):
    x, y, ql, cl, gs, kw = _inputs('a')
    lq, lc = _lens(ql, cl)
    torch.library.opcheck(torch.ops.aspire.ot_pair_scores, (x.cuda().requires_grad_(), lq, y.cuda().requires_grad_(), lc, 0.05, 0.9, 1.0, 4, 0))
    torch.library.opcheck(torch.ops.aspire.ot_pair_backward, (gs.cuda(), x.cuda(), lq, y.cuda(), lc, 0.05, 0.9, 1.0, 4, 0))


def test_reference_triplet_loss_end_to_end(amd):
    """(k) The reference's triplet loss (disent_models.py:241-250: nn.TripletMarginWithDistanceLoss over compute_distance) on CPU
    tensors [B, 768, S] with requires_grad: one backward() fills .grad in the caller's shape on the caller's device, within the bound
    of the yardstick -- the same loss over the restatement in float64, the bound 4 x the fp32 restatement's deviation per tensor
    (floored at 1e-6).  Without requires_grad the result is torch.equal to today's call."""
    gen = torch.Generator().manual_seed(4200)
    qlens, plens, nlens = [8, 3, 1, 5, 6], [8, 8, 2, 1, 4], [2, 6, 8, 3, 7]
    q, pos = _padded((8, 8), list(zip(qlens, plens)), gen)
    _, neg = _padded((8, 8), list(zip(qlens, nlens)), gen)
    margin = 1.0
    loss_fn = torch.nn.TripletMarginWithDistanceLoss
    assert min(ref.pick_margins(q, pos, qlens, plens), ref.pick_margins(q, neg, qlens, nlens)) > 1e-4

    def yard(dtype, direct):
        t = [v.to(dtype).clone().requires_grad_() for v in (q, pos, neg)]
        lens = {id(t[0]): qlens, id(t[1]): plens, id(t[2]): nlens}

        def dist(a, b):
            return ref.restated_distance(a, b, lens[id(a)], lens[id(b)], direct=direct)
        hinge = dist(t[0], t[1]) - dist(t[0], t[2]) + margin
        loss_fn(distance_function=dist, margin=margin, reduction='sum')(t[0], t[1], t[2]).backward()
        return [v.grad for v in t], hinge.detach()

    g64, hinge = yard(torch.float64, False)
    g32, _ = yard(torch.float32, True)
    assert (hinge.abs() > 1e-3).all() and (hinge > 0).any()         # no pair sits on the hinge's corner, some are active
    # the product, in the caller's layout
    e = [t.permute(0, 2, 1).contiguous().requires_grad_() for t in (q, pos, neg)]
    tup = amd.pd.rep_len_tup
    lens_of = {id(e[0]): qlens, id(e[1]): plens, id(e[2]): nlens}
    fn = amd.pd.AllPairMaskedWasserstein({}).compute_distance

    def dist(a, b):
        return fn(tup(embed=a, abs_lens=lens_of[id(a)]), tup(embed=b, abs_lens=lens_of[id(b)]))
    d_pos = dist(e[0], e[1])
    assert d_pos.grad_fn is not None and d_pos.device.type == 'cpu'
    loss_fn(distance_function=dist, margin=margin, reduction='sum')(e[0], e[1], e[2]).backward()
    for name, got, w64, w32, lens in zip(('query', 'pos', 'neg'), e, g64, g32, (qlens, plens, nlens)):
        assert got.grad is not None and got.grad.shape == got.shape == (5, D, 8) and got.grad.device.type == 'cpu'
        grad = got.grad.permute(0, 2, 1)
        dev32 = max((w32[b, :n].double() - w64[b, :n]).abs().max().item() for b, n in enumerate(lens))
        assert dev32 < 1e-4
        tol = max(4.0 * dev32, 1e-6)
        err = max((grad[b, :n].double() - w64[b, :n]).abs().max().item() for b, n in enumerate(lens))
        print(f'OTBWD triplet {name} kernel |error| {err:.3e}, CPU fp32 restatement deviation {dev32:.3e} -> bound {tol:.3e}')
        assert err <= tol
        for b, n in enumerate(lens):
            assert torch.count_nonzero(grad[b, n:]) == 0
    # return_pair_sims stays detached
    out = fn(tup(embed=e[0], abs_lens=qlens), tup(embed=e[1], abs_lens=plens), return_pair_sims=True)
    assert out[0].grad_fn is None and all(t.grad_fn is None and not t.requires_grad for t in out[1])
    # without requires_grad: no graph, and the bits of today's call
    plain = [t.detach() for t in e]
    d_plain = fn(tup(embed=plain[0], abs_lens=qlens), tup(embed=plain[1], abs_lens=plens))
    assert d_plain.grad_fn is None and not d_plain.requires_grad
    assert torch.equal(d_plain, d_pos.detach())
    with torch.no_grad():
        assert fn(tup(embed=e[0], abs_lens=qlens), tup(embed=e[1], abs_lens=plens)).grad_fn is None
    qs, ps = amd.ops.DeviceRepSet.from_padded(q, qlens), amd.ops.DeviceRepSet.from_padded(pos, plens)
    today = amd.ops.ot_sinkhorn(qs, ps, pairing=amd.lib.PAIR_PAIRED, diameter=amd.ops.group_diameter(qs, ps, amd.lib.PAIR_PAIRED, 5),
                                diam_group=5, want=amd.lib.OT_DISTANCE)
    assert torch.equal(d_plain, today.cpu())
