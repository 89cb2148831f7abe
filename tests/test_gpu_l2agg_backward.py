"""GPU: the backward of the three L2 aggregations (aspire_l2agg_backward_f32, ops.l2agg_backward, torch.ops.aspire.l2agg_pair_scores /
l2agg_pair_backward, and the reference's names in aspire_amd.pair_distances) against float64 torch autograd on the CPU over a
restatement of the reference's three functions (pair_distances.py:138-186, :295-345, :95-135 with activations.py:35-61): torch.cdist,
the -10e8 pad mask, torch.max / torch.topk(k = 2), the -1e32-masked 2-D soft-max.

Pad rows of the inputs are zero, as the reference's batches have them.  (That also settles what the restatement's top-2 does with ONE
valid entry: its second pick is then a masked entry between two zero pad rows, distance 0, whose gradient is 0 -- the kernel drops
that pick.)

Tolerance, per aggregation: the same restatement run in fp32 on the CPU is compared with the float64 gradient over every shape of
GROUPS; the kernel gets 4 x the largest absolute deviation (the summation order differs: 4 is margin for that and nothing else),
floored at 1e-6.  Measured (valid rows, largest |fp32 - fp64| over the three groups -> bound); the fp32 restatement's deviation is
itself asserted to stay below 1e-4 (_tol).  The kernel's own error on an MI355X: not measured.

    aggregation        CPU fp32 deviation   bound
    max                3.5e-08              1.0e-06
    top2               3.5e-08              1.0e-06
    attention t=1.0    4.4e-07              1.7e-06
    attention t=0.05   1.0e-05              4.2e-05

Every comparison prints its figures before it asserts (pytest -s shows them)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
D = 768
# padded extent, [(q_len, c_len)] -- ragged pairs in one call
GROUPS = {
    'p8': (8, [(1, 1), (1, 3), (3, 8), (8, 8), (8, 2)]),        # small documents, one-row ones among them
    'p32': (32, [(26, 30), (17, 9)]),                            # the forward's matmul-formula side (> 25 rows); crosses 16-row tiles
    'p40': (40, [(40, 33)]),                                     # the long-document kernel's range
}
AGGS = {'max': (0, 1.0), 'top2': (1, 1.0), 'att1': (2, 1.0), 'att005': (2, 0.05)}      # _lib.AGG_*, temp


@pytest.fixture(scope='module')
def amd():
    from aspire_amd import ops, pair_distances, _lib
    import aspire_amd.torch_ops as torch_ops
    assert torch.cuda.is_available()
    return type('NS', (), dict(ops=ops, pd=pair_distances, lib=_lib, to=torch_ops))


def _padded(ext, lens, gen):
    """(q, c) [B, ext, 768] fp32: N(0, 1) valid rows, zero pad rows"""
    q, c = torch.zeros(len(lens), ext, D), torch.zeros(len(lens), ext, D)
    for b, (ql, cl) in enumerate(lens):
        q[b, :ql] = torch.randn(ql, D, generator=gen)
        c[b, :cl] = torch.randn(cl, D, generator=gen)
    return q, c


@functools.lru_cache(maxsize=None)
def _inputs(group):
    ext, lens = GROUPS[group]
    gen = torch.Generator().manual_seed(1000 + ext)
    q, c = _padded(ext, lens, gen)
    gs = torch.randn(len(lens), generator=gen)
    if group == 'p8':
        gs[2] = 0.0                     # a zero ...
        gs[3] = -gs[3].abs()            # ... and a negative upstream gradient
    return q, c, lens, gs


def _restated_sims(q, c, lens, agg, temp):
    """The reference's three functions, similarity side ([B, S, 768] inputs: its permute already applied), in q's dtype."""
    b, sq, _ = q.shape
    sc = c.shape[1]
    neg_pair_dists = -1 * torch.cdist(q, c)
    if agg in (0, 1):
        pad_mask = torch.ones(b, sq, sc, dtype=q.dtype) * -10e8
        for i, (ql, cl) in enumerate(lens):
            pad_mask[i, :ql, :cl] = 0.0
        neg_pair_dists = neg_pair_dists + pad_mask
        flat = neg_pair_dists.view(b, sq * sc)
        if agg == 0:
            return torch.max(flat, dim=1)[0]
        return torch.topk(flat, dim=1, k=2)[0].sum(dim=1)
    logit_mask = torch.zeros(b, sq, sc, dtype=q.dtype)
    for i, (ql, cl) in enumerate(lens):
        logit_mask[i, ql:, :] = -1e32
        logit_mask[i, :, cl:] = -1e32
    log_probs = torch.log_softmax((neg_pair_dists / temp + logit_mask).view(b, sq * sc), dim=1).view(b, sq, sc)
    return (log_probs.exp() * neg_pair_dists).sum(dim=1).sum(dim=1)


def _autograd(q, c, lens, gs, agg, temp, dtype):
    q = q.to(dtype).clone().requires_grad_()
    c = c.to(dtype).clone().requires_grad_()
    (_restated_sims(q, c, lens, agg, temp) * gs.to(dtype)).sum().backward()
    return q.grad, c.grad


def _valid_dev(got_q, got_c, want_q, want_c, lens):
    """largest |got - want| over the valid rows"""
    dev = 0.0
    for b, (ql, cl) in enumerate(lens):
        dev = max(dev, (got_q[b, :ql].double() - want_q[b, :ql]).abs().max().item(),
                  (got_c[b, :cl].double() - want_c[b, :cl]).abs().max().item())
    return dev


@functools.lru_cache(maxsize=None)
def _yardstick(group, aggname):
    """(float64 grad_q, grad_c, the fp32 restatement's largest deviation from them over the valid rows) -- computed once"""
    q, c, lens, gs = _inputs(group)
    agg, temp = AGGS[aggname]
    gq64, gc64 = _autograd(q, c, lens, gs, agg, temp, torch.float64)
    gq32, gc32 = _autograd(q, c, lens, gs, agg, temp, torch.float32)
    return gq64, gc64, _valid_dev(gq32, gc32, gq64, gc64, lens)


@functools.lru_cache(maxsize=None)
def _tol(aggname):
    dev32 = max(_yardstick(group, aggname)[2] for group in GROUPS)
    # fp32 rounding of gradients of size <= 1 is far below this.  A deviation beyond it would mean that the fp32 restatement itself
    # took another pick (in fp32 every masked entry of top-2 rounds to exactly -1e9: its second pick on a one-entry block is a choice
    # among ties), and the bound must not grow from that unnoticed.
    assert dev32 < 1e-4, (aggname, dev32)
    tol = max(4.0 * dev32, 1e-6)
    print(f'[{aggname}] CPU fp32 restatement deviation {dev32:.3e} -> bound {tol:.3e}')
    return tol


def _nan_like(t):
    return torch.full_like(t, float('nan'))


def _backward(amd, qs, cs, aggname, gs):
    """ops.l2agg_backward into NaN-filled buffers: a row the kernel does not write shows"""
    agg, temp = AGGS[aggname]
    return amd.ops.l2agg_backward(qs, cs, agg, gs.cuda(), temp=temp, out=(_nan_like(qs.rows), _nan_like(cs.rows)))


@pytest.mark.parametrize('aggname', list(AGGS))
@pytest.mark.parametrize('group', list(GROUPS))
def test_padded_backward_matches_float64_autograd(amd, group, aggname):
    q, c, lens, gs = _inputs(group)
    ext = GROUPS[group][0]
    gq64, gc64, _ = _yardstick(group, aggname)
    tol = _tol(aggname)
    qs = amd.ops.DeviceRepSet.from_padded(q, [l[0] for l in lens])
    cs = amd.ops.DeviceRepSet.from_padded(c, [l[1] for l in lens])
    gq, gc = _backward(amd, qs, cs, aggname, gs)
    gq, gc = gq.view(-1, ext, D).cpu(), gc.view(-1, ext, D).cpu()
    err = _valid_dev(gq, gc, gq64, gc64, lens)
    print(f'[{group} {aggname}] kernel |error| {err:.3e}, bound {tol:.3e}')
    assert not torch.isnan(gq).any() and not torch.isnan(gc).any()
    for b, (ql, cl) in enumerate(lens):
        assert torch.count_nonzero(gq[b, ql:]) == 0 and torch.count_nonzero(gc[b, cl:]) == 0, 'pad rows must be exact zeros'
    assert err <= tol


@pytest.mark.parametrize('aggname', list(AGGS))
def test_row_limit_shape(amd, aggname):
    """Documents at the 128-row limit: the distance block then needs more LDS than a launch gets by default (the launcher raises the
    kernel's limit).  Not one of the tolerance's shapes: the bound here is the same recipe on this shape alone (4 x the fp32
    restatement's deviation from float64, floored at 1e-6)."""
    agg, temp = AGGS[aggname]
    lens = [(128, 128), (5, 127)]
    gen = torch.Generator().manual_seed(128)
    q, c = _padded(128, lens, gen)
    gs = torch.tensor([0.8, -1.1])
    gq64, gc64 = _autograd(q, c, lens, gs, agg, temp, torch.float64)
    tol = max(4.0 * _valid_dev(*_autograd(q, c, lens, gs, agg, temp, torch.float32), gq64, gc64, lens), 1e-6)
    gq, gc = _backward(amd, amd.ops.DeviceRepSet.from_padded(q, [128, 5]), amd.ops.DeviceRepSet.from_padded(c, [128, 127]), aggname, gs)
    gq, gc = gq.view(2, 128, D).cpu(), gc.view(2, 128, D).cpu()
    err = _valid_dev(gq, gc, gq64, gc64, lens)
    print(f'[128 rows {aggname}] kernel |error| {err:.3e}, bound {tol:.3e}, largest |gradient| {gq64.abs().max().item():.3e}')
    assert not torch.isnan(gq).any() and not torch.isnan(gc).any()
    assert torch.count_nonzero(gq[1, 5:]) == 0 and torch.count_nonzero(gc[1, 127:]) == 0
    assert err <= tol


@pytest.mark.parametrize('aggname', list(AGGS))
def test_csr_backward_matches_float64_autograd(amd, aggname):
    q, c, lens, gs = _inputs('p8')
    gq64, gc64, _ = _yardstick('p8', aggname)
    tol = _tol(aggname)
    qs = amd.ops.DeviceRepSet.from_list([q[b, :ql] for b, (ql, _) in enumerate(lens)])
    cs = amd.ops.DeviceRepSet.from_list([c[b, :cl] for b, (_, cl) in enumerate(lens)])
    gq, gc = _backward(amd, qs, cs, aggname, gs)
    want_q = torch.cat([gq64[b, :ql] for b, (ql, _) in enumerate(lens)])
    want_c = torch.cat([gc64[b, :cl] for b, (_, cl) in enumerate(lens)])
    err = max((gq.cpu().double() - want_q).abs().max().item(), (gc.cpu().double() - want_c).abs().max().item())
    print(f'[csr {aggname}] kernel |error| {err:.3e}, bound {tol:.3e}')
    assert err <= tol          # (a row left unwritten is NaN: it fails here)
    # the padded form of the same documents: the same bits, row by row
    pq, pc = _backward(amd, amd.ops.DeviceRepSet.from_padded(q, [l[0] for l in lens]),
                       amd.ops.DeviceRepSet.from_padded(c, [l[1] for l in lens]), aggname, gs)
    pq, pc = pq.view(-1, 8, D), pc.view(-1, 8, D)
    assert torch.equal(gq, torch.cat([pq[b, :ql] for b, (ql, _) in enumerate(lens)]))
    assert torch.equal(gc, torch.cat([pc[b, :cl] for b, (_, cl) in enumerate(lens)]))


@pytest.mark.parametrize('aggname', list(AGGS))
def test_coincident_rows(amd, aggname):
    """A candidate row copied from the query: d = 0 there.  Finite gradients; for MAX that entry is the pick and the pair's gradient is
    exactly 0 (A = 0 where d == 0, torch.cdist's backward rule); the other aggregations agree with float64 autograd, which follows the
    same rule."""
    gen = torch.Generator().manual_seed(7)
    lens = [(3, 4), (2, 2)]
    q, c = _padded(8, lens, gen)
    c[0, 1] = q[0, 2]
    gs = torch.tensor([1.5, -0.75])
    agg, temp = AGGS[aggname]
    qs, cs = amd.ops.DeviceRepSet.from_padded(q, [3, 2]), amd.ops.DeviceRepSet.from_padded(c, [4, 2])
    gq, gc = _backward(amd, qs, cs, aggname, gs)
    gq, gc = gq.view(2, 8, D).cpu(), gc.view(2, 8, D).cpu()
    assert torch.isfinite(gq).all() and torch.isfinite(gc).all()
    if aggname == 'max':
        assert torch.count_nonzero(gq[0]) == 0 and torch.count_nonzero(gc[0]) == 0
    gq64, gc64 = _autograd(q, c, lens, gs, agg, temp, torch.float64)
    err = _valid_dev(gq, gc, gq64, gc64, lens)
    print(f'[coincident {aggname}] kernel |error| {err:.3e}, bound {_tol(aggname):.3e}')
    assert err <= _tol(aggname)


def test_tie_rule_first_in_row_major_order(amd):
    """Two identical candidate rows nearest to one query row: entries (1, 1) and (1, 3) tie for the maximum.  MAX takes (1, 1), TOP2
    takes (1, 1) and then (1, 3); the expected gradients are written out here from that choice."""
    gen = torch.Generator().manual_seed(11)
    q, c = _padded(8, [(3, 5)], gen)
    c[0, 1] = q[0, 1] + 0.1 * torch.randn(D, generator=gen)
    c[0, 3] = c[0, 1]
    g = -1.25
    qd, cd = q[0, :3].double(), c[0, :5].double()
    dist = (qd[:, None, :] - cd[None, :, :]).norm(dim=2)
    order = sorted(range(15), key=lambda e: (dist[e // 5, e % 5].item(), e))
    assert order[:2] == [1 * 5 + 1, 1 * 5 + 3] and dist[1, 1] == dist[1, 3]          # the tie is the maximum of -d
    unit = (qd[1] - cd[1]) / dist[1, 1]
    qs, cs = amd.ops.DeviceRepSet.from_padded(q, [3]), amd.ops.DeviceRepSet.from_padded(c, [5])
    for aggname, picks in (('max', [(1, 1)]), ('top2', [(1, 1), (1, 3)])):
        want_q, want_c = torch.zeros(8, D, dtype=torch.float64), torch.zeros(8, D, dtype=torch.float64)
        for i, j in picks:
            want_q[i] += -g * unit
            want_c[j] += g * unit
        gq, gc = _backward(amd, qs, cs, aggname, torch.tensor([g]))
        gq, gc = gq.cpu(), gc.cpu()
        err = max((gq.double() - want_q).abs().max().item(), (gc.double() - want_c).abs().max().item())
        print(f'[tie {aggname}] kernel |error| {err:.3e}, bound {_tol(aggname):.3e}')
        assert err <= _tol(aggname)
        # rows outside the choice are exact zeros: for MAX the twin (1, 3) gets nothing
        assert torch.count_nonzero(gq[[0, 2]]) == 0 and torch.count_nonzero(gq[3:]) == 0
        untouched = [j for j in range(8) if j not in [pj for _, pj in picks]]
        assert torch.count_nonzero(gc[untouched]) == 0
        assert torch.count_nonzero(gc[1]) > 0


@pytest.mark.parametrize('aggname', list(AGGS))
def test_same_bits_across_runs_and_pad_rows_are_not_read(amd, aggname):
    q, c, lens, gs = _inputs('p8')
    ql, cl = [l[0] for l in lens], [l[1] for l in lens]
    first = _backward(amd, amd.ops.DeviceRepSet.from_padded(q, ql), amd.ops.DeviceRepSet.from_padded(c, cl), aggname, gs)
    again = _backward(amd, amd.ops.DeviceRepSet.from_padded(q, ql), amd.ops.DeviceRepSet.from_padded(c, cl), aggname, gs)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    q2, c2 = q.clone(), c.clone()
    for b, (a, k) in enumerate(lens):       # other values in the pad rows: nothing moves
        q2[b, a:] = 7.0
        c2[b, k:] = -3.0
    other = _backward(amd, amd.ops.DeviceRepSet.from_padded(q2, ql), amd.ops.DeviceRepSet.from_padded(c2, cl), aggname, gs)
    assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])


@pytest.mark.parametrize('aggname', list(AGGS))
@pytest.mark.parametrize('group', list(GROUPS))
def test_differentiable_forward_is_todays_forward(amd, group, aggname):
    q, c, lens, _ = _inputs(group)
    agg, temp = AGGS[aggname]
    ql = torch.tensor([l[0] for l in lens], dtype=torch.int32).cuda()
    cl = torch.tensor([l[1] for l in lens], dtype=torch.int32).cuda()
    qg, cg = q.cuda().requires_grad_(), c.cuda().requires_grad_()
    sims = torch.ops.aspire.l2agg_pair_scores(qg, ql, cg, cl, agg, temp)
    assert sims.grad_fn is not None and sims.shape == (len(lens),)
    qs = amd.ops.DeviceRepSet.from_padded(q, [l[0] for l in lens])
    cs = amd.ops.DeviceRepSet.from_padded(c, [l[1] for l in lens])
    if agg == 0:
        want = amd.ops.l2max_scores(qs, cs, pairing=amd.lib.PAIR_PAIRED)
    else:
        want = amd.ops.l2agg_scores(qs, cs, agg, temp=temp, pairing=amd.lib.PAIR_PAIRED)
    assert torch.equal(sims.detach(), want)


@pytest.mark.parametrize('aggname', list(AGGS))
def test_opcheck_both_operators(amd, aggname):
    q, c, lens, gs = _inputs('p8')
    agg, temp = AGGS[aggname]
    ql = torch.tensor([l[0] for l in lens], dtype=torch.int32).cuda()
    cl = torch.tensor([l[1] for l in lens], dtype=torch.int32).cuda()
    torch.library.opcheck(torch.ops.aspire.l2agg_pair_scores, (q.cuda().requires_grad_(), ql, c.cuda().requires_grad_(), cl, agg, temp))
    torch.library.opcheck(torch.ops.aspire.l2agg_pair_backward, (gs.cuda(), q.cuda(), ql, c.cuda(), cl, agg, temp))


def _reference_distance(amd, name):
    if name == 'l2max':
        return amd.pd.allpair_masked_dist_l2max, 'max'
    if name == 'l2topk':
        return amd.pd.allpair_masked_dist_l2topk, 'top2'
    return amd.pd.AllPairMaskedAttention({'cdatt_sm_temp': 1.0}).compute_distance, 'att1'


@pytest.mark.parametrize('name', ['l2max', 'l2topk', 'l2attention'])
def test_reference_names_triplet_loss_end_to_end(amd, name):
    """CPU inputs [B, 768, S] with requires_grad through the reference's names: relu(d(q, pos) - d(q, neg) + margin).sum(), one
    backward(); .grad has the caller's shape and device and matches the float64 yardstick.  The bound is the aggregation's bound of
    _tol (taken from GROUPS' inputs, not from this test's: the same sizes and the same N(0, 1) rows) for pos and neg, which receive
    one kernel result each, and twice it for the query, whose gradient is the sum of two (its pair with pos and its pair with neg)."""
    fn, aggname = _reference_distance(amd, name)
    agg, temp = AGGS[aggname]
    gen = torch.Generator().manual_seed(23)
    qlens, plens, nlens = [1, 3, 8, 8, 5], [1, 8, 8, 2, 4], [2, 1, 6, 8, 3]
    q, pos = _padded(8, list(zip(qlens, plens)), gen)
    _, neg = _padded(8, list(zip(qlens, nlens)), gen)
    margin = 1.0
    # the yardstick: the same loss over the restatement in float64
    y = [t.double().clone().requires_grad_() for t in (q, pos, neg)]
    hinge = (-_restated_sims(y[0], y[1], list(zip(qlens, plens)), agg, temp)
             + _restated_sims(y[0], y[2], list(zip(qlens, nlens)), agg, temp) + margin)
    assert (hinge.abs() > 1e-3).all() and (hinge > 0).any()         # no pair sits on the hinge's corner, some are active
    torch.relu(hinge).sum().backward()
    # the product, in the caller's layout
    e = [t.permute(0, 2, 1).contiguous().requires_grad_() for t in (q, pos, neg)]
    tup = amd.pd.rep_len_tup
    d_pos = fn(tup(embed=e[0], abs_lens=qlens), tup(embed=e[1], abs_lens=plens))
    d_neg = fn(tup(embed=e[0], abs_lens=qlens), tup(embed=e[2], abs_lens=nlens))
    assert d_pos.grad_fn is not None and d_pos.device.type == 'cpu'
    torch.relu(d_pos - d_neg + margin).sum().backward()
    for got, want, lens, tol in zip(e, y, (qlens, plens, nlens), (2 * _tol(aggname), _tol(aggname), _tol(aggname))):
        assert got.grad.shape == got.shape == (5, D, 8) and got.grad.device.type == 'cpu'
        grad = got.grad.permute(0, 2, 1)
        err = max((grad[b, :n].double() - want.grad[b, :n]).abs().max().item() for b, n in enumerate(lens))
        print(f'[{name}] kernel |error| {err:.3e}, bound {tol:.3e}')
        assert err <= tol
        for b, n in enumerate(lens):
            assert torch.count_nonzero(grad[b, n:]) == 0
    # return_pair_sims: the sims are attached, the pair matrices are not
    out = fn(tup(embed=e[0], abs_lens=qlens), tup(embed=e[1], abs_lens=plens), return_pair_sims=True)
    extras = out[1] if isinstance(out[1], (list, tuple)) else [out[1]]
    assert out[0].grad_fn is not None and all(t.grad_fn is None and not t.requires_grad for t in extras)
    assert torch.equal(out[0].detach(), -d_pos.detach())
    # without requires_grad: no graph, and the bits of the scoring call
    plain = [t.detach() for t in e]
    d_plain = fn(tup(embed=plain[0], abs_lens=qlens), tup(embed=plain[1], abs_lens=plens))
    assert d_plain.grad_fn is None and not d_plain.requires_grad
    assert torch.equal(d_plain, d_pos.detach())
    with torch.no_grad():
        assert fn(tup(embed=e[0], abs_lens=qlens), tup(embed=e[1], abs_lens=plens)).grad_fn is None
    qs = amd.ops.DeviceRepSet.from_padded(q, qlens)
    ps = amd.ops.DeviceRepSet.from_padded(pos, plens)
    if agg == 0:
        sims = amd.ops.l2max_scores(qs, ps, pairing=amd.lib.PAIR_PAIRED)
    else:
        sims = amd.ops.l2agg_scores(qs, ps, agg, temp=temp, pairing=amd.lib.PAIR_PAIRED)
    assert torch.equal(d_plain, (-1 * sims).cpu())
