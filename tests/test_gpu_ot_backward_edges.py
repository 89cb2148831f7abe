"""GPU: the backward of the otAspire distance (aspire_ot_backward_f32, ops.ot_backward, torch.ops.aspire.ot_pair_scores,
AllPairMaskedWasserstein.compute_distance) where tests/test_gpu_ot_backward.py does not take it: solver settings off their defaults,
rows of other scales, a marginal that is exactly zero in fp32, documents of 128 x 1 rows, several diameter groups in one call, the
schedule length at its discontinuities, and the Python route with every setting off its default.  The backward repeats the forward's
solve in its own code (its own float64 schedule length, its own -100000 rule, its own C - c0 shift, its own diameter[p / diam_group]
read), so each of these can be wrong in the backward alone.

Inputs, yardsticks and the bound are tests/ot_backward_cases.py's -- the recipe of tests/test_gpu_ot_backward.py, unchanged: float64
autograd over the restatement is the yardstick, the kernel gets max(4 x the fp32 restatement's deviation, 1e-6).  What the reference
alone decides (pick gaps, the deviation below 1e-4, zero marginals, schedule lengths, and that a backward which ignored a setting, a
group index or one schedule step would land more than 10 x outside the bound) is asserted on the CPU, in
tests/test_ot_backward_cpu.py.  Measured in one run (largest absolute values over the valid rows; the fp32 restatement on that host's
CPU, where torch's fp32 sums differ from host to host -- 'rows1' gave 1.1e-06 there and 2.0e-06 on the build host --, the kernel on
its MI355X):

    case                    CPU fp32 deviation   bound      kernel's error
    scaling0.5              2.9e-07              1.1e-06    4.6e-08
    scaling0.99             2.3e-07              1.0e-06    5.8e-08
    blur0.5scaling0.99      1.2e-07              1.0e-06    2.8e-08
    blur_above_diam         8.1e-09              1.0e-06    1.2e-08
    temp10                  2.7e-07              1.1e-06    3.1e-08
    temp5000                2.0e-07              1.0e-06    3.3e-08
    rows1                   1.1e-06              4.4e-06    1.1e-07
    rows3                   7.9e-06              3.1e-05    2.1e-07
    rows1e-2                1.3e-08              1.0e-06    1.0e-08
    rows1e-3                1.3e-08              1.0e-06    1.1e-08
    offset                  6.4e-08              1.0e-06    1.6e-08
    zero_marginal           1.9e-05              7.4e-05    4.0e-07
    aspect                  3.2e-07              1.3e-06    4.8e-08
    groups2                 1.6e-07              1.0e-06    3.5e-08
    groups1                 1.9e-07              1.0e-06    3.9e-08
    schedule                3.8e-07              1.5e-06    1.7e-07   (the forward's distances: 6.8e-06 of 1e-04)
    route, compute_distance 8.5e-07              3.4e-06    1.6e-07

In 'zero_marginal' 9 of the 17 entries of a and 8 of the 19 of b are exactly 0.0 in fp32 and none is denormal (the smallest positive
one is 2.6e-30), so whether a device's expf flushes denormals does not enter: the kernel follows the reference's -100000 rule there
as it stands.

Every comparison prints an `OTBWD ...` line before it asserts (pytest -s shows them)."""
import pytest
import torch

import ot_backward_cases as cases

pytestmark = pytest.mark.gpu
ROUTE = dict(blur=0.1, scaling=0.5, temp=0.2)


@pytest.fixture(scope='module')
def amd():
    from aspire_amd import ops, pair_distances, _lib
    import aspire_amd.torch_ops  # noqa: F401  (registers torch.ops.aspire)
    assert torch.cuda.is_available()
    return type('NS', (), dict(ops=ops, pd=pair_distances, lib=_lib))


def _nan_like(t):
    return torch.full_like(t, float('nan'))


def _padded_sets(amd, inp):
    return amd.ops.DeviceRepSet.from_padded(inp.x, inp.ql), amd.ops.DeviceRepSet.from_padded(inp.y, inp.cl)


def _diameters(amd, inp, qs, cs):
    """(diameter tensor, diam_group): the case's own, or ONE epsilon schedule for the batch from the box of all its rows, pad rows
    included, as AllPairMaskedWasserstein.compute_distance has it"""
    if inp.group is not None:
        return inp.diams.cuda(), inp.group
    return amd.ops.group_diameter(qs, cs, amd.lib.PAIR_PAIRED, qs.n), qs.n


def _backward(amd, inp, qs, cs, diam, group):
    """ops.ot_backward under the case's settings into NaN-filled buffers (a row the kernel does not write shows)"""
    s = cases.settings(inp.kw)
    return amd.ops.ot_backward(qs, cs, inp.gs.cuda(), blur=s['blur'], scaling=s['scaling'], sent_sm_temp=s['temp'], diameter=diam,
                               diam_group=group, out=(_nan_like(qs.rows), _nan_like(cs.rows)))


def _check_padded(inp, gq, gc, yard, what):
    """the structural assertions and the bound, on gradients shaped like the padded inputs (on the CPU)"""
    err = cases.dev(inp, (gq, gc), yard[:2])
    print(f'OTBWD {what} kernel |error| {err:.3e}, bound {yard.tol:.3e}')
    assert torch.isfinite(gq).all() and torch.isfinite(gc).all()
    for b in range(len(inp.ql)):
        assert torch.count_nonzero(gq[b, inp.ql[b]:]) == 0 and torch.count_nonzero(gc[b, inp.cl[b]:]) == 0, 'pad rows must be exact zeros'
    assert err <= yard.tol


@pytest.mark.parametrize('name', cases.STRUCTURAL + ('groups2', 'groups1'))
def test_padded_backward_matches_float64_autograd(amd, name):
    """Cases 1 to 6: within the bound of the float64 yardstick, finite, pad rows exactly 0.0.  In 'groups2' / 'groups1' the kernel
    reads diameter[p / diam_group] from three / five diameters that differ."""
    inp, yard = cases.inputs(name), cases.yardstick(name)
    qs, cs = _padded_sets(amd, inp)
    gq, gc = _backward(amd, inp, qs, cs, *_diameters(amd, inp, qs, cs))
    _check_padded(inp, gq.view(inp.x.shape).cpu(), gc.view(inp.y.shape).cpu(), yard, f'padded ({name})')


@pytest.mark.parametrize('name', cases.CSR)
def test_csr_sets_give_the_padded_bits(amd, name):
    """CSR sets of a case's documents under the same diameter: the bits of the padded call on the valid rows"""
    inp = cases.inputs(name)
    ps, pc = _padded_sets(amd, inp)
    diam, group = _diameters(amd, inp, ps, pc)
    pq, pcand = _backward(amd, inp, ps, pc, diam, group)
    pq, pcand = pq.view(inp.x.shape), pcand.view(inp.y.shape)
    qs = amd.ops.DeviceRepSet.from_list([inp.x[b, :n] for b, n in enumerate(inp.ql)])
    cs = amd.ops.DeviceRepSet.from_list([inp.y[b, :n] for b, n in enumerate(inp.cl)])
    gq, gc = _backward(amd, inp, qs, cs, diam, group)
    assert torch.equal(gq, torch.cat([pq[b, :n] for b, n in enumerate(inp.ql)]))          # (a row left unwritten is NaN: it fails here)
    assert torch.equal(gc, torch.cat([pcand[b, :n] for b, n in enumerate(inp.cl)]))


def test_schedule_length_at_its_discontinuities(amd):
    """Case 7, the backward's counterpart of tests/test_gpu_edges.py's test of the forward: one 6 x 7 pair under 33 given diameters
    on, and a few ulps either side of, blur * scaling**-k, where the schedule gains a step (the float64 gradient then moves by 100 x
    the bound).  Every pair is held to the yardstick of ITS diameter; and the forward, handed the same diameter tensor in the same
    test, gives the float64 distance of every diameter (one step moves it by more than twice the tolerance): forward and backward
    follow one schedule."""
    inp, yard = cases.inputs('schedule'), cases.yardstick('schedule')
    qs, cs = _padded_sets(amd, inp)
    diam = inp.diams.cuda()
    gq, gc = _backward(amd, inp, qs, cs, diam, 1)
    _check_padded(inp, gq.view(inp.x.shape).cpu(), gc.view(inp.y.shape).cpu(), yard, 'padded (schedule)')
    scores = amd.ops.ot_sinkhorn(qs, cs, pairing=amd.lib.PAIR_PAIRED, diameter=diam, diam_group=1, want=amd.lib.OT_DISTANCE).cpu()
    err = (scores.double() - torch.tensor(cases.schedule_values(), dtype=torch.float64)).abs().max().item()
    print(f'OTBWD schedule: forward |error| {err:.3e}, tolerance {cases.FORWARD_ATOL:.0e}')
    assert err <= cases.FORWARD_ATOL


def _lens(inp):
    return torch.tensor(inp.ql, dtype=torch.int32).cuda(), torch.tensor(inp.cl, dtype=torch.int32).cuda()


@pytest.mark.parametrize('group', [2, 0])
def test_operator_carries_its_settings_to_the_backward(amd, group):
    """Case 8, operator level: ot_pair_scores with blur 0.1, scaling 0.5, temp 0.2 and one schedule per 2 pairs / per pair gives the
    bits of ot_sinkhorn_scores(paired=True) with the same arguments, and its backward the bits of ops.ot_backward handed the same
    settings and the matching diameters.  With one input detached the other's gradient has the same bits."""
    inp = cases.inputs('route')
    assert inp.kw == ROUTE
    lq, lc = _lens(inp)
    prm = (ROUTE['blur'], ROUTE['scaling'], ROUTE['temp'], group, amd.lib.OT_DISTANCE)
    xg, yg = inp.x.cuda().requires_grad_(), inp.y.cuda().requires_grad_()
    scores = torch.ops.aspire.ot_pair_scores(xg, lq, yg, lc, *prm)
    assert scores.grad_fn is not None and scores.shape == (len(inp.ql),)
    today = torch.ops.aspire.ot_sinkhorn_scores(inp.x.cuda(), lq, inp.y.cuda(), lc, *prm, True, False)[0]
    assert torch.equal(scores.detach(), today)
    (scores * inp.gs.cuda()).sum().backward()
    qs, cs = _padded_sets(amd, inp)
    diam = amd.ops.group_diameter(qs, cs, amd.lib.PAIR_PAIRED, group) if group > 0 else None
    gq, gc = _backward(amd, inp, qs, cs, diam, group)
    gq, gc = gq.view(inp.x.shape), gc.view(inp.y.shape)
    assert torch.equal(xg.grad, gq) and torch.equal(yg.grad, gc)
    # the settings reach the kernel: at their defaults the gradient is another one
    plain = amd.ops.ot_backward(qs, cs, inp.gs.cuda(), diameter=diam, diam_group=group)
    assert not torch.equal(plain[0].view(inp.x.shape), gq)
    # one side detached
    x1, y1 = inp.x.cuda().requires_grad_(), inp.y.cuda()
    (torch.ops.aspire.ot_pair_scores(x1, lq, y1, lc, *prm) * inp.gs.cuda()).sum().backward()
    assert y1.grad is None and torch.equal(x1.grad, gq)
    x2, y2 = inp.x.cuda(), inp.y.cuda().requires_grad_()
    (torch.ops.aspire.ot_pair_scores(x2, lq, y2, lc, *prm) * inp.gs.cuda()).sum().backward()
    assert x2.grad is None and torch.equal(y2.grad, gc)


def test_public_route_with_its_own_settings(amd):
    """Case 8, the public route: AllPairMaskedWasserstein with geoml_blur 0.1, geoml_scaling 0.5, sent_sm_temp 0.2 on embeds
    [B, 768, S] that require grad, held to the float64 yardstick under those settings (at the default settings the float64 gradient
    is more than 1000 x the bound away: tests/test_ot_backward_cpu.py)."""
    inp, yard = cases.inputs('route'), cases.yardstick('route')
    q = inp.x.permute(0, 2, 1).contiguous().requires_grad_()
    c = inp.y.permute(0, 2, 1).contiguous().requires_grad_()
    fn = amd.pd.AllPairMaskedWasserstein({'geoml_blur': ROUTE['blur'], 'geoml_scaling': ROUTE['scaling'], 'sent_sm_temp': ROUTE['temp']})
    dist = fn.compute_distance(amd.pd.rep_len_tup(embed=q, abs_lens=inp.ql), amd.pd.rep_len_tup(embed=c, abs_lens=inp.cl))
    assert dist.grad_fn is not None and dist.shape == (len(inp.ql),)
    (dist * inp.gs).sum().backward()
    assert q.grad.shape == q.shape and c.grad.shape == c.shape
    _check_padded(inp, q.grad.permute(0, 2, 1), c.grad.permute(0, 2, 1), yard, 'compute_distance (route)')
