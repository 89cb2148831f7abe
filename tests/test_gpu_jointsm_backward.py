"""GPU: the backward of the joint soft-max alignment score (aspire_jointsm_backward_f32, ops.jointsm_backward,
torch.ops.aspire.jointsm_pair_scores / jointsm_pair_backward, and allpair_joint_sm_negscore in aspire_amd.pair_distances) against
float64 torch autograd on the CPU over the closed form S = 2 sum_ij p_ij d_ij (tests/golden/trainside_inputs.py), on the eight CASES
of tests/golden/jointsm_inputs.py: the 1 x 1 block, one-row documents against 8 and 30 rows, lengths that are no multiple of 4 or 16,
97 / 100 / 113 / 127 / 128 rows, the 128 x 128 limit (more than 64 KiB of LDS), a peaked soft-max (s8pk, full: a duplicated document
at scale 1.0, d_ii of about 950) and a flat one (nb, long, fullf: scale 0.3).

Tolerance, per case: bound = max(4 * ref_err, 4 * 2^-23 * max_grad) with ref_err the reference's OWN fp32 autograd deviation from the
float64 yardstick and max_grad the largest float64 gradient entry, both recorded in tests/golden/trainside.npz by
make_golden_trainside.py (tests/test_trainside_backward_cpu.py holds the yardstick against the reference's stored gradients).  4 is
the margin for another summation order and nothing else; the floor is four fp32 roundings of the largest entry (on a 1 x 1 block p = 1
exactly and the reference's error is a single lucky rounding).  The upstream gradients gs are the fixture's (s8 holds a zero and a
negative one).  Largest |kernel - float64| over the valid rows on an MI355X:

    case    kernel error   bound
    one     1.743e-07      2.196e-06
    s8      2.148e-06      2.362e-05
    s8pk    2.536e-06      3.632e-05
    nb      8.452e-07      9.210e-06
    mid     1.665e-06      1.337e-05
    long    5.790e-08      5.294e-07
    full    7.440e-06      1.219e-04
    fullf   3.579e-08      3.980e-07

Every comparison prints its figures before it asserts (pytest -s shows them)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import trainside_inputs as ti  # noqa: E402

pytestmark = pytest.mark.gpu
D = 768


@pytest.fixture(scope='module')
def amd():
    from aspire_amd import ops, pair_distances, _lib
    import aspire_amd.torch_ops as torch_ops
    assert torch.cuda.is_available()
    return type('NS', (), dict(ops=ops, pd=pair_distances, lib=_lib, to=torch_ops))


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'trainside.npz'))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(q, c [B, S, 768] fp32 tensors, qlens, clens, gs, float64 grad_q, grad_c, bound) -- computed once, never written to"""
    q, c, qlens, clens = ti.case_inputs(ti.CASES[name])
    fx = _fixture()
    gs = fx[f'jointsm_{name}_gs']
    wq, wc = ti.jointsm_grad64(q, c, qlens, clens, gs)
    tol = ti.bound(fx[f'jointsm_{name}_ref_err'], fx[f'jointsm_{name}_max_grad'])
    return torch.from_numpy(q), torch.from_numpy(c), qlens, clens, torch.from_numpy(gs), torch.from_numpy(wq), torch.from_numpy(wc), tol


def _valid_dev(got_q, got_c, want_q, want_c, qlens, clens):
    """largest |got - want| over the valid rows"""
    return max(max((got_q[b, :n].double() - want_q[b, :n]).abs().max().item() for b, n in enumerate(qlens)),
               max((got_c[b, :n].double() - want_c[b, :n]).abs().max().item() for b, n in enumerate(clens)))


def _nan_like(t):
    return torch.full_like(t, float('nan'))


def _backward(amd, qs, cs, gs):
    """ops.jointsm_backward into NaN-filled buffers: a row the kernel does not write shows"""
    return amd.ops.jointsm_backward(qs, cs, gs.cuda(), out=(_nan_like(qs.rows), _nan_like(cs.rows)))


def _padded_backward(amd, q, c, qlens, clens, gs):
    gq, gc = _backward(amd, amd.ops.DeviceRepSet.from_padded(q, qlens), amd.ops.DeviceRepSet.from_padded(c, clens), gs)
    return gq.view(q.shape), gc.view(c.shape)


@pytest.mark.parametrize('name', list(ti.CASES))
def test_padded_backward_matches_float64_autograd(amd, name):
    q, c, qlens, clens, gs, wq, wc, tol = _case(name)
    gq, gc = (t.cpu() for t in _padded_backward(amd, q, c, qlens, clens, gs))
    err = _valid_dev(gq, gc, wq, wc, qlens, clens)
    print(f'[{name}] kernel |error| {err:.3e}, bound {tol:.3e}, largest |gradient| {max(wq.abs().max().item(), wc.abs().max().item()):.3e}')
    assert not torch.isnan(gq).any() and not torch.isnan(gc).any()
    for b, (ql, cl) in enumerate(zip(qlens, clens)):
        assert torch.count_nonzero(gq[b, ql:]) == 0 and torch.count_nonzero(gc[b, cl:]) == 0, 'pad rows must be exact zeros'
        if gs[b] == 0:
            assert torch.count_nonzero(gq[b]) == 0 and torch.count_nonzero(gc[b]) == 0, 'g == 0 gives exact zeros'
    assert (gs == 0).any() or name != 's8'
    assert err <= tol


@pytest.mark.parametrize('name', ['s8', 'nb'])
def test_csr_backward_matches_float64_and_the_padded_bits(amd, name):
    q, c, qlens, clens, gs, wq, wc, tol = _case(name)
    qs = amd.ops.DeviceRepSet.from_list([q[b, :n] for b, n in enumerate(qlens)])
    cs = amd.ops.DeviceRepSet.from_list([c[b, :n] for b, n in enumerate(clens)])
    gq, gc = _backward(amd, qs, cs, gs)
    want_q = torch.cat([wq[b, :n] for b, n in enumerate(qlens)])
    want_c = torch.cat([wc[b, :n] for b, n in enumerate(clens)])
    err = max((gq.cpu().double() - want_q).abs().max().item(), (gc.cpu().double() - want_c).abs().max().item())
    print(f'[csr {name}] kernel |error| {err:.3e}, bound {tol:.3e}')
    assert err <= tol          # (a row left unwritten is NaN: it fails here)
    pq, pc = _padded_backward(amd, q, c, qlens, clens, gs)
    assert torch.equal(gq, torch.cat([pq[b, :n] for b, n in enumerate(qlens)]))
    assert torch.equal(gc, torch.cat([pc[b, :n] for b, n in enumerate(clens)]))


@pytest.mark.parametrize('name', ['s8', 'mid'])
def test_same_bits_across_runs_and_pad_rows_are_not_read(amd, name):
    q, c, qlens, clens, gs = _case(name)[:5]
    first = _padded_backward(amd, q, c, qlens, clens, gs)
    again = _padded_backward(amd, q, c, qlens, clens, gs)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    q2, c2 = q.clone(), c.clone()
    for b, (ql, cl) in enumerate(zip(qlens, clens)):       # other values in the pad rows: nothing moves
        q2[b, ql:] = 7.0
        c2[b, cl:] = -3.0
    other = _padded_backward(amd, q2, c2, qlens, clens, gs)
    assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])


def _lens_gpu(lens):
    return torch.tensor(lens, dtype=torch.int32).cuda()


@pytest.mark.parametrize('name', ['one', 's8', 'mid', 'full'])
def test_differentiable_forward_is_todays_forward(amd, name):
    q, c, qlens, clens = _case(name)[:4]
    sims = torch.ops.aspire.jointsm_pair_scores(q.cuda().requires_grad_(), _lens_gpu(qlens), c.cuda().requires_grad_(), _lens_gpu(clens))
    assert sims.grad_fn is not None and sims.shape == (len(qlens),)
    want = amd.ops.jointsm_scores(amd.ops.DeviceRepSet.from_padded(q, qlens), amd.ops.DeviceRepSet.from_padded(c, clens),
                                  pairing=amd.lib.PAIR_PAIRED)
    assert torch.equal(sims.detach(), want)


def test_opcheck_both_operators(amd):
    q, c, qlens, clens, gs = _case('s8')[:5]
    ql, cl = _lens_gpu(qlens), _lens_gpu(clens)
    torch.library.opcheck(torch.ops.aspire.jointsm_pair_scores, (q.cuda().requires_grad_(), ql, c.cuda().requires_grad_(), cl))
    torch.library.opcheck(torch.ops.aspire.jointsm_pair_backward, (gs.cuda(), q.cuda(), ql, c.cuda(), cl))


def test_reference_name_triplet_loss_end_to_end(amd):
    """CPU inputs [B, 768, S] with requires_grad through allpair_joint_sm_negscore: relu(d(q, pos) - d(q, neg) + margin).sum(), one
    backward(); .grad has the caller's shape and device and matches the float64 yardstick.  The rows are case s8's: pos its candidates,
    neg the same candidates moved on by one pair; the hinge's upstream gradients are 0 and +-1 where the case's are N(0, 1) draws.  The
    bound is s8's for pos and neg, which receive one kernel result each, and twice it for the query, whose gradient is the sum of two."""
    fn = amd.pd.allpair_joint_sm_negscore
    q, pos, qlens, plens = _case('s8')[:4]
    tol = _case('s8')[7]
    neg, nlens = torch.roll(pos, 1, dims=0), plens[-1:] + plens[:-1]
    margin = 1.0
    y = [t.double().clone().requires_grad_() for t in (q, pos, neg)]
    hinge = -ti.jointsm_sims(y[0], y[1], qlens, plens) + ti.jointsm_sims(y[0], y[2], qlens, nlens) + margin
    assert (hinge.abs() > 1e-3).all() and (hinge > 0).any() and (hinge < 0).any()      # no pair on the hinge's corner, some active
    torch.relu(hinge).sum().backward()
    e = [t.permute(0, 2, 1).contiguous().requires_grad_() for t in (q, pos, neg)]
    tup = amd.pd.rep_len_tup
    d_pos = fn(tup(embed=e[0], abs_lens=qlens), tup(embed=e[1], abs_lens=plens))
    d_neg = fn(tup(embed=e[0], abs_lens=qlens), tup(embed=e[2], abs_lens=nlens))
    assert d_pos.grad_fn is not None and d_pos.device.type == 'cpu'
    torch.relu(d_pos - d_neg + margin).sum().backward()
    for what, got, want, lens, t in zip(('query', 'pos', 'neg'), e, y, (qlens, plens, nlens), (2 * tol, tol, tol)):
        assert got.grad.shape == got.shape == (len(qlens), D, 8) and got.grad.device.type == 'cpu'
        grad = got.grad.permute(0, 2, 1)
        err = max((grad[b, :n].double() - want.grad[b, :n]).abs().max().item() for b, n in enumerate(lens))
        print(f'[negscore {what}] kernel |error| {err:.3e}, bound {t:.3e}')
        assert err <= t
        for b, n in enumerate(lens):
            assert torch.count_nonzero(grad[b, n:]) == 0
    # return_pair_sims: the distance is attached, pair_sm is not
    dist, pair_sm = fn(tup(embed=e[0], abs_lens=qlens), tup(embed=e[1], abs_lens=plens), return_pair_sims=True)
    assert dist.grad_fn is not None and pair_sm.grad_fn is None and not pair_sm.requires_grad
    assert torch.equal(dist.detach(), d_pos.detach())
    # without requires_grad and under no_grad: no graph, and the bits of the scoring call
    plain = [t.detach() for t in e]
    d_plain = fn(tup(embed=plain[0], abs_lens=qlens), tup(embed=plain[1], abs_lens=plens))
    assert d_plain.grad_fn is None and not d_plain.requires_grad
    assert torch.equal(d_plain, d_pos.detach())
    with torch.no_grad():
        assert fn(tup(embed=e[0], abs_lens=qlens), tup(embed=e[1], abs_lens=plens)).grad_fn is None
    sims = amd.ops.jointsm_scores(amd.ops.DeviceRepSet.from_padded(q, qlens), amd.ops.DeviceRepSet.from_padded(pos, plens),
                                  pairing=amd.lib.PAIR_PAIRED)
    assert torch.equal(d_plain, (-1.0 * sims).cpu())
