"""GPU: the supervised-alignment distances l2sup / l2sup_weighted, forward and backward (aspire_l2sup_scores_f32,
aspire_l2sup_backward_f32, ops.l2sup_scores / l2sup_backward, torch.ops.aspire.l2sup_pair_scores / l2sup_pair_backward, and
allpair_masked_dist_l2sup / allpair_masked_dist_l2sup_weighted in aspire_amd.pair_distances) against the reference's fp32 distances
in tests/golden/trainside.npz and against float64 torch autograd on the CPU through torch.cdist of the two aligned rows
(tests/golden/trainside_inputs.py).  Cases (L2SUP_CASES): extent 8 with lens (1, 1), (3, 8), (8, 2), (5, 5) and indices in range
(e8), at the last valid row (e8last), beyond the length (e8clip: clipped to e8last's) and on coincident rows (e8co: d == 0); one
pair at extent 40 (e40) and one at 128 x 128 (full).

Tolerance, per case and form (w0 plain, w1 weighted): gradients max(4 * ref_err, 4 * 2^-23 * max_grad), distances
max(4 * dist_err, 4 * 2^-23 * max_dist), every figure the reference's OWN fp32 deviation from the float64 yardstick as
make_golden_trainside.py recorded it; 4 is the margin for another summation order, the floor four fp32 roundings of the largest
entry.  The kernel's distance is also held to the reference's stored fp32 distance within dist_err plus that bound (both sit that
close to float64).  Largest |kernel - float64| on an MI355X (gradient over the valid rows; distance):

    case      gradient error   bound       distance error   bound
    e8 w0     6.438e-09        6.740e-08   1.299e-06        2.127e-05
    e8 w1     3.114e-09        2.276e-08   1.299e-06        2.045e-05
    e8last w0 5.840e-09        8.117e-08   3.123e-07        3.049e-05
    e8last w1 5.840e-09        8.117e-08   5.080e-08        3.049e-05
    e8co w0   2.669e-08        1.093e-07   3.051e-07        1.157e-05
    e8co w1   1.309e-08        9.421e-08   3.051e-07        1.148e-05
    e40 w0    1.657e-08        9.276e-08   2.193e-07        1.167e-05
    e40 w1    1.348e-11        8.144e-11   4.258e-10        9.154e-09
    full w0   5.312e-09        3.239e-08   5.937e-08        1.147e-05
    full w1   3.242e-13        1.977e-12   3.623e-12        7.001e-10

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
FORMS = [0, 1]


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
def _inputs(name):
    q, c, qlens, clens, align, gs = ti.l2sup_inputs(ti.L2SUP_CASES[name])
    return torch.from_numpy(q), torch.from_numpy(c), qlens, clens, align, torch.from_numpy(gs)


@functools.lru_cache(maxsize=None)
def _yardstick(name, weighted):
    """(float64 dist, grad_q, grad_c, gradient bound, distance bound) -- computed once, never written to"""
    q, c, qlens, clens, align, gs = _inputs(name)
    wd, wq, wc = ti.l2sup_ref64(q.numpy(), c.numpy(), qlens, clens, align, weighted, gs.numpy())
    fx, key = _fixture(), f'l2sup_{name}_w{weighted}'
    return (torch.from_numpy(wd), torch.from_numpy(wq), torch.from_numpy(wc), ti.bound(fx[f'{key}_ref_err'], fx[f'{key}_max_grad']),
            ti.bound(fx[f'{key}_dist_err'], fx[f'{key}_max_dist']))


def _clipped(name):
    _, _, qlens, clens, align, _ = _inputs(name)
    return [[min(a0, ql - 1), min(a1, cl - 1)] for (a0, a1), ql, cl in zip(align, qlens, clens)]


def _align_gpu(align):
    return torch.tensor(align, dtype=torch.int32).reshape(-1, 2).cuda()


def _nan_like(t):
    return torch.full_like(t, float('nan'))


def _run(amd, qs, cs, align, gs, weighted):
    """(sims, grad_q_rows, grad_c_rows): the gradients into NaN-filled buffers, so a row the kernel does not write shows"""
    a = _align_gpu(align)
    sims = amd.ops.l2sup_scores(qs, cs, a, weighted)
    gq, gc = amd.ops.l2sup_backward(qs, cs, a, gs.cuda(), weighted, out=(_nan_like(qs.rows), _nan_like(cs.rows)))
    return sims, gq, gc


def _run_padded(amd, name, weighted, align=None):
    q, c, qlens, clens, case_align, gs = _inputs(name)
    sims, gq, gc = _run(amd, amd.ops.DeviceRepSet.from_padded(q, qlens), amd.ops.DeviceRepSet.from_padded(c, clens),
                        case_align if align is None else align, gs, weighted)
    return sims, gq.view(q.shape), gc.view(c.shape)


@pytest.mark.parametrize('weighted', FORMS)
@pytest.mark.parametrize('name', list(ti.L2SUP_CASES))
def test_forward_and_backward_match_the_reference_and_float64(amd, name, weighted):
    q, c, qlens, clens, align, gs = _inputs(name)
    wd, wq, wc, tol, tol_d = _yardstick(name, weighted)
    fx, key = _fixture(), f'l2sup_{name}_w{weighted}'
    sims, gq, gc = (t.cpu() for t in _run_padded(amd, name, weighted))
    dist = -sims
    err_d = (dist.double() - wd).abs().max().item()
    err_ref = (dist.double() - torch.from_numpy(fx[f'{key}_dist']).double()).abs().max().item()
    err = max(max((gq[b, :n].double() - wq[b, :n]).abs().max().item() for b, n in enumerate(qlens)),
              max((gc[b, :n].double() - wc[b, :n]).abs().max().item() for b, n in enumerate(clens)))
    print(f'[{name} w{weighted}] gradient |error| {err:.3e}, bound {tol:.3e}; distance |error| {err_d:.3e}, bound {tol_d:.3e}; '
          f'against the reference\'s fp32 distance {err_ref:.3e}')
    assert torch.isfinite(sims).all() and torch.isfinite(gq).all() and torch.isfinite(gc).all()
    assert err_d <= tol_d and err_ref <= tol_d + float(fx[f'{key}_dist_err'])
    # exactly two non-zero rows per pair (none where the aligned rows coincide); every other row, pads included, exact zeros
    for b, (i, j) in enumerate(_clipped(name)):
        rest_q, rest_c = [r for r in range(q.shape[1]) if r != i], [r for r in range(c.shape[1]) if r != j]
        assert torch.count_nonzero(gq[b, rest_q]) == 0 and torch.count_nonzero(gc[b, rest_c]) == 0
        if b in ti.L2SUP_CASES[name]['same']:
            assert dist[b] == 0 and torch.count_nonzero(gq[b]) == 0 and torch.count_nonzero(gc[b]) == 0, 'd == 0: no gradient'
        else:
            assert torch.count_nonzero(gq[b, i]) > 0 and torch.count_nonzero(gc[b, j]) > 0
    assert err <= tol


def test_indices_beyond_the_length_are_clipped_on_the_device(amd):
    """e8clip's indices are e8last's after clipping, on the same rows: the same bits as the clipped index passed directly."""
    assert _clipped('e8clip') == ti.L2SUP_CASES['e8last']['align'] and _clipped('e8clip') != ti.L2SUP_CASES['e8clip']['align']
    for weighted in FORMS:
        beyond, direct = _run_padded(amd, 'e8clip', weighted), _run_padded(amd, 'e8last', weighted)
        assert all(torch.equal(a, b) for a, b in zip(beyond, direct))
        assert all(torch.equal(a, b) for a, b in zip(beyond, _run_padded(amd, 'e8clip', weighted, align=_clipped('e8clip'))))


@pytest.mark.parametrize('name', ['e8', 'e40'])
def test_weighted_is_unweighted_over_the_block_size(amd, name):
    """within one rounding: both kernels divide what the plain form stores by (float)(q_len * c_len)"""
    _, _, qlens, clens, _, _ = _inputs(name)
    n = torch.tensor([ql * cl for ql, cl in zip(qlens, clens)], dtype=torch.float64)
    plain, weighted = _run_padded(amd, name, 0), _run_padded(amd, name, 1)
    for p, w, div in zip(plain, weighted, (n, n[:, None, None], n[:, None, None])):
        want = p.cpu().double() / div
        assert ((w.cpu().double() - want).abs() <= 2.0 ** -24 * want.abs()).all()


@pytest.mark.parametrize('weighted', FORMS)
def test_csr_equals_padded_bit_for_bit(amd, weighted):
    q, c, qlens, clens, align, gs = _inputs('e8')
    qs = amd.ops.DeviceRepSet.from_list([q[b, :n] for b, n in enumerate(qlens)])
    cs = amd.ops.DeviceRepSet.from_list([c[b, :n] for b, n in enumerate(clens)])
    sims, gq, gc = _run(amd, qs, cs, align, gs, weighted)
    psims, pq, pc = _run_padded(amd, 'e8', weighted)
    assert torch.equal(sims, psims)
    assert torch.equal(gq, torch.cat([pq[b, :n] for b, n in enumerate(qlens)]))          # (a row left unwritten is NaN: it fails here)
    assert torch.equal(gc, torch.cat([pc[b, :n] for b, n in enumerate(clens)]))
    again = _run(amd, qs, cs, align, gs, weighted)
    assert torch.equal(sims, again[0]) and torch.equal(gq, again[1]) and torch.equal(gc, again[2])


def _lens_gpu(lens):
    return torch.tensor(lens, dtype=torch.int32).cuda()


@pytest.mark.parametrize('weighted', [False, True])
def test_operator_forward_bits_and_opcheck(amd, weighted):
    q, c, qlens, clens, align, gs = _inputs('e8')
    ql, cl, a = _lens_gpu(qlens), _lens_gpu(clens), _align_gpu(align)
    sims = torch.ops.aspire.l2sup_pair_scores(q.cuda().requires_grad_(), ql, c.cuda().requires_grad_(), cl, a, weighted)
    assert sims.grad_fn is not None and torch.equal(sims.detach(), _run_padded(amd, 'e8', int(weighted))[0])
    torch.library.opcheck(torch.ops.aspire.l2sup_pair_scores, (q.cuda().requires_grad_(), ql, c.cuda().requires_grad_(), cl, a, weighted))
    torch.library.opcheck(torch.ops.aspire.l2sup_pair_backward, (gs.cuda(), q.cuda(), ql, c.cuda(), cl, a, weighted))


@pytest.mark.parametrize('weighted', FORMS)
def test_reference_names_triplet_loss_end_to_end(amd, weighted):
    """CPU inputs [B, 768, S] with requires_grad through the two reference names: relu(d(q, pos) - d(q, neg) + margin).sum(), one
    backward().  The rows are case e8's: pos its candidates with its alignment, neg the same candidates and their aligned rows moved on
    by one pair.  The bound is e8's for pos and neg, which receive one kernel result each, and twice it for the query, whose gradient
    is the sum of two.  The caller's align_idxs list is left as it was given."""
    fn = amd.pd.allpair_masked_dist_l2sup_weighted if weighted else amd.pd.allpair_masked_dist_l2sup
    q, pos, qlens, plens, pal, _ = _inputs('e8')
    tol = _yardstick('e8', weighted)[3]
    neg, nlens = torch.roll(pos, 1, dims=0), plens[-1:] + plens[:-1]
    nal = [[a[0], pal[i - 1][1] + 10] for i, a in enumerate(pal)]          # (candidate indices beyond the lengths: clipped)
    nal64 = [[a[0], min(a[1], nl - 1)] for a, nl in zip(nal, nlens)]
    margin = 0.5
    y = [t.double().clone().requires_grad_() for t in (q, pos, neg)]
    hinge = ti.l2sup_dists(y[0], y[1], qlens, plens, pal, weighted) - ti.l2sup_dists(y[0], y[2], qlens, nlens, nal64, weighted) + margin
    assert (hinge.abs() > 1e-3).all() and (hinge > 0).any() and (hinge < 0).any()      # no pair on the hinge's corner, some active
    torch.relu(hinge).sum().backward()
    e = [t.permute(0, 2, 1).contiguous().requires_grad_() for t in (q, pos, neg)]
    tup, ali = amd.pd.rep_len_tup, amd.pd.rep_len_ali_tup
    given = [list(a) for a in nal]
    d_pos = fn(tup(embed=e[0], abs_lens=qlens), ali(embed=e[1], abs_lens=plens, align_idxs=pal))
    d_neg = fn(tup(embed=e[0], abs_lens=qlens), ali(embed=e[2], abs_lens=nlens, align_idxs=nal))
    assert nal == given, 'the clipped indices are not written back'
    assert d_pos.grad_fn is not None and d_pos.device.type == 'cpu' and d_pos.shape == (len(qlens),)
    wd, _, _, _, tol_d = _yardstick('e8', weighted)
    assert ((d_pos.detach().double() - wd).abs() <= tol_d).all()
    torch.relu(d_pos - d_neg + margin).sum().backward()
    for what, got, want, lens, t in zip(('query', 'pos', 'neg'), e, y, (qlens, plens, nlens), (2 * tol, tol, tol)):
        assert got.grad.shape == got.shape == (len(qlens), D, 8) and got.grad.device.type == 'cpu'
        grad = got.grad.permute(0, 2, 1)
        err = max((grad[b, :n].double() - want.grad[b, :n]).abs().max().item() for b, n in enumerate(lens))
        print(f'[l2sup w{weighted} {what}] kernel |error| {err:.3e}, bound {t:.3e}')
        assert err <= t
        for b, n in enumerate(lens):
            assert torch.count_nonzero(grad[b, n:]) == 0
    # without requires_grad and under no_grad: no graph, the same bits
    plain = [t.detach() for t in e]
    d_plain = fn(tup(embed=plain[0], abs_lens=qlens), ali(embed=plain[1], abs_lens=plens, align_idxs=pal))
    assert d_plain.grad_fn is None and not d_plain.requires_grad and torch.equal(d_plain, d_pos.detach())
    with torch.no_grad():
        assert fn(tup(embed=e[0], abs_lens=qlens), ali(embed=e[1], abs_lens=plens, align_idxs=pal)).grad_fn is None
    assert torch.equal(d_plain, (-1 * _run_padded(amd, 'e8', weighted)[0]).cpu())
