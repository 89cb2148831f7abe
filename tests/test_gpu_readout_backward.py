"""GPU: the read-out under autograd -- the backward of the span mean pool (aspire_span_mean_pool_backward_f32,
ops.span_mean_pool_backward, torch.ops.aspire.span_mean_pool_backward and the autograd of torch.ops.aspire.span_mean_pool), the
backward of the CLS distance (aspire_cls_l2_backward_f32, torch.ops.aspire.cls_l2_pair) and aspire_amd.RankLoss.forward_rank, the
reference's rank loss from last_hidden_state to the loss and back, for every aggregation, explicit and in-batch negatives,
abs_loss_prop 0 and 0.5.  Inputs, yardsticks (float64 torch on the CPU) and cases: tests/golden/readout_inputs.py; the reference's own
fp32 figures: tests/golden/readout.npz (make_golden_readout.py).

Tolerance, everywhere: trainside_inputs.bound = max(4 * ref_err, 4 * 2^-23 * max|grad|), ref_err the REFERENCE's fp32 deviation from
the float64 yardstick as the generator recorded it (for 'l2wasserstein' the fp32 run of the restatement the OT backward's tests use),
4 the margin for another summation order, the floor four fp32 roundings of the largest entry; losses the same way from loss_err and
|loss|.  Pool case 'c' (positions listed twice, shared by two slots, unsorted: nothing the reference's mask can express) is held to
the stated sum order bit for bit instead, and to float64 within the floor.

Largest |kernel - float64| on an MI355X (pool and CLS cases: the gradient; rank-loss cases: the loss, then the largest gradient error
over the query / positive / negative hidden states):

    case                        error       bound        loss error  bound       gradient error  bound
    pool a                      2.384e-08   1.948e-06
    pool b                      1.192e-07   2.393e-06
    pool c                      1.192e-07   1.675e-06
    pool d                      3.974e-08   1.623e-06
    pool a gs=True gc=False     2.384e-08   1.948e-06
    pool a gs=False gc=True     0.000e+00   1.948e-06
    pool a gs=False gc=False    0.000e+00   1.948e-06
    cls b5                      2.286e-08   1.246e-07
    cls same                    7.161e-09   4.036e-08
    cls b1                      2.397e-09   1.533e-08
    l2max_neg_a0                                         2.189e-07   4.690e-06   9.732e-09       4.172e-08
    l2max_neg_a5                                         7.538e-08   5.478e-06   9.970e-09       4.172e-08
    l2max_inb_a0                                         4.462e-07   7.752e-06   2.633e-09       3.661e-08
    l2max_inb_a5                                         5.347e-07   7.398e-06   7.957e-09       3.661e-08
    l2top2_neg_a0                                        1.003e-06   6.910e-06   1.124e-08       5.785e-08
    l2top2_neg_a5                                        1.297e-06   8.458e-06   1.124e-08       5.785e-08
    l2top2_inb_a0                                        9.208e-07   5.854e-06   3.708e-09       4.052e-08
    l2top2_inb_a5                                        1.009e-06   5.499e-06   7.957e-09       4.052e-08
    l2attention_neg_a0                                   1.260e-07   4.319e-06   4.676e-09       3.371e-08
    l2attention_neg_a5                                   4.203e-07   5.496e-06   9.970e-09       3.988e-08
    l2attention_inb_a0                                   2.562e-07   1.979e-06   1.717e-09       3.201e-08
    l2attention_inb_a5                                   1.677e-07   1.624e-06   7.957e-09       3.299e-08
    l2wasserstein_neg_a0                                 5.786e-07   3.867e-06   8.094e-09       1.590e-07
    l2wasserstein_neg_a5                                 2.843e-07   5.414e-06   9.970e-09       1.590e-07
    l2wasserstein_inb_a0                                 4.931e-07   1.019e-06   3.175e-09       8.428e-08
    l2wasserstein_inb_a5                                 4.045e-07   1.378e-06   7.957e-09       8.428e-08
    jointsm_neg_a0                                       1.888e-06   1.478e-05   1.236e-08       9.567e-08
    jointsm_neg_a5                                       1.594e-06   1.633e-05   1.236e-08       9.567e-08
    jointsm_inb_a0                                       5.435e-08   5.185e-07   1.325e-08       7.740e-08
    jointsm_inb_a5                                       1.429e-07   9.714e-07   1.325e-08       7.740e-08
    small_l2max_neg_a5                                   9.047e-08   2.547e-06   8.271e-09       3.961e-08
    small_l2top2_inb_a0                                  3.839e-07   5.350e-06   1.119e-08       6.152e-08
    small_l2attention_inb_a5                             1.410e-07   2.297e-06   9.155e-09       4.258e-08

Every pool case equals the fp32 restatement of the stated sum order in every bit.

Every comparison prints its figures before it asserts (pytest -s shows them)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import readout_inputs as ri  # noqa: E402

pytestmark = pytest.mark.gpu
D = 768


@pytest.fixture(scope='module')
def amd():
    import aspire_amd
    from aspire_amd import ops, _lib, batch_prep
    import aspire_amd.torch_ops as torch_ops
    assert torch.cuda.is_available()
    return type('NS', (), dict(pkg=aspire_amd, ops=ops, lib=_lib, to=torch_ops, prep=batch_prep))


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'readout.npz'))


@functools.lru_cache(maxsize=None)
def _pool_case(name):
    return ri.pool_case(name)


@functools.lru_cache(maxsize=None)
def _pool_yardstick(name, use_gs=True, use_gc=True):
    """(float64 gradient, the stated order in fp32) -- computed once, never written to"""
    case = _pool_case(name)
    return ri.pool_grad64(case, use_gs, use_gc), ri.pool_grad32_ordered(case, use_gs, use_gc)


def _pool_bound(name, g64):
    fx = _fixture()
    ref_err = float(fx[f'pool_{name}_ref_err']) if f'pool_{name}_ref_err' in fx else 0.0
    return ri.bound(ref_err, np.abs(g64).max())


def _csr(amd, case):
    tok_idx, span_off = amd.prep.spans_to_csr(case['spans'], case['S'])
    return tok_idx.cuda(), span_off.cuda()


def _abi(amd, case, use_gs=True, use_gc=True, fill=float('nan')):
    """the C ABI through ops, into a NaN-filled buffer: an element the kernel does not write shows"""
    tok_idx, span_off = _csr(amd, case)
    gs = torch.from_numpy(case['gs']).cuda() if use_gs else None
    gc = torch.from_numpy(case['gc']).cuda() if use_gc else None
    out = torch.full((case['B'], case['L'], D), fill, device='cuda', dtype=torch.float32)
    got = amd.ops.span_mean_pool_backward(gs, gc, tok_idx, span_off, case['B'], case['L'], case['S'], out=out)
    assert got is out
    return out.cpu().numpy()


def _free_rows(case):
    used = {(b, t) for b, doc in enumerate(case['spans']) for span in doc for t in span} | {(b, 0) for b in range(case['B'])}
    return [(b, t) for b in range(case['B']) for t in range(case['L']) if (b, t) not in used]


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd'])
def test_pool_backward_abi_and_operator_match_float64(amd, name):
    case = _pool_case(name)
    g64, g32 = _pool_yardstick(name)
    got = _abi(amd, case)
    assert not np.isnan(got).any(), 'an element was not written'
    tok_idx, span_off = _csr(amd, case)
    op = torch.ops.aspire.span_mean_pool_backward(torch.from_numpy(case['gs']).cuda(), torch.from_numpy(case['gc']).cuda(), tok_idx,
                                                  span_off, case['B'], case['L'], case['S']).cpu().numpy()
    assert np.array_equal(op.view(np.int32), got.view(np.int32)), 'operator and C ABI differ in bits'
    err, tol = float(np.abs(got - g64).max()), _pool_bound(name, g64)
    print(f'[pool {name}] |kernel - float64| {err:.3e}, bound {tol:.3e}; differs from the stated order in {(got != g32).sum()} entries')
    assert err <= tol
    assert np.array_equal(got.view(np.int32), g32.view(np.int32)), 'not the stated sum order'
    free = _free_rows(case)
    assert all((got[b, t] == 0).all() for b, t in free)
    if name == 'd':
        assert len(free) > case['B'] * case['L'] // 2       # the largest part of the rows is in no span


def test_pool_backward_through_autograd_gives_the_abi_bits(amd):
    """loss = sum(gs * sent) + sum(gc * cls): the formula receives gs and gc themselves"""
    for name in ('a', 'c'):
        case = _pool_case(name)
        tok_idx, span_off = _csr(amd, case)
        hidden = torch.randn(case['B'], case['L'], D, device='cuda', generator=torch.Generator('cuda').manual_seed(7)).requires_grad_(True)
        plain = amd.ops.span_mean_pool(hidden.detach(), tok_idx, span_off, case['S'])
        cls, sent = torch.ops.aspire.span_mean_pool(hidden, tok_idx, span_off, case['S'])
        assert torch.equal(cls, plain[0]) and torch.equal(sent, plain[1]), 'the forward keeps its bits'
        ((sent * torch.from_numpy(case['gs']).cuda()).sum() + (cls * torch.from_numpy(case['gc']).cuda()).sum()).backward()
        assert np.array_equal(hidden.grad.cpu().numpy().view(np.int32), _abi(amd, case).view(np.int32))
        cls, sent = torch.ops.aspire.span_mean_pool(hidden.detach(), tok_idx, span_off, case['S'])
        assert not cls.requires_grad and not sent.requires_grad


@pytest.mark.parametrize('use_gs,use_gc', [(True, False), (False, True), (False, False)])
def test_pool_backward_with_a_term_absent(amd, use_gs, use_gc):
    """a NULL gradient is an absent term; with both NULL every element is an exact zero (and still written)"""
    case = _pool_case('a')
    g64, g32 = _pool_yardstick('a', use_gs, use_gc)
    got = _abi(amd, case, use_gs, use_gc)
    err, tol = float(np.abs(got - g64).max()), _pool_bound('a', _pool_yardstick('a')[0])
    print(f'[pool a gs={use_gs} gc={use_gc}] |kernel - float64| {err:.3e}, bound {tol:.3e}')
    assert not np.isnan(got).any() and err <= tol
    assert np.array_equal(got.view(np.int32), g32.view(np.int32))
    if not use_gs and not use_gc:
        assert (got == 0).all()
    # through autograd: the output the loss does not read arrives as None
    tok_idx, span_off = _csr(amd, case)
    if use_gs or use_gc:
        hidden = torch.zeros(case['B'], case['L'], D, device='cuda', requires_grad=True)
        cls, sent = torch.ops.aspire.span_mean_pool(hidden, tok_idx, span_off, case['S'])
        ((sent * torch.from_numpy(case['gs']).cuda()).sum() if use_gs else (cls * torch.from_numpy(case['gc']).cuda()).sum()).backward()
        assert np.array_equal(hidden.grad.cpu().numpy().view(np.int32), got.view(np.int32))


def test_pool_backward_repeats_its_bits_and_ignores_indices_outside_the_sequence(amd):
    for name in ('c', 'd'):
        assert np.array_equal(_abi(amd, _pool_case(name)).view(np.int32), _abi(amd, _pool_case(name), fill=1.0).view(np.int32))
    # positions outside [0, L) count in the slot's divisor (as the forward would count them) and land nowhere
    case = dict(_pool_case('c'))
    case['spans'] = [[[5, -1, 6, 33], [7, 1 << 30, 8], [0, 32, -(1 << 31)]], [[1, 2, 3], [40, 41], []]]
    got = _abi(amd, case)
    want = ri.pool_grad32_ordered(case)
    assert not np.isnan(got).any() and np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize('name', ['b5', 'same', 'b1'])
def test_cls_l2_backward_matches_float64_autograd(amd, name):
    q, c, g = ri.cls_case(name)
    d64, q64, c64 = ri.cls_ref(q, c, g, torch.float64)
    fx = _fixture()
    tol = ri.bound(fx[f'cls_{name}_ref_err'], fx[f'cls_{name}_max_grad'])
    qt, ct = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    nan = torch.full_like(qt, float('nan'))
    gq, gc = amd.ops.cls_l2_backward(qt, ct, torch.from_numpy(g).cuda(), out=(nan, nan.clone()))
    err = max(float(np.abs(gq.cpu().numpy() - q64).max()), float(np.abs(gc.cpu().numpy() - c64).max()))
    print(f'[cls {name}] dist {d64.min():.4g} .. {d64.max():.4g}: |kernel - float64| {err:.3e}, bound {tol:.3e}')
    assert not torch.isnan(gq).any() and not torch.isnan(gc).any() and err <= tol
    assert torch.equal(gc, -gq)
    if name == 'same':
        assert abs(d64[1] - 1e-6 * np.sqrt(768.0)) < 1e-12
    # the operator: today's forward bits, the same gradient bits
    ql, cl = qt.clone().requires_grad_(True), ct.clone().requires_grad_(True)
    dist = torch.ops.aspire.cls_l2_pair(ql, cl, 1e-6)
    assert torch.equal(dist, amd.ops.cls_l2(qt, ct)) and float(np.abs(dist.detach().cpu().numpy() - d64).max()) <= ri.bound(0.0, d64.max())
    (dist * torch.from_numpy(g).cuda()).sum().backward()
    assert torch.equal(ql.grad, gq) and torch.equal(cl.grad, gc)
    with pytest.raises(NotImplementedError, match='ASPIRE_PAIR_PAIRED'):
        amd.lib.check(amd.lib.lib.aspire_cls_l2_backward_f32(amd.ops._ptr(qt), len(q), amd.ops._ptr(ct), len(q), D, amd.lib.PAIR_CROSS, 1e-6,
                                                             amd.ops._ptr(qt), amd.ops._ptr(gq), amd.ops._ptr(gc), None))


# ---- RankLoss.forward_rank ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rank_inputs(size):
    return ri.rank_inputs(size)


@functools.lru_cache(maxsize=None)
def _rank_yardstick(name):
    """(float64 loss, float64 hidden-state gradients) -- computed once per case, never written to"""
    size, agg, neg, prop = ri.RANK_CASES[name]
    loss, grads, _ = ri.rank_loss64(_rank_inputs(size), agg, neg, prop)
    return loss, grads


@pytest.mark.parametrize('name', list(ri.RANK_CASES))
def test_forward_rank_loss_and_hidden_gradients(amd, name):
    size, agg, neg, prop = ri.RANK_CASES[name]
    inp, fx = _rank_inputs(size), _fixture()
    want_loss, want = _rank_yardstick(name)
    leaves, batch = {}, {}
    for w, key in (('q', 'query'), ('p', 'pos'), ('n', 'neg'))[:3 if neg else 2]:
        leaves[w] = torch.from_numpy(inp[w + '_hidden']).cuda().requires_grad_(True)
        batch[key + '_bert_batch'] = {'which': w}
        batch[key + '_abs_lens'] = list(inp[w + '_lens'])
        batch[key + '_senttok_idxs'] = inp[w + '_idxs']
    calls = []

    def encoder(bert_batch):
        calls.append(bert_batch['which'])
        return leaves[bert_batch['which']]

    loss = amd.pkg.RankLoss(ri.hparams(agg, prop)).forward_rank(batch, encoder, random_idxs=None if neg else torch.tensor(inp['perm']))
    assert calls == list(leaves) and loss.is_cuda and loss.dim() == 0
    loss.backward()
    loss_tol = ri.bound(fx[f'{name}_loss_err'], fx[f'{name}_max_loss'])
    grad_tol = ri.bound(fx[f'{name}_ref_err'], fx[f'{name}_max_grad'])
    loss_err = abs(loss.item() - want_loss)
    errs = [float(np.abs(leaves[w].grad.cpu().numpy() - g).max()) for w, g in zip(leaves, want)]
    print(f'[{name}] loss {loss.item():.6f} |kernel - float64| {loss_err:.3e} bound {loss_tol:.3e} (reference {float(fx[f"{name}_loss"]):.6f}); '
          f'gradients {" ".join(f"{e:.3e}" for e in errs)} bound {grad_tol:.3e}')
    assert loss_err <= loss_tol
    if agg in ri.REF_AGGS:        # the reference's own fp32 loss sits loss_err from float64
        assert abs(loss.item() - float(fx[f'{name}_loss'])) <= loss_tol + float(fx[f'{name}_loss_err'])
    assert max(errs) <= grad_tol
    for w in leaves:
        g = leaves[w].grad.cpu().numpy()
        for b, doc in enumerate(inp[w + '_idxs']):
            free = sorted(set(range(1, inp['L'])) - {t for span in doc for t in span})
            assert free and (g[b, free] == 0).all(), 'a token of no span has a gradient'
            if prop == 0:
                assert (g[b, 0] == 0).all()       # the CLS rows took no part in the loss
    if name in ri.SMALL_CASES:        # the reference's stored gradients themselves
        for w in leaves:
            dev = float(np.abs(leaves[w].grad.cpu().numpy() - fx[f'{name}_grad_{w}']).max())
            assert dev <= grad_tol + float(fx[f'{name}_ref_err'])


def test_forward_rank_without_grad_attaches_nothing_and_keeps_the_loss(amd):
    inp = _rank_inputs('std')
    hid = {w: torch.from_numpy(inp[w + '_hidden']).cuda() for w in 'qp'}
    batch = {}
    for w, key in (('q', 'query'), ('p', 'pos')):
        batch.update({key + '_bert_batch': w, key + '_abs_lens': inp[w + '_lens'], key + '_senttok_idxs': inp[w + '_idxs']})
    rank = amd.pkg.RankLoss(ri.hparams('l2max', 0.5))
    plain = rank.forward_rank(batch, lambda w: hid[w], random_idxs=inp['perm'])
    assert not plain.requires_grad
    attached = rank.forward_rank(batch, lambda w: hid[w].clone().requires_grad_(True), random_idxs=inp['perm'])
    assert attached.requires_grad and torch.equal(plain, attached.detach())
    with pytest.raises(IndexError, match='out of range'):
        amd.pkg.sent_reps_from_hidden(hid['q'], inp['q_lens'], [[[1, inp['L']]]] * inp['B'])
