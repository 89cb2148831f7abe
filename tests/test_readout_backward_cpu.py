"""CPU: the read-out's backward without a GPU -- the two new C-ABI entries (aspire_span_mean_pool_backward_f32,
aspire_cls_l2_backward_f32: declared, exported, signed; ABI still 6), their argument checks that return before any launch, the three
new operators with their fakes and the autograd of span_mean_pool / cls_l2_pair on meta tensors, RankLoss's refusals, torch's
sub-gradient at the hinge's kink, and the fixture tests/golden/readout.npz held against the yardsticks the GPU tests use: the float64
restatements of tests/golden/readout_inputs.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import readout_inputs as ri  # noqa: E402

FAKE = 16            # a non-null, 16-byte aligned "device pointer" that no call of this file reaches
DECLS = {
    'aspire_span_mean_pool_backward_f32': ['const float* grad_sent', 'const float* grad_cls', 'int64_t B', 'int64_t L', 'int64_t D',
                                           'const int32_t* tok_idx', 'const int32_t* span_off', 'int64_t S', 'float* grad_hidden',
                                           'void* stream'],
    'aspire_cls_l2_backward_f32': ['const float* q_cls', 'int64_t Q', 'const float* c_cls', 'int64_t C', 'int64_t D', 'int pairing',
                                   'double eps', 'const float* grad_dist', 'float* grad_q', 'float* grad_c', 'void* stream'],
}
F64_SLACK = 1e-12    # the float64 yardstick is formed again on the machine that runs the test (tests/test_trainside_backward_cpu.py)


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'readout.npz'))


def test_entries_are_declared_exported_and_signed():
    from aspire_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'aspire_hip.h')).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    for name, want in DECLS.items():
        decl = [a.strip() for a in re.search(name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')]
        assert decl == want, name
        assert hasattr(raw, name), f'{name} is not exported'
    assert _lib.SIGNATURES['aspire_span_mean_pool_backward_f32'] == (i, [vp, vp, i64, i64, i64, vp, vp, i64, vp, vp])
    assert _lib.SIGNATURES['aspire_cls_l2_backward_f32'] == (i, [vp, i64, vp, i64, i64, i, ctypes.c_double, vp, vp, vp, vp])
    assert all(callable(getattr(ops, f)) for f in ('span_mean_pool_backward', 'cls_l2_backward'))
    assert _lib.lib.aspire_abi_version() == 6
    assert '#define ASPIRE_ABI_VERSION 6' in open(os.path.join(root, 'include', 'aspire_hip.h')).read()


def test_pool_backward_validation_without_gpu():
    from aspire_amd import _lib
    INVALID, UNSUPPORTED, OK = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED, _lib.ASPIRE_OK
    err = _lib.lib.aspire_last_error
    base = dict(gs=FAKE, gc=FAKE, B=2, L=8, D=768, tok=FAKE, off=FAKE, S=3, out=None)

    def status(**kw):
        a = dict(base, **kw)
        return _lib.lib.aspire_span_mean_pool_backward_f32(a['gs'], a['gc'], a['B'], a['L'], a['D'], a['tok'], a['off'], a['S'], a['out'], None)

    # (grad_hidden is null in every call that passes the other checks: it ends in "null pointer", never in a launch)
    assert status() == INVALID and b'null pointer' in err()
    assert status(gs=None, gc=None) == INVALID and b'null pointer' in err()
    assert status(off=None, out=FAKE) == INVALID and b'null pointer' in err()        # span_off beside grad_sent
    assert status(D=512, out=FAKE) == UNSUPPORTED and b'768' in err()
    with pytest.raises(NotImplementedError, match='768'):
        _lib.check(status(D=512, out=FAKE))
    assert status(S=0) == INVALID and b'bad shape' in err()
    assert status(B=-1) == INVALID and b'bad shape' in err()
    assert status(L=-1) == INVALID and b'bad shape' in err()
    assert status(gs=FAKE + 4, out=FAKE) == INVALID and b'16-byte aligned' in err()
    assert status(gs=None, off=None, out=FAKE + 8) == INVALID and b'16-byte aligned' in err()
    assert status(B=0, gs=None, gc=None, tok=None, off=None) == OK        # nothing to do: no buffers needed, no launch
    assert status(L=0, gs=None, gc=None, tok=None, off=None) == OK
    assert status(B=1 << 31, L=64) == INVALID       # (null grad_hidden comes first; with it the grid check answers:)
    assert status(B=1 << 31, L=64, out=FAKE) == UNSUPPORTED and b'in one call' in err()


def test_cls_l2_backward_validation_without_gpu():
    from aspire_amd import _lib
    INVALID, UNSUPPORTED, OK = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED, _lib.ASPIRE_OK
    err = _lib.lib.aspire_last_error
    base = dict(q=FAKE, Q=3, c=FAKE, C=3, D=768, pairing=_lib.PAIR_PAIRED, eps=1e-6, g=FAKE, gq=FAKE, gc=None)

    def status(**kw):
        a = dict(base, **kw)
        return _lib.lib.aspire_cls_l2_backward_f32(a['q'], a['Q'], a['c'], a['C'], a['D'], a['pairing'], a['eps'], a['g'], a['gq'], a['gc'], None)

    assert status() == INVALID and b'null pointer' in err()
    for name in ('q', 'c', 'g', 'gq'):
        assert status(gc=FAKE, **{name: None}) == INVALID and b'null pointer' in err()
    assert status(pairing=_lib.PAIR_CROSS, gc=FAKE) == UNSUPPORTED and b'accumulation across pairs' in err()
    with pytest.raises(NotImplementedError, match='ASPIRE_PAIR_PAIRED'):
        _lib.check(status(pairing=_lib.PAIR_CROSS, gc=FAKE))
    assert status(pairing=2) == INVALID and b'bad pairing' in err()
    assert status(C=4) == INVALID and b'equal batch sizes' in err()
    assert status(D=512, gc=FAKE) == UNSUPPORTED and b'768' in err()
    assert status(gc=FAKE + 4) == INVALID and b'16-byte aligned' in err()
    assert status(Q=0, C=0, q=None, c=None, g=None, gq=None) == OK            # no pairs: nothing to do, no buffers needed


def _m(*s, dt=torch.float32):
    return torch.empty(*s, device='meta', dtype=dt)


def test_new_operators_are_registered_with_fakes():
    import aspire_amd.torch_ops as to
    i32 = torch.int32
    for name in ('span_mean_pool_backward', 'cls_l2_pair', 'cls_l2_pair_backward'):
        assert name in to.OPS and hasattr(torch.ops.aspire, name)
    assert len(set(to.OPS)) == len(to.OPS)
    for gs, gc in ((_m(2, 3, 768), _m(2, 768)), (None, _m(2, 768)), (_m(2, 3, 768), None), (None, None)):
        g = torch.ops.aspire.span_mean_pool_backward(gs, gc, _m(11, dt=i32), _m(7, dt=i32), 2, 9, 3)
        assert g.shape == (2, 9, 768) and g.dtype == torch.float32 and g.device.type == 'meta'
    d = torch.ops.aspire.cls_l2_pair(_m(4, 768), _m(4, 768), 1e-6)
    assert d.shape == (4,) and d.dtype == torch.float32 and d.device.type == 'meta'
    gq, gc = torch.ops.aspire.cls_l2_pair_backward(_m(4), _m(4, 768), _m(4, 768), 1e-6)
    assert gq.shape == gc.shape == (4, 768) and gq.dtype == gc.dtype == torch.float32
    with pytest.raises(AssertionError):      # paired rows: equal batch sizes
        torch.ops.aspire.cls_l2_pair(_m(3, 768), _m(5, 768), 1e-6)


@pytest.mark.parametrize('use', ['sent', 'cls', 'both'])
def test_span_mean_pool_carries_an_autograd_formula(use):
    """a fake forward of a hidden state that requires grad is attached to the graph, whichever output the loss reads (the other one
    arrives at the formula as None, not as zeros: set_materialize_grads(False)); without requires_grad nothing is attached"""
    import aspire_amd.torch_ops  # noqa: F401
    h = torch.empty(2, 9, 768, device='meta', requires_grad=True)
    cls, sent = torch.ops.aspire.span_mean_pool(h, _m(11, dt=torch.int32), _m(7, dt=torch.int32), 3)
    assert cls.shape == (2, 768) and sent.shape == (2, 3, 768) and sent.requires_grad and cls.requires_grad
    loss = {'sent': sent.sum(), 'cls': cls.sum(), 'both': sent.sum() + cls.sum()}[use]
    loss.backward()
    assert h.grad.shape == (2, 9, 768)
    cls, sent = torch.ops.aspire.span_mean_pool(_m(2, 9, 768), _m(11, dt=torch.int32), _m(7, dt=torch.int32), 3)
    assert not cls.requires_grad and not sent.requires_grad and sent.grad_fn is None


def test_cls_l2_pair_carries_an_autograd_formula():
    import aspire_amd.torch_ops  # noqa: F401
    q = torch.empty(3, 768, device='meta', requires_grad=True)
    c = torch.empty(3, 768, device='meta', requires_grad=True)
    d = torch.ops.aspire.cls_l2_pair(q, c, 1e-6)
    assert d.requires_grad and d.grad_fn is not None
    d.sum().backward()
    assert q.grad.shape == (3, 768) and c.grad.shape == (3, 768)
    assert not torch.ops.aspire.cls_l2_pair(_m(3, 768), _m(3, 768), 1e-6).requires_grad


def test_no_cpu_kernel_behind_the_new_operators():
    import aspire_amd.torch_ops  # noqa: F401
    z, i = torch.zeros(1, 768), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.span_mean_pool_backward(torch.zeros(1, 1, 768), z, i, i, 1, 4, 1)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.cls_l2_pair(z, z, 1e-6)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.cls_l2_pair_backward(torch.zeros(1), z, z, 1e-6)


def test_rank_loss_refusals_and_defaults():
    import aspire_amd
    from aspire_amd import pair_distances as pd
    from aspire_amd.rank_loss import RankLoss
    assert aspire_amd.RankLoss is RankLoss and callable(aspire_amd.sent_reps_from_hidden)
    with pytest.raises(ValueError, match='Unknown aggregation'):
        RankLoss({'score_aggregation': 'cosine'})
    with pytest.raises(KeyError):
        RankLoss({})
    for key in ('cd_l1_prop', 'cd_svalue_l1_prop'):
        with pytest.raises(NotImplementedError, match=key):
            RankLoss({'score_aggregation': 'l2max', key: 0.1})
        RankLoss({'score_aggregation': 'l2max', key: 0.0})
    loss = RankLoss({'score_aggregation': 'l2max'})
    assert loss.sent_loss_prop == 1.0 and loss.abs_loss_prop == 0.0 and loss.dist_function is pd.allpair_masked_dist_l2max
    assert RankLoss({'score_aggregation': 'l2top2'}).dist_function is pd.allpair_masked_dist_l2topk
    assert RankLoss({'score_aggregation': 'jointsm'}).dist_function is pd.allpair_joint_sm_negscore
    att = RankLoss({'score_aggregation': 'l2attention', 'cdatt_sm_temp': 2.0}).dist_function
    assert isinstance(att.__self__, pd.AllPairMaskedAttention) and att.__self__.cdatt_sm_temp == 2.0
    ot = RankLoss({'score_aggregation': 'l2wasserstein', 'geoml_blur': 0.1, 'abs_loss_prop': '0.5', 'sent_loss_prop': 2}).dist_function
    assert isinstance(ot.__self__, pd.AllPairMaskedWasserstein) and ot.__self__.geoml_blur == 0.1


def test_sent_reps_from_hidden_checks_ranges_before_the_gpu():
    from aspire_amd.rank_loss import sent_reps_from_hidden
    hidden = torch.zeros(2, 10, 768)
    for bad in ([[[1, 2], [10]], [[3]]], [[[1, 2]], [[-1, 3]]]):
        with pytest.raises(IndexError, match='out of range'):
            sent_reps_from_hidden(hidden, [2, 1], bad)


def test_hinge_subgradient_at_the_kink_is_torchs():
    """what RankLoss's docstring says: clamp_min passes the gradient where the input equals the bound"""
    x = torch.tensor([-1.0, 0.0, 1.0], requires_grad=True)
    torch.clamp_min(x, 0).sum().backward()
    assert x.grad.tolist() == [0.0, 1.0, 1.0]


def test_fixture_is_small_and_names_every_case(fixture, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, 'readout.npz')) < 1000 * 1000
    assert list(fixture['rank_cases']) == list(ri.RANK_CASES)
    for name, (size, agg, neg, prop) in ri.RANK_CASES.items():
        assert list(fixture[f'{name}_perm']) == ri.SIZES[size]['perm']
        assert fixture[f'{name}_ref_err'] > 0 and fixture[f'{name}_max_grad'] > 0 and fixture[f'{name}_loss'] > 0
    assert any(i == p for i, p in enumerate(ri.SIZES['std']['perm'])), 'the in-batch permutation keeps a fixed point'
    for name in ('a', 'b', 'd'):
        assert fixture[f'pool_{name}_max_grad'] > 0


@pytest.mark.parametrize('name', list(ri.SMALL_CASES))
def test_rank_yardstick_is_the_reference(fixture, name):
    """The float64 restatement the GPU test holds RankLoss to sits within ref_err of the reference's stored fp32 gradients and
    loss_err of its loss; both give exact zeros to the tokens of no span (position 0 aside)."""
    size, agg, neg, prop = ri.RANK_CASES[name]
    inp = ri.rank_inputs(size)
    loss, grads, parts = ri.rank_loss64(inp, agg, neg, prop)
    assert (parts['sent'] > 0).any() and (parts['sent'] < 0).any() and np.abs(parts['sent']).min() > 1e-3
    assert abs(float(fixture[f'{name}_loss']) - loss) <= float(fixture[f'{name}_loss_err']) + F64_SLACK
    assert abs(max(np.abs(g).max() for g in grads) - float(fixture[f'{name}_max_grad'])) <= 1e-12
    err = 0.0
    for g64, key in zip(grads, 'qpn'):
        ref = fixture[f'{name}_grad_{key}']
        assert ref.shape == g64.shape and ref.dtype == np.float32
        err = max(err, float(np.abs(ref - g64).max()))
        for b, doc in enumerate(inp[key + '_idxs']):
            free = sorted(set(range(1, inp['L'])) - {t for span in doc for t in span})
            assert free and not ref[b, free].any() and not g64[b, free].any()
    print(f'[{name}] |float64 - reference| {err:.3e}, ref_err {float(fixture[f"{name}_ref_err"]):.3e}')
    assert err <= float(fixture[f'{name}_ref_err']) + F64_SLACK


@pytest.mark.parametrize('agg', ri.AGGS)
def test_rank_cases_have_an_active_and_an_inactive_triple_clear_of_the_kink(agg):
    for neg in (True, False):
        inp = ri.rank_inputs('std')
        _, _, parts = ri.rank_loss64(inp, agg, neg, 0.5)
        for h in (parts['sent'], parts['doc']):
            assert (h > 0).any() and (h < 0).any() and np.abs(h).min() > 1e-3, (agg, neg, h)
        if not neg:
            assert abs(parts["sent"][3] - 1.0) < 1e-12      # the permutation's fixed point: a positive that is its own negative


def test_pool_yardsticks_agree_with_the_stated_order():
    """float64 autograd over the pooling and the fp32 restatement of the stated sum order say the same, within fp32 roundings of
    the few terms a row has; rows of no span are exact zeros in both"""
    for name in ('a', 'b', 'c', 'd'):
        case = ri.pool_case(name)
        g64, g32 = ri.pool_grad64(case), ri.pool_grad32_ordered(case)
        top = float(np.abs(g64).max())
        assert np.abs(g32 - g64).max() <= ri.bound(0.0, top), name
        used = {(b, t) for b, doc in enumerate(case['spans']) for span in doc for t in span} | {(b, 0) for b in range(case['B'])}
        free = [(b, t) for b in range(case['B']) for t in range(case['L']) if (b, t) not in used]
        assert all(not g64[b, t].any() and not g32[b, t].any() for b, t in free)
        if name == 'd':
            assert len(free) > case['B'] * case['L'] // 2
