"""CPU: the training of the CLS-row models without a GPU -- the float64 restatements of tests/cls_train_ref.py against torch's own
nn.TripletMarginLoss, nn.CrossEntropyLoss and autograd, the four new C-ABI symbols against the header's declarations, their argument
checks (every one stands before the first launch: the pointers here are dummies) and the new operators' fake kernels.  The state-dict
key sets of BiEncTrain / SentEncTrain / IctEncTrain need a GPU (HipBertTrainEncoder moves the model there): tests/test_gpu_cls_train.py."""
import ctypes
import os
import re

import pytest
import torch

import cls_train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('aspire_bert_cls_mix_train_f32', 'aspire_bert_layers_backward_cls_f32', 'aspire_inbatch_xent_f32', 'aspire_inbatch_xent_backward_f32')


# ---- 1. the restatements ---------------------------------------------------------------------------------------------------------------
def test_layer_mix_restatement_is_a_linear_layer_over_the_stacked_states():
    g = torch.Generator().manual_seed(0)
    hs = [torch.randn(2, 5, 8, generator=g, dtype=torch.float64) for _ in range(4)]
    weight = torch.randn(1, 4, generator=g, dtype=torch.float64, requires_grad=True)
    got = ref.layer_mix_cls(hs, weight)
    want = torch.nn.functional.linear(torch.stack(hs, dim=3), torch.softmax(weight, dim=1)).squeeze(3)[:, 0, :]
    assert got.shape == (2, 8) and torch.allclose(got, want, rtol=1e-14, atol=1e-14)
    assert torch.equal(ref.layer_cls_rows(hs)[2], hs[2][:, 0])
    one = ref.layer_mix_cls(hs[:1], torch.zeros(1, 1, dtype=torch.float64))          # one state: the mix is 1
    assert torch.equal(one, hs[0][:, 0])


@pytest.mark.parametrize('b', [1, 3])
def test_triplet_restatement_equals_torch(b):
    g = torch.Generator().manual_seed(1)
    a, p, n = (torch.randn(b, 768, generator=g, dtype=torch.float64, requires_grad=True) for _ in range(3))
    scale = 0.02        # distances near the margin: both sides of the hinge occur
    got = ref.triplet_sum(a * scale, p * scale, n * scale)
    want = torch.nn.TripletMarginLoss(margin=1, p=2, reduction='sum')(a * scale, p * scale, n * scale)
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
    for x, y in zip(torch.autograd.grad(got, (a, p, n)), torch.autograd.grad(want, (a, p, n))):
        assert torch.allclose(x, y, rtol=1e-10, atol=1e-14)
    # in-batch negatives with a fixed point: that pair's loss is the margin
    perm = torch.arange(b).roll(1) if b > 1 else torch.arange(b)
    perm[-1] = b - 1
    fixed = ref.triplet_sum(a[-1:], p[-1:], p[perm][-1:])
    assert abs(float(fixed.detach()) - 1.0) <= 1e-12


@pytest.mark.parametrize('b', [1, 2, 17])
def test_inbatch_xent_restatement_equals_torch(b):
    g = torch.Generator().manual_seed(2)
    q, c = (torch.randn(b, 768, generator=g, dtype=torch.float64, requires_grad=True) for _ in range(2))
    got, lse = ref.inbatch_xent(q * 0.2, c * 0.2)
    want = torch.nn.CrossEntropyLoss(reduction='sum')(torch.matmul(q * 0.2, (c * 0.2).T), torch.arange(b))
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-12 * max(abs(float(want.detach())), 1.0)
    assert lse.shape == (b,)
    if b == 1:
        assert float(got.detach()) == 0.0
    for x, y in zip(torch.autograd.grad(got, (q, c)), torch.autograd.grad(want, (q, c))):
        assert torch.allclose(x, y, rtol=1e-10, atol=1e-14)


# ---- 2. the symbols ----------------------------------------------------------------------------------------------------------------------
def _c_type(decl):
    decl = decl.strip()
    if '*' in decl:
        if 'aspire_bert_weights' in decl or 'aspire_bert_grads' in decl or 'aspire_bert_dropout' in decl:
            return 'struct*'
        return ctypes.c_void_p
    return {'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'int': ctypes.c_int}[decl.split()[-2]]


def test_new_symbols_are_exported_with_the_headers_signatures():
    from aspire_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'aspire_hip.h')).read(), flags=re.S)
    want_names = {
        'aspire_bert_cls_mix_train_f32': 'w B L tape tape_bytes hidden_out mix cls_out layer_cls stream',
        'aspire_bert_layers_backward_cls_f32': 'w attn_mask B L grad_hidden grad_cls mix layer_cls tape tape_bytes grad_emb_sum grads grad_mix ws '
                                               'ws_bytes dropout stream',
        'aspire_inbatch_xent_f32': 'q c B D loss row_lse stream',
        'aspire_inbatch_xent_backward_f32': 'q c B D row_lse grad_loss grad_q grad_c stream'}
    for name in NEW:
        assert hasattr(raw, name), name
        res, args = _lib.SIGNATURES[name]
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m, name
        params = [p.strip() for p in m.group(1).split(',')]
        assert [p.split()[-1].lstrip('*') for p in params] == want_names[name].split(), name
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            t = _c_type(p)
            assert (t == 'struct*' and issubclass(a, ctypes._Pointer)) or t is a, (name, p, a)
    assert _lib.lib.aspire_abi_version() == 6          # functions were only added


# ---- 3. the argument checks ---------------------------------------------------------------------------------------------------------------
def _weights(n_layers=2):
    from aspire_amd import _lib
    layers = (_lib.BertLayer * max(n_layers, 1))()
    for i in range(n_layers):
        for f, _ in _lib.BertLayer._fields_:
            setattr(layers[i], f, 16)
    bw = _lib.BertWeights(None, None, None, 16, 16, layers, n_layers, 12, 768, 128, 0, 0, 0, 1e-12, None)
    bw._keep = layers
    return bw


def _grads(n_layers=2):
    from aspire_amd import _lib
    layers = (_lib.BertLayerGrads * max(n_layers, 1))()
    for i in range(n_layers):
        for f, _ in _lib.BertLayerGrads._fields_:
            setattr(layers[i], f, 16)
    bg = _lib.BertGrads(16, 16, layers)
    bg._keep = layers
    return bg


def test_encoder_entry_points_check_their_arguments_before_the_first_launch():
    from aspire_amd import _lib
    lib = _lib.lib
    bw, bg = _weights(), _grads()
    need_t = lib.aspire_bert_tape_bytes(ctypes.byref(bw), 3, 37)
    need_w = lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), 3, 37)
    inval, ok = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_OK

    def tap(b=3, l=37, tape=16, tape_bytes=need_t, hidden=16, mix=16, cls=16, layer_cls=16):
        return lib.aspire_bert_cls_mix_train_f32(ctypes.byref(bw), b, l, tape, tape_bytes, hidden, mix, cls, layer_cls, None)

    assert tap(hidden=None) == inval and b'null' in lib.aspire_last_error()
    assert tap(cls=None) == inval
    assert tap(layer_cls=None) == inval and b'layer_cls' in lib.aspire_last_error()         # a mix needs its rows kept
    assert tap(l=513) == inval and b'513' in lib.aspire_last_error()
    assert tap(tape=None) == inval and tap(tape_bytes=need_t - 1) == inval and str(need_t).encode() in lib.aspire_last_error()
    assert tap(b=0) == ok and tap(b=0, mix=None, layer_cls=None) == ok                     # nothing to do: no launch

    def bwd(b=3, gh=None, gc=16, mix=16, layer_cls=16, tape=16, g=bg, grad_mix=16, ws_bytes=need_w, drop=None):
        return lib.aspire_bert_layers_backward_cls_f32(ctypes.byref(bw), 16, b, 37, gh, gc, mix, layer_cls, tape, need_t, None,
                                                       ctypes.byref(g) if g is not None else None, grad_mix, 16, ws_bytes,
                                                       ctypes.byref(drop) if drop is not None else None, None)

    assert bwd(gc=None, grad_mix=None) == inval and b'grad_hidden and grad_cls' in lib.aspire_last_error()
    assert bwd(layer_cls=None) == inval and b'grad_mix' in lib.aspire_last_error()
    assert bwd(mix=None) == inval and b'grad_mix' in lib.aspire_last_error()
    assert bwd(g=None) == inval
    assert bwd(tape=None) == inval and bwd(ws_bytes=need_w - 1) == inval and str(need_w).encode() in lib.aspire_last_error()
    assert bwd(drop=_lib.BertDropout(0.1, 1.5, 1, 0), b=0) == inval and b'p_attn = 1.5' in lib.aspire_last_error()
    for kw in ({}, dict(gh=16), dict(gh=16, gc=None, mix=None, layer_cls=None, grad_mix=None), dict(mix=None, layer_cls=None, grad_mix=None),
               dict(drop=_lib.BertDropout(0.1, 0.1, 1, 0))):
        assert bwd(b=0, **kw) == ok, kw                                                     # nothing to do: no launch
    # the size queries answer what they answered before
    assert need_t == lib.aspire_bert_tape_bytes(ctypes.byref(_weights()), 3, 37) > 0 and need_w > 0


def test_xent_entry_points_check_their_arguments_before_the_first_launch():
    from aspire_amd import _lib
    lib = _lib.lib
    inval, unsup, ok = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED, _lib.ASPIRE_OK

    def fwd(b=3, d=768, q=16, c=16, loss=16, lse=16):
        return lib.aspire_inbatch_xent_f32(q, c, b, d, loss, lse, None)

    def bwd(b=3, d=768, q=16, c=16, lse=16, gl=16, gq=16, gc=16):
        return lib.aspire_inbatch_xent_backward_f32(q, c, b, d, lse, gl, gq, gc, None)

    for call in (fwd, bwd):
        assert call(b=129) == unsup and b'129' in lib.aspire_last_error()
        assert call(d=767) == unsup and b'767' in lib.aspire_last_error()
        assert call(b=-1) == inval and b'-1' in lib.aspire_last_error()
        assert call(q=None) == inval and b'null' in lib.aspire_last_error()
        assert call(c=None) == inval and call(lse=None) == inval
        assert call(q=8) == inval and b'aligned' in lib.aspire_last_error()
        assert call(b=0) == ok                                                              # nothing to do: no launch
    assert fwd(loss=None) == inval and bwd(gl=None) == inval and bwd(gq=None) == inval and bwd(gc=None) == inval
    with pytest.raises(NotImplementedError, match='129'):
        _lib.check(fwd(b=129))


# ---- 4. the operators' fake kernels -----------------------------------------------------------------------------------------------------
def test_fake_implementations_propagate_shapes():
    import aspire_amd.torch_ops as to
    for name in ('bert_layers_train_cls', 'bert_layers_backward_cls', 'inbatch_xent', 'inbatch_xent_backward'):
        assert name in to.OPS and hasattr(torch.ops.aspire, name)
    assert len(set(to.OPS)) == len(to.OPS)

    def m(*s, dt=torch.float32):
        return torch.empty(*s, device='meta', dtype=dt)

    layer = [m(2304, 768), m(2304), m(768, 768), m(768), m(768), m(768), m(128, 768), m(128), m(768, 128), m(768), m(768), m(768)]
    key = (12, 1e-12, 0.1, 0.2, 5, 0)
    for n in (0, 2):
        w = [m(768), m(768)] + layer * n
        mask = m(3, 37, dt=torch.int64)
        plain = torch.ops.aspire.bert_layers_train(m(3, 37, 768), mask, w, 12, 1e-12)[1]
        for mix in (m(n + 1), None):
            cls, layer_cls, tape = torch.ops.aspire.bert_layers_train_cls(m(3, 37, 768), mask, w, mix, *key)
            assert cls.shape == (3, 768) and cls.dtype == torch.float32
            assert layer_cls.shape == ((n + 1, 3, 768) if mix is not None else (0,))
            assert tape.dtype == torch.uint8 and tape.numel() == plain.numel()               # the tape does not grow
            ge, grads, gm = torch.ops.aspire.bert_layers_backward_cls(m(3, 768), layer_cls, tape, mask, w, mix, *key)
            assert ge.shape == (3, 37, 768) and [g.shape for g in grads] == [t.shape for t in w]
            assert gm.shape == ((n + 1,) if mix is not None else (0,))
    loss, lse = torch.ops.aspire.inbatch_xent(m(5, 768), m(5, 768))
    assert loss.shape == (1,) and lse.shape == (5,)
    gq, gc = torch.ops.aspire.inbatch_xent_backward(m(1), m(5, 768), m(5, 768), lse)
    assert gq.shape == gc.shape == (5, 768)
    with pytest.raises(NotImplementedError, match='CPU'):          # no CPU kernel behind them
        torch.ops.aspire.inbatch_xent(torch.zeros(2, 768), torch.zeros(2, 768))
