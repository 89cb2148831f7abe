"""CPU: the encoder backward's host side -- the new C-ABI symbols, the tape / workspace queries, the argument checks that stand in front
of the first launch, the two operators' fake implementations -- and the formulas of its row kernels (tests/encoder_backward_ref.py)
against torch autograd in float64."""
import ctypes
import math

import pytest
import torch

import encoder_backward_ref as ref

NEW = ('aspire_bert_tape_bytes', 'aspire_bert_train_workspace_bytes', 'aspire_bert_layers_forward_train_f32',
       'aspire_bert_layers_backward_f32')


def _weights(n_layers=2, hidden=768, heads=12, ffn=128, layer_ptr=16):
    """struct aspire_bert_weights with dummy non-null pointers (never dereferenced: every check fails, or returns, before a launch)."""
    from aspire_amd import _lib
    layers = (_lib.BertLayer * max(n_layers, 1))()
    for i in range(n_layers):
        for f, _ in _lib.BertLayer._fields_:
            setattr(layers[i], f, layer_ptr)
    bw = _lib.BertWeights(None, None, None, 16, 16, layers, n_layers, heads, hidden, ffn, 0, 0, 0, 1e-12, None)
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


def test_new_symbols_are_exported_and_bound():
    from aspire_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert [f for f, _ in _lib.BertLayerGrads._fields_] == [f for f, _ in _lib.BertLayer._fields_]
    assert [f for f, _ in _lib.BertGrads._fields_] == ['emb_ln_g', 'emb_ln_b', 'layers']
    assert _lib.lib.aspire_abi_version() == 6          # functions were only added


def test_tape_and_workspace_sizes():
    from aspire_amd import _lib
    lib = _lib.lib

    def sizes(n, b, l, ffn=128):
        bw = _weights(n, ffn=ffn)
        return lib.aspire_bert_tape_bytes(ctypes.byref(bw), b, l), lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), b, l)

    base = sizes(2, 3, 37)
    assert all(x > 0 and x % 256 == 0 for x in base)
    for n, b, l in ((2, 4, 37), (2, 3, 38), (2, 3, 41), (2, 3, 512)):          # monotone in B and L
        bigger = sizes(n, b, l)
        assert bigger[0] > base[0] and bigger[1] > base[1] and all(x % 256 == 0 for x in bigger)
    t = [sizes(n, 3, 37)[0] for n in (0, 1, 2, 3)]                             # ... and the tape in the layer count: one slot per layer
    assert t[0] == math.ceil(3 * 37 * 768 * 4 / 256) * 256                     # n_layers == 0: the embedding sum alone
    assert t[1] > t[0] and t[2] - t[1] == t[1] - t[0] == t[3] - t[2]
    assert sizes(3, 3, 37)[1] >= sizes(2, 3, 37)[1]
    # the activations a layer keeps: 5 x 768 (input, context, both pre-LayerNorm sums, LN1 output) + 2304 + ffn floats per token row, and the probabilities [B, 12, L, Lp]
    assert t[1] - t[0] >= 4 * (3 * 37 * (5 * 768 + 2304 + 128) + 3 * 12 * 37 * 40)
    # BERT-base at 5 x 512, 12 layers: the figure DESIGN.md states
    assert sizes(12, 5, 512, ffn=3072)[0] == 1895301120
    assert lib.aspire_bert_tape_bytes(None, 3, 37) == 0 and sizes(2, 0, 37) == (0, 0)


def test_argument_checks_stand_before_the_first_launch():
    from aspire_amd import _lib
    lib = _lib.lib
    bw, bg = _weights(), _grads()
    need_t = lib.aspire_bert_tape_bytes(ctypes.byref(bw), 3, 37)
    need_w = lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), 3, 37)

    def fwd(w=bw, emb=16, mask=16, b=3, l=37, out=16, tape=16, tb=need_t, ws=16, wb=need_w):
        return lib.aspire_bert_layers_forward_train_f32(ctypes.byref(w) if w is not None else None, emb, mask, b, l, out, tape, tb, ws, wb, None)

    def bwd(w=bw, mask=16, b=3, l=37, gh=16, tape=16, tb=need_t, ge=None, g=bg, ws=16, wb=need_w):
        return lib.aspire_bert_layers_backward_f32(ctypes.byref(w) if w is not None else None, mask, b, l, gh, tape, tb, ge,
                                                   ctypes.byref(g) if g is not None else None, ws, wb, None)

    inval, unsup = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED
    for call in (fwd, bwd):
        assert call(w=None) == inval and b'null' in lib.aspire_last_error()
        assert call(mask=None) == inval
        assert call(tape=None) == inval
        assert call(ws=None) == inval
        assert call(l=0) == inval and b'512' in lib.aspire_last_error()
        assert call(l=513) == inval
        assert call(w=_weights(hidden=1024)) == unsup and b'768' in lib.aspire_last_error()
        assert call(w=_weights(heads=8)) == unsup
        assert call(w=_weights(ffn=100)) == unsup
        assert call(w=_weights(layer_ptr=None)) == inval
        assert call(tb=need_t - 1) == inval and b'aspire_bert_tape_bytes' in lib.aspire_last_error()
        assert call(wb=need_w - 1) == inval and b'aspire_bert_train_workspace_bytes' in lib.aspire_last_error()
        assert call(b=0) == _lib.ASPIRE_OK                 # nothing to do: no launch
    assert fwd(emb=None) == inval and fwd(out=None) == inval
    assert bwd(gh=None) == inval and bwd(g=None) == inval
    bad = _grads()
    bad.layers[1].w_ffn2 = None
    assert bwd(g=bad) == inval and b'layer 1' in lib.aspire_last_error()
    with pytest.raises(AssertionError):
        _lib.check(fwd(l=513))
    with pytest.raises(NotImplementedError):
        _lib.check(fwd(w=_weights(hidden=1024)))


def test_fake_implementations_propagate_shapes():
    import aspire_amd.torch_ops as to
    assert 'bert_layers_train' in to.OPS and 'bert_layers_backward' in to.OPS

    def m(*s, dt=torch.float32):
        return torch.empty(*s, device='meta', dtype=dt)

    layer = [m(2304, 768), m(2304), m(768, 768), m(768), m(768), m(768), m(128, 768), m(128), m(768, 128), m(768), m(768), m(768)]
    for n in (0, 2):
        w = [m(768), m(768)] + layer * n
        hidden, tape = torch.ops.aspire.bert_layers_train(m(3, 37, 768), m(3, 37, dt=torch.int64), w, 12, 1e-12)
        assert hidden.shape == (3, 37, 768) and hidden.dtype == torch.float32
        assert tape.dtype == torch.uint8 and tape.dim() == 1 and tape.numel() > 0
        ge, grads = torch.ops.aspire.bert_layers_backward(m(3, 37, 768), tape, m(3, 37, dt=torch.int64), w, 12, 1e-12)
        assert ge.shape == (3, 37, 768) and [g.shape for g in grads] == [t.shape for t in w]
    with pytest.raises(NotImplementedError, match='CPU'):          # no CPU kernel behind them
        torch.ops.aspire.bert_layers_train(torch.zeros(1, 2, 768), torch.ones(1, 2, dtype=torch.int64), [torch.ones(768), torch.zeros(768)],
                                           12, 1e-12)


# ---- the formulas, float64 against autograd --------------------------------------------------------------------------------------
TOL = 1e-12


def _close(a, b):
    return float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


def test_layernorm_backward_formula():
    g = torch.Generator().manual_seed(0)
    rows, d, eps = 7, 768, 1e-12
    x = (3.0 * torch.randn(rows, d, generator=g, dtype=torch.float64) + 0.7).requires_grad_()
    gamma = (1.0 + 0.1 * torch.randn(d, generator=g, dtype=torch.float64)).requires_grad_()
    beta = (0.1 * torch.randn(d, generator=g, dtype=torch.float64)).requires_grad_()
    dy, dy_res = (torch.randn(rows, d, generator=g, dtype=torch.float64) for _ in range(2))
    y = torch.nn.functional.layer_norm(x, (d,), gamma, beta, eps)
    assert _close(ref.layernorm_forward(x, gamma, beta, eps).detach(), y.detach())
    for res in (None, dy_res):
        want = torch.autograd.grad(y, (x, gamma, beta), dy if res is None else dy + res, retain_graph=True)
        got = ref.layernorm_backward(x.detach(), gamma.detach(), eps, dy, res)
        for a, b in zip(got, want):
            assert _close(a, b)


def test_gelu_backward_formula():
    u = torch.cat([torch.linspace(-9, 9, 1801, dtype=torch.float64), torch.tensor([0.0, -0.0, 1e-30, -40.0, 40.0], dtype=torch.float64)])
    u.requires_grad_()
    dy = torch.randn(u.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    y = torch.nn.functional.gelu(u)
    assert _close(ref.gelu_forward(u.detach()), y.detach())
    assert _close(ref.gelu_backward(dy, u.detach()), torch.autograd.grad(y, u, dy)[0])


def test_softmax_backward_formula_with_masks():
    g = torch.Generator().manual_seed(2)
    b, h, l, scale = 3, 2, 9, 0.125
    s = (4.0 * torch.randn(b, h, l, l, generator=g, dtype=torch.float64)).requires_grad_()
    mask = torch.ones(b, l, dtype=torch.int64)
    mask[0, 6:] = 0                 # right padding
    mask[1, :2] = 0                 # left padding
    mask[1, 5] = 0                  # and a hole
    mask[2] = 0                     # a document whose mask is all zero: uniform over its keys
    dp = torch.randn(b, h, l, l, generator=g, dtype=torch.float64)
    # BertModel's extended mask on the scaled scores, then the soft-max
    p = torch.softmax(s * scale + (1.0 - mask[:, None, None, :].double()) * torch.finfo(torch.float32).min, dim=-1)
    got_p = ref.softmax_mask_forward(s.detach(), mask, scale)
    assert _close(got_p, p.detach())
    assert torch.equal(got_p[0, :, :, 6:], torch.zeros(h, l, 3, dtype=torch.float64))         # a masked key: exactly 0
    assert _close(got_p[2], torch.full((h, l, l), 1.0 / l, dtype=torch.float64))
    ds = ref.softmax_backward(dp, got_p, scale)
    assert _close(ds, torch.autograd.grad(p, s, dp)[0])
    assert torch.equal(ds[0, :, :, 6:], torch.zeros(h, l, 3, dtype=torch.float64))           # ... and its dS exactly 0
    assert float(ds[2].abs().max()) > 0                                                      # the all-zero row: the ordinary formula


def test_bias_and_layernorm_parameter_sums():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 16, generator=g, dtype=torch.float64)
    w = torch.randn(24, 16, generator=g, dtype=torch.float64)
    bias = torch.randn(24, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 5, 24, generator=g, dtype=torch.float64)
    y = torch.nn.functional.linear(x, w, bias)
    assert _close(ref.colsum(dy), torch.autograd.grad(y, bias, dy)[0])
