"""GPU: dropout in the encoder under training -- aspire_bert_layers_forward_train_dropout_f32 / aspire_bert_layers_backward_dropout_f32 /
aspire_bert_dropout_mask_u8 behind torch.ops.aspire.bert_layers_train_dropout / bert_layers_backward_dropout / bert_dropout_mask and
HipBertTrainEncoder(bert, dropout=True).

Yardsticks, neither of which reads the code under test: the masks against the numpy Philox4x32-10 of tests/dropout_ref.py (pinned to the
published known-answer vectors by tests/test_dropout_cpu.py), and the arithmetic against HuggingFace BertModel.train() in float64 on the
CPU whose torch.nn.functional.dropout hands out those masks in call order (dropout_ref.given_masks: it asserts every call's shape and
p).  Models, inputs, loss and bound are tests/test_gpu_encoder_backward.py's: loss = (hidden * G).sum(); per tensor
trainside_inputs.bound(ref_err, max|grad|) = max(4 ref_err, 4 * 2^-23 max|grad|), ref_err the deviation of the same masked model's
fp32 CPU autograd from float64; the key bias is held to the query bias's scale.

Largest |kernel - float64| on an MI355X per tensor group over the nine parity cases, the case where error / bound is largest
(n_layers x (B, L), (p_hidden, p_attn)); every comparison prints its figures before it asserts (pytest -s shows them):

    group                                  error       bound       case
    hidden                                 1.355e-06   3.528e-06   1 x (2, 5), p (0.1, 0.1)
    tables                                 4.070e-05   9.973e-05   1 x (2, 5), p (0.1, 0.1)
    emb LayerNorm                          3.849e-06   1.046e-05   1 x (2, 8), p (0.1, 0.1)
    attention.self.query.weight            5.972e-06   8.939e-06   2 x (2, 130), p (0.1, 0.1)
    attention.self.query.bias              1.492e-06   2.808e-06   2 x (2, 130), p (0.0, 0.3)
    attention.self.key.weight              7.478e-06   1.300e-05   2 x (2, 130), p (0.5, 0.0)
    attention.self.key.bias                2.831e-07   1.013e-06   2 x (3, 37), p (0.0, 0.3)
    attention.self.value.weight            9.233e-06   1.561e-05   1 x (2, 8), p (0.1, 0.1)
    attention.self.value.bias              1.602e-05   2.989e-05   2 x (2, 130), p (0.1, 0.1)
    attention.output.dense.weight          7.091e-06   1.150e-05   1 x (2, 5), p (0.1, 0.1)
    attention.output.dense.bias            8.485e-06   2.608e-05   2 x (3, 37), p (0.5, 0.0)
    attention.output.LayerNorm.weight      1.363e-05   3.369e-05   2 x (2, 130), p (0.1, 0.1)
    attention.output.LayerNorm.bias        1.091e-05   2.496e-05   2 x (3, 37), p (0.1, 0.1)
    intermediate.dense.weight              3.930e-05   6.983e-05   2 x (2, 130), p (0.5, 0.0)
    intermediate.dense.bias                1.036e-05   1.899e-05   2 x (2, 130), p (0.1, 0.1)
    output.dense.weight                    4.148e-06   6.655e-06   1 x (1, 1), p (0.1, 0.1)
    output.dense.bias                      9.888e-06   2.954e-05   2 x (3, 37), p (0.1, 0.1)
    output.LayerNorm.weight                1.118e-05   2.581e-05   2 x (3, 37), p (0.5, 0.0)
    output.LayerNorm.bias                  1.266e-05   3.540e-05   2 x (2, 130), p (0.1, 0.1)

Every tensor is inside its bound; nothing in the kernels was changed to get there.
"""
import copy
import ctypes
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from trainside_inputs import bound  # noqa: E402
import readout_inputs as ri  # noqa: E402
import dropout_ref as dr  # noqa: E402
from test_gpu_encoder_backward import VOCAB, _bert, _compare, _group, _mask, _rank_batch  # noqa: E402,F401  (_group: _compare's table)

pytestmark = pytest.mark.gpu
SEED, STEP = 0x9E3779B97F4A7C15, 3          # a seed with a high word: both key words matter


def _mask_u8(seed, step, site, p, first, n):
    import aspire_amd.torch_ops  # noqa: F401
    return torch.ops.aspire.bert_dropout_mask(seed - 2 ** 64 if seed >= 2 ** 63 else seed, step, site, p, first, n)


# ---- 1. the mask's bits ---------------------------------------------------------------------------------------------------------------
def test_mask_bits_equal_the_numpy_restatement():
    windows = [(first, n) for first in (0, 3) for n in (1, 5, 4099)] + [(2 ** 34 - 2, 11)]       # the last: the block index carries
    for seed in (SEED, 5):
        for p in (0.1, 0.5):
            for site, step in ((0, 0), (4, 0), (4, 7), (0, 2 ** 32 - 1)):
                for first, n in windows:
                    got = _mask_u8(seed, step, site, p, first, n).cpu().numpy()
                    want = dr.keep_mask(seed, step, site, p, first, n)
                    assert got.dtype == np.uint8 and got.shape == (n,)
                    assert np.array_equal(got, want), (seed, p, site, step, first, n)
    assert _mask_u8(SEED, 0, 0, 0.5, 0, 0).shape == (0,)
    with pytest.raises(AssertionError, match='outside'):
        _mask_u8(SEED, 0, 0, 1.0, 0, 4)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _ragged_mask(b, l):
    m = _mask(b, l)
    if (b, l) == (2, 8):
        m[1, 5:] = 0
    return m


def _model(n_layers, b, p_hidden, p_attn):
    """test_gpu_encoder_backward's random-init model with the two probabilities set (given_masks asserts the p of every call)"""
    m = _bert(n_layers, seed=10 * n_layers + b)
    m.config.hidden_dropout_prob, m.config.attention_probs_dropout_prob = p_hidden, p_attn
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p_hidden
    for layer in m.encoder.layer:
        layer.attention.self.dropout.p = p_attn
    return m


def _site_masks(n_layers, b, l, p_hidden, p_attn, seed, step):
    """[(keep or None, p)] in HuggingFace's call order = site order, the masks from the library's own mask entry point"""
    def site(s, shape, p):
        return (_mask_u8(seed, step, s, p, 0, int(np.prod(shape))).cpu().reshape(shape) if p > 0 else None, p)

    masks = [site(0, (b, l, 768), p_hidden)]
    for i in range(n_layers):
        masks += [site(1 + 3 * i, (b, 12, l, l), p_attn), site(2 + 3 * i, (b, l, 768), p_hidden), site(3 + 3 * i, (b, l, 768), p_hidden)]
    return masks


@functools.lru_cache(maxsize=None)
def _case(n_layers, b, l, p_hidden, p_attn):
    """the model, its inputs, the masks and both CPU reference runs under them -- computed once per case, never written to"""
    m = _model(n_layers, b, p_hidden, p_attn)
    g = torch.Generator().manual_seed(100 + l)
    tok = torch.randint(0, VOCAB, (b, l), generator=g)
    typ = torch.randint(0, 2, (b, l), generator=g)
    mask = _ragged_mask(b, l)
    G = torch.randn(b, l, 768, generator=g)
    masks = _site_masks(n_layers, b, l, p_hidden, p_attn, SEED, STEP)
    runs = {}
    for dt in (torch.float64, torch.float32):
        mm = copy.deepcopy(m).to(dt).train()
        with dr.given_masks(masks):
            hidden = mm(tok, token_type_ids=typ, attention_mask=mask).last_hidden_state
        (hidden * G.to(dt)).sum().backward()
        runs[dt] = (hidden.detach(), {n: p.grad for n, p in mm.named_parameters()})
    return m, tok, typ, mask, G, runs


def _op_inputs(n_layers=2, b=3, l=37):
    from aspire_amd import HipBertTrainEncoder
    import aspire_amd.torch_ops  # noqa: F401
    m = _model(n_layers, b, 0.0, 0.0)
    g = torch.Generator().manual_seed(100 + l)
    tok = torch.randint(0, VOCAB, (b, l), generator=g)
    typ = torch.randint(0, 2, (b, l), generator=g)
    G = torch.randn(b, l, 768, generator=g)
    enc = HipBertTrainEncoder(m)
    with torch.no_grad():
        emb = enc.bert.embeddings
        emb_sum = (emb.word_embeddings(tok.cuda()) + emb.token_type_embeddings(typ.cuda())) + emb.position_embeddings.weight[:l]
        weights = [w.detach().clone() for w in enc.layer_weights()]
    return emb_sum, _ragged_mask(b, l).cuda(), weights, G.cuda()


def _raw_forward(emb_sum, mask, weights, drop):
    """the C entry point itself; drop: a _lib.BertDropout or None (NULL)"""
    from aspire_amd import _lib, ops
    from aspire_amd.encoder import pack_layer_stack
    bw = pack_layer_stack(weights, 12, 1e-12)
    b, l, _ = emb_sum.shape
    out = torch.full_like(emb_sum, float('nan'))
    tape = torch.empty(_lib.lib.aspire_bert_tape_bytes(ctypes.byref(bw), b, l), device='cuda', dtype=torch.uint8)
    ws = torch.full((_lib.lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), b, l),), 0xFF, device='cuda', dtype=torch.uint8)
    _lib.check(_lib.lib.aspire_bert_layers_forward_train_dropout_f32(ctypes.byref(bw), ops._ptr(emb_sum), ops._ptr(mask), b, l, ops._ptr(out),
                                                                     ops._ptr(tape), tape.numel(), ops._ptr(ws), ws.numel(),
                                                                     ctypes.byref(drop) if drop is not None else None, ops._stream()))
    return out, tape


def _raw_backward(G, tape, mask, weights, drop, want_emb=True):
    """the C entry point itself on gradient buffers and a workspace pre-filled with NaN bits"""
    from aspire_amd import _lib, ops
    from aspire_amd.encoder import pack_layer_stack
    bw = pack_layer_stack(weights, 12, 1e-12)
    nan = float('nan')
    grads = [torch.full_like(w, nan) for w in weights]
    grad_emb = torch.full_like(G, nan) if want_emb else None
    n_layers = (len(weights) - 2) // 12
    layers = (_lib.BertLayerGrads * max(n_layers, 1))()
    for i in range(n_layers):
        for (f, _), t in zip(_lib.BertLayerGrads._fields_, grads[2 + 12 * i:14 + 12 * i]):
            setattr(layers[i], f, ctypes.c_void_p(t.data_ptr()))
    bg = _lib.BertGrads(ctypes.c_void_p(grads[0].data_ptr()), ctypes.c_void_p(grads[1].data_ptr()), layers)
    b, l, _ = G.shape
    ws = torch.full((_lib.lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), b, l),), 0xFF, device='cuda', dtype=torch.uint8)   # NaN bits
    _lib.check(_lib.lib.aspire_bert_layers_backward_dropout_f32(ctypes.byref(bw), ops._ptr(mask), b, l, ops._ptr(G), ops._ptr(tape),
                                                                tape.numel(), ops._ptr(grad_emb), ctypes.byref(bg), ops._ptr(ws), ws.numel(),
                                                                ctypes.byref(drop) if drop is not None else None, ops._stream()))
    return grad_emb, grads


def _same(a, b):
    return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


# ---- 2. p = 0 is today's path -------------------------------------------------------------------------------------------------------------
def test_probability_zero_and_null_give_the_existing_entry_points_bits():
    from aspire_amd import _lib
    emb_sum, mask, weights, G = _op_inputs()
    hidden, tape = torch.ops.aspire.bert_layers_train(emb_sum, mask, weights, 12, 1e-12)
    want = torch.ops.aspire.bert_layers_backward(G, tape, mask, weights, 12, 1e-12)
    assert all(torch.isfinite(x).all() for x in want[1])
    h0, tape0 = torch.ops.aspire.bert_layers_train_dropout(emb_sum, mask, weights, 12, 1e-12, 0.0, 0.0, SEED - 2 ** 64, STEP)
    assert torch.equal(h0, hidden)
    assert _same(torch.ops.aspire.bert_layers_backward_dropout(G, tape0, mask, weights, 12, 1e-12, 0.0, 0.0, SEED - 2 ** 64, STEP), want)
    for drop in (None, _lib.BertDropout(0.0, 0.0, SEED, STEP)):
        h1, tape1 = _raw_forward(emb_sum, mask, weights, drop)
        assert torch.equal(h1, hidden)
        assert _same(_raw_backward(G, tape1, mask, weights, drop), want)


# ---- 3. parity with the masks given -------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (1, 2, 5), (1, 2, 8), (2, 3, 37), (2, 2, 130)]
PARITY = [s + (0.1, 0.1) for s in SHAPES] + [s + p for p in ((0.5, 0.0), (0.0, 0.3)) for s in SHAPES[3:]]


@pytest.mark.parametrize('n_layers,b,l,p_hidden,p_attn', PARITY)
def test_gradients_match_float64_under_the_same_masks(n_layers, b, l, p_hidden, p_attn):
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, runs = _case(n_layers, b, l, p_hidden, p_attn)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                      # dropout=True: nothing to warn about
        enc = HipBertTrainEncoder(copy.deepcopy(m), dropout=True, seed=SEED).train()
    enc.set_dropout_state(SEED, STEP)
    hidden = enc(tok, token_type_ids=typ, attention_mask=mask)
    assert hidden.is_cuda and hidden.shape == (b, l, 768) and hidden.requires_grad and enc.dropout_state() == (SEED, STEP + 1)
    (hidden * G.cuda()).sum().backward()
    tag = f'{n_layers} x ({b}, {l}), p ({p_hidden}, {p_attn})'
    h64, h32 = runs[torch.float64][0], runs[torch.float32][0]
    tol = bound(float((h32.double() - h64).abs().max()), float(h64.abs().max()))
    err = float((hidden.detach().double().cpu() - h64).abs().max())
    print(f'[{tag}] {"hidden":42s} |kernel - float64| {err:.3e}  bound {tol:.3e}')
    got = {n: p.grad for n, p in enc.bert.named_parameters()}
    assert all(g is not None and torch.isfinite(g).all() for g in got.values())
    _compare(got, runs, tag)
    assert err <= tol


# ---- 4. same key, same bits ---------------------------------------------------------------------------------------------------------------
def test_same_key_gives_the_same_bits_and_another_step_does_not():
    emb_sum, mask, weights, G = _op_inputs()
    key = (0.1, 0.1, SEED - 2 ** 64, STEP)
    hidden, tape = torch.ops.aspire.bert_layers_train_dropout(emb_sum, mask, weights, 12, 1e-12, *key)
    hidden2, tape2 = torch.ops.aspire.bert_layers_train_dropout(emb_sum, mask, weights, 12, 1e-12, *key)
    assert torch.isfinite(hidden).all() and torch.equal(hidden, hidden2)
    a = torch.ops.aspire.bert_layers_backward_dropout(G, tape, mask, weights, 12, 1e-12, *key)
    b = torch.ops.aspire.bert_layers_backward_dropout(G, tape2, mask, weights, 12, 1e-12, *key)
    assert all(torch.isfinite(x).all() for x in a[1]) and _same(a, b)
    for other in ((0.1, 0.1, SEED - 2 ** 64, STEP + 1), (0.1, 0.1, SEED - 2 ** 64 + 1, STEP), (0.0, 0.1, SEED - 2 ** 64, STEP),
                  (0.1, 0.0, SEED - 2 ** 64, STEP)):
        assert not torch.equal(torch.ops.aspire.bert_layers_train_dropout(emb_sum, mask, weights, 12, 1e-12, *other)[0], hidden), other
    assert not torch.equal(torch.ops.aspire.bert_layers_train(emb_sum, mask, weights, 12, 1e-12)[0], hidden)


# ---- 5. the backward writes every buffer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('l', [37, 8])          # the ragged and the aligned probability pass
def test_backward_writes_every_gradient_buffer(l):
    """gradient buffers and workspace pre-filled with NaN bits come back finite and equal to the operator's (which allocates its own)"""
    from aspire_amd import _lib
    emb_sum, mask, weights, G = _op_inputs(2, 3 if l == 37 else 2, l)
    key = (0.1, 0.1, SEED - 2 ** 64, STEP)
    hidden, tape = torch.ops.aspire.bert_layers_train_dropout(emb_sum, mask, weights, 12, 1e-12, *key)
    want = torch.ops.aspire.bert_layers_backward_dropout(G, tape, mask, weights, 12, 1e-12, *key)
    drop = _lib.BertDropout(0.1, 0.1, SEED, STEP)
    h1, tape1 = _raw_forward(emb_sum, mask, weights, drop)             # (its workspace holds NaN bits too)
    assert torch.equal(h1, hidden)
    for want_emb in (True, False):           # grad_emb_sum may be NULL: the parameter gradients are the same
        grad_emb, grads = _raw_backward(G, tape1, mask, weights, drop, want_emb)
        assert grad_emb is None or (torch.isfinite(grad_emb).all() and torch.equal(grad_emb, want[0]))
        for x, y in zip(grads, want[1]):
            assert torch.isfinite(x).all() and torch.equal(x, y)


# ---- 6. the module ------------------------------------------------------------------------------------------------------------------------
def test_module_counts_steps_and_resumes():
    from aspire_amd import HipBertTrainEncoder
    m = _bert(1, dropout=0.1)
    tok = torch.randint(0, VOCAB, (2, 6), generator=torch.Generator().manual_seed(0))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        enc = HipBertTrainEncoder(copy.deepcopy(m), dropout=True).train()
        assert enc.dropout_state() == (torch.initial_seed() % 2 ** 64, 0)
        first = enc(tok).detach().clone()
        second = enc(tok).detach().clone()
    assert not [w for w in caught if 'dropout' in str(w.message)]
    seed, step = enc.dropout_state()
    assert step == 2 and not torch.equal(first, second)
    enc.set_dropout_state(seed, 0)
    assert torch.equal(enc(tok).detach(), first) and enc.dropout_state() == (seed, 1)
    enc.set_dropout_state(seed, 2 ** 32 - 1)                                # the counter is a uint32
    enc(tok)
    assert enc.dropout_state() == (seed, 0)
    # eval() and no_grad(): the plain inference forward, the bits of a module without dropout, and the counter stays
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        plain = HipBertTrainEncoder(copy.deepcopy(m))
    with torch.no_grad():
        assert torch.equal(enc.train()(tok), plain.train()(tok))
    assert torch.equal(enc.eval()(tok), plain.eval()(tok))
    assert enc.dropout_state() == (seed, 0)
    assert not torch.equal(enc.train()(tok).detach(), plain.train()(tok).detach())


def test_rank_loss_trains_the_dropout_encoder(tmp_path_factory):
    from aspire_amd import HipBertTrainEncoder, RankLoss
    batch = _rank_batch(str(tmp_path_factory.getbasetemp()))
    enc = HipBertTrainEncoder(_bert(2, seed=7, dropout=0.1), dropout=True, seed=11).train()
    loss = RankLoss(ri.hparams('l2max', 0.0)).forward_rank(batch, enc, random_idxs=torch.tensor([1, 2, 0]))
    assert loss.is_cuda and loss.requires_grad and torch.isfinite(loss)
    loss.backward()
    assert enc.dropout_state() == (11, 2)                                   # one forward per side of the batch
    for n, p in enc.bert.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


# ---- 7. opcheck ---------------------------------------------------------------------------------------------------------------------------
def test_opcheck_both_operators():
    """the forward without test_aot_dispatch_dynamic: that one compares output VALUES of two runs, and the tape is opaque bytes whose
    gaps between slots are unwritten; the backward's outputs are all written and take every check"""
    emb_sum, mask, weights, G = _op_inputs(1, 2, 5)
    key = (0.1, 0.1, SEED - 2 ** 64, STEP)
    torch.library.opcheck(torch.ops.aspire.bert_layers_train_dropout,
                          (emb_sum.clone().requires_grad_(), mask, [w.clone().requires_grad_() for w in weights], 12, 1e-12) + key,
                          test_utils=('test_schema', 'test_autograd_registration', 'test_faketensor'))
    hidden, tape = torch.ops.aspire.bert_layers_train_dropout(emb_sum, mask, weights, 12, 1e-12, *key)
    torch.library.opcheck(torch.ops.aspire.bert_layers_backward_dropout, (G, tape, mask, weights, 12, 1e-12) + key)
