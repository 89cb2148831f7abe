"""GPU: training the CLS-row models -- aspire_bert_cls_mix_train_f32 / aspire_bert_layers_backward_cls_f32 behind
torch.ops.aspire.bert_layers_train_cls, aspire_inbatch_xent_f32 / _backward_f32 behind torch.ops.aspire.inbatch_xent,
HipBertTrainEncoder.forward_cls, BiEncTrain / SentEncTrain / IctEncTrain, ClsTripletLoss / IctLoss and RankTrainer over them.

The yardstick is the same model in float64 on the CPU under torch autograd: HuggingFace BertModel(output_hidden_states=True), the
restatements of tests/cls_train_ref.py (pinned to torch's own losses by tests/test_cls_train_cpu.py), nn.TripletMarginLoss(margin=1,
p=2, reduction='sum') and, under dropout, the masks of aspire_bert_dropout_mask_u8 handed to HuggingFace's dropout calls
(dropout_ref.given_masks).  Models are tests/test_gpu_encoder_backward.py's small random-init BERTs.  Per tensor the bound is
trainside_inputs.bound(ref_err, max|ref|) = max(4 ref_err, 4 * 2^-23 max|ref|), ref_err the deviation of the fp32 CPU autograd from
float64, computed here; the key bias is held to the query bias's scale and the mix logits' gradient at n_layers = 0 (zero in exact
arithmetic) to 4 * 2^-23 max|grad_mix|.  Every comparison prints its figures before it asserts (pytest -s shows them).

The trained eval() forward against the inference classes on model_final.pt is held to 1e-4: tests/test_gpu_bienc.py's TOL and
tests/test_gpu_sentenc.py's ENC_TOL, the bar their CLS forward is held to against HuggingFace.

Largest |kernel - float64| on an MI355X per tensor group, the case where error / bound is largest (every tensor is inside its bound):

    group                                  error       bound       case
    cls                                    5.579e-07   1.912e-06   mix 1 x (1, 1)
    layer_cls                              1.330e-06   2.496e-06   mix 1 x (1, 1)
    grad_emb_sum                           3.016e-05   9.819e-05   mix 2 x (3, 37)
    mix logits                             1.588e-07   2.364e-07   triplet bienc, in-batch negatives
    mix logits at n_layers = 0             0.000e+00   3.609e-06   mix 0 x (2, 5)
    grad_mix (C ABI)                       7.727e-06   6.143e-05   both sources 2 x (3, 37)
    tables                                 2.185e-05   6.661e-05   mix 2 x (2, 130)
    emb LayerNorm                          1.088e-07   2.643e-07   triplet sentenc, in-batch negatives
    attention.self.query.weight            7.687e-08   9.444e-08   dropout 1 x (2, 8), p (0.5, 0.0)
    attention.self.query.bias              1.221e-08   1.579e-08   dropout 1 x (2, 8), p (0.5, 0.0)
    attention.self.key.weight              9.354e-07   1.422e-06   mix 2 x (3, 37)
    attention.self.key.bias                1.077e-09   3.085e-09   triplet bienc, explicit negatives
    attention.self.value.weight            1.262e-06   1.690e-06   mix 2 x (2, 130)
    attention.self.value.bias              1.801e-06   3.292e-06   mix 1 x (5, 5)
    attention.output.dense.weight          8.746e-07   1.854e-06   mix 1 x (1, 1)
    attention.output.dense.bias            7.650e-07   2.572e-06   mix 1 x (5, 5)
    attention.output.LayerNorm.weight      3.330e-07   7.585e-07   mix 1 x (1, 1)
    attention.output.LayerNorm.bias        8.739e-08   2.528e-07   triplet sentenc, in-batch negatives
    intermediate.dense.weight              4.108e-06   7.046e-06   mix 2 x (3, 37)
    intermediate.dense.bias                6.814e-08   1.100e-07   triplet sentenc, in-batch negatives
    output.dense.weight                    7.108e-07   1.015e-06   mix 1 x (1, 1)
    output.dense.bias                      1.307e-06   3.805e-06   mix 2 x (3, 37)
    output.LayerNorm.weight                4.634e-07   7.328e-07   triplet sentenc, explicit negatives
    output.LayerNorm.bias                  8.369e-06   2.938e-05   both sources 2 x (3, 37)
    triplet loss                           2.808e-06   4.028e-06   triplet bienc, explicit negatives
    xent loss                              4.949e-05   3.381e-04   B = 128, max|s| = 4.8
    xent row_lse                           6.569e-07   2.742e-06   B = 128, max|s| = 4.8
    xent grad_q / grad_c                   5.870e-07   2.348e-06   B = 128, max|s| = 4.8 (grad_c)
    xent at max|s| = 309 (B = 33)          loss 3.1e-04 / 2.9e-03, row_lse 3.3e-05 / 3.0e-04, grad_q 8.6e-05 / 4.6e-04, grad_c 6.0e-05 / 3.2e-04
    ict loss                               2.981e-05   3.336e-05   ict 1 x (3, 37)
    ict towers, largest error / bound      5.901e-06   8.918e-06   ctx tower, intermediate.dense.weight
    trainer: eval() vs the inference class 0.000e+00   1.0e-04     all three models

Two earlier forms of the cross-entropy backward missed the two-tower case (CLS rows of one model: |s| about 700) and were replaced, not
the bound: direct FMA dot products against the forward's row_lse (sent tower's tables 1.487e-03 against 1.553e-04), then the forward's
own products against row_lse (ctx tower's top LayerNorm bias 2.503e-06 against 1.907e-06); the kernel now forms every row's maximum
and normaliser again and keeps them apart (enc_cls_train.hip).
"""
import copy
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from trainside_inputs import bound  # noqa: E402
import cls_train_ref as ref  # noqa: E402
import dropout_ref as dr  # noqa: E402
from test_gpu_encoder_backward import VOCAB, _bert, _compare, _group, _mask  # noqa: E402,F401  (_group: _compare's table)
from test_gpu_encoder_dropout import _model, _ragged_mask, _raw_backward, _raw_forward, _site_masks  # noqa: E402
from test_gpu_trainer import TABLES, _batches, _train_hparams  # noqa: E402

pytestmark = pytest.mark.gpu
SEED, STEP = 0x9E3779B97F4A7C15, 3
ENC_TOL = 1e-4          # tests/test_gpu_bienc.py: TOL, tests/test_gpu_sentenc.py: ENC_TOL


def _check(tag, name, got, want64, want32, scale=None, floor=None):
    """|got - float64| within bound(|fp32 - float64|, max|float64|) (or `floor` alone); prints first"""
    want64 = torch.as_tensor(want64, dtype=torch.float64)
    got = torch.as_tensor(got).detach().double().cpu().reshape(want64.shape)
    ref_err = float((torch.as_tensor(want32).detach().double().reshape(want64.shape) - want64).abs().max())
    tol = bound(ref_err, float(want64.abs().max()) if scale is None else scale) if floor is None else floor
    err = float((got - want64).abs().max())
    print(f'[{tag}] {name:42s} |kernel - float64| {err:.3e}  bound {tol:.3e}')
    assert torch.isfinite(got).all() and err <= tol, (tag, name, err, tol)


def _hf_states(mm, tok, typ, mask):
    """(hidden_states, the embedding sum in front of the embedding LayerNorm -- kept for its gradient)"""
    kept = []

    def hook(mod, inp):
        inp[0].retain_grad()
        kept.append(inp[0])

    h = mm.embeddings.LayerNorm.register_forward_pre_hook(hook)
    try:
        out = mm(tok, token_type_ids=typ, attention_mask=mask, output_hidden_states=True)
    finally:
        h.remove()
    return out.hidden_states, kept[0]


def _emb_sum(enc, tok, typ):
    emb = enc.bert.embeddings
    return (emb.word_embeddings(tok.cuda()) + emb.token_type_embeddings(typ.cuda())) + emb.position_embeddings.weight[:tok.shape[1]]


# ---- 1. the mix, forward and backward ---------------------------------------------------------------------------------------------------
MIX_CASES = [(0, 2, 5), (1, 1, 1), (1, 5, 5), (2, 3, 37), (2, 2, 130)]


@functools.lru_cache(maxsize=None)
def _mix_case(n_layers, b, l, with_hidden=False):
    """the model, its inputs and both CPU reference runs of loss = (cls * g).sum() [+ (hidden * G).sum()] -- computed once, never written to"""
    m = _bert(n_layers, seed=10 * n_layers + b)
    gen = torch.Generator().manual_seed(200 + l)
    tok = torch.randint(0, VOCAB, (b, l), generator=gen)
    typ = torch.randint(0, 2, (b, l), generator=gen)
    mask = _mask(b, l)
    g = torch.randn(b, 768, generator=gen)
    G = torch.randn(b, l, 768, generator=gen)
    logits = torch.randn(1, n_layers + 1, generator=gen)
    runs = {}
    for dt in (torch.float64, torch.float32):
        mm = copy.deepcopy(m).to(dt)
        w = logits.clone().to(dt).requires_grad_()
        hs, emb_sum = _hf_states(mm, tok, typ, mask)
        for h in hs:
            h.retain_grad()
        cls = ref.layer_mix_cls(hs, w)
        loss = (cls * g.to(dt)).sum()
        if with_hidden:
            loss = loss + (hs[-1] * G.to(dt)).sum()
        loss.backward()
        rows = ref.layer_cls_rows(hs).detach()
        grad_mix = torch.stack([(g.to(dt) * rows[i]).sum() for i in range(n_layers + 1)])        # the post-soft-max weights' gradient
        runs[dt] = dict(cls=cls.detach(), layer_cls=rows, grads={n: p.grad for n, p in mm.named_parameters()}, logits=w.grad,
                        emb_sum=emb_sum.grad, grad_mix=grad_mix)
    return m, tok, typ, mask, g, G, logits, runs


def _grad_runs(runs):
    return {dt: (None, runs[dt]['grads']) for dt in runs}


@pytest.mark.parametrize('n_layers,b,l', MIX_CASES)
def test_mix_forward_and_backward_match_float64(n_layers, b, l):
    from aspire_amd import HipBertTrainEncoder
    import aspire_amd.torch_ops  # noqa: F401
    m, tok, typ, mask, g, G, logits, runs = _mix_case(n_layers, b, l)
    r64, r32 = runs[torch.float64], runs[torch.float32]
    tag = f'mix {n_layers} x ({b}, {l})'
    enc = HipBertTrainEncoder(copy.deepcopy(m)).train()
    w = logits.cuda().requires_grad_()
    emb_sum = _emb_sum(enc, tok, typ)
    emb_sum.retain_grad()
    cls, layer_cls, tape = torch.ops.aspire.bert_layers_train_cls(emb_sum, mask.cuda(), enc.layer_weights(), torch.softmax(w, dim=1)[0], 12,
                                                                  1e-12, 0.0, 0.0, 0, 0)
    assert cls.shape == (b, 768) and layer_cls.shape == (n_layers + 1, b, 768) and cls.requires_grad and not layer_cls.requires_grad
    (cls * g.cuda()).sum().backward()
    _check(tag, 'cls', cls, r64['cls'], r32['cls'])
    _check(tag, 'layer_cls', layer_cls, r64['layer_cls'], r32['layer_cls'])
    _check(tag, 'grad_emb_sum', emb_sum.grad, r64['emb_sum'], r32['emb_sum'])
    if n_layers == 0:
        _check(tag, 'mix logits (zero in exact arithmetic)', w.grad, r64['logits'], r32['logits'],
               floor=4 * 2.0 ** -23 * float(r64['grad_mix'].abs().max()))
    else:
        _check(tag, 'mix logits', w.grad, r64['logits'], r32['logits'])
    got = {n: p.grad for n, p in enc.bert.named_parameters()}
    assert all(x is not None and torch.isfinite(x).all() for x in got.values())
    _compare(got, _grad_runs(runs), tag)
    # the method is the same operator behind the same plumbing
    enc2 = HipBertTrainEncoder(copy.deepcopy(m)).train()
    cls2 = enc2.forward_cls((tok, typ, mask), mix=torch.softmax(logits.cuda(), dim=1)[0])
    assert torch.equal(cls2.detach(), cls.detach()) and cls2.requires_grad
    with torch.no_grad():
        plain = enc2.forward_cls({'tokid_tt': tok, 'seg_tt': typ, 'attnmask_tt': mask}, mix=torch.softmax(logits.cuda(), dim=1)[0])
    assert plain.grad_fn is None and float((plain - cls.detach()).abs().max()) <= ENC_TOL


# ---- the C entry points themselves ------------------------------------------------------------------------------------------------------
def _raw_tap(weights, b, l, tape, hidden, mix, want_layers):
    from aspire_amd import _lib, ops
    from aspire_amd.encoder import pack_layer_stack
    bw = pack_layer_stack(weights, 12, 1e-12)
    n_states = (len(weights) - 2) // 12 + 1
    cls = torch.full((b, 768), float('nan'), device='cuda')
    layer_cls = torch.full((n_states, b, 768), float('nan'), device='cuda') if want_layers else None
    _lib.check(_lib.lib.aspire_bert_cls_mix_train_f32(ctypes.byref(bw), b, l, ops._ptr(tape), tape.numel(), ops._ptr(hidden), ops._ptr(mix),
                                                      ops._ptr(cls), ops._ptr(layer_cls), ops._stream()))
    return cls, layer_cls


def _raw_backward_cls(mask, weights, tape, grad_hidden, grad_cls, mix, layer_cls, drop=None, want_mix=True):
    """gradient buffers and a workspace pre-filled with NaN bits -> (grad_emb_sum, grads in weights' order, grad_mix or None)"""
    from aspire_amd import _lib, ops
    from aspire_amd.encoder import fill_layers, pack_layer_stack
    bw = pack_layer_stack(weights, 12, 1e-12)
    nan = float('nan')
    b, l = mask.shape
    grads = [torch.full_like(w, nan) for w in weights]
    grad_emb = torch.full((b, l, 768), nan, device='cuda')
    grad_mix = torch.full(((len(weights) - 2) // 12 + 1,), nan, device='cuda') if want_mix and mix is not None else None
    layers = fill_layers(_lib.BertLayerGrads, grads[2:])
    bg = _lib.BertGrads(ctypes.c_void_p(grads[0].data_ptr()), ctypes.c_void_p(grads[1].data_ptr()), layers)
    ws = torch.full((_lib.lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), b, l),), 0xFF, device='cuda', dtype=torch.uint8)
    _lib.check(_lib.lib.aspire_bert_layers_backward_cls_f32(
        ctypes.byref(bw), ops._ptr(mask), b, l, ops._ptr(grad_hidden), ops._ptr(grad_cls), ops._ptr(mix), ops._ptr(layer_cls), ops._ptr(tape),
        tape.numel(), ops._ptr(grad_emb), ctypes.byref(bg), ops._ptr(grad_mix), ops._ptr(ws), ws.numel(),
        ctypes.byref(drop) if drop is not None else None, ops._stream()))
    return grad_emb, grads, grad_mix


def _named(grads, n_layers):
    """the packed gradient list under HuggingFace's parameter names (the fused query / key / value rows split again)"""
    from aspire_amd.encoder import _LAYER_KEYS
    out = {'embeddings.LayerNorm.weight': grads[0], 'embeddings.LayerNorm.bias': grads[1]}
    for i in range(n_layers):
        p, t = f'encoder.layer.{i}.', grads[2 + 12 * i:14 + 12 * i]
        for j, name in enumerate(('query', 'key', 'value')):
            out[p + f'attention.self.{name}.weight'] = t[0][768 * j:768 * (j + 1)]
            out[p + f'attention.self.{name}.bias'] = t[1][768 * j:768 * (j + 1)]
        out.update({p + k: x for k, x in zip(_LAYER_KEYS, t[2:])})
    return out


def _stack_inputs(m, tok, typ):
    from aspire_amd import HipBertTrainEncoder
    import aspire_amd.torch_ops  # noqa: F401
    enc = HipBertTrainEncoder(copy.deepcopy(m))
    with torch.no_grad():
        return _emb_sum(enc, tok, typ), [w.detach().clone() for w in enc.layer_weights()]


def test_both_gradient_sources_at_the_c_abi():
    """grad_hidden and grad_cls together: the float64 gradient of (hidden * G).sum() + (cls * g).sum()"""
    n_layers, b, l = 2, 3, 37
    m, tok, typ, mask, g, G, logits, runs = _mix_case(n_layers, b, l, True)
    r64, r32 = runs[torch.float64], runs[torch.float32]
    emb_sum, weights = _stack_inputs(m, tok, typ)
    mix = torch.softmax(logits.cuda(), dim=1)[0].contiguous()
    hidden, tape = _raw_forward(emb_sum, mask.cuda(), weights, None)
    cls, layer_cls = _raw_tap(weights, b, l, tape, hidden, mix, True)
    grad_emb, grads, grad_mix = _raw_backward_cls(mask.cuda(), weights, tape, G.cuda(), g.cuda(), mix, layer_cls)
    tag = f'both sources {n_layers} x ({b}, {l})'
    _check(tag, 'cls', cls, r64['cls'], r32['cls'])
    _check(tag, 'grad_emb_sum', grad_emb, r64['emb_sum'], r32['emb_sum'])
    _check(tag, 'grad_mix', grad_mix, r64['grad_mix'], r32['grad_mix'])
    named = _named(grads, n_layers)
    assert all(torch.isfinite(x).all() for x in grads)
    _compare(named, {dt: (None, {n: runs[dt]['grads'][n] for n in named}) for dt in runs}, tag)
    # the same call twice: the same bits
    again = _raw_backward_cls(mask.cuda(), weights, tape, G.cuda(), g.cuda(), mix, layer_cls)
    assert torch.equal(again[0], grad_emb) and torch.equal(again[2], grad_mix) and all(torch.equal(x, y) for x, y in zip(again[1], grads))


@pytest.mark.parametrize('n_layers,b,l', [(2, 3, 37), (0, 2, 5)])
def test_null_mix_gives_the_existing_backwards_bits(n_layers, b, l):
    from aspire_amd import _lib, ops
    from aspire_amd.encoder import fill_layers, pack_layer_stack
    m, tok, typ, mask, g, G, logits, runs = _mix_case(n_layers, b, l)
    emb_sum, weights = _stack_inputs(m, tok, typ)
    mask = mask.cuda()
    hidden, tape = _raw_forward(emb_sum, mask, weights, None)
    cls, none = _raw_tap(weights, b, l, tape, hidden, None, False)
    assert none is None and torch.equal(cls, hidden[:, 0])
    cls2, layer_cls = _raw_tap(weights, b, l, tape, hidden, None, True)           # the rows may be asked for without a mix
    assert torch.equal(cls2, cls) and torch.equal(layer_cls[n_layers], cls) and torch.isfinite(layer_cls).all()
    grad_emb, grads, none = _raw_backward_cls(mask, weights, tape, None, g.cuda(), None, None)
    assert none is None
    # the comparison run: the existing entry point on a gradient that is zero except for the CLS rows
    sparse = torch.zeros(b, l, 768, device='cuda')
    sparse[:, 0] = g.cuda()
    bw = pack_layer_stack(weights, 12, 1e-12)
    want = [torch.full_like(w, float('nan')) for w in weights]
    want_emb = torch.full_like(sparse, float('nan'))
    layers = fill_layers(_lib.BertLayerGrads, want[2:])
    bg = _lib.BertGrads(ctypes.c_void_p(want[0].data_ptr()), ctypes.c_void_p(want[1].data_ptr()), layers)
    ws = torch.empty(_lib.lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), b, l), device='cuda', dtype=torch.uint8)
    _lib.check(_lib.lib.aspire_bert_layers_backward_f32(ctypes.byref(bw), ops._ptr(mask), b, l, ops._ptr(sparse), ops._ptr(tape), tape.numel(),
                                                        ops._ptr(want_emb), ctypes.byref(bg), ops._ptr(ws), ws.numel(), ops._stream()))
    assert torch.isfinite(grad_emb).all() and torch.equal(grad_emb, want_emb)
    for x, y in zip(grads, want):
        assert torch.isfinite(x).all() and torch.equal(x, y)


# ---- 2. dropout ---------------------------------------------------------------------------------------------------------------------------
def _op(emb_sum, mask, weights, mix, key, g):
    """the operator pair called directly -> (cls, grad_emb_sum, grads, grad_mix)"""
    cls, layer_cls, tape = torch.ops.aspire.bert_layers_train_cls(emb_sum, mask, weights, mix, 12, 1e-12, *key)
    return (cls,) + tuple(torch.ops.aspire.bert_layers_backward_cls(g, layer_cls, tape, mask, weights, mix, 12, 1e-12, *key))


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and torch.equal(a[3], b[3])


def test_dropout_same_key_same_bits_and_probability_zero_is_the_plain_call():
    from aspire_amd import _lib
    n_layers, b, l = 2, 3, 37
    m, tok, typ, mask, g, G, logits, runs = _mix_case(n_layers, b, l)
    emb_sum, weights = _stack_inputs(m, tok, typ)
    mask, g = mask.cuda(), g.cuda()
    mix = torch.softmax(logits.cuda(), dim=1)[0].contiguous()
    key = (0.1, 0.1, SEED - 2 ** 64, STEP)
    first, second = _op(emb_sum, mask, weights, mix, key, g), _op(emb_sum, mask, weights, mix, key, g)
    assert all(torch.isfinite(x).all() for x in (first[0], first[1], first[3]) + tuple(first[2])) and _same(first, second)
    other = _op(emb_sum, mask, weights, mix, (0.1, 0.1, SEED - 2 ** 64, STEP + 1), g)
    assert not torch.equal(other[0], first[0])
    # p = 0: the launches and the bits of the entry points called without a dropout struct
    zero = _op(emb_sum, mask, weights, mix, (0.0, 0.0, SEED - 2 ** 64, STEP), g)
    hidden, tape = _raw_forward(emb_sum, mask, weights, None)
    cls, layer_cls = _raw_tap(weights, b, l, tape, hidden, mix, True)
    for drop in (None, _lib.BertDropout(0.0, 0.0, SEED, STEP)):
        grad_emb, grads, grad_mix = _raw_backward_cls(mask, weights, tape, None, g, mix, layer_cls, drop)
        assert _same(zero, (cls, grad_emb, grads, grad_mix))
    assert not torch.equal(zero[0], first[0])


@functools.lru_cache(maxsize=None)
def _dropout_case():
    """1 layer, p_hidden = 0.5, the mix concentrated on state 0: HuggingFace's hidden_states[0] is the embedding output AFTER site 0's
    dropout, and its gradient passes through that dropout's backward"""
    n_layers, b, l, p_hidden, p_attn = 1, 2, 8, 0.5, 0.0
    m = _model(n_layers, b, p_hidden, p_attn)
    gen = torch.Generator().manual_seed(300)
    tok = torch.randint(0, VOCAB, (b, l), generator=gen)
    typ = torch.randint(0, 2, (b, l), generator=gen)
    mask = _ragged_mask(b, l)
    g = torch.randn(b, 768, generator=gen)
    logits = torch.tensor([[3.0, -1.0]])
    masks = _site_masks(n_layers, b, l, p_hidden, p_attn, SEED, STEP)
    runs = {}
    for dt in (torch.float64, torch.float32):
        mm = copy.deepcopy(m).to(dt).train()
        w = logits.clone().to(dt).requires_grad_()
        with dr.given_masks(masks):
            hs, emb_sum = _hf_states(mm, tok, typ, mask)
        cls = ref.layer_mix_cls(hs, w)
        (cls * g.to(dt)).sum().backward()
        runs[dt] = dict(cls=cls.detach(), grads={n: p.grad for n, p in mm.named_parameters()}, logits=w.grad, emb_sum=emb_sum.grad)
    return m, tok, typ, mask, g, logits, runs


def test_dropout_state_zero_is_tapped_after_its_dropout():
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, g, logits, runs = _dropout_case()
    r64, r32 = runs[torch.float64], runs[torch.float32]
    enc = HipBertTrainEncoder(copy.deepcopy(m), dropout=True, seed=SEED).train()
    enc.set_dropout_state(SEED, STEP)
    w = logits.cuda().requires_grad_()
    cls = enc.forward_cls((tok, typ, mask), mix=torch.softmax(w, dim=1)[0])
    assert enc.dropout_state() == (SEED, STEP + 1)
    (cls * g.cuda()).sum().backward()
    tag = 'dropout 1 x (2, 8), p (0.5, 0.0)'
    _check(tag, 'cls', cls, r64['cls'], r32['cls'])
    _check(tag, 'mix logits', w.grad, r64['logits'], r32['logits'])
    _compare({n: p.grad for n, p in enc.bert.named_parameters()}, _grad_runs(runs), tag)
    # eval() and no_grad(): the inference read-out, and the counter stays
    with torch.no_grad():
        enc.forward_cls((tok, typ, mask))
    enc.eval().forward_cls((tok, typ, mask))
    assert enc.dropout_state() == (SEED, STEP + 1)


# ---- 3. the triplet loss over the two single-tower models ---------------------------------------------------------------------------------
def _bert_batch(seed, b=3, l=37, ragged=True):
    gen = torch.Generator().manual_seed(seed)
    return {'tokid_tt': torch.randint(0, VOCAB, (b, l), generator=gen), 'seg_tt': torch.randint(0, 2, (b, l), generator=gen),
            'attnmask_tt': _mask(b, l) if ragged else torch.ones(b, l, dtype=torch.int64)}


def _hf_cls(mm, bb, weight=None):
    out = mm(bb['tokid_tt'], token_type_ids=bb['seg_tt'], attention_mask=bb['attnmask_tt'], output_hidden_states=weight is not None)
    return out.last_hidden_state[:, 0, :] if weight is None else ref.layer_mix_cls(out.hidden_states, weight)


@functools.lru_cache(maxsize=None)
def _triplet_case(kind, explicit):
    m = _bert(2, seed=31)
    logits = torch.randn(1, 3, generator=torch.Generator().manual_seed(32)) if kind == 'bienc' else None
    batch = {'query_bert_batch': _bert_batch(41), 'pos_bert_batch': _bert_batch(42, ragged=False)}
    if explicit:
        batch['neg_bert_batch'] = _bert_batch(43)
    perm = torch.tensor([1, 0, 2])          # a fixed point: that pair's distance gradients cancel
    runs = {}
    for dt in (torch.float64, torch.float32):
        mm = copy.deepcopy(m).to(dt)
        w = logits.clone().to(dt).requires_grad_() if logits is not None else None
        q, p = _hf_cls(mm, batch['query_bert_batch'], w), _hf_cls(mm, batch['pos_bert_batch'], w)
        n = _hf_cls(mm, batch['neg_bert_batch'], w) if explicit else p[perm]
        loss = torch.nn.TripletMarginLoss(margin=1, p=2, reduction='sum')(q, p, n)
        loss.backward()
        runs[dt] = dict(loss=loss.detach(), grads={k: x.grad for k, x in mm.named_parameters()}, logits=w.grad if w is not None else None)
    return m, logits, batch, perm, runs


@pytest.mark.parametrize('explicit', [True, False])
@pytest.mark.parametrize('kind', ['sentenc', 'bienc'])
def test_triplet_loss_matches_float64(kind, explicit):
    from aspire_amd import BiEncTrain, ClsTripletLoss, SentEncTrain
    m, logits, batch, perm, runs = _triplet_case(kind, explicit)
    r64, r32 = runs[torch.float64], runs[torch.float32]
    if kind == 'bienc':
        model = BiEncTrain(copy.deepcopy(m), {'fine_tune': True}).train()
        with torch.no_grad():
            model.bert_layer_weights.weight.copy_(logits)
        enc = model.bert_encoder
    else:
        model = SentEncTrain(copy.deepcopy(m)).train()
        enc = model.sent_encoder
    loss = ClsTripletLoss().forward_rank(batch, model, random_idxs=perm)
    assert loss.is_cuda and loss.dim() == 0 and loss.requires_grad and float(r64['loss']) > 0
    loss.backward()
    tag = f'triplet {kind}, {"explicit" if explicit else "in-batch"} negatives'
    _check(tag, 'loss', loss, r64['loss'], r32['loss'])
    if kind == 'bienc':
        _check(tag, 'mix logits', model.bert_layer_weights.weight.grad, r64['logits'], r32['logits'])
    _compare({n: p.grad for n, p in enc.bert.named_parameters()}, _grad_runs(runs), tag)


def test_state_dict_keys_and_a_batch_of_one():
    from aspire_amd import BiEncTrain, ClsTripletLoss, IctEncTrain, IctLoss, SentEncTrain
    from aspire_amd import bienc, sentenc
    hf = set(_bert(1).state_dict())
    bi = BiEncTrain(_bert(1), {'fine_tune': False})
    assert set(bi.state_dict()) == {'bert_encoder.' + k for k in hf} | {'bert_layer_weights.weight'}
    assert bi.bert_layer_weights.weight.shape == (1, 2) and bi.bert_layer_weights.bias is None
    assert [n for n, p in bi.named_parameters() if p.requires_grad] == ['bert_layer_weights.weight']          # fine_tune: False
    enc_sd, mix = bienc.split_state_dict(bi.state_dict())
    assert set(enc_sd) == hf and mix.shape == (1, 2)
    se = SentEncTrain(_bert(1))
    assert set(se.state_dict()) == {'sent_encoder.' + k for k in hf} and set(sentenc.split_state_dict(se.state_dict())) == hf
    ict = IctEncTrain(_bert(1, seed=1), _bert(1, seed=2), dropout=True, seed=2 ** 64 - 1)
    assert set(ict.state_dict()) == {t + k for t in ('sent_encoder.', 'context_encoder.') for k in hf}
    assert set(sentenc.split_state_dict(ict.state_dict())) == hf
    assert ict.dropout_state() == (2 ** 64 - 1, 0, 0, 0)                 # the context tower: seed + 1 mod 2^64
    ict.set_dropout_state(5, 6, 7, 8)
    assert ict.sent_encoder.dropout_state() == (5, 6) and ict.context_encoder.dropout_state() == (7, 8)
    # load_state_dict speaks the same names, and refuses others
    other = BiEncTrain(_bert(1, seed=9), {'fine_tune': True})
    other.load_state_dict({k: v.cpu() for k, v in bi.state_dict().items()})
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), bi.state_dict().values()))
    with pytest.raises(KeyError):
        other.load_state_dict({**bi.state_dict(), 'criterion.weight': torch.zeros(1)})
    # one row: [1, 768] reps, the triplet's value of that row, and an in-batch cross-entropy of exactly 0
    one = {k: _bert_batch(50 + i, b=1, l=5, ragged=False) for i, k in enumerate(('query_bert_batch', 'pos_bert_batch', 'neg_bert_batch'))}
    se.train()
    reps = [se(one[k]) for k in one]
    assert all(r.shape == (1, 768) for r in reps)
    loss = ClsTripletLoss().forward_rank(one, se)
    want = ref.triplet_sum(*[r.detach().double().cpu() for r in reps])
    want32 = torch.nn.TripletMarginLoss(margin=1, p=2, reduction='sum')(*[r.detach().cpu() for r in reps])
    assert loss.dim() == 0
    _check('one row', 'triplet loss on the kernel\'s own reps', loss, want, want32)
    ict.train()
    zero = IctLoss().forward_rank(one, ict)
    assert zero.dim() == 0 and float(zero.detach()) == 0.0
    zero.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for n, p in ict.named_parameters() if 'encoder.layer' in n)


# ---- 4. the in-batch cross-entropy ----------------------------------------------------------------------------------------------------------
def _xent_rows(b, scale, seed=0):
    gen = torch.Generator().manual_seed(1000 * b + seed)
    return torch.randn(b, 768, generator=gen) * scale, torch.randn(b, 768, generator=gen) * scale


def _xent_reference(q, c):
    runs = {}
    for dt in (torch.float64, torch.float32):
        qq, cc = q.clone().to(dt).requires_grad_(), c.clone().to(dt).requires_grad_()
        if dt == torch.float64:
            loss, lse = ref.inbatch_xent(qq, cc)
        else:           # the reference's own fp32 path
            s = torch.matmul(qq, cc.T)
            loss, lse = torch.nn.functional.cross_entropy(s, torch.arange(q.shape[0]), reduction='sum'), torch.logsumexp(s, dim=1)
        loss.backward()
        runs[dt] = dict(loss=loss.detach(), lse=lse.detach(), gq=qq.grad, gc=cc.grad, smax=float((qq @ cc.T).detach().abs().max()))
    return runs


XENT_CASES = [(1, 0.2), (2, 0.2), (16, 0.2), (17, 0.2), (33, 0.2), (128, 0.2), (33, 1.8)]      # the last: |s_ij| reaches about 300


@pytest.mark.parametrize('b,scale', XENT_CASES)
def test_inbatch_xent_matches_float64(b, scale):
    import aspire_amd.torch_ops  # noqa: F401
    q, c = _xent_rows(b, scale)
    runs = _xent_reference(q, c)
    r64, r32 = runs[torch.float64], runs[torch.float32]
    if scale > 1:
        assert 250 <= r64['smax'] <= 400 and r64['smax'] > 88.8          # exp overflows in fp32 without the max shift
    qd, cd = q.cuda().requires_grad_(), c.cuda().requires_grad_()
    loss, lse = torch.ops.aspire.inbatch_xent(qd, cd)
    assert loss.shape == (1,) and lse.shape == (b,) and torch.isfinite(loss).all() and torch.isfinite(lse).all()
    loss.sum().backward()
    tag = f'xent B = {b}, max|s| = {r64["smax"]:.1f}'
    _check(tag, 'loss', loss, r64['loss'], r32['loss'])
    _check(tag, 'row_lse', lse, r64['lse'], r32['lse'])
    _check(tag, 'grad_q', qd.grad, r64['gq'], r32['gq'])
    _check(tag, 'grad_c', cd.grad, r64['gc'], r32['gc'])
    if b == 1:
        assert float(loss.detach()) == 0.0
    # two runs: the same bits; grad_loss = 0: exact zeros
    loss2, lse2 = torch.ops.aspire.inbatch_xent(qd.detach(), cd.detach())
    assert torch.equal(loss2, loss.detach()) and torch.equal(lse2, lse.detach())
    one = torch.ones(1, device='cuda')
    a = torch.ops.aspire.inbatch_xent_backward(one, qd.detach(), cd.detach(), lse2)
    a2 = torch.ops.aspire.inbatch_xent_backward(one, qd.detach(), cd.detach(), lse2)
    assert torch.equal(a[0], qd.grad) and torch.equal(a[1], cd.grad) and torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])
    z = torch.ops.aspire.inbatch_xent_backward(torch.zeros(1, device='cuda'), qd.detach(), cd.detach(), lse2)
    assert torch.equal(z[0], torch.zeros_like(z[0])) and torch.equal(z[1], torch.zeros_like(z[1]))


def test_inbatch_xent_refuses_what_is_not_built_and_passes_opcheck():
    import aspire_amd.torch_ops  # noqa: F401
    with pytest.raises(NotImplementedError, match='129'):
        torch.ops.aspire.inbatch_xent(torch.zeros(129, 768, device='cuda'), torch.zeros(129, 768, device='cuda'))
    with pytest.raises(NotImplementedError, match='64'):
        torch.ops.aspire.inbatch_xent(torch.zeros(3, 64, device='cuda'), torch.zeros(3, 64, device='cuda'))
    q, c = (x.cuda() for x in _xent_rows(5, 0.2))
    torch.library.opcheck(torch.ops.aspire.inbatch_xent, (q.clone().requires_grad_(), c.clone().requires_grad_()))
    torch.library.opcheck(torch.ops.aspire.inbatch_xent_backward, (torch.ones(1, device='cuda'), q, c, torch.ops.aspire.inbatch_xent(q, c)[1]))


def test_ict_loss_matches_float64():
    from aspire_amd import IctEncTrain, IctLoss
    ms, mc = _bert(1, seed=51), _bert(1, seed=52)
    batch = {'query_bert_batch': _bert_batch(61), 'pos_bert_batch': _bert_batch(62, ragged=False)}
    runs = {}
    for dt in (torch.float64, torch.float32):
        a, b = copy.deepcopy(ms).to(dt), copy.deepcopy(mc).to(dt)
        q, c = _hf_cls(a, batch['query_bert_batch']), _hf_cls(b, batch['pos_bert_batch'])
        loss = torch.nn.CrossEntropyLoss(reduction='sum')(torch.matmul(q, c.T), torch.arange(3))
        loss.backward()
        runs[dt] = dict(loss=loss.detach(), sent={n: p.grad for n, p in a.named_parameters()}, ctx={n: p.grad for n, p in b.named_parameters()})
    model = IctEncTrain(copy.deepcopy(ms), copy.deepcopy(mc)).train()
    loss = IctLoss().forward_rank(batch, model)
    assert loss.is_cuda and loss.dim() == 0 and loss.requires_grad
    loss.backward()
    _check('ict 1 x (3, 37)', 'loss', loss, runs[torch.float64]['loss'], runs[torch.float32]['loss'])
    for tower, key in ((model.sent_encoder, 'sent'), (model.context_encoder, 'ctx')):
        _compare({n: p.grad for n, p in tower.bert.named_parameters()}, {dt: (None, runs[dt][key]) for dt in runs}, f'ict {key} tower')


# ---- 5. the trainer ------------------------------------------------------------------------------------------------------------------------
def _trainer_model(kind, seed):
    from aspire_amd import BiEncTrain, ClsTripletLoss, IctEncTrain, IctLoss, SentEncTrain

    def bert(s):
        m = _bert(2, seed=s, dropout=0.1)
        for n, p in m.named_parameters():
            if n in TABLES:
                p.requires_grad_(False)     # (the tables' scatter gradient is torch's, with atomics: not the same bits run to run)
        return m

    if kind == 'bienc':
        return BiEncTrain(bert(seed), {'fine_tune': True}, dropout=True, seed=SEED), ClsTripletLoss().forward_rank
    if kind == 'sentenc':
        return SentEncTrain(bert(seed), dropout=True, seed=SEED), ClsTripletLoss().forward_rank
    return IctEncTrain(bert(seed), bert(seed + 1), dropout=True, seed=SEED), IctLoss().forward_rank


@pytest.mark.parametrize('kind', ['bienc', 'sentenc', 'ict'])
def test_trainer_resumes_bit_for_bit_and_the_result_loads_for_inference(kind, tmp_path, tmp_path_factory):
    """four RankTrainer iterations (2 layers, batch_size 3, Adam, dropout on): a run checkpointed after two and resumed equals the straight
    run bit for bit (tests/test_gpu_trainer.py's criterion); model_final.pt loads into the inference class, whose forward agrees with the
    training module's eval() forward within ENC_TOL = 1e-4 (tests/test_gpu_bienc.py: TOL, tests/test_gpu_sentenc.py: ENC_TOL)"""
    from aspire_amd import HipAdam, RankTrainer
    from aspire_amd.bienc import AspireBiEnc
    from aspire_amd.sentenc import AspireSentEnc
    batches = _batches(str(tmp_path_factory.getbasetemp()))

    def make(seed, tag):
        model, loss_fn = _trainer_model(kind, seed)
        return RankTrainer(model, {}, _train_hparams(), str(tmp_path / tag), lambda epoch: batches, loss_fn=loss_fn)

    straight = make(5, 'straight')
    assert isinstance(straight.optimizer, HipAdam)
    before = {n: p.detach().clone() for n, p in straight.encoder.named_parameters()}
    assert straight.train() is True and straight.iteration == 4
    assert straight.loss_checked_iters == [0] and straight.loss_history['loss'][0] > 0
    first = make(5, 'first')
    first.train(max_iterations=2)
    first.save_checkpoint(tmp_path / 'ck.pt')
    second = make(99, 'second')                    # other weights: everything must come from the checkpoint
    second.encoder.set_dropout_state(*([1, 0] * (2 if kind == 'ict' else 1)))
    second.load_checkpoint(tmp_path / 'ck.pt')
    assert (second.iteration, second.epoch, second.batch_in_epoch) == (2, 1, 0)
    assert second.train() is True and second.iteration == 4
    want_state = (SEED, 4, (SEED + 1) % 2 ** 64, 4) if kind == 'ict' else (SEED, 12)      # forwards per tower per iteration: 1 / 3
    assert second.encoder.dropout_state() == straight.encoder.dropout_state() == want_state
    assert second.scheduler.state_dict() == straight.scheduler.state_dict()
    trained = 0
    for (n, a), (_, b) in zip(second.encoder.named_parameters(), straight.encoder.named_parameters()):
        assert torch.equal(a, b), n
        sa, sb = second.optimizer.state.get(a, {}), straight.optimizer.state.get(b, {})
        assert set(sa) == set(sb), n
        for key in sa:
            assert torch.equal(sa[key], sb[key]), (n, key)
        if sa and bool(sb['exp_avg'].abs().max() > 0):
            assert not torch.equal(b.detach(), before[n]), n
            trained += 1
    assert trained >= (64 if kind == 'ict' else 32)
    if kind == 'bienc':
        assert not torch.equal(straight.encoder.bert_layer_weights.weight.detach(), before['bert_layer_weights.weight'])
    # model_final.pt: the reference's key names, into the inference class
    sd = torch.load(tmp_path / 'second' / 'model_final.pt', weights_only=True)
    assert set(sd) == set(straight.encoder.state_dict())
    assert all(torch.equal(sd[k].cpu(), v.cpu()) for k, v in straight.encoder.state_dict().items())
    bb = batches[0]['query_bert_batch']
    model = straight.encoder.eval()
    want = model(bb)
    if kind == 'bienc':
        inf = AspireBiEnc(bert_model=_bert(2, seed=0)).load_state_dict(sd)
        got = inf.partial_forward(bb)
    else:
        inf = AspireSentEnc(bert_model=_bert(2, seed=0), tokenizer=object()).load_state_dict(sd)        # (the context tower is dropped)
        got = inf.forward_device(bb['tokid_tt'], bb['seg_tt'], bb['attnmask_tt'])
    diff = float((got - want).abs().max())
    print(f'[trainer {kind}] eval() forward vs the inference class on model_final.pt: max |diff| {diff:.3e}  bound {ENC_TOL:.1e}')
    assert want.shape == got.shape == (3, 768) and torch.isfinite(got).all() and diff <= ENC_TOL
    assert model.dropout_state() == want_state                      # eval(): the counter stays
