"""GPU: the encoder backward (encoder_bwd.hip, enc_bwd.hip, the TN form of enc_gemm.hip) at the shapes and weight statistics it is
trained at -- every GEMM tile the launch rules can reach with BERT-base geometry, the FFN width 3072, score rows of up to 512 keys, a
checkpoint with trained statistics, and grad_emb_sum itself.  tests/test_gpu_encoder_backward.py runs 0 - 2 layers at up to 260 token
rows with intermediate_size 128: every product there takes the 64 x 64 tile and no score row has more than 130 keys.

Yardstick, as there (its _bert, _mask, _case, _compare and _group are used here): the same model in float64 on the CPU, loss =
(hidden * G).sum() with a seeded G; per tensor bound(ref_err, max|grad|) = max(4 ref_err, 4 * 2^-23 max|grad|), ref_err the deviation of
the same model's fp32 CPU autograd from float64, computed here; the key bias is held to the query bias's scale.  Every comparison prints
its figures before it asserts (pytest -s shows them).

Cases (all BertModel, hidden 768, 12 heads, eager attention, dropout 0):
    tiles    1 layer, ffn 3072, (B, L) = (11, 509): 5 599 token rows = 44 row tiles of 128, Lp = 512.  Document 1 is right-padded by six
             tokens, document 4 has a hole at keys 200 - 202 (zero columns of P inside a 128-row tile), document 7 one across the tile
             edge at keys 127 - 129.  11 is the smallest batch at which the per-head products leave the 64 x 64 tile
             (ceil(L / 128) * 12 B >= 512 with ceil(L / 128) = 4), and 5 599 >= 5 377 rows is what dh / dctx / dx need; L > 448 fills the
             eighth chunk of softmax_backward_kernel, L = 509 leaves it partial with three pad columns.
    row512   1 layer, ffn 64, (1, 512), full mask: Lp == L, all eight chunks full.
    row257   1 layer, ffn 64, (2, 257): document 1 masked from key 250 on and at keys 64 - 66; Lp = 260, chunk 4 holds one key.
    heavy    heavy_bert.heavy_tailed_bert(2) (ffn 3072; logits of +-50, LayerNorm gains of 10 - 30, outlier dimensions at 30 - 100, FFN
             rows x 20), (3, 96), the (3, 37) masks of the existing file stretched: left padding, a hole, right padding, one all-zero
             document.  The batch is first asserted to have logits beyond +-30 in both layers and FFN pre-activations beyond 10.
    base     the 2 x (3, 37) case of the existing file (grad_emb_sum only).

Which instantiation every product takes, from launch_gemm_bkn / launch_gemm_tn as they stand (f32 = gemm_f32_kernel<BM, BN, 16, B_KN>,
TN = gemm_f32_kernel<BM, BN, 16, true, 2, true>, x3 = gemm_bf16x3_kernel<BM, BN>; rule: with rt = ceil(M / 128) row tiles, 128 x 128 when
rt * ceil(N / 128) * batch >= 512 (x3: 256) and N >= 128, else 128 x 64 when rt * ceil(N / 64) * batch >= 512 (x3: 256), else 64 x 64):

    product (M x N over K, batch)                  tiles              row512 / row257     heavy               existing file
    backward (twelve GEMM launches per layer: six TN, five B_KN, dP)
     1 dW2   TN   768 x ffn over rows              TN 64 x 64         TN 64 x 64          TN 64 x 64          TN 64 x 64
     2 da    B_KN rows x ffn over 768              f32 128 x 128      f32 64 x 64         f32 64 x 64         f32 64 x 64
     3 dW1   TN   ffn x 768 over rows              TN 64 x 64         TN 64 x 64          TN 64 x 64          TN 64 x 64
     4 dh    B_KN rows x 768 over ffn              f32 128 x 64       f32 64 x 64         f32 64 x 64         f32 64 x 64
     5 dWo   TN   768 x 768 over rows              TN 64 x 64         TN 64 x 64          TN 64 x 64          TN 64 x 64
     6 dctx  B_KN rows x 768 over 768              f32 128 x 64       f32 64 x 64         f32 64 x 64         f32 64 x 64
     7 dV    TN   L x 64 over L, 12 B              TN 128 x 64        TN 64 x 64          TN 64 x 64          TN 64 x 64
     8 dP    Linear form L x L over 64, 12 B       x3 128 x 128       x3 128 x 64         x3 64 x 64          x3 64 x 64
     9 dQ    B_KN L x 64 over L, 12 B              f32 128 x 64       f32 64 x 64         f32 64 x 64         f32 64 x 64
    10 dK    TN   L x 64 over L, 12 B              TN 128 x 64        TN 64 x 64          TN 64 x 64          TN 64 x 64
    11 dWqkv TN   2304 x 768 over rows             TN 64 x 64         TN 64 x 64          TN 64 x 64          TN 64 x 64
    12 dx    B_KN rows x 768 over 2304             f32 128 x 64       f32 64 x 64         f32 64 x 64         f32 64 x 64
    forward
       QKV, Wo, FFN1, FFN2 (Linear form)           x3 128 x 128       x3 64 x 64          x3 64 x 64          x3 64 x 64
       QK^T  L x L over 64, 12 B                   x3 128 x 128       x3 128 x 64         x3 64 x 64          x3 64 x 64
       PV    B_KN L x 64 over L, 12 B              f32 128 x 64       f32 64 x 64         f32 64 x 64         f32 64 x 64
    softmax_backward chunks that hold keys         8 (last partial)   8 / 5 (last: 1 key) 2                   <= 3

The weight gradients of `tiles` contract over K = 5 599 rows (K % 16 = 15: the last k tile is partial).  Not reachable with BERT-base
geometry (ffn 3072, L <= 512), and run by no test: TN 128 x 128 -- per head N = 64 < 128, and the weight gradients have at most
6 * 24 = 144 tiles of 128 x 128 (it takes ffn >= 10 944); TN 128 x 64 for a WEIGHT gradient (ffn >= 5 440); B_KN 128 x 128 per head
(N = 64).  B_KN 128 x 128 (da), B_KN 128 x 64 and TN 128 x 64 are run by `tiles` alone.

Largest |kernel - float64| on an MI355X per tensor group, the case where error / bound is largest:

    group                                  error       bound       case
    hidden                                 4.026e-06   6.647e-06   tiles 1 x (11, 509)
    tables                                 1.391e-02   2.098e-02   heavy 2 x (3, 96)
    emb LayerNorm                          1.706e-04   2.914e-04   heavy 2 x (3, 96)
    attention.self.query.weight            9.493e-06   1.767e-05   row257 1 x (2, 257)
    attention.self.query.bias              2.558e-06   3.479e-06   row512 1 x (1, 512)
    attention.self.key.weight              5.865e-06   1.667e-05   row257 1 x (2, 257)
    attention.self.key.bias                1.037e-05   3.666e-05   heavy 2 x (3, 96)
    attention.self.value.weight            1.441e-04   3.039e-04   tiles 1 x (11, 509)
    attention.self.value.bias              9.752e-05   1.816e-04   tiles 1 x (11, 509)
    attention.output.dense.weight          1.363e-03   2.723e-03   heavy 2 x (3, 96)
    attention.output.dense.bias            1.145e-04   2.050e-04   tiles 1 x (11, 509)
    attention.output.LayerNorm.weight      8.284e-05   2.077e-04   heavy 2 x (3, 96)
    attention.output.LayerNorm.bias        3.085e-05   5.571e-05   heavy 2 x (3, 96)
    intermediate.dense.weight              3.089e-03   7.175e-03   heavy 2 x (3, 96)
    intermediate.dense.bias                1.178e-05   2.232e-05   row257 1 x (2, 257)
    output.dense.weight                    3.143e-03   6.510e-03   heavy 2 x (3, 96)
    output.dense.bias                      1.004e-05   2.738e-05   heavy 2 x (3, 96)
    output.LayerNorm.weight                1.202e-04   3.450e-04   tiles 1 x (11, 509)
    output.LayerNorm.bias                  6.824e-05   2.422e-04   heavy 2 x (3, 96)
    grad_emb_sum                           1.203e-02   2.320e-02   heavy

(grad_emb_sum of the 2 x (3, 37) case: 4.371e-05 of 1.924e-04, the worst row a masked one -- document 2, position 32; of `heavy`:
the worst row document 0, position 58, a real token.)

On their first run `tiles` and `heavy` were outside: the six weight gradients of `tiles` at 1.1 - 2.3 x their bounds (value weight
6.996e-04 of 3.039e-04: one fp32 accumulator summed over 5 599 rows in k order; torch's own fp32 GEMM on the GPU sums the same way and
was as far, 6.843e-04, the fp32 CPU reference 7.6e-05), and layer 1's FFN2 bias gradient of `heavy` at 3.014e-05 of 2.738e-05 (a column
summed as one running sum).  No bound was moved: the TN GEMM now sums in two levels and the column sums in four chains (NOTES.md)."""
import copy
import ctypes
import functools

import pytest
import torch

from heavy_bert import attention_logit_range, heavy_tailed_bert
from test_gpu_encoder_backward import _bert, _case, _compare, _group, _mask  # noqa: F401  (_group: _compare's table)
from trainside_inputs import bound  # noqa: E402  (tests/golden: on the path once the line above has run)

pytestmark = pytest.mark.gpu

SHAPES = {
    'tiles': dict(n_layers=1, b=11, l=509, ffn=3072, seed=21),
    'row512': dict(n_layers=1, b=1, l=512, ffn=64, seed=22),
    'row257': dict(n_layers=1, b=2, l=257, ffn=64, seed=23),
    'heavy': dict(n_layers=2, b=3, l=96, ffn=3072, seed=24),
}


def _shape_mask(name):
    s = SHAPES[name]
    b, l = s['b'], s['l']
    m = torch.ones(b, l, dtype=torch.int64)
    if name == 'tiles':
        m[1, 503:] = 0
        m[4, 200:203] = 0
        m[7, 127:130] = 0
    elif name == 'row257':
        m[1, 250:] = 0
        m[1, 64:67] = 0
    elif name == 'heavy':
        m = _mask(3, 37)[:, torch.arange(l) * 37 // l]          # the (3, 37) pattern stretched to 96 keys
    return m


def _tag(name):
    s = SHAPES[name]
    return f"{name} {s['n_layers']} x ({s['b']}, {s['l']})"


@functools.lru_cache(maxsize=None)
def _inputs(name):
    s = SHAPES[name]
    if name == 'heavy':
        m = heavy_tailed_bert(s['n_layers'], seed=s['seed'])
        m.config.hidden_dropout_prob = m.config.attention_probs_dropout_prob = 0.0       # (eval(): no dropout ran; no warning either)
        m.config._attn_implementation = 'eager'
        lo = 5
    else:
        m = _bert(s['n_layers'], seed=s['seed'], intermediate_size=s['ffn'])
        lo = 0
    assert m.config.intermediate_size == s['ffn'] and m.config.layer_norm_eps == 1e-12
    g = torch.Generator().manual_seed(100 + s['l'])
    tok = torch.randint(lo, m.config.vocab_size, (s['b'], s['l']), generator=g)
    typ = torch.randint(0, 2, (s['b'], s['l']), generator=g)
    G = torch.randn(s['b'], s['l'], 768, generator=g)
    return m, tok, typ, _shape_mask(name), G


@functools.lru_cache(maxsize=None)
def _shape_case(name):
    """_case of the existing file for this file's models: both CPU reference runs, computed once per case, never written to; and the
    largest |u| (FFN pre-activation) of the float64 run"""
    m, tok, typ, mask, G = _inputs(name)
    runs, umax = {}, []
    for dt in (torch.float64, torch.float32):
        mm = copy.deepcopy(m).to(dt)
        if dt == torch.float64:
            for ly in mm.encoder.layer:
                ly.intermediate.dense.register_forward_hook(lambda mod, args, out: umax.append(float(out.detach().abs().max())))
        hidden = mm(tok, token_type_ids=typ, attention_mask=mask).last_hidden_state
        (hidden * G.to(dt)).sum().backward()
        runs[dt] = (hidden.detach(), {n: p.grad for n, p in mm.named_parameters()})
    return m, tok, typ, mask, G, runs, max(umax)


def _any_case(name):
    return _case(2, 3, 37)[:6] if name == 'base' else _shape_case(name)[:6]


@functools.lru_cache(maxsize=None)
def _emb_case(name):
    """d loss / d emb_sum in float64 and fp32 on the CPU: emb_sum a leaf, given to BertModel as inputs_embeds of a copy whose position
    and token-type tables are zero (x + 0 + 0 is exact: the copy's hidden states are the model's)"""
    m, tok, typ, mask, G, runs = _any_case(name)
    out = {}
    for dt in (torch.float64, torch.float32):
        mm = copy.deepcopy(m).to(dt)
        emb = mm.embeddings
        with torch.no_grad():
            leaf = (emb.word_embeddings(tok) + emb.token_type_embeddings(typ)) + emb.position_embeddings.weight[:tok.shape[1]]
            emb.position_embeddings.weight.zero_()
            emb.token_type_embeddings.weight.zero_()
        leaf.requires_grad_(True)
        hidden = mm(inputs_embeds=leaf, token_type_ids=torch.zeros_like(typ), attention_mask=mask).last_hidden_state
        assert float((hidden.detach() - runs[dt][0]).abs().max()) <= 1e-12
        (hidden * G.to(dt)).sum().backward()
        out[dt] = leaf.grad
    return out


def _assert_heavy_statistics():
    m, tok, typ, mask, G, runs, umax = _shape_case('heavy')
    for layer in range(SHAPES['heavy']['n_layers']):
        lo, hi = attention_logit_range(m, tok, typ, mask, layer)
        print(f'[heavy] layer {layer} logits {lo:.1f} .. {hi:.1f}')
        assert lo < -30 and hi > 30, (layer, lo, hi)
    print(f'[heavy] largest |u| {umax:.1f}')
    assert umax > 10


def test_the_heavy_batch_has_trained_statistics():
    _assert_heavy_statistics()


@pytest.mark.parametrize('name', list(SHAPES))
def test_gradients_match_float64(name):
    from aspire_amd import HipBertTrainEncoder
    if name == 'heavy':
        _assert_heavy_statistics()
    m, tok, typ, mask, G, runs, _ = _shape_case(name)
    b, l = tok.shape
    enc = HipBertTrainEncoder(copy.deepcopy(m)).train()
    hidden = enc(tok, token_type_ids=typ, attention_mask=mask)
    assert hidden.is_cuda and hidden.shape == (b, l, 768) and hidden.requires_grad
    (hidden * G.cuda()).sum().backward()
    h64, h32 = runs[torch.float64][0], runs[torch.float32][0]
    tol = bound(float((h32.double() - h64).abs().max()), float(h64.abs().max()))
    err = float((hidden.detach().double().cpu() - h64).abs().max())
    print(f'[{_tag(name)}] hidden |kernel - float64| {err:.3e}  bound {tol:.3e}')
    got = {n: p.grad for n, p in enc.bert.named_parameters()}
    assert all(g is not None and torch.isfinite(g).all() for g in got.values())
    _compare(got, runs, _tag(name))
    assert err <= tol


def _op_inputs(name):
    from aspire_amd import HipBertTrainEncoder
    import aspire_amd.torch_ops  # noqa: F401
    m, tok, typ, mask, G, _ = _any_case(name)
    enc = HipBertTrainEncoder(copy.deepcopy(m))
    with torch.no_grad():
        emb = enc.bert.embeddings
        emb_sum = (emb.word_embeddings(tok.cuda()) + emb.token_type_embeddings(typ.cuda())) + emb.position_embeddings.weight[:tok.shape[1]]
        weights = [w.detach().clone() for w in enc.layer_weights()]
    return emb_sum, mask.cuda(), weights, G.cuda()


def test_tiles_backward_same_bits_twice_and_every_buffer_written():
    """on one tape of `tiles` (multi-tile grids of every instantiation): two backwards give the same bits (no atomics), and the C entry
    point with its workspace filled with 0xFF bytes (NaN bits) and the gradient buffers with NaN gives finite outputs equal to the
    operator's"""
    from aspire_amd import _lib, ops
    from aspire_amd.encoder import pack_layer_stack
    emb_sum, mask, weights, G = _op_inputs('tiles')
    hidden, tape = torch.ops.aspire.bert_layers_train(emb_sum, mask, weights, 12, 1e-12)
    want_emb, want = torch.ops.aspire.bert_layers_backward(G, tape, mask, weights, 12, 1e-12)
    again_emb, again = torch.ops.aspire.bert_layers_backward(G, tape, mask, weights, 12, 1e-12)
    assert torch.isfinite(want_emb).all() and torch.equal(want_emb, again_emb) and len(want) == len(again) == len(weights)
    for x, y in zip(want, again):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    del again_emb, again
    bw = pack_layer_stack(weights, 12, 1e-12)
    nan = float('nan')
    grads = [torch.full_like(w, nan) for w in weights]
    grad_emb = torch.full_like(emb_sum, nan)
    n_layers = (len(weights) - 2) // 12
    layers = (_lib.BertLayerGrads * n_layers)()
    for i in range(n_layers):
        for (f, _), t in zip(_lib.BertLayerGrads._fields_, grads[2 + 12 * i:14 + 12 * i]):
            setattr(layers[i], f, ctypes.c_void_p(t.data_ptr()))
    bg = _lib.BertGrads(ctypes.c_void_p(grads[0].data_ptr()), ctypes.c_void_p(grads[1].data_ptr()), layers)
    b, l, _ = emb_sum.shape
    ws = torch.full((_lib.lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), b, l),), 0xFF, device='cuda', dtype=torch.uint8)
    _lib.check(_lib.lib.aspire_bert_layers_backward_f32(ctypes.byref(bw), ops._ptr(mask), b, l, ops._ptr(G), ops._ptr(tape), tape.numel(),
                                                        ops._ptr(grad_emb), ctypes.byref(bg), ops._ptr(ws), ws.numel(), ops._stream()))
    assert torch.isfinite(grad_emb).all() and torch.equal(grad_emb, want_emb)
    for x, y in zip(grads, want):
        assert torch.isfinite(x).all() and torch.equal(x, y)


@pytest.mark.parametrize('name', ['base', 'heavy'])
def test_grad_emb_sum_row_by_row(name):
    """the operator's first output against the float64 gradient of the embedding sum itself -- not after torch's scatter-add into the
    three tables, which sums rows and cannot tell a masked row, a padded document or a row's tail from the others"""
    m, tok, typ, mask, G, _ = _any_case(name)
    ref = _emb_case(name)
    g64, g32 = ref[torch.float64], ref[torch.float32]
    emb_sum, cmask, weights, cG = _op_inputs(name)
    hidden, tape = torch.ops.aspire.bert_layers_train(emb_sum, cmask, weights, 12, 1e-12)
    got, _ = torch.ops.aspire.bert_layers_backward(cG, tape, cmask, weights, 12, 1e-12)
    assert got.shape == g64.shape and torch.isfinite(got).all()
    tol = bound(float((g32.double() - g64).abs().max()), float(g64.abs().max()))
    rows = (got.double().cpu() - g64).abs().amax(-1)                # [B, L]
    d, p = divmod(int(rows.argmax()), rows.shape[1])
    print(f'[{name}] grad_emb_sum |kernel - float64| {float(rows.max()):.3e}  bound {tol:.3e}  worst row: document {d} position {p} '
          f'({"masked" if int(mask[d, p]) == 0 else "real"}), max|grad| {float(g64.abs().max()):.3e}')
    bad = (rows > tol).nonzero().tolist()
    assert not bad, [(dd, pp, float(rows[dd, pp]), int(mask[dd, pp])) for dd, pp in bad[:8]]
