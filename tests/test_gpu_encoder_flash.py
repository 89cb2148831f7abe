"""GPU: the training encoder's fused attention mode -- aspire_amd.HipBertTrainEncoder(bert, matmul='bf16', attention='flash')
(torch.ops.aspire.bert_layers_train_attn / bert_layers_train_cls_attn over aspire_bert_layers_forward_train_attn_f32 /
aspire_bert_layers_backward_attn_f32; the kernels: aspire_amd/csrc/enc_attn_train.hip, tested bare in tests/test_gpu_flash_attn_train.py).

Yardstick and bound are tests/test_gpu_encoder_bf16.py's: the EXACT float64 CPU model on 1 x (2, 5), 2 x (3, 37), 2 x (2, 130), per tensor
trainside_inputs.bound(ref_err, max|x|) = max(4 ref_err, 4 * 2^-23 max|x|) with ref_err the deviation from float64 of the bf16 mode's
arithmetic emulated on the CPU in fp32 (tests/bf16_matmul_ref.py).  With dropout (p_hidden = p_attn = 0.1 on 2 x (3, 37) and
2 x (2, 130)) both CPU runs draw the library's masks (dropout_ref.given_masks), the emulation inside them.

Largest |kernel - float64| / bound per tensor group on an MI355X, the case where the ratio is largest (every comparison prints its
figures before it asserts; also DESIGN.md section 7, "fused training attention"):

    group                                  error       bound       ratio  case
    hidden                                 4.541e-03   1.737e-02   0.26   dropout 2 x (3, 37)
    tables                                 1.712e-01   5.410e-01   0.32   dropout 2 x (3, 37)
    emb LayerNorm                          7.903e-02   2.448e-01   0.32   dropout 2 x (2, 130)
    attention.self.query.weight            4.227e-02   1.284e-01   0.33   2 x (2, 130)
    attention.self.query.bias              1.133e-02   3.184e-02   0.36   dropout 2 x (2, 130)
    attention.self.key.weight              2.563e-02   7.929e-02   0.32   dropout 2 x (3, 37)
    attention.self.key.bias                5.442e-03   8.958e-03   0.61   dropout 2 x (3, 37)
    attention.self.value.weight            1.850e-01   5.937e-01   0.31   dropout 2 x (2, 130)
    attention.self.value.bias              1.045e-01   3.431e-01   0.30   dropout 2 x (2, 130)
    attention.output.dense.weight          1.510e-01   4.958e-01   0.30   dropout 2 x (3, 37)
    attention.output.dense.bias            4.859e-02   1.399e-01   0.35   2 x (3, 37)
    attention.output.LayerNorm.weight      5.238e-02   1.284e-01   0.41   dropout 2 x (3, 37)
    attention.output.LayerNorm.bias        4.499e-02   1.386e-01   0.32   2 x (3, 37)
    intermediate.dense.weight              1.190e-01   4.206e-01   0.28   2 x (3, 37)
    intermediate.dense.bias                5.530e-02   1.640e-01   0.34   dropout 2 x (2, 130)
    output.dense.weight                    4.081e-02   1.328e-01   0.31   1 x (2, 5)
    output.dense.bias                      4.280e-02   1.482e-01   0.29   2 x (3, 37)
    output.LayerNorm.weight                4.686e-02   1.320e-01   0.36   dropout 2 x (3, 37)
    output.LayerNorm.bias                  4.363e-02   1.470e-01   0.30   2 x (3, 37)
    cls, learned mix                       2.493e-03   9.637e-03   0.26   2 x (3, 37)
    mix logits' gradient                   5.488e-03   7.019e-03   0.78   2 x (3, 37)

The CLS case's parameter gradients: at most 0.62 (the key bias).  The key bias's gradient is zero in exact arithmetic -- the rows of dS
sum to zero -- and what is left of it measures how well the fused backward's row term D = rowsum(bf16(dctx) . ctx) agrees with
rowsum(dP . P): with D formed from the UNrounded dctx it stood at 1.4 - 2.3 times the bound at 2 x (2, 130), which is why the kernel
rounds dctx there as the products with it do.
"""
import copy
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import bf16_matmul_ref as br  # noqa: E402
import dropout_ref as dr  # noqa: E402
import readout_inputs as ri  # noqa: E402
from trainside_inputs import bound  # noqa: E402

pytestmark = pytest.mark.gpu
FLASH = dict(matmul='bf16', attention='flash')
SEED, STEP = 0x9E3779B97F4A7C15, 3


def _step(enc, tok, typ, mask, G):
    """one training forward + backward -> (hidden, {name: grad})"""
    enc.zero_grad(set_to_none=True)
    hidden = enc(tok, token_type_ids=typ, attention_mask=mask)
    (hidden * G.cuda()).sum().backward()
    return hidden.detach(), {n: p.grad.clone() for n, p in enc.bert.named_parameters()}


@functools.lru_cache(maxsize=None)
def _gpu_run(n_layers, b, l, attention):
    """a bf16-mode step on a case, computed once and shared (never written to); attention None: the keyword left out"""
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, _ = br.case(n_layers, b, l)
    kw = dict(matmul='bf16') if attention is None else dict(matmul='bf16', attention=attention)
    return _step(HipBertTrainEncoder(copy.deepcopy(m), **kw).train(), tok, typ, mask, G)


def _hidden_inside(tag, hidden, h, h32):
    tol = bound(float((h32.double() - h).abs().max()), float(h.abs().max()))
    err = float((hidden.double().cpu() - h).abs().max())
    print(f'[{tag}] hidden |kernel - float64| {err:.3e}  bound {tol:.3e}  ratio {err / tol:.2f}')
    return err <= tol


# ---- 3. parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_layers,b,l', br.CASES)
def test_parity_with_the_exact_float64_model(n_layers, b, l):
    m, tok, typ, mask, G, runs = br.case(n_layers, b, l)
    hidden, got = _gpu_run(n_layers, b, l, 'flash')
    assert hidden.is_cuda and hidden.shape == (b, l, 768)
    assert all(g is not None and torch.isfinite(g).all() for g in got.values())
    (h, g, _), (h32, g32, _) = runs['exact'], runs['emu32']
    tag = f'flash {n_layers} x ({b}, {l})'
    ok = _hidden_inside(tag, hidden, h, h32)
    br.compare_grads(got, g, g32, bound, tag)
    assert ok


def test_cls_readout_with_a_learned_mix():
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, logits, runs = br.cls_case()
    enc = HipBertTrainEncoder(copy.deepcopy(m), **FLASH).train()
    lg = logits.clone().cuda().requires_grad_(True)
    cls = enc.forward_cls((tok, typ, mask), mix=torch.softmax(lg, 0))
    assert cls.shape == (3, 768) and cls.requires_grad
    (cls * G.cuda()).sum().backward()
    (c, g, gl), (c32, g32, gl32) = runs['exact'], runs['emu32']
    tol = bound(float((c32.double() - c).abs().max()), float(c.abs().max()))
    err = float((cls.detach().double().cpu() - c).abs().max())
    print(f'[flash cls 2 x (3, 37)] cls |kernel - float64| {err:.3e}  bound {tol:.3e}  ratio {err / tol:.2f}')
    tol_l = bound(float((gl32.double() - gl).abs().max()), float(gl.abs().max()))
    err_l = float((lg.grad.double().cpu() - gl).abs().max())
    print(f'[flash cls 2 x (3, 37)] mix logits\' gradient |kernel - float64| {err_l:.3e}  bound {tol_l:.3e}  ratio {err_l / tol_l:.2f}')
    br.compare_grads({n: p.grad for n, p in enc.bert.named_parameters()}, g, g32, bound, 'flash cls 2 x (3, 37)')
    assert err <= tol and err_l <= tol_l
    # without a mix: the CLS rows of the mode's last hidden state
    enc2 = HipBertTrainEncoder(copy.deepcopy(m), **FLASH).train()
    assert torch.equal(enc2.forward_cls((tok, typ, mask)).detach(), _gpu_run(2, 3, 37, 'flash')[0][:, 0, :])


# ---- 4. dropout parity ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _drop_case(n_layers, b, l, p):
    """tests/test_gpu_encoder_dropout.py's _case with the mode's emulation inside the masks: the float64 model and the fp32 emulation,
    both under the library's masks of (SEED, STEP)"""
    import test_gpu_encoder_dropout as ted
    m = ted._model(n_layers, b, p, p)
    g = torch.Generator().manual_seed(100 + l)
    tok = torch.randint(0, ted.VOCAB, (b, l), generator=g)
    typ = torch.randint(0, 2, (b, l), generator=g)
    mask = ted._ragged_mask(b, l)
    G = torch.randn(b, l, 768, generator=g)
    masks = ted._site_masks(n_layers, b, l, p, p, SEED, STEP)
    runs = {}
    for key, dt, emulate in (('exact', torch.float64, False), ('emu32', torch.float32, True)):
        mm = copy.deepcopy(m).to(dt).train()
        with dr.given_masks(masks):
            if emulate:
                with br.bf16_matmul():
                    hidden = mm(tok, token_type_ids=typ, attention_mask=mask).last_hidden_state
                    (hidden * G.to(dt)).sum().backward()
            else:
                hidden = mm(tok, token_type_ids=typ, attention_mask=mask).last_hidden_state
                (hidden * G.to(dt)).sum().backward()
        runs[key] = (hidden.detach(), {n: q.grad for n, q in mm.named_parameters()})
    return m, tok, typ, mask, G, runs


@pytest.mark.parametrize('n_layers,b,l', [(2, 3, 37), (2, 2, 130)])
def test_dropout_parity_under_the_same_masks(n_layers, b, l):
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, runs = _drop_case(n_layers, b, l, 0.1)
    enc = HipBertTrainEncoder(copy.deepcopy(m), dropout=True, seed=SEED, **FLASH).train()
    enc.set_dropout_state(SEED, STEP)
    hidden, got = _step(enc, tok, typ, mask, G)
    assert enc.dropout_state() == (SEED, STEP + 1)
    (h, g), (h32, g32) = runs['exact'], runs['emu32']
    tag = f'flash dropout {n_layers} x ({b}, {l})'
    ok = _hidden_inside(tag, hidden, h, h32)
    br.compare_grads(got, g, g32, bound, tag)
    assert ok


# ---- 5. the default is untouched ----------------------------------------------------------------------------------------------------------
def _op_inputs(n_layers=2, b=3, l=37):
    from aspire_amd import HipBertTrainEncoder
    import aspire_amd.torch_ops  # noqa: F401
    m, tok, typ, mask, G, _ = br.case(n_layers, b, l)
    enc = HipBertTrainEncoder(copy.deepcopy(m))
    with torch.no_grad():
        emb = enc.bert.embeddings
        emb_sum = (emb.word_embeddings(tok.cuda()) + emb.token_type_embeddings(typ.cuda())) + emb.position_embeddings.weight[:l]
        weights = [w.detach().clone() for w in enc.layer_weights()]
    return emb_sum, mask.cuda(), weights, G.cuda()


@pytest.mark.parametrize('matmul', [0, 1, 3])
def test_gemm_mode_of_the_attn_operators_gives_the_prec_operators_bits(matmul):
    emb_sum, mask, weights, G = _op_inputs()
    drop = (0.1, 0.1, 12345, 3)
    h0, t0 = torch.ops.aspire.bert_layers_train_prec(emb_sum, mask, weights, 12, 1e-12, *drop, matmul)
    h1, t1 = torch.ops.aspire.bert_layers_train_attn(emb_sum, mask, weights, 12, 1e-12, *drop, matmul, 0)
    assert torch.equal(h0, h1) and t0.numel() == t1.numel()
    a = torch.ops.aspire.bert_layers_backward_prec(G, t0, mask, weights, 12, 1e-12, *drop, matmul)
    c = torch.ops.aspire.bert_layers_backward_attn(G, t1, mask, weights, 12, 1e-12, *drop, matmul, 0)
    assert torch.equal(a[0], c[0]) and all(torch.equal(x, y) for x, y in zip(a[1], c[1]))
    mix = torch.softmax(torch.tensor([0.3, -0.2, 0.5], device='cuda'), 0)
    c0 = torch.ops.aspire.bert_layers_train_cls_prec(emb_sum, mask, weights, mix, 12, 1e-12, *drop, matmul)
    c1 = torch.ops.aspire.bert_layers_train_cls_attn(emb_sum, mask, weights, mix, 12, 1e-12, *drop, matmul, 0)
    assert torch.equal(c0[0], c1[0]) and torch.equal(c0[1], c1[1])
    g = G[:, 0, :].contiguous()
    b0 = torch.ops.aspire.bert_layers_backward_cls_prec(g, c0[1], c0[2], mask, weights, mix, 12, 1e-12, *drop, matmul)
    b1 = torch.ops.aspire.bert_layers_backward_cls_attn(g, c1[1], c1[2], mask, weights, mix, 12, 1e-12, *drop, matmul, 0)
    assert torch.equal(b0[0], b1[0]) and all(torch.equal(x, y) for x, y in zip(b0[1], b1[1])) and torch.equal(b0[2], b1[2])
    with pytest.raises(AssertionError):                    # an unknown mode, before any launch
        torch.ops.aspire.bert_layers_train_attn(emb_sum, mask, weights, 12, 1e-12, *drop, matmul, 2)
    if matmul != 1:
        with pytest.raises(NotImplementedError):           # the fused attention is bf16's alone
            torch.ops.aspire.bert_layers_train_attn(emb_sum, mask, weights, 12, 1e-12, *drop, matmul, 1)


def test_the_default_keyword_is_the_gemm_mode():
    """HipBertTrainEncoder(m, matmul='bf16') and (..., attention='gemm'): the same bits for hidden and every gradient"""
    h0, g0 = _gpu_run(2, 3, 37, None)
    h1, g1 = _gpu_run(2, 3, 37, 'gemm')
    assert torch.equal(h0, h1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ---- 6. the mode does something, and repeats ----------------------------------------------------------------------------------------------
def test_the_mode_does_something_and_repeats():
    from aspire_amd import HipBertTrainEncoder
    h_flash, g1 = _gpu_run(2, 2, 130, 'flash')
    h_gemm, _ = _gpu_run(2, 2, 130, 'gemm')
    diff = float((h_flash - h_gemm).abs().max())
    print(f'max |hidden flash - hidden gemm| at 2 x (2, 130): {diff:.3e}')
    assert not torch.equal(h_flash, h_gemm) and diff > 1e-6
    m, tok, typ, mask, G, _ = br.case(2, 2, 130)
    h2, g2 = _step(HipBertTrainEncoder(copy.deepcopy(m), **FLASH).train(), tok, typ, mask, G)
    assert torch.equal(h_flash, h2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    # eval() and no_grad forwards are the inference path, untouched by the mode
    enc = HipBertTrainEncoder(copy.deepcopy(m), **FLASH).train()
    ref = HipBertTrainEncoder(copy.deepcopy(m)).eval()(tok, token_type_ids=typ, attention_mask=mask)
    with torch.no_grad():
        plain = enc(tok, token_type_ids=typ, attention_mask=mask)
    assert plain.grad_fn is None and torch.equal(plain, ref) and torch.equal(enc.eval()(tok, token_type_ids=typ, attention_mask=mask), ref)


def test_dropout_in_the_mode_repeats_and_draws_the_gemm_modes_masks():
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, _ = br.case(2, 3, 37)

    def run(p, state, **kw):
        mm = copy.deepcopy(m)
        mm.config.hidden_dropout_prob = mm.config.attention_probs_dropout_prob = p
        enc = HipBertTrainEncoder(mm, dropout=True, seed=77, **kw).train()
        enc.set_dropout_state(*state)
        return _step(enc, tok, typ, mask, G)

    h1, g1 = run(0.1, (77, 5), **FLASH)
    h2, g2 = run(0.1, (77, 5), **FLASH)
    assert torch.equal(h1, h2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    assert not torch.equal(h1, run(0.1, (77, 6), **FLASH)[0])
    h0, g0 = run(0.0, (77, 5), **FLASH)
    hn, gn = _gpu_run(2, 3, 37, 'flash')
    assert torch.equal(h0, hn) and all(torch.equal(g0[n], gn[n]) for n in g0)
    # the same masks as the three-kernel form: the two modes differ by rounding alone, far less than another step's masks would
    hg, _ = run(0.1, (77, 5), matmul='bf16')
    same, other = float((h1 - hg).abs().max()), float((h1 - run(0.1, (77, 6), matmul='bf16')[0]).abs().max())
    print(f'max |hidden flash - hidden gemm| under dropout: same masks {same:.3e}, another step\'s masks {other:.3e}')
    assert same < 0.1 * other


# ---- 7. every buffer written ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('l', [5, 130])
def test_every_gradient_buffer_is_written(l):
    """the C entries themselves on gradient buffers and a workspace pre-filled with NaN bits; the operator's tape has the query's size"""
    from aspire_amd import _lib, ops
    from aspire_amd.encoder import pack_layer_stack
    lib = _lib.lib
    emb_sum, mask, weights, G = _op_inputs(2, 2, l)
    b = 2
    bw = pack_layer_stack(weights, 12, 1e-12)
    need_t = lib.aspire_bert_tape_bytes_attn(ctypes.byref(bw), b, l, 1)
    need_w = lib.aspire_bert_train_workspace_bytes_attn(ctypes.byref(bw), b, l, 1)
    assert torch.ops.aspire.bert_layers_train_attn(emb_sum, mask, weights, 12, 1e-12, 0.1, 0.1, 5, 0, 1, 1)[1].numel() == need_t
    assert need_t < lib.aspire_bert_tape_bytes(ctypes.byref(bw), b, l)
    drop = _lib.BertDropout(0.1, 0.1, SEED, STEP)
    for d in (None, drop):
        out = torch.full_like(emb_sum, float('nan'))
        tape = torch.full((need_t,), 0xFF, device='cuda', dtype=torch.uint8)
        ws = torch.full((need_w,), 0xFF, device='cuda', dtype=torch.uint8)
        dp = ctypes.byref(d) if d is not None else None
        _lib.check(lib.aspire_bert_layers_forward_train_attn_f32(ctypes.byref(bw), ops._ptr(emb_sum), ops._ptr(mask), b, l, ops._ptr(out),
                                                                 ops._ptr(tape), need_t, ops._ptr(ws), need_w, dp, 1, 1, ops._stream()))
        assert torch.isfinite(out).all()
        grads = [torch.full_like(w, float('nan')) for w in weights]
        grad_emb = torch.full_like(G, float('nan'))
        layers = (_lib.BertLayerGrads * 2)()
        for i in range(2):
            for (f, _), t in zip(_lib.BertLayerGrads._fields_, grads[2 + 12 * i:14 + 12 * i]):
                setattr(layers[i], f, ctypes.c_void_p(t.data_ptr()))
        bg = _lib.BertGrads(ctypes.c_void_p(grads[0].data_ptr()), ctypes.c_void_p(grads[1].data_ptr()), layers)
        ws.fill_(0xFF)
        _lib.check(lib.aspire_bert_layers_backward_attn_f32(ctypes.byref(bw), ops._ptr(mask), b, l, ops._ptr(G), None, None, None, ops._ptr(tape),
                                                            need_t, ops._ptr(grad_emb), ctypes.byref(bg), None, ops._ptr(ws), need_w, dp, 1, 1,
                                                            ops._stream()))
        assert torch.isfinite(grad_emb).all() and all(torch.isfinite(g).all() for g in grads)
        # one byte less than the mode's own tape size is refused
        assert lib.aspire_bert_layers_backward_attn_f32(ctypes.byref(bw), ops._ptr(mask), b, l, ops._ptr(G), None, None, None, ops._ptr(tape),
                                                        need_t - 1, ops._ptr(grad_emb), ctypes.byref(bg), None, ops._ptr(ws), need_w, dp, 1, 1,
                                                        ops._stream()) == _lib.ASPIRE_ERR_INVALID_ARG


# ---- 8. operators and trainer -------------------------------------------------------------------------------------------------------------
def test_opcheck_the_new_operators():
    """the forwards without test_aot_dispatch_dynamic (it compares output VALUES of two runs, and the tape is opaque bytes whose gaps
    between slots are unwritten); the backwards' outputs are all written and take every check"""
    emb_sum, mask, weights, G = _op_inputs(1, 2, 5)
    key = (12, 1e-12, 0.1, 0.1, SEED - 2 ** 64, STEP, 1, 1)
    fwd_utils = ('test_schema', 'test_autograd_registration', 'test_faketensor')
    torch.library.opcheck(torch.ops.aspire.bert_layers_train_attn,
                          (emb_sum.clone().requires_grad_(), mask, [w.clone().requires_grad_() for w in weights]) + key, test_utils=fwd_utils)
    hidden, tape = torch.ops.aspire.bert_layers_train_attn(emb_sum, mask, weights, *key)
    torch.library.opcheck(torch.ops.aspire.bert_layers_backward_attn, (G, tape, mask, weights) + key)
    mix = torch.softmax(torch.tensor([0.3, -0.2], device='cuda'), 0)
    torch.library.opcheck(torch.ops.aspire.bert_layers_train_cls_attn,
                          (emb_sum.clone().requires_grad_(), mask, [w.clone().requires_grad_() for w in weights], mix) + key, test_utils=fwd_utils)
    cls, layer_cls, tape = torch.ops.aspire.bert_layers_train_cls_attn(emb_sum, mask, weights, mix, *key)
    torch.library.opcheck(torch.ops.aspire.bert_layers_backward_cls_attn, (G[:, 0, :].contiguous(), layer_cls, tape, mask, weights, mix) + key)


def test_trainer_resumes_on_the_straight_runs_bits(tmp_path):
    """RankTrainer in the mode with dropout, the tables frozen (their scatter gradient is torch's): two updates straight, and one + a
    checkpoint + one, end on the same bits; the checkpoint names both modes and a gemm-mode encoder refuses it"""
    import test_gpu_encoder_bf16 as teb
    from aspire_amd import HipBertTrainEncoder, RankTrainer
    batches = teb._batches(str(tmp_path))
    hparams = ri.hparams('l2wasserstein', 0.0)
    train_hparams = dict(es_check_every=1000, train_size=6, dev_size=3, batch_size=3, num_epochs=2, update_rule='adam', learning_rate=1e-3,
                         lr_decay_method='exponential', decay_lr_by=0.7, decay_lr_every=1)

    def make(seed, tag, **kw):
        model = teb._trainer_bert(seed)
        for n, p in model.named_parameters():
            if n in teb.TABLES:
                p.requires_grad_(False)
        enc = HipBertTrainEncoder(model, dropout=True, seed=0x9E3779B97F4A7C15, **kw)
        return RankTrainer(enc, hparams, train_hparams, str(tmp_path / tag), lambda epoch: batches)

    straight = make(5, 'straight', **FLASH)
    straight.train(max_iterations=2)
    first = make(5, 'first', **FLASH)
    first.train(max_iterations=1)
    first.save_checkpoint(tmp_path / 'ck.pt')
    state = torch.load(tmp_path / 'ck.pt', weights_only=True)
    assert state['matmul'] == 'bf16' and state['attention'] == 'flash'
    second = make(99, 'second', **FLASH)
    second.load_checkpoint(tmp_path / 'ck.pt')
    second.train(max_iterations=1)
    assert second.iteration == straight.iteration == 2
    trained = 0
    for (n, a), (_, b) in zip(second.encoder.bert.named_parameters(), straight.encoder.bert.named_parameters()):
        assert torch.isfinite(a).all() and torch.equal(a, b), n
        sa, sb = second.optimizer.state.get(a, {}), straight.optimizer.state.get(b, {})
        assert set(sa) == set(sb), n
        for key in sa:
            assert torch.equal(sa[key], sb[key]), (n, key)
        trained += bool(sa)
    assert trained >= 16
    other = make(5, 'other', matmul='bf16')
    with pytest.raises(ValueError, match="'flash'.*'gemm'"):
        other.load_checkpoint(tmp_path / 'ck.pt')
