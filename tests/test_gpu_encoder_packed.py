"""GPU: the training encoder's padding-free mode -- aspire_amd.HipBertTrainEncoder(bert, matmul='bf16', attention='flash', packed=True)
(torch.ops.aspire.bert_layers_train_packed / bert_layers_train_cls_packed over aspire_bert_layers_forward_train_packed_f32 /
aspire_bert_layers_backward_packed_f32; the kernels: enc_pack.hip and the PackedDocs instantiations of enc_attn_train.hip, tested bare
in tests/test_gpu_flash_attn_packed.py).  Modelled on tests/test_gpu_encoder_flash.py.

Yardstick: the EXACT float64 CPU model on the padded batch with the loss zeroed on masked rows, G * mask (a pad row buys nothing:
tests/test_packed_rows_cpu.py pins that it equals the per-document runs).  Bound per tensor: trainside_inputs.bound(ref_err, max|x|) with
ref_err the deviation from float64 of the bf16 mode's arithmetic emulated in fp32 on the same padded batch.  ``hidden`` is compared on
valid rows; every parameter gradient is compared, the key bias included.  Masked rows of ``hidden`` and of the embedding sum's gradient
must be exact zeros.

Largest |kernel - float64| / bound on an MI355X (every comparison prints its figures before it asserts): hidden on valid rows 0.25 - 0.26
(0.23 - 0.24 under dropout 0.1, 0.27 with a full mask); the key bias, the tensor nearest its bound, 0.37 at 1 x (2, 5), 0.35 at
2 x (3, 37), 0.41 at 2 x (2, 130), 0.43 / 0.45 under dropout, 0.48 with a full mask, 0.73 in the CLS case; cls with a learned mix 0.25,
the mix logits' gradient 0.23.  Under the same (seed, step) the packed and the padded flash hidden differ on valid rows by 0 at
2 x (3, 37) and 1.8e-03 at 2 x (2, 130), against 5.4 and 4.9 under another step's masks.  With a full mask the packed mode equals the
padded flash mode bit for bit.  Tape bytes at 2 x 5 (8 of 10 rows): 427 520 against 534 528; at 2 x 130 (251 of 260): 13 413 888 against
13 894 656.
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
PACKED = dict(packed=True, **FLASH)
SEED, STEP = 0x9E3779B97F4A7C15, 3


def _step(enc, tok, typ, mask, G):
    """one training forward + backward -> (hidden, {name: grad})"""
    enc.zero_grad(set_to_none=True)
    hidden = enc(tok, token_type_ids=typ, attention_mask=mask)
    (hidden * G.cuda()).sum().backward()
    return hidden.detach(), {n: p.grad.clone() for n, p in enc.bert.named_parameters()}


@functools.lru_cache(maxsize=None)
def _masked_runs(n_layers, b, l):
    """br.case's model and inputs with G * mask: the float64 run and the fp32 emulation, computed once, never written to"""
    m, tok, typ, mask, G, _ = br.case(n_layers, b, l)
    Gm = G * mask[..., None]
    return m, tok, typ, mask, Gm, br._run(m, torch.float64, False, tok, typ, mask, Gm), br._run(m, torch.float32, True, tok, typ, mask, Gm)


@functools.lru_cache(maxsize=None)
def _gpu_run(n_layers, b, l, **kw):
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, Gm = _masked_runs(n_layers, b, l)[:5]
    return _step(HipBertTrainEncoder(copy.deepcopy(m), **kw).train(), tok, typ, mask, Gm)


def _hidden_inside(tag, hidden, h, h32, mask):
    v = mask.bool()
    tol = bound(float((h32[v].double() - h[v]).abs().max()), float(h[v].abs().max()))
    err = float((hidden.double().cpu()[v] - h[v]).abs().max())
    print(f'[{tag}] hidden (valid rows) |kernel - float64| {err:.3e}  bound {tol:.3e}  ratio {err / tol:.2f}')
    return err <= tol


# ---- parity -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_layers,b,l', br.CASES)
def test_parity_with_the_exact_float64_model(n_layers, b, l):
    m, tok, typ, mask, Gm, (h, g, _), (h32, g32, _) = _masked_runs(n_layers, b, l)
    hidden, got = _gpu_run(n_layers, b, l, **PACKED)
    assert hidden.is_cuda and hidden.shape == (b, l, 768)
    assert all(x is not None and torch.isfinite(x).all() for x in got.values())
    assert bool((hidden.cpu()[~mask.bool()] == 0).all())                       # masked rows: exact zeros
    tag = f'packed {n_layers} x ({b}, {l})'
    ok = _hidden_inside(tag, hidden, h, h32, mask)
    br.compare_grads(got, g, g32, bound, tag)
    assert ok


def _op_inputs(n_layers, b, l, mask=None):
    from aspire_amd import HipBertTrainEncoder, packed_rows
    import aspire_amd.torch_ops  # noqa: F401
    m, tok, typ, case_mask, G, _ = br.case(n_layers, b, l)
    mask = case_mask if mask is None else mask
    enc = HipBertTrainEncoder(copy.deepcopy(m))
    with torch.no_grad():
        emb = enc.bert.embeddings
        emb_sum = (emb.word_embeddings(tok.cuda()) + emb.token_type_embeddings(typ.cuda())) + emb.position_embeddings.weight[:l]
        weights = [w.detach().clone() for w in enc.layer_weights()]
    pr = packed_rows(mask.cuda())
    return emb_sum, mask.cuda(), weights, G.cuda(), (pr.doc_start, pr.row_src, pr.row_dst, pr.max_len, pr.prefix)


def test_output_layout():
    """masked rows of hidden and of the embedding sum's gradient are exact zeros -- the all-zero document throughout -- and the incoming
    gradient is read on valid rows only (NaN on masked rows changes nothing); R == 0: zeros"""
    emb_sum, mask, weights, G, lists = _op_inputs(2, 3, 37)
    key = (12, 1e-12, 0.1, 0.1, SEED - 2 ** 64, STEP)
    hidden, tape = torch.ops.aspire.bert_layers_train_packed(emb_sum, *lists, weights, *key)
    v = mask.bool()
    assert torch.isfinite(hidden).all() and bool((hidden[~v] == 0).all()) and bool((hidden[2] == 0).all()) and bool((hidden[v] != 0).any())
    grad_emb, grads = torch.ops.aspire.bert_layers_backward_packed(G, tape, *lists, weights, *key)
    assert torch.isfinite(grad_emb).all() and bool((grad_emb[~v] == 0).all()) and bool((grad_emb[2] == 0).all())
    poisoned = torch.where(v[..., None], G, torch.full_like(G, float('nan')))
    grad_emb2, grads2 = torch.ops.aspire.bert_layers_backward_packed(poisoned, tape, *lists, weights, *key)
    assert torch.equal(grad_emb, grad_emb2) and all(torch.equal(x, y) for x, y in zip(grads, grads2))
    # no valid token at all
    from aspire_amd import packed_rows
    pr = packed_rows(torch.zeros_like(mask))
    none = (pr.doc_start, pr.row_src, pr.row_dst, pr.max_len, pr.prefix)
    assert pr.rows == 0 and pr.max_len == 0
    hidden0, tape0 = torch.ops.aspire.bert_layers_train_packed(emb_sum, *none, weights, *key)
    assert bool((hidden0 == 0).all())
    grad_emb0, grads0 = torch.ops.aspire.bert_layers_backward_packed(G, tape0, *none, weights, *key)
    assert bool((grad_emb0 == 0).all()) and all(bool((x == 0).all()) for x in grads0)


# ---- dropout ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _drop_case(n_layers, b, l, p):
    """tests/test_gpu_encoder_flash.py's _drop_case with G * mask: the float64 model and the fp32 emulation under the library's masks"""
    import test_gpu_encoder_dropout as ted
    m = ted._model(n_layers, b, p, p)
    g = torch.Generator().manual_seed(100 + l)
    tok = torch.randint(0, ted.VOCAB, (b, l), generator=g)
    typ = torch.randint(0, 2, (b, l), generator=g)
    mask = ted._ragged_mask(b, l)
    G = torch.randn(b, l, 768, generator=g) * mask[..., None]
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
def test_dropout_parity_repeats_and_draws_the_padded_modes_masks(n_layers, b, l):
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, runs = _drop_case(n_layers, b, l, 0.1)

    def run(step, **kw):
        enc = HipBertTrainEncoder(copy.deepcopy(m), dropout=True, seed=SEED, **kw).train()
        enc.set_dropout_state(SEED, step)
        out = _step(enc, tok, typ, mask, G)
        assert enc.dropout_state() == (SEED, step + 1)
        return out

    hidden, got = run(STEP, **PACKED)
    (h, g), (h32, g32) = runs['exact'], runs['emu32']
    tag = f'packed dropout {n_layers} x ({b}, {l})'
    ok = _hidden_inside(tag, hidden, h, h32, mask)
    br.compare_grads(got, g, g32, bound, tag)
    assert ok
    h2, g2 = run(STEP, **PACKED)                                           # the step repeats bit for bit
    assert torch.equal(hidden, h2) and all(torch.equal(got[n], g2[n]) for n in got)
    v = mask.bool().cuda()
    other_step = run(STEP + 1, **PACKED)[0]
    assert not torch.equal(hidden, other_step)                             # another step's masks differ
    # the same (seed, step) draws the padded flash mode's masks at valid positions: rounding apart, far less than other masks would give
    same = float((hidden[v] - run(STEP, **FLASH)[0][v]).abs().max())
    other = float((hidden[v] - run(STEP + 1, **FLASH)[0][v]).abs().max())
    print(f'[{tag}] max |hidden packed - hidden padded flash| on valid rows: same masks {same:.3e}, another step\'s masks {other:.3e}')
    assert same < 0.1 * other


# ---- the CLS read-out -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cls_case():
    """lengths (37, 29, 1) at L = 37 with a hole past position 0 in the first document: every mask starts with a valid token"""
    m, tok, typ, _, _, _ = br.case(2, 3, 37)
    mask = torch.ones(3, 37, dtype=torch.int64)
    mask[0, 20] = 0
    mask[0, 5:7] = 0
    mask[1, 29:] = 0
    mask[2, 1:] = 0
    g = torch.Generator().manual_seed(7)
    G = torch.randn(3, 768, generator=g)
    logits = torch.randn(3, generator=g)
    runs = {'exact': br._run(m, torch.float64, False, tok, typ, mask, G, logits), 'emu32': br._run(m, torch.float32, True, tok, typ, mask, G, logits)}
    return m, tok, typ, mask, G, logits, runs


def test_cls_readout_with_a_learned_mix():
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, logits, runs = _cls_case()
    enc = HipBertTrainEncoder(copy.deepcopy(m), **PACKED).train()
    lg = logits.clone().cuda().requires_grad_(True)
    cls = enc.forward_cls((tok, typ, mask), mix=torch.softmax(lg, 0))
    assert cls.shape == (3, 768) and cls.requires_grad
    (cls * G.cuda()).sum().backward()
    (c, g, gl), (c32, g32, gl32) = runs['exact'], runs['emu32']
    tol = bound(float((c32.double() - c).abs().max()), float(c.abs().max()))
    err = float((cls.detach().double().cpu() - c).abs().max())
    print(f'[packed cls (37, 29, 1)] cls |kernel - float64| {err:.3e}  bound {tol:.3e}  ratio {err / tol:.2f}')
    tol_l = bound(float((gl32.double() - gl).abs().max()), float(gl.abs().max()))
    err_l = float((lg.grad.double().cpu() - gl).abs().max())
    print(f'[packed cls (37, 29, 1)] mix logits\' gradient |kernel - float64| {err_l:.3e}  bound {tol_l:.3e}  ratio {err_l / tol_l:.2f}')
    br.compare_grads({n: p.grad for n, p in enc.bert.named_parameters()}, g, g32, bound, 'packed cls (37, 29, 1)')
    assert err <= tol and err_l <= tol_l
    # without a mix: the CLS rows of the mode's last hidden state, bit for bit
    enc2 = HipBertTrainEncoder(copy.deepcopy(m), **PACKED).train()
    hidden = HipBertTrainEncoder(copy.deepcopy(m), **PACKED).train()(tok, token_type_ids=typ, attention_mask=mask)
    assert torch.equal(enc2.forward_cls((tok, typ, mask)).detach(), hidden.detach()[:, 0, :])
    # a document that does not start with a valid token has no CLS row: refused on the host
    with pytest.raises(ValueError, match=r'attention_mask\[:, 0\] == 1'):
        enc2.forward_cls((tok, typ, br._mask(3, 37)))


# ---- every buffer written ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('l', [5, 130])
def test_every_gradient_buffer_is_written(l):
    """the C entries themselves on a tape, a workspace and gradient buffers pre-filled with 0xFF bytes (NaN); the packed tape query is at
    most the _attn query and strictly below it when a row is masked; one byte less than it is refused"""
    from aspire_amd import _lib, ops, packed_rows
    from aspire_amd.encoder import pack_layer_stack
    lib = _lib.lib
    emb_sum, mask, weights, G, lists = _op_inputs(2, 2, l)
    b = 2
    pr = packed_rows(mask)
    assert pr.rows < b * l
    pk = _lib.BertPacking(pr.rows, pr.max_len, int(pr.prefix), *(ctypes.c_void_p(t.data_ptr()) for t in (pr.doc_start, pr.row_src, pr.row_dst)))
    bw = pack_layer_stack(weights, 12, 1e-12)
    need_t = lib.aspire_bert_tape_bytes_packed(ctypes.byref(bw), b, l, pr.rows)
    need_w = lib.aspire_bert_train_workspace_bytes_packed(ctypes.byref(bw), b, l, pr.rows)
    attn_t = lib.aspire_bert_tape_bytes_attn(ctypes.byref(bw), b, l, 1)
    print(f'tape bytes at 2 x {l} ({pr.rows} of {b * l} rows): packed {need_t}, padded flash {attn_t}')
    assert 0 < need_t < attn_t and lib.aspire_bert_tape_bytes_packed(ctypes.byref(bw), b, l, b * l) <= attn_t
    assert torch.ops.aspire.bert_layers_train_packed(emb_sum, *lists, weights, 12, 1e-12, 0.1, 0.1, 5, 0)[1].numel() == need_t
    drop = _lib.BertDropout(0.1, 0.1, SEED, STEP)
    for d in (None, drop):
        out = torch.full_like(emb_sum, float('nan'))
        tape = torch.full((need_t,), 0xFF, device='cuda', dtype=torch.uint8)
        ws = torch.full((need_w,), 0xFF, device='cuda', dtype=torch.uint8)
        dp = ctypes.byref(d) if d is not None else None
        _lib.check(lib.aspire_bert_layers_forward_train_packed_f32(ctypes.byref(bw), ops._ptr(emb_sum), ctypes.byref(pk), b, l, ops._ptr(out),
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
        args = (ctypes.byref(bw), ctypes.byref(pk), b, l, ops._ptr(G), None, None, None, ops._ptr(tape))
        tail = (ops._ptr(grad_emb), ctypes.byref(bg), None, ops._ptr(ws), need_w, dp)
        _lib.check(lib.aspire_bert_layers_backward_packed_f32(*args, need_t, *tail, 1, 1, ops._stream()))
        assert torch.isfinite(grad_emb).all() and all(torch.isfinite(g).all() for g in grads)
        assert lib.aspire_bert_layers_backward_packed_f32(*args, need_t - 1, *tail, 1, 1, ops._stream()) == _lib.ASPIRE_ERR_INVALID_ARG
        # the modes: anything but (bf16, flash) is refused before a launch
        assert lib.aspire_bert_layers_backward_packed_f32(*args, need_t, *tail, 1, 0, ops._stream()) == _lib.ASPIRE_ERR_UNSUPPORTED
        assert lib.aspire_bert_layers_backward_packed_f32(*args, need_t, *tail, 0, 1, ops._stream()) == _lib.ASPIRE_ERR_UNSUPPORTED


# ---- mode equivalence -------------------------------------------------------------------------------------------------------------------
def test_packed_false_is_the_padded_mode():
    """HipBertTrainEncoder(m, **FLASH) and (..., packed=False): the same bits for hidden and every gradient"""
    h0, g0 = _gpu_run(2, 3, 37, **FLASH)
    h1, g1 = _gpu_run(2, 3, 37, packed=False, **FLASH)
    assert torch.equal(h0, h1) and all(torch.equal(g0[n], g1[n]) for n in g0)


def test_a_full_mask_agrees_with_the_padded_flash_mode():
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, _, G, _ = br.case(2, 3, 37)
    mask = torch.ones(3, 37, dtype=torch.int64)
    (h, g, _), (h32, g32, _) = br._run(m, torch.float64, False, tok, typ, mask, G), br._run(m, torch.float32, True, tok, typ, mask, G)
    hp, gp = _step(HipBertTrainEncoder(copy.deepcopy(m), **PACKED).train(), tok, typ, mask, G)
    hf, gf = _step(HipBertTrainEncoder(copy.deepcopy(m), **FLASH).train(), tok, typ, mask, G)
    same = torch.equal(hp, hf) and all(torch.equal(gp[n], gf[n]) for n in gp)
    print(f'full mask 2 x (3, 37): packed and padded flash bit-equal: {same}; max |hidden difference| {float((hp - hf).abs().max()):.3e}')
    ok = _hidden_inside('packed, full mask', hp, h, h32, mask)
    br.compare_grads(gp, g, g32, bound, 'packed, full mask')
    assert ok


# ---- operators and trainer --------------------------------------------------------------------------------------------------------------
def test_opcheck_the_new_operators():
    """the forwards without test_aot_dispatch_dynamic, as tests/test_gpu_encoder_flash.py restricts them (the tape is opaque bytes whose
    gaps between slots are unwritten); the backwards take every check"""
    mask = torch.ones(2, 5, dtype=torch.int64)
    mask[1, 3:] = 0
    emb_sum, mask, weights, G, lists = _op_inputs(1, 2, 5, mask)
    key = (12, 1e-12, 0.1, 0.1, SEED - 2 ** 64, STEP)
    fwd_utils = ('test_schema', 'test_autograd_registration', 'test_faketensor')
    torch.library.opcheck(torch.ops.aspire.bert_layers_train_packed,
                          (emb_sum.clone().requires_grad_(), *lists, [w.clone().requires_grad_() for w in weights]) + key, test_utils=fwd_utils)
    hidden, tape = torch.ops.aspire.bert_layers_train_packed(emb_sum, *lists, weights, *key)
    torch.library.opcheck(torch.ops.aspire.bert_layers_backward_packed, (G, tape, *lists, weights) + key)
    mix = torch.softmax(torch.tensor([0.3, -0.2], device='cuda'), 0)
    torch.library.opcheck(torch.ops.aspire.bert_layers_train_cls_packed,
                          (emb_sum.clone().requires_grad_(), *lists, [w.clone().requires_grad_() for w in weights], mix) + key,
                          test_utils=fwd_utils)
    cls, layer_cls, tape = torch.ops.aspire.bert_layers_train_cls_packed(emb_sum, *lists, weights, mix, *key)
    torch.library.opcheck(torch.ops.aspire.bert_layers_backward_cls_packed, (G[:, 0, :].contiguous(), layer_cls, tape, *lists, weights, mix) + key)


def test_trainer_resumes_on_the_straight_runs_bits(tmp_path):
    """RankTrainer in the mode with dropout, the tables frozen (their scatter gradient is torch's): two updates straight, and one + a
    checkpoint + one, end on the same bits; the checkpoint says packed: True and a padded encoder refuses it"""
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

    straight = make(5, 'straight', **PACKED)
    straight.train(max_iterations=2)
    first = make(5, 'first', **PACKED)
    first.train(max_iterations=1)
    first.save_checkpoint(tmp_path / 'ck.pt')
    state = torch.load(tmp_path / 'ck.pt', weights_only=True)
    assert state['matmul'] == 'bf16' and state['attention'] == 'flash' and state['packed'] is True
    second = make(99, 'second', **PACKED)
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
    other = make(5, 'other', **FLASH)
    with pytest.raises(ValueError, match='packed=True.*packed=False'):
        other.load_checkpoint(tmp_path / 'ck.pt')
    # a checkpoint from before the key means packed=False: a packed encoder refuses it
    del state['packed']
    torch.save(state, tmp_path / 'old.pt')
    with pytest.raises(ValueError, match='packed=False.*packed=True'):
        make(5, 'third', **PACKED).load_checkpoint(tmp_path / 'old.pt')
    make(5, 'fourth', **FLASH).load_checkpoint(tmp_path / 'old.pt')
