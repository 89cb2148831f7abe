"""GPU: the inference encoder's opt-in fp16 matmul mode -- aspire_amd.HipBertEncoder(bert, matmul='fp16') over
aspire_bert_forward_prec_f32 / aspire_bert_forward_cls_prec_f32 (include/aspire_hip.h, A1h).

Yardstick: the EXACT float64 CPU model (nothing rounded to fp16), on valid rows.  Bound per tensor: trainside_inputs.bound(ref_err,
max|exact|) = max(4 ref_err, 4 * 2^-23 max|exact|), ref_err the deviation from the exact model of the mode's arithmetic emulated on the
CPU in float64 (tests/fp16_matmul_ref.py: both operands of the four projections of a layer rounded to fp16 once, the weights as
fp16(64 w); the CLS forward's emulation keeps the last layer's tail behind its QKV projection exact, as the kernels do).  What the bound
checks: the kernels round what the mode says is rounded, once, and nothing else -- an operand rounded twice, left unrounded or
truncated moves a tensor by about ref_err itself.

Largest |kernel - float64| / bound per tensor group on an MI355X, the case where the ratio is largest (every comparison prints its
figures before it asserts; also DESIGN.md section 7, "fp16 matrix products in the inference encoder"):

    group                          error       bound       ratio  case
    hidden                         1.062e-03   4.232e-03   0.25   2 x (3, 37)
    hidden                         3.951e-04   1.580e-03   0.25   1 x (2, 5)
    hidden                         9.774e-04   4.236e-03   0.23   2 x (2, 130)
    hidden                         1.101e-03   4.363e-03   0.25   2 x (3, 100)
    hidden, heavy-tailed weights   2.137e-02   8.415e-02   0.25   4 x (4, 128)
    cls                            6.557e-04   2.435e-03   0.27   2 x (3, 37)
    cls, layer mix                 5.342e-04   1.996e-03   0.27   2 x (3, 37)
    cls of every layer             6.557e-04   2.435e-03   0.27   2 x (3, 37)
    pooled: cls                    5.855e-04   2.375e-03   0.25   2 x (3, 37)
    pooled: pooler_output          2.681e-04   9.779e-04   0.27   2 x (3, 37)
    mean, RoBERTa-shaped           6.940e-04   3.295e-03   0.21   2 x (3, 37)
    hidden, RoBERTa-shaped         1.036e-03   4.407e-03   0.23   2 x (3, 37)
    mean, MPNet-shaped             7.496e-04   2.826e-03   0.27   2 x (3, 37)
    hidden, MPNet-shaped           1.167e-03   4.324e-03   0.27   2 x (3, 37)

A ratio of 0.25 is the emulation's own error: the bound is four times it.  Every tensor sits at 0.21 - 0.27, so the kernels' error IS
the mode's rounding.  The mode against the default at 2 x (2, 130): 9.8e-4 apart, 271 x the default's own 3.6e-6 against float64; the
fall-back case returns HuggingFace's sentence reps at 2.1e-5 (bar 1e-4).
"""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import fp16_matmul_ref as fr  # noqa: E402
from trainside_inputs import bound  # noqa: E402

pytestmark = pytest.mark.gpu


def _compare(tag, got, exact, emu, rows=None):
    """prints error, bound and ratio, then asserts |got - exact| <= bound(ref_err, max|exact|) over `rows` (a bool index or None)"""
    got, exact, emu = got.double().cpu(), exact.double(), emu.double()
    if rows is not None:
        got, exact, emu = got[rows], exact[rows], emu[rows]
    assert got.numel() > 0 and bool(torch.isfinite(got).all()), tag
    ref_err = (emu - exact).abs().max().item()
    err = (got - exact).abs().max().item()
    bd = bound(ref_err, exact.abs().max().item())
    print(f'{tag:<44} error {err:.3e}  bound {bd:.3e}  ratio {err / bd:.2f}  (emulation {ref_err:.3e})')
    assert err <= bd, (tag, err, bd)
    return err


@functools.lru_cache(maxsize=None)
def _encoder(n_layers, b, l, ffn, matmul, pooler=False):
    """one encoder per case and mode, shared (never written to); matmul None: the default-constructed encoder"""
    from aspire_amd.encoder import HipBertEncoder
    m = fr.case(n_layers, b, l, ffn, pooler)[0]
    return HipBertEncoder(m) if matmul is None else HipBertEncoder(m, matmul=matmul)


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_layers,b,l,ffn', fr.CASES)
def test_hidden_parity_with_the_exact_float64_model(n_layers, b, l, ffn):
    m, tok, typ, mask, exact, emu, _ = fr.case(n_layers, b, l, ffn)
    enc = _encoder(n_layers, b, l, ffn, 'fp16')
    assert enc.matmul == 'fp16'
    got = enc.forward_hidden(tok, typ, mask)
    assert got.is_cuda and got.shape == (b, l, 768) and got.dtype == torch.float32
    _compare(f'hidden {n_layers} x ({b}, {l})', got, exact.last_hidden_state, emu.last_hidden_state, mask.bool())
    assert enc.status() == 0


def test_hidden_parity_on_heavy_tailed_weights():
    from aspire_amd.encoder import HipBertEncoder
    m, tok, typ, mask, exact, emu, _ = fr.heavy_case()
    enc = HipBertEncoder(m, matmul='fp16')
    assert enc.matmul == 'fp16'
    _compare('hidden heavy-tailed 4 x (4, 128)', enc.forward_hidden(tok, typ, mask), exact.last_hidden_state, emu.last_hidden_state, mask.bool())


@pytest.mark.parametrize('n_layers,b,l,ffn', fr.CASES)
def test_cls_parity_with_and_without_a_layer_mix(n_layers, b, l, ffn):
    m, tok, typ, mask, exact, _, emu = fr.case(n_layers, b, l, ffn)             # emu: the CLS forward's emulation (exact last-layer tail)
    enc = _encoder(n_layers, b, l, ffn, 'fp16')
    docs = mask[:, 0].bool()                                                    # documents whose CLS row is a valid row
    cls, layers = enc.forward_cls(tok, typ, mask)
    assert layers is None
    _compare(f'cls {n_layers} x ({b}, {l})', cls, exact.last_hidden_state[:, 0], emu.last_hidden_state[:, 0], docs)
    mix = torch.softmax(torch.linspace(-1.0, 1.0, n_layers + 1), 0).tolist()
    want = sum(w * h[:, 0] for w, h in zip(mix, exact.hidden_states))
    want_emu = sum(w * h[:, 0] for w, h in zip(mix, emu.hidden_states))
    cls, layers = enc.forward_cls(tok, typ, mask, layer_mix=mix, want_layers=True)
    _compare(f'cls, layer mix {n_layers} x ({b}, {l})', cls, want, want_emu, docs)
    assert layers.shape == (n_layers + 1, b, 768)
    _compare(f'cls of every layer {n_layers} x ({b}, {l})', layers.permute(1, 0, 2), torch.stack([h[:, 0] for h in exact.hidden_states], 1),
             torch.stack([h[:, 0] for h in emu.hidden_states], 1), docs)


def test_pooled_parity():
    n_layers, b, l, ffn = fr.CASES[1]
    m, tok, typ, mask, exact, _, emu = fr.case(n_layers, b, l, ffn, True)
    enc = _encoder(n_layers, b, l, ffn, 'fp16', True)
    docs = mask[:, 0].bool()
    cls, pooled = enc.forward_pooled(tok, typ, mask)
    _compare('pooled: cls', cls, exact.last_hidden_state[:, 0], emu.last_hidden_state[:, 0], docs)
    _compare('pooled: pooler_output', pooled, exact.pooler_output, emu.pooler_output, docs)


@pytest.mark.parametrize('kind', ['roberta', 'mpnet'])
def test_mean_parity_on_roberta_and_mpnet_shaped_models(kind):
    from aspire_amd.encoder import HipBertEncoder
    m, ids, mask, exact, emu = fr.sbert_case(kind)
    enc = HipBertEncoder(m, matmul='fp16')
    assert enc.kind == kind and enc.matmul == 'fp16'
    got = enc.forward_mean(ids, None, mask)
    _compare(f'mean {kind} 2 x (3, 37)', got, fr.masked_mean(exact.last_hidden_state, mask), fr.masked_mean(emu.last_hidden_state, mask))
    _compare(f'hidden {kind} 2 x (3, 37)', enc.forward_hidden(ids, None, mask), exact.last_hidden_state, emu.last_hidden_state, mask.bool())


# ---- the default is untouched ------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('b,l', [(3, 37), (8, 128)])             # 8 x 128 = 1024 rows: the default's P path
def test_default_and_fp32_keyword_give_the_same_bits(b, l):
    from aspire_amd.encoder import HipBertEncoder
    m = fr.bert(2, seed=23, pooler=False)
    g = torch.Generator().manual_seed(b * l)
    tok, typ = torch.randint(0, fr.VOCAB, (b, l), generator=g), torch.randint(0, 2, (b, l), generator=g)
    mask = (torch.arange(l)[None, :] < torch.randint(l // 3, l + 1, (b, 1), generator=g)).long()
    e0, e1 = HipBertEncoder(m), HipBertEncoder(m, matmul='fp32')
    assert e0.matmul == e1.matmul == 'fp32' and e1._hplanes is None
    h0, h1 = e0.forward_hidden(tok, typ, mask), e1.forward_hidden(tok, typ, mask)
    assert torch.equal(_bits(h0), _bits(h1))
    mix = torch.softmax(torch.arange(3.0), 0).tolist()
    (c0, l0), (c1, l1) = e0.forward_cls(tok, typ, mask, mix, True), e1.forward_cls(tok, typ, mask, mix, True)
    assert torch.equal(_bits(c0), _bits(c1)) and torch.equal(_bits(l0), _bits(l1))
    # the _prec entries with ASPIRE_MATMUL_FP32 ARE the plain entries (hplanes is not read)
    from aspire_amd import _lib, ops
    lib, w = _lib.lib, ctypes.byref(e0._w)
    tk, ty, mk = e0.device_inputs(tok, typ, mask)
    ws = torch.empty(lib.aspire_bert_cls_workspace_bytes_prec(w, b, l, _lib.MATMUL_FP32), dtype=torch.uint8, device='cuda')
    hp = torch.empty_like(h0)
    _lib.check(lib.aspire_bert_forward_prec_f32(w, None, None, _lib.MATMUL_FP32, ops._ptr(tk), ops._ptr(ty), ops._ptr(mk), b, l, ops._ptr(hp),
                                                ops._ptr(ws), ws.numel(), ops._stream()))
    assert torch.equal(_bits(hp), _bits(h0))
    cp, lp = torch.empty_like(c0), torch.empty_like(l0)
    mixc = (ctypes.c_float * 3)(*mix)
    _lib.check(lib.aspire_bert_forward_cls_prec_f32(w, None, _lib.MATMUL_FP32, ops._ptr(tk), ops._ptr(ty), ops._ptr(mk), b, l,
                                                    ctypes.cast(mixc, ctypes.c_void_p), ops._ptr(cp), ops._ptr(lp), ops._ptr(ws), ws.numel(),
                                                    ops._stream()))
    assert torch.equal(_bits(cp), _bits(c0)) and torch.equal(_bits(lp), _bits(l0))


# ---- the mode does something -------------------------------------------------------------------------------------------------------
def test_the_mode_changes_the_arithmetic_and_is_deterministic():
    from aspire_amd.encoder import HipBertEncoder
    n_layers, b, l, ffn = fr.CASES[2]                                           # 2 x (2, 130)
    m, tok, typ, mask, exact, _, _ = fr.case(n_layers, b, l, ffn)
    valid = mask.bool()
    h16 = _encoder(n_layers, b, l, ffn, 'fp16').forward_hidden(tok, typ, mask)
    h32 = _encoder(n_layers, b, l, ffn, None).forward_hidden(tok, typ, mask)
    d = (h16 - h32).abs().cpu()[valid].max().item()
    e32 = (h32.double().cpu() - exact.last_hidden_state).abs()[valid].max().item()
    print(f'|fp16 mode - default| {d:.3e}, the default against float64 {e32:.3e}: {d / e32:.0f} x')
    assert d > 10 * e32, (d, e32)
    other = HipBertEncoder(m, matmul='fp16')                                    # a second encoder of the mode: its own planes and workspace
    assert torch.equal(_bits(other.forward_hidden(tok, typ, mask)), _bits(h16))
    assert torch.equal(_bits(_encoder(n_layers, b, l, ffn, 'fp16').forward_hidden(tok, typ, mask)), _bits(h16))
    # ... and under a GEMM pin the mode steps aside: the default's bits under the same pin
    from aspire_amd._lib import pinned
    with pinned(GEMM='bf16x3', ATTN='f32'):
        a = _encoder(n_layers, b, l, ffn, 'fp16').forward_hidden(tok, typ, mask)
        c = _encoder(n_layers, b, l, ffn, None).forward_hidden(tok, typ, mask)
    assert torch.equal(_bits(a), _bits(c))


# ---- the fall-back -----------------------------------------------------------------------------------------------------------------
def test_an_activation_beyond_fp16_falls_back_through_the_pins():
    """tests/test_gpu_encoder_heavy.py's fall-back test in the mode: ONE FFN unit whose activation is 90 000 (> 65 504) is inf in FFN2's
    operand -- the bare forward is non-finite -- and AspireConSent.forward hands the batch to the full-range kernels (run_checked's pins
    override the mode): HuggingFace's sentence reps at that test's bar, max(1e-4, 1.5 x HuggingFace's own fp32 error against float64)."""
    from heavy_bert import heavy_tailed_bert
    from test_gpu_encoder import _batch
    from aspire_amd.consent import AspireConSent
    m = heavy_tailed_bert(2, seed=5, ffn_overflow=True)
    tok, seg, mask, lens = _batch(8, 128, 3000, seed=29)
    with torch.no_grad():
        w32 = m(tok, token_type_ids=seg, attention_mask=mask).last_hidden_state
        w64 = m.double()(tok, token_type_ids=seg, attention_mask=mask).last_hidden_state
        m.float()
    model = AspireConSent(bert_model=m, matmul='fp16')
    assert model.bert_encoder.matmul == 'fp16'
    assert not bool(torch.isfinite(model.bert_encoder.forward_hidden(tok, seg, mask)).all())
    spans = [[list(range(1, 1 + (n - 1) // 2)), list(range(1 + (n - 1) // 2, n))] for n in lens]
    with pytest.warns(UserWarning, match='non-finite'):
        _, sent = model.forward({'tokid_tt': tok, 'seg_tt': seg, 'attnmask_tt': mask, 'seq_lens': lens}, [2] * len(lens), spans)
    want32 = torch.stack([torch.stack([w32[i, s].mean(0) for s in sp]) for i, sp in enumerate(spans)])
    want64 = torch.stack([torch.stack([w64[i, s].mean(0) for s in sp]) for i, sp in enumerate(spans)])
    ref_err = (want32.double() - want64).abs().max().item()
    err = (sent.double().cpu() - want64).abs().max().item()
    print(f'fall-back: error {err:.3e}, bar {max(1e-4, 1.5 * ref_err):.3e}')
    assert err <= max(1e-4, 1.5 * ref_err), (err, ref_err)


# ---- refusals and plumbing ---------------------------------------------------------------------------------------------------------
def test_refusals():
    from aspire_amd.encoder import HipBertEncoder
    m = fr.bert(1, seed=2, intermediate_size=128)
    with pytest.raises(ValueError, match='matmul'):
        HipBertEncoder(m, matmul='bf16')
    with torch.no_grad():
        m.encoder.layer[0].output.dense.weight[3, 5] = 2000.0                   # |64 w| > 65504
    with pytest.warns(UserWarning, match="matmul='fp32'"):
        enc = HipBertEncoder(m, matmul='fp16')
    assert enc.matmul == 'fp32' and enc.matmul_asked == 'fp16' and enc._hplanes is None
    tok = torch.randint(0, fr.VOCAB, (2, 9), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = m(tok).last_hidden_state
    assert (enc.forward_hidden(tok).cpu() - want).abs().max().item() < 1e-3 * want.abs().max().item()     # it runs, as 'fp32'
    odd = fr.bert(1, seed=2, intermediate_size=192)                             # an ffn width the mode is not built for
    with pytest.warns(UserWarning, match="matmul='fp32'"):
        assert HipBertEncoder(odd, matmul='fp16').matmul == 'fp32'


class _Tok:
    """a tokenizer nobody calls: the model classes only keep it"""
    pad_token_id = 0


def test_every_model_class_carries_the_keyword():
    import aspire_amd
    from aspire_amd import baselines, bienc, consent, contextner, models, polyenc, sbert, sentenc
    m = fr.bert(1, seed=4, intermediate_size=128, pooler=True)
    tok = _Tok()
    built = {
        'AspireConSent': consent.AspireConSent(bert_model=m, matmul='fp16'),
        'AspireBiEnc': bienc.AspireBiEnc(bert_model=m, matmul='fp16'),
        'AspireSentEnc': sentenc.AspireSentEnc(bert_model=m, tokenizer=tok, matmul='fp16'),
        'BertMLM': baselines.BertMLM(bert_model=m, tokenizer=tok, matmul='fp16'),
        'BertNER': baselines.BertNER(bert_model=m, tokenizer=tok, matmul='fp16'),
        'SimCSE': baselines.SimCSE(bert_model=m, tokenizer=tok, matmul='fp16'),
        'SentenceModel': sbert.SentenceModel('sbtinybertsota', model=m, tokenizer=tok, matmul='fp16'),
        'AspireConSenContextual': contextner.AspireConSenContextual(bert_model=m, matmul='fp16'),
        'WordSentAlignPolyEnc': polyenc.WordSentAlignPolyEnc(bert_model=m, matmul='fp16'),
    }
    wrapped = {
        'AspireNER': contextner.AspireNER(bert_model=m, tokenizer=tok, matmul='fp16'),
        'AspireContextNER': contextner.AspireContextNER(bert_model=m, tokenizer=tok, matmul='fp16'),
        'AspireModel': models.AspireModel(bert_model=m, tokenizer=tok, matmul='fp16'),
    }
    for name in ('aspire_compsci', 'aspire_ner_compsci', 'aspire_context_ner_compsci'):
        wrapped['get_model ' + name] = aspire_amd.models.get_model(name, bert_model=m, tokenizer=tok, matmul='fp16')
    for name in ('specter', 'supsimcse', 'specter_ner', 'cospecter', 'cosentbert'):
        built['get_model ' + name] = aspire_amd.models.get_model(name, bert_model=m, tokenizer=tok, matmul='fp16')
    for name, model in list(built.items()) + [(k, v.model) for k, v in wrapped.items()]:
        assert model.bert_encoder.matmul == 'fp16' and model.bert_encoder._hplanes is not None, name
    # the default stays 'fp32', and a checkpoint loaded later keeps the model's mode
    assert consent.AspireConSent(bert_model=m).bert_encoder.matmul == 'fp32'
    assert aspire_amd.models.get_model('specter', bert_model=m, tokenizer=tok).bert_encoder.matmul == 'fp32'
    be = built['AspireBiEnc']
    be.load_state_dict({'bert_encoder.' + k: v for k, v in m.state_dict().items()})
    assert be.bert_encoder.matmul == 'fp16'
    se = built['AspireSentEnc']
    se.load_state_dict(m.state_dict())
    assert se.bert_encoder.matmul == 'fp16'
