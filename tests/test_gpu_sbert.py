"""GPU parity of the SentenceTransformer baselines (aspire_amd/sbert.py) and of what they add to the encoder: the RoBERTa / MPNet
forward (aspire_bert_forward_var_f32: position ids, the relative-position bias in every attention form) against HuggingFace's fp32
CPU forward of seeded random-init models, the masked-mean kernel (aspire_token_mean_pool_f32) against float64, forward_mean and
SentenceModel against sentence-transformers' Pooling + Normalize restated on HF's output, and the cosine ranking route.

One shape serves the encoder tests, L = 200 with lengths [200, 137, 2, 129, 128, 9]: all six rows are 1200 token rows (the fp16-plane
forms), the first three 600 (f16x2); 200 keys cross the 128-key tile and the 128-query block, key - query runs through the bucket
function's exact range (< 8), its log range and its saturation (>= 128) in both signs, 128 and 129 sit on the tile edge, 2 is
'<s></s>' alone."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gpu_baselines import _papers, _tokenizer, _written_order
from test_gpu_encoder import _batch, _bert

pytestmark = pytest.mark.gpu
ENC_TOL = 1e-4           # the encoder suite's bar (include/aspire_hip.h A1; tests/test_gpu_baselines.py)
L = 200
LENS = [200, 137, 2, 129, 128, 9]
KINDS = ('mpnet', 'roberta')


@functools.lru_cache(maxsize=None)
def _model(kind):
    """2 layers, vocab 3000, 514 positions, random init with LayerNorms and biases perturbed (tests/test_gpu_encoder.py's _bert);
    MPNet's bias weights N(0, 1): at the init's 0.02 a wrong bucket would hide under the tolerance."""
    if kind == 'bert':
        return _bert(2, seed=5)
    from transformers import MPNetConfig, MPNetModel, RobertaConfig, RobertaModel
    torch.manual_seed({'mpnet': 11, 'roberta': 12}[kind])
    kw = dict(vocab_size=3000, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072,
              max_position_embeddings=514, layer_norm_eps=1e-5, pad_token_id=1)
    m = (MPNetModel(MPNetConfig(**kw), add_pooling_layer=False) if kind == 'mpnet'
         else RobertaModel(RobertaConfig(type_vocab_size=1, **kw), add_pooling_layer=False)).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'LayerNorm' in n or n.endswith('.bias'):
                p.add_(0.1 * torch.randn_like(p))
        if kind == 'mpnet':
            m.encoder.relative_attention_bias.weight.copy_(torch.randn(32, 12))
    return m


@functools.lru_cache(maxsize=None)
def _encoder(kind):
    from aspire_amd.encoder import HipBertEncoder
    return HipBertEncoder(_model(kind))


@functools.lru_cache(maxsize=None)
def _inputs(kind):
    """(ids, mask) [6, 200]: right-padded with the model's pad id (1; BertModel: 0)."""
    g = torch.Generator().manual_seed(21)
    pad = 0 if kind == 'bert' else 1
    mask = (torch.arange(L)[None, :] < torch.tensor(LENS)[:, None]).long()
    ids = torch.randint(5, 3000, (len(LENS), L), generator=g) * mask + pad * (1 - mask)
    return ids, mask


@functools.lru_cache(maxsize=None)
def _oracle(kind):
    """HF's fp32 CPU last_hidden_state [6, 200, 768] (a row does not depend on its batch mates: the 3-row shape is its first three)."""
    ids, mask = _inputs(kind)
    with torch.no_grad():
        return _model(kind)(ids, attention_mask=mask).last_hidden_state


def _err(got, want, mask):
    return float((got.cpu() - want).abs()[mask.bool()].max())


# ---- 1. the forward against HuggingFace, in every form that carries the extras -----------------------------------------------------
@pytest.mark.parametrize('form', ['default-1200', 'default-600', 'full-range', 'gemm'])
@pytest.mark.parametrize('kind', KINDS)
def test_forward_matches_transformers(kind, form):
    from aspire_amd._lib import pinned
    enc = _encoder(kind)
    assert enc.kind == kind and (enc._rel_bias is not None) == (kind == 'mpnet')
    ids, mask = _inputs(kind)
    want = _oracle(kind)
    n = 3 if form == 'default-600' else 6
    pins = {'full-range': dict(GEMM='bf16x3', ATTN='f32'), 'gemm': dict(ATTN='gemm')}.get(form, {})
    with pinned(**pins):
        got = enc.forward_hidden(ids[:n], None, mask[:n])
    assert got.shape == (n, L, 768) and got.dtype == torch.float32 and got.is_cuda
    e = _err(got, want[:n], mask[:n])
    print(f'{kind} {form}: max abs error over valid positions {e:.3e}')
    assert e < ENC_TOL, (kind, form, e)
    assert enc.status() == 0


# ---- 2. the oracle is sensitive to what the extras carry ---------------------------------------------------------------------------
def test_oracle_depends_on_bias_and_position_ids():
    """On HF alone: without the bias, or with BertModel's arange positions, the outputs move by far more than the tolerance -- so
    test 1 cannot pass with either left out."""
    ids, mask = _inputs('mpnet')
    valid = mask.bool()
    m = _model('mpnet')
    w = m.encoder.relative_attention_bias.weight
    keep = w.detach().clone()
    try:
        with torch.no_grad():
            w.zero_()
            no_bias = m(ids, attention_mask=mask).last_hidden_state
    finally:
        with torch.no_grad():
            w.copy_(keep)
    d_bias = float((no_bias - _oracle('mpnet')).abs()[valid].max())
    assert d_bias > 100 * ENC_TOL, d_bias
    arange = torch.arange(L)[None, :].expand(len(LENS), L)
    for kind in KINDS:
        with torch.no_grad():
            moved = _model(kind)(ids, attention_mask=mask, position_ids=arange).last_hidden_state
        d_pos = float((moved - _oracle(kind)).abs()[valid].max())
        print(f'{kind}: arange positions move the output by {d_pos:.2f}' + (f', no bias by {d_bias:.2f}' if kind == 'mpnet' else ''))
        assert d_pos > 100 * ENC_TOL, (kind, d_pos)


# ---- 3. no extras = aspire_bert_forward_f32 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('b,l', [(5, 37), (9, 128)])
def test_var_forward_without_extras_is_the_bert_forward(b, l):
    """5 x 37: the forms below 1024 token rows; 9 x 128 = 1152: the fp16-plane forms.  x NULL and x with both pointers NULL."""
    from aspire_amd import _lib, ops
    enc = _encoder('bert')
    tok, seg, mask, _ = _batch(b, l, 3000, seed=3 * b)
    tok, seg, mask = enc.device_inputs(tok, seg, mask)
    want = enc.forward_hidden(tok, seg, mask).clone()
    ws = enc._workspace(_lib.lib.aspire_bert_workspace_bytes(ctypes.byref(enc._w), b, l))
    for x in (None, _lib.BertExtras(None, None, 0)):
        got = torch.full_like(want, float('nan'))
        _lib.check(_lib.lib.aspire_bert_forward_var_f32(ctypes.byref(enc._w), ctypes.byref(x) if x is not None else None, ops._ptr(tok),
                                                        ops._ptr(seg), ops._ptr(mask), b, l, ops._ptr(got), ops._ptr(ws), ws.numel(),
                                                        ops._stream()))
        assert torch.equal(got, want)


# ---- 4. the masked-mean kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalize', [False, True])
@pytest.mark.parametrize('B', [1, 3, 65])
def test_token_mean_pool_against_float64(B, normalize):
    """The kernel's max error against float64 is at most max(4 e_ref, 1e-6), e_ref the error of torch's fp32 CPU Pooling
    (+ F.normalize) on the same inputs (tests/test_gpu_baselines.py's rule for the pooler: both are fp32 sums in some order).
    L = 37 is no multiple of the kernel's eight rows in flight; lengths are ragged, row 1 (B >= 3) has no valid token and gives
    zeros; the row behind the output is a sentinel."""
    from aspire_amd import _lib, ops
    g = torch.Generator().manual_seed(100 * B + normalize)
    l = 37
    hidden = torch.randn(B, l, 768, generator=g)
    lens = torch.randint(1, l + 1, (B,), generator=g)
    lens[0] = l
    if B >= 3:
        lens[1], lens[2] = 0, 1
    mask = (torch.arange(l)[None, :] < lens[:, None]).long()

    def pooled(h):
        m = mask[:, :, None].to(h.dtype)
        x = (h * m).sum(1) / torch.clamp(m.sum(1), min=1e-9)
        return torch.nn.functional.normalize(x, p=2, dim=1) if normalize else x

    want = pooled(hidden.double())
    e_ref = float((pooled(hidden).double() - want).abs().max())
    out = torch.full((B + 1, 768), -7.25, device='cuda')
    hd, md = hidden.cuda(), mask.cuda()
    _lib.check(_lib.lib.aspire_token_mean_pool_f32(ops._ptr(hd), ops._ptr(md), B, l, 768, int(normalize), ops._ptr(out), ops._stream()))
    out = out.cpu()
    assert bool((out[B] == -7.25).all()), 'the row behind the output was written'
    e_kernel = float((out[:B].double() - want).abs().max())
    print(f'token_mean_pool B={B} normalize={normalize}: kernel {e_kernel:.3e}  torch fp32 CPU {e_ref:.3e}')
    assert e_kernel <= max(4 * e_ref, 1e-6), (e_kernel, e_ref)
    if B >= 3:
        assert bool((out[1] == 0).all())
    # the host layer and the torch op are the same launch
    import aspire_amd.torch_ops  # noqa: F401
    assert torch.equal(ops.token_mean_pool(hd, md, normalize).cpu(), out[:B])
    assert torch.equal(torch.ops.aspire.token_mean_pool(hd, md, normalize).cpu(), out[:B])


# ---- 5. forward_mean ---------------------------------------------------------------------------------------------------------------
def _st_pool(hidden, mask, normalize):
    """sentence-transformers' Pooling (mean mode) and Normalize, restated."""
    m = mask[:, :, None].float()
    x = (hidden * m).sum(1) / torch.clamp(m.sum(1), min=1e-9)
    return torch.nn.functional.normalize(x, p=2, dim=1) if normalize else x


@pytest.mark.parametrize('kind', ('bert',) + KINDS)
def test_forward_mean_matches_pooling_on_transformers(kind):
    """All three model kinds (a 2-layer BertModel stands in for TinyBERT), with and without the normalisation."""
    enc = _encoder(kind)
    ids, mask = _inputs(kind)
    want = _oracle(kind)
    for normalize in (False, True):
        got = enc.forward_mean(ids, None, mask, normalize=normalize)
        assert got.shape == (len(LENS), 768) and got.is_cuda and got.dtype == torch.float32
        e = float((got.cpu() - _st_pool(want, mask, normalize)).abs().max())
        print(f'forward_mean {kind} normalize={normalize}: {e:.3e}')
        assert e < ENC_TOL, (kind, normalize, e)
    if kind != 'bert':
        with pytest.raises(NotImplementedError, match='forward_cls'):
            enc.forward_cls(ids, None, mask)


# ---- 6. SentenceModel end to end ---------------------------------------------------------------------------------------------------
def test_sentence_model_encode_and_rank(tmp_path):
    """encode against tokenizer -> HF -> Pooling -> Normalize restated per sentence batch; then the store through method='cosine'
    against float64 max cosine and Python's stable sorted."""
    from aspire_amd import SentenceModel
    tok, words = _tokenizer(tmp_path)
    m = _model('bert')
    model = SentenceModel('sbtinybertsota', model=m, tokenizer=tok, max_seq_length=24, normalize=True)
    assert model.name == 'sbtinybertsota' and model.max_seq_length == 24 and model.normalize is True
    assert SentenceModel('sbtinybertsota', model=m, tokenizer=tok).max_seq_length == 128
    # sentence counts 2, 1, 3, 0, 2, 4, 2; two sentences are beyond 24 tokens
    papers = _papers(words, [[8, 5], [3], [12, 40, 9], [], [6, 6], [5, 7, 30, 11], [9, 2]], seed=17)
    sents = [s for p in papers for s in p['ABSTRACT']]
    enc = [tok(s.strip(), truncation=True, max_length=24)['input_ids'] for s in sents]
    assert max(len(x) for x in enc) == 24 and sum(len(x) == 24 for x in enc) == 2
    width = max(len(x) for x in enc)
    ids = torch.tensor([x + [tok.pad_token_id] * (width - len(x)) for x in enc])
    mask = torch.tensor([[1] * len(x) + [0] * (width - len(x)) for x in enc])
    with torch.no_grad():
        want = _st_pool(m(ids, attention_mask=mask).last_hidden_state, mask, True).numpy()
    want = np.split(want, np.cumsum([len(p['ABSTRACT']) for p in papers])[:-1])
    got = model.encode(papers)
    assert [r.shape for r in got] == [(2, 768), (1, 768), (3, 768), (0, 768), (2, 768), (4, 768), (2, 768)]
    for r, w in zip(got, want):
        assert r.dtype == np.float32 and (r.size == 0 or float(np.abs(r - w).max()) < ENC_TOL)

    ranked = [p for p in papers if p['ABSTRACT']]
    pids = [f'p{i}' for i in range(len(ranked))]
    store = model.encode_to_store(ranked, pids)
    assert [store.get(p).shape[0] for p in pids] == [len(x['ABSTRACT']) for x in ranked]

    def unit(x):
        x = x.astype(np.float64)
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    sims = [float((unit(store.get(pids[0])) @ unit(store.get(c)).T).max()) for c in pids[1:]]
    order, by_pid = _written_order(tmp_path, store, pids, 'cosine')
    assert order == [pids[1:][i] for i in sorted(range(len(sims)), key=lambda i: sims[i], reverse=True)]
    for c, s in zip(pids[1:], sims):
        assert abs(by_pid[c] - s) < 4e-6, (c, by_pid[c], s)           # tests/test_gpu_sentenc.py's bar for the cosine kernel
        assert abs(model.get_similarity(store.get(pids[0]), store.get(c)) - s) < 1e-6


# ---- 7. the one form without the bias ----------------------------------------------------------------------------------------------
def test_bias_with_64_key_tiles_is_refused():
    """aspire_debug_set("ATTN", "p64") with a relative-position bias: ASPIRE_ERR_UNSUPPORTED before any launch (the header says so);
    RoBERTa, which has no bias, runs that form."""
    from aspire_amd._lib import pinned
    with pinned(ATTN='p64'):
        with pytest.raises(NotImplementedError, match='p64'):
            _encoder('mpnet').forward_hidden(_inputs('mpnet')[0], None, _inputs('mpnet')[1])
        ids, mask = _inputs('roberta')
        assert _err(_encoder('roberta').forward_hidden(ids, None, mask), _oracle('roberta'), mask) < ENC_TOL
