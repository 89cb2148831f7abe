"""CPU side of the SentenceTransformer baselines (aspire_amd/sbert.py, the RoBERTa / MPNet part of aspire_amd/encoder.py): the
per-distance bias table and the position ids against HuggingFace's own functions, the argument checks of
aspire_bert_forward_var_f32 and aspire_token_mean_pool_f32 (no device needed), SentenceModel around a stub encoder, the torch
op's registration and get_model's message."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch


# ---- 1. the bias table ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mpnet_encoder():
    """An MPNetEncoder for its compute_position_bias alone (tiny: the bias does not depend on the hidden size), the bias weights
    N(0, 1): at the init's 0.02 two buckets would be hard to tell apart."""
    from transformers import MPNetConfig
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    torch.manual_seed(3)
    enc = MPNetEncoder(MPNetConfig(vocab_size=50, hidden_size=24, num_hidden_layers=1, num_attention_heads=12, intermediate_size=32))
    with torch.no_grad():
        enc.relative_attention_bias.weight.copy_(torch.randn(32, 12))
    return enc.eval()


@pytest.mark.parametrize('L', [512, 5])
def test_bias_table_is_hfs_position_bias(L):
    """tab[h, (j - i) + 511] is MPNetEncoder.compute_position_bias bit for bit: bucket edges (the float32 logarithm) included.
    Checked here too: HF's bias is exactly Toeplitz, which is what lets one row per head stand for the [L, L] matrix."""
    from aspire_amd.encoder import REL_SPAN, relative_bias_table
    enc = _mpnet_encoder()
    tab = relative_bias_table(enc.relative_attention_bias.weight)
    assert REL_SPAN == 512 and tab.shape == (12, 1023) and tab.dtype == torch.float32 and tab.is_contiguous()
    with torch.no_grad():
        want = enc.compute_position_bias(torch.zeros(1, L, 24))[0]          # [12, L, L]: [h, query i, key j]
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    assert torch.equal(tab[:, (j - i) + 511], want)
    for d in range(-(L - 1), L):
        diag = torch.diagonal(want, offset=d, dim1=1, dim2=2)
        assert bool((diag == diag[:, :1]).all()), d
    if L == 512:      # every bucket but 16 (distance 0 on the key > query side: there is none) is in use: exact, log and saturated ranges
        assert len({float(x) for x in tab[0]}) == 31


# ---- 2. the position ids ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad', [1, 0])
def test_position_ids_are_hfs(pad):
    from transformers.models.mpnet.modeling_mpnet import create_position_ids_from_input_ids
    from aspire_amd.encoder import position_ids_from_input_ids
    g = torch.Generator().manual_seed(7)
    L = 11
    ids = torch.randint(2, 90, (4, L), generator=g)
    for row, n in enumerate([L, 2, 7, 1]):           # a row of real tokens only, <s></s> alone, ...
        ids[row, n:] = pad
    got = position_ids_from_input_ids(ids, pad)
    assert got.dtype == torch.int64 and torch.equal(got, create_position_ids_from_input_ids(ids, pad))
    assert got[0].tolist() == list(range(pad + 1, pad + 1 + L)) and got[1].tolist() == [pad + 1, pad + 2] + [pad] * (L - 2)


# ---- 3. argument checks -----------------------------------------------------------------------------------------------------------
def test_entry_point_argument_errors_without_a_device():
    from aspire_amd import _lib
    lib = _lib.lib
    assert 'aspire_bert_forward_var_f32' in _lib.SIGNATURES and 'aspire_token_mean_pool_f32' in _lib.SIGNATURES
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    ok, inv, uns = _lib.ASPIRE_OK, _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED

    def pool(hidden=p, mask=p, B=4, L=9, D=768, normalize=0, out=q):
        return lib.aspire_token_mean_pool_f32(hidden, mask, B, L, D, normalize, out, None)

    assert pool(D=512) == uns and b'768' in lib.aspire_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(pool(D=512))
    assert pool(B=-1) == inv and pool(L=0) == inv
    for null in ('hidden', 'mask', 'out'):
        assert pool(**{null: None}) == inv, null
    assert pool(B=0) == ok and pool(B=0, hidden=None, mask=None, out=None) == ok          # nothing to do, nothing launched
    assert pool(B=0, D=512) == uns                                                         # the geometry is checked first

    layers = (_lib.BertLayer * 1)()
    w = _lib.BertWeights(p, p, p, p, p, layers, 1, 12, 768, 3072, 3000, 514, 1, 1e-5, None)

    def fwd(w=w, x=None, tok=p, mask=p, B=2, L=16, out=q, ws=None, ws_bytes=0):
        return lib.aspire_bert_forward_var_f32(ctypes.byref(w) if w is not None else None, ctypes.byref(x) if x is not None else None,
                                               tok, None, mask, B, L, out, ws, ws_bytes, None)

    bias = _lib.BertExtras(p, p, 512)
    for x in (None, bias):
        for null in ('w', 'tok', 'mask', 'out'):
            assert fwd(x=x, **{null: None}) == inv, null
        assert fwd(x=x, L=513) == inv                                                      # beyond the forward's 512
        assert fwd(x=x, B=0) == ok
        assert fwd(x=x) == inv and b'workspace' in lib.aspire_last_error()                 # valid so far: the workspace is checked last
    short = _lib.BertWeights(p, p, p, p, p, layers, 1, 12, 768, 3072, 3000, 12, 1, 1e-5, None)
    assert fwd(w=short, x=bias, L=13) == inv and b'max_position_embeddings' in lib.aspire_last_error()      # L > max_pos
    assert fwd(x=_lib.BertExtras(p, p, 15)) == inv and b'rel_span' in lib.aspire_last_error()               # rel_span < L
    assert fwd(x=_lib.BertExtras(p, p, 15), B=0) == inv                                    # ... checked before the empty-batch return
    assert fwd(x=_lib.BertExtras(p, None, 0), B=0) == ok                                   # no bias: rel_span is not looked at
    assert fwd(x=_lib.BertExtras(p, p, 16), B=0) == ok
    wide = _lib.BertWeights(p, p, p, p, p, layers, 1, 16, 1024, 4096, 3000, 514, 1, 1e-5, None)
    assert fwd(w=wide, x=bias) == uns
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'aspire_hip.h')).read()
    for word in ('aspire_bert_extras', 'aspire_bert_forward_var_f32', 'aspire_token_mean_pool_f32', 'models.py:402', 'p64'):
        assert word in hdr, word


# ---- 4. SentenceModel around a stub encoder ---------------------------------------------------------------------------------------
class _StubTokenizer:
    """'<s> w1 w2 ... </s>': id 0 / 2 around one id per word (the word's number + 10), cut to max_length keeping the end token."""
    pad_token_id = 1

    def __call__(self, text, truncation=None, max_length=None):
        assert isinstance(text, str) and text == text.strip() and truncation is True
        ids = [0] + [int(w) + 10 for w in text.split()] + [2]
        if max_length is not None and len(ids) > max_length:
            ids = ids[:max_length - 1] + [2]
        return {'input_ids': ids}


class _StubEncoder:
    """forward_mean = (sum of the row's real ids, its token count, normalize, 0, ...): every sentence's rep names the sentence."""
    device = torch.device('cpu')

    def __init__(self):
        self.calls = []

    def device_inputs(self, tok, typ, msk, check_ids=True):
        return tok, typ, msk

    def checked(self, run, outputs_finite, who):
        out = run()
        assert outputs_finite(out) and who == 'SentenceModel'
        return out

    def forward_mean(self, tok, typ, msk, normalize=False, check_ids=True):
        assert tok.dtype == msk.dtype == torch.int64 and check_ids is False
        assert bool((tok[msk == 0] == _StubTokenizer.pad_token_id).all())              # padded with the tokenizer's pad id
        self.calls.append(tuple(tok.shape))
        out = torch.zeros(tok.shape[0], 768)
        out[:, 0] = (tok * msk).sum(1).float()
        out[:, 1] = msk.sum(1).float()
        out[:, 2] = float(normalize)
        return out


def _stub_model(max_seq_length=8, normalize=True):
    from aspire_amd import SentenceModel
    model = SentenceModel.__new__(SentenceModel)
    model.name, model.tokenizer, model.bert_encoder = 'sbmpnet1B', _StubTokenizer(), _StubEncoder()
    model.max_seq_length, model.normalize = max_seq_length, normalize
    return model


def test_sentence_model_encode_with_a_stub_encoder():
    from aspire_amd import SentenceModel
    import aspire_amd.sbert as sbert
    assert SentenceModel is sbert.SentenceModel and SentenceModel.encoding_type == 'sentence'
    assert SentenceModel.MODEL_PATHS == {'sbtinybertsota': 'paraphrase-TinyBERT-L6-v2', 'sbrobertanli': 'nli-roberta-base-v2',
                                         'sbmpnet1B': 'sentence-transformers/all-mpnet-base-v2'}
    assert SentenceModel.hub_name('sbrobertanli') == 'sentence-transformers/nli-roberta-base-v2'
    assert SentenceModel.hub_name('sbmpnet1B') == 'sentence-transformers/all-mpnet-base-v2'
    assert SentenceModel.DEFAULTS == {'sbtinybertsota': (128, False), 'sbrobertanli': (75, False), 'sbmpnet1B': (384, True)}
    assert 'recalled' in SentenceModel.__doc__.lower()

    model = _stub_model(max_seq_length=8)
    # sentences of 5, 1, 9 | - | 3 | 2, 12, 4 words, with blanks around some: lengths out of order, two beyond the cut
    words = [[5, 1, 9], [], [3], [2, 12, 4]]
    it = iter(range(1, 1000))
    papers = [{'TITLE': 't', 'ABSTRACT': [' ' + ' '.join(str(next(it)) for _ in range(n)) + '  ' for n in ns]} for ns in words]
    reps = model.encode(papers)
    assert [r.shape for r in reps] == [(3, 768), (0, 768), (1, 768), (3, 768)]
    assert all(isinstance(r, np.ndarray) and r.dtype == np.float32 for r in reps)
    for paper, rep in zip(papers, reps):                 # input order restored after the length sort, per paper
        for sent, row in zip(paper['ABSTRACT'], rep):
            ids = _StubTokenizer()(sent.strip(), truncation=True, max_length=8)['input_ids']
            assert len(ids) <= 8 and ids[0] == 0 and ids[-1] == 2
            assert row[0] == sum(ids) and row[1] == len(ids) and row[2] == 1.0
    assert max(r[:, 1].max() for r in reps if len(r)) == 8                # truncation at max_seq_length, specials included
    assert model.bert_encoder.calls == [(7, 8)]                           # one call for the lot, padded to the longest
    # several encoder calls give the same rows
    again = _stub_model(max_seq_length=8)
    sents = [s for p in papers for s in p['ABSTRACT']]
    few = again._encode_sentences(sents, max_tokens=16)
    assert len(again.bert_encoder.calls) > 1 and np.array_equal(few, np.concatenate(reps))
    assert [r.shape for r in model.encode([])] == [(0, 768)] and model.bert_encoder.calls == [(7, 8)]
    assert model.eval() is model

    facets = {'FACETS': ['objective_label', 'method_label', 'result_label']}
    assert np.array_equal(model.get_faceted_encoding(reps[0], 'background', facets), reps[0][[0]])
    assert model.get_faceted_encoding(reps[0], 'other', facets).shape == (0, 768)


def test_sentence_model_store_and_similarity():
    import sklearn.metrics.pairwise as skp
    from aspire_amd import SentenceModel
    model = _stub_model()
    papers = [{'ABSTRACT': ['1 2', '3']}, {'ABSTRACT': []}, {'ABSTRACT': ['4 5 6']}]
    store = model.encode_to_store(papers, ['a', 'b', 'c'])
    assert [store.get(p).shape for p in 'abc'] == [(2, 768), (0, 768), (1, 768)]
    with pytest.raises(ValueError, match='pids'):
        model.encode_to_store(papers, ['a'])
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((4, 768)).astype(np.float32), rng.standard_normal((7, 768)).astype(np.float32)
    y[3] = 0.0                                           # sklearn takes a zero row's norm as 1
    got = SentenceModel.get_similarity(x, y)
    assert isinstance(got, float) and abs(got - float(np.max(skp.cosine_similarity(x, y)))) < 1e-6
    assert abs(SentenceModel.get_similarity(x[:1], x[:1]) - 1.0) < 1e-6


def test_local_directory_settings(tmp_path):
    from aspire_amd import SentenceModel
    assert SentenceModel.read_local_settings(str(tmp_path)) == (None, None)
    (tmp_path / 'sentence_bert_config.json').write_text(json.dumps({'max_seq_length': 256, 'do_lower_case': False}))
    (tmp_path / 'modules.json').write_text(json.dumps([
        {'idx': 0, 'name': '0', 'path': '', 'type': 'sentence_transformers.models.Transformer'},
        {'idx': 1, 'name': '1', 'path': '1_Pooling', 'type': 'sentence_transformers.models.Pooling'}]))
    assert SentenceModel.read_local_settings(str(tmp_path)) == (256, False)
    (tmp_path / 'modules.json').write_text(json.dumps([
        {'idx': 1, 'name': '1', 'path': '1_Pooling', 'type': 'sentence_transformers.models.Pooling'},
        {'idx': 2, 'name': '2', 'path': '2_Normalize', 'type': 'sentence_transformers.models.Normalize'}]))
    assert SentenceModel.read_local_settings(str(tmp_path)) == (256, True)


def test_token_mean_pool_op_is_registered_with_a_fake():
    import aspire_amd.torch_ops as to
    assert 'token_mean_pool' in to.OPS and hasattr(torch.ops.aspire, 'token_mean_pool')
    hidden = torch.empty(5, 9, 768, device='meta', dtype=torch.float32)
    mask = torch.empty(5, 9, device='meta', dtype=torch.int64)
    out = torch.ops.aspire.token_mean_pool(hidden, mask, True)
    assert out.shape == (5, 768) and out.dtype == torch.float32
    assert torch.ops.aspire.token_mean_pool(hidden[:0], mask[:0], False).shape == (0, 768)
    with pytest.raises(NotImplementedError, match='CPU'):          # no CPU kernel behind it
        torch.ops.aspire.token_mean_pool(torch.zeros(2, 3, 768), torch.ones(2, 3, dtype=torch.int64), False)


# ---- 5. the factory ---------------------------------------------------------------------------------------------------------------
def test_get_model_points_to_sentence_model():
    from aspire_amd import models
    for name in ('sbtinybertsota', 'sbrobertanli', 'sbmpnet1B'):
        assert name not in models.MODEL_TABLE
        with pytest.raises(NotImplementedError, match=f'SentenceModel\\({name!r}') as e:
            models.get_model(name)
        assert 'aspire_amd.SentenceModel' in str(e.value)
