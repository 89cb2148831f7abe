"""CPU side of the SPECTER / SimCSE baselines (aspire_amd/baselines.py, aspire_amd/models.py): aspire_bert_pooler_f32's argument
checks (no device needed), the inputs bit for bit against the reference's own _prepare_batch / _pre_process_input_batch
(tests/golden/baselines_prep.json, tests/golden/make_golden_baselines.py), SimCSE.encode's split, get_similarity, get_model."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch


def _tokenizers(vocab, tmp_path):
    from transformers import BertTokenizer, BertTokenizerFast
    p = tmp_path / 'vocab.txt'
    p.write_text('\n'.join(vocab) + '\n')
    return BertTokenizer(str(p), do_lower_case=True), BertTokenizerFast(str(p), do_lower_case=True)


def test_pooler_argument_errors_without_a_device():
    from aspire_amd import _lib
    lib = _lib.lib
    assert 'aspire_bert_pooler_f32' in _lib.SIGNATURES
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)

    def call(cls=p, B=4, D=768, w=p, b=p, out=q):
        return lib.aspire_bert_pooler_f32(cls, B, D, w, b, out, None)

    inv = _lib.ASPIRE_ERR_INVALID_ARG
    assert call(D=512) == _lib.ASPIRE_ERR_UNSUPPORTED
    assert b'768' in lib.aspire_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(call(D=512))
    assert call(B=-1) == inv
    for null in ('cls', 'w', 'b', 'out'):
        assert call(**{null: None}) == inv, null
    assert call(out=p) == inv                                       # pooled == cls
    assert call(B=0) == _lib.ASPIRE_OK                              # nothing to do, nothing launched
    assert call(B=0, cls=None, w=None, b=None, out=None) == _lib.ASPIRE_OK
    assert call(B=0, D=512) == _lib.ASPIRE_ERR_UNSUPPORTED         # the geometry is checked first
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'aspire_hip.h')).read()
    assert 'aspire_bert_pooler_f32' in hdr and 'models.py:350' in hdr


def _same(bb, want):
    for k in ('tokid_tt', 'seg_tt', 'attnmask_tt'):
        assert bb[k].dtype == torch.int64
        assert bb[k].tolist() == want[k], k
    assert bb['seq_lens'] == want['seq_lens']


def test_baseline_inputs_match_reference(golden_dir, tmp_path):
    """prepare_eval_seqs = BertMLM's input, prepare_eval_ner_seqs = BertNER's (entities in some sentences, none at all, the 500-piece
    cap), and the sentences of a SimCSE batch through the tokenisation SimCSE._encode_sentences uses; slow and fast tokenizers."""
    from aspire_amd.batch_prep import (MAX_NUM_TOKS, _with_special_tokens, _word_pieces, pad_sentences, prepare_eval_ner_seqs,
                                       prepare_eval_seqs)
    z = json.load(open(os.path.join(golden_dir, 'baselines_prep.json')))
    papers = z['papers']
    assert any(n == 502 for c in z['cases'] for n in c['specter']['seq_lens'])
    assert any(p['ENTITIES'] == [] for p in papers) and any(p['ENTITIES'] and not any(p['ENTITIES']) for p in papers)
    assert any(any(p['ENTITIES']) and not all(p['ENTITIES']) for p in papers)
    for tok in _tokenizers(z['vocab'], tmp_path):
        for case in z['cases']:
            batch = [papers[i] for i in case['doc_ids']]
            _same(prepare_eval_seqs(batch, tok), case['specter'])
            _same(prepare_eval_ner_seqs(batch, tok), case['specter_ner'])
        # a paper without entities: the text still ends in ' .'
        assert all(t.endswith(' .') for c in z['cases'] for i, t in zip(c['doc_ids'], c['specter_ner']['texts'])
                   if not any(papers[i]['ENTITIES']))
        s = z['simcse']
        sents = [x for i in s['doc_ids'] for x in papers[i]['ABSTRACT']]
        ids = [_with_special_tokens(tok, piece_ids[:MAX_NUM_TOKS]) for _, piece_ids in _word_pieces(tok, sents, want_text=False)]
        tokid, seg, att = pad_sentences(ids, [[0] * len(x) for x in ids], range(len(ids)), tok.pad_token_id)
        assert tokid.tolist() == s['tokid_tt'] and seg.tolist() == s['seg_tt'] and att.tolist() == s['attnmask_tt']
        assert [len(papers[i]['ABSTRACT']) for i in s['doc_ids']] == s['split_sizes']


def test_simcse_encode_splits_like_np_split():
    """SimCSE.encode with the encoder call replaced: sentence counts 2, 0, 1, 4 come back as [2, 768], [0, 768], [1, 768], [4, 768]
    float32 blocks of the sentences' rows in order; no sentence at all: no encoder call."""
    from aspire_amd.baselines import SimCSE
    model = SimCSE.__new__(SimCSE)
    calls = []

    def fake(sents):
        calls.append(list(sents))
        return np.stack([np.full(768, float(s), np.float32) for s in sents]) if sents else np.zeros((0, 768), np.float32)

    model._encode_sentences = fake
    counts = [2, 0, 1, 4]
    it = iter(range(100))
    papers = [{'TITLE': 't', 'ABSTRACT': [str(next(it)) for _ in range(n)]} for n in counts]
    reps = model.encode(papers)
    assert calls == [[str(i) for i in range(7)]]
    assert [r.shape for r in reps] == [(n, 768) for n in counts]
    assert all(r.dtype == np.float32 for r in reps)
    assert [r[:, 0].tolist() for r in reps] == [[0.0, 1.0], [], [2.0], [3.0, 4.0, 5.0, 6.0]]
    empty = model.encode([{'TITLE': 't', 'ABSTRACT': []}, {'TITLE': 'u', 'ABSTRACT': []}])
    assert [r.shape for r in empty] == [(0, 768), (0, 768)] and len(calls) == 1


def test_get_similarity_is_minus_euclidean():
    from scipy.spatial.distance import euclidean
    from aspire_amd.baselines import BertMLM, BertNER, SimCSE
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal((2, 768)).astype(np.float32)
    for cls in (BertMLM, BertNER):
        got = cls.get_similarity(x, y)
        assert isinstance(got, float) and got == pytest.approx(-euclidean(x, y), rel=1e-6)
        assert cls.get_similarity(torch.from_numpy(x), torch.from_numpy(y)) == got
        assert cls.get_similarity(x, x) == 0.0
    # SimCSE: two one-row reps give the distance; anything else is scipy's ValueError on 2-D input
    assert SimCSE.get_similarity(x[None], y[None]) == pytest.approx(-euclidean(x, y), rel=1e-6)
    two = rng.standard_normal((2, 768)).astype(np.float32)
    with pytest.raises(ValueError):
        euclidean(two, two)
    for a, b in ((two, two), (two, y[None]), (x[None], two), (np.zeros((0, 768), np.float32), y[None])):
        with pytest.raises(ValueError):
            SimCSE.get_similarity(a, b)
    assert BertMLM.get_faceted_encoding(x, 'background', {'FACETS': []}) is x


REFERENCE_NAMES = {      # src/evaluation/utils/models.py:745-768, the SentenceTransformer names apart
    'aspire_compsci': 'AspireModel', 'aspire_biomed': 'AspireModel', 'specter': 'BertMLM', 'supsimcse': 'SimCSE', 'unsupsimcse': 'SimCSE',
    'specter_ner': 'BertNER', 'aspire_ner_compsci': 'AspireNER', 'aspire_ner_biomed': 'AspireNER',
    'aspire_context_ner_compsci': 'AspireContextNER', 'aspire_context_ner_biomed': 'AspireContextNER', 'cospecter': 'AspireBiEnc',
    'cosentbert': 'AspireSentEnc', 'ictsentbert': 'AspireSentEnc'}


def test_get_model_table_and_errors():
    import aspire_amd
    from aspire_amd import baselines, bienc, contextner, models, sentenc
    assert {k: v.__name__ for k, v in models.MODEL_TABLE.items()} == REFERENCE_NAMES
    assert models.MODEL_TABLE['specter'] is baselines.BertMLM is aspire_amd.BertMLM
    assert models.MODEL_TABLE['specter_ner'] is baselines.BertNER is aspire_amd.BertNER
    assert models.MODEL_TABLE['supsimcse'] is baselines.SimCSE is aspire_amd.SimCSE
    assert models.MODEL_TABLE['cospecter'] is bienc.AspireBiEnc and models.MODEL_TABLE['cosentbert'] is sentenc.AspireSentEnc
    assert models.MODEL_TABLE['aspire_ner_biomed'] is contextner.AspireNER
    assert models.MODEL_TABLE['aspire_context_ner_biomed'] is contextner.AspireContextNER
    assert issubclass(models.MODEL_TABLE['aspire_compsci'], object) and models.AspireModel.encoding_type == 'sentence'
    assert aspire_amd.get_model is models.get_model
    assert baselines.BertMLM.MODEL_PATHS == {'specter': 'allenai/specter', 'supsimcse': 'princeton-nlp/sup-simcse-bert-base-uncased',
                                             'unsupsimcse': 'princeton-nlp/unsup-simcse-bert-base-uncased'}
    assert baselines.BertMLM.encoding_type == baselines.SimCSE.encoding_type == 'abstract'
    for name in ('sbtinybertsota', 'sbrobertanli', 'sbmpnet1B'):
        with pytest.raises(NotImplementedError, match='SentenceTransformer baselines .*RoBERTa / MPNet.* not built'):
            models.get_model(name)
    with pytest.raises(NotImplementedError) as e:
        models.get_model('bert_nli')
    assert str(e.value) == 'No Implementation for model bert_nli'


def test_bert_pooler_op_is_registered_with_a_fake():
    import aspire_amd.torch_ops as to
    assert 'bert_pooler' in to.OPS and hasattr(torch.ops.aspire, 'bert_pooler')
    m = lambda *s: torch.empty(*s, device='meta', dtype=torch.float32)
    out = torch.ops.aspire.bert_pooler(m(5, 768), m(768, 768), m(768))
    assert out.shape == (5, 768) and out.dtype == torch.float32
    assert torch.ops.aspire.bert_pooler(m(0, 768), m(768, 768), m(768)).shape == (0, 768)
    with pytest.raises(NotImplementedError, match='CPU'):          # no CPU kernel behind it
        torch.ops.aspire.bert_pooler(torch.zeros(2, 768), torch.zeros(768, 768), torch.zeros(768))
