"""CPU side of the SPECTER-CoCite bi-encoder (aspire_amd/bienc.py): the batch preparation bit for bit against the reference's own
batchers (tests/golden/bienc_prep.json, tests/golden/make_golden_bienc.py), the state-dict key split, and the C ABI's new entry
points -- present, and refusing bad arguments before any launch (no device needed)."""
import ctypes
import json
import os

import pytest
import torch


def _tokenizers(vocab, tmp_path):
    from transformers import BertTokenizer, BertTokenizerFast
    p = tmp_path / 'vocab.txt'
    p.write_text('\n'.join(vocab) + '\n')
    return BertTokenizer(str(p), do_lower_case=True), BertTokenizerFast(str(p), do_lower_case=True)


def _same(bb, want):
    for k in ('tokid_tt', 'seg_tt', 'attnmask_tt'):
        assert bb[k].dtype == torch.int64
        assert bb[k].tolist() == want[k], k
    assert bb['seq_lens'] == want['seq_lens']


def test_bienc_prep_matches_reference(golden_dir, tmp_path):
    """prepare_abstract_seqs = AbsTripleBatcher.prepare_abstracts (literal [SEP] removed, ' [SEP] ' joins), prepare_eval_seqs = the
    evaluate route, prepare_bert_seqs = SentTripleBatcher.prepare_bert_sentences (500-piece cap, pad id in all three tensors); slow and
    fast tokenizers alike."""
    from aspire_amd.batch_prep import prepare_abstract_seqs, prepare_bert_seqs, prepare_eval_seqs
    z = json.load(open(os.path.join(golden_dir, 'bienc_prep.json')))
    assert any(n > 500 for c in z['cases'] for n in c['abs']['seq_lens']) or any(n == 502 for c in z['cases'] for n in c['abs']['seq_lens'])
    assert any('[SEP]' in s for d in z['docs'] for s in [d['TITLE']] + d['ABSTRACT'])
    for tok in _tokenizers(z['vocab'], tmp_path):
        for case in z['cases']:
            batch = [z['docs'][i] for i in case['doc_ids']]
            _same(prepare_abstract_seqs(batch, tok), case['abs'])
            _same(prepare_eval_seqs(batch, tok), case['eval'])
            bb, text, ids = prepare_bert_seqs(case['seqs'], tok)
            _same(bb, case['sents'])
            assert ids == case['sents']['tokid_tt']
            if not getattr(tok, 'is_fast', False):
                assert text == case['seqs_text']
    # the cap: the 520-word sequence comes out as [CLS] + 500 pieces + [SEP]
    assert max(max(c['sents']['seq_lens']) for c in z['cases']) == 502


def test_state_dict_key_split():
    from aspire_amd.bienc import split_state_dict
    w = torch.randn(1, 13)
    sd = {'bert_encoder.embeddings.word_embeddings.weight': torch.zeros(3, 768), 'bert_encoder.pooler.dense.bias': torch.zeros(768),
          'bert_encoder.encoder.layer.0.output.dense.weight': torch.zeros(768, 3072), 'bert_layer_weights.weight': w}
    enc, mix = split_state_dict(sd)
    assert sorted(enc) == ['embeddings.word_embeddings.weight', 'encoder.layer.0.output.dense.weight', 'pooler.dense.bias']
    assert mix is w
    enc, mix = split_state_dict({k: v for k, v in sd.items() if k != 'bert_layer_weights.weight'})
    assert mix is None and len(enc) == 3
    with pytest.raises(KeyError, match='criterion'):
        split_state_dict(dict(sd, **{'criterion.weight': torch.zeros(1)}))
    with pytest.raises(ValueError):
        split_state_dict(dict(sd, **{'bert_layer_weights.weight': torch.zeros(13)}))


def test_new_exports_are_present():
    from aspire_amd import _lib
    for name in ('aspire_bert_cls_workspace_bytes', 'aspire_bert_forward_cls_f32'):
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name) is not None
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'aspire_hip.h')).read()
    assert 'aspire_bert_forward_cls_f32' in hdr and 'ex_aspire_bienc.py' in hdr
    import aspire_amd.torch_ops as to
    assert 'bert_cls_forward' in to.OPS
    m = lambda *s, dt=torch.float32: torch.empty(*s, device='meta', dtype=dt)
    w = [m(100, 768), m(512, 768), m(2, 768), m(768), m(768)]
    i64 = torch.int64
    assert torch.ops.aspire.bert_cls_forward(m(3, 9, dt=i64), m(3, 9, dt=i64), m(3, 9, dt=i64), w, 12, 1e-12, [1.0]).shape == (3, 768)


def _weights(n_layers=2):
    from aspire_amd._lib import BertLayer, BertWeights
    layers = (BertLayer * n_layers)()
    for ly in layers:
        for f, _ in BertLayer._fields_:
            setattr(ly, f, ctypes.c_void_p(4096))
    w = BertWeights(*(ctypes.c_void_p(4096) for _ in range(5)), layers, n_layers, 12, 768, 3072, 3000, 512, 2, 1e-12, None)
    return w, layers


def test_cls_forward_argument_errors_without_a_device():
    from aspire_amd import _lib
    lib = _lib.lib
    w, _keep = _weights()
    p = ctypes.c_void_p(4096)
    B, L = 4, 64
    need = lib.aspire_bert_cls_workspace_bytes(ctypes.byref(w), B, L)
    assert need > lib.aspire_bert_workspace_bytes(ctypes.byref(w), B, L) > 0
    assert lib.aspire_bert_cls_workspace_bytes(ctypes.byref(w), 0, L) == 0
    mix = (ctypes.c_float * 3)(0.2, 0.3, 0.5)
    bad_mix = (ctypes.c_float * 3)(0.2, float('nan'), 0.5)

    def call(tok=p, mask=p, B=B, L=L, mix=mix, out=p, ws=p, nbytes=need, weights=w):
        return lib.aspire_bert_forward_cls_f32(ctypes.byref(weights) if weights is not None else None, tok, None, mask, B, L,
                                               ctypes.cast(mix, ctypes.c_void_p) if mix is not None else None, out, None, ws, nbytes, None)

    inv = _lib.ASPIRE_ERR_INVALID_ARG
    assert call(L=513) == inv                                       # beyond 512
    assert b'513' in lib.aspire_last_error()
    w.max_pos = 128
    assert call(L=129) == inv                                       # beyond max_position_embeddings
    w.max_pos = 512
    assert call(L=0) == inv
    assert call(tok=None) == inv
    assert call(mask=None) == inv
    assert call(out=None) == inv
    assert call(weights=None) == inv
    assert call(ws=None) == inv
    assert call(nbytes=need - 1) == inv                             # short workspace
    assert b'workspace' in lib.aspire_last_error()
    assert call(nbytes=lib.aspire_bert_workspace_bytes(ctypes.byref(w), B, L)) == inv     # the full forward's size is not enough
    assert call(mix=bad_mix) == inv
    assert call(B=0) == _lib.ASPIRE_OK                              # nothing to do, nothing launched
    w.n_heads = 16
    assert call() == _lib.ASPIRE_ERR_UNSUPPORTED
