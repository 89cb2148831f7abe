"""CPU side of the cosentbert / ictsentbert sentence encoder (aspire_amd/sentenc.py): the tokenisation route against a direct
BertTokenizer call with sentence-transformers' arguments, the encoder-call plan, the state-dict split, and the three new C entry
points refusing bad arguments before any launch (no device needed)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch


def _tokenizer(golden_dir, tmp_path):
    from transformers import BertTokenizer
    vocab = json.load(open(os.path.join(golden_dir, 'bienc_prep.json')))['vocab']
    p = tmp_path / 'vocab.txt'
    p.write_text('\n'.join(vocab) + '\n')
    return BertTokenizer(str(p), do_lower_case=True), [w for w in vocab if not w.startswith('[')]


def _sents(words):
    rng = np.random.default_rng(0)
    long = ' '.join(rng.choice(words, 600))
    return ['  ' + ' '.join(rng.choice(words, 7)) + '\t\n', long, 'x', ' '.join(rng.choice(words, 30)) + '   ',
            '\n' + ' '.join(rng.choice(words, 3))]


def test_prepare_sentence_batch_matches_tokenizer(golden_dir, tmp_path):
    from aspire_amd.batch_prep import pad_sentences, prepare_sentence_batch, tokenize_sentences
    tok, words = _tokenizer(golden_dir, tmp_path)
    sents = _sents(words)
    got = prepare_sentence_batch(sents, tok)
    want = tok([s.strip() for s in sents], padding=True, truncation='longest_first', max_length=512, return_tensors='pt')
    for k in ('input_ids', 'token_type_ids', 'attention_mask'):
        assert torch.equal(got[k], want[k]), k
    assert got['input_ids'].shape[1] == 512                                # the 600-piece sentence, cut to 512 with [SEP]
    assert got['input_ids'][1, -1].item() == tok.sep_token_id
    # whitespace-padded texts tokenise as their strip()
    assert got['input_ids'][0].tolist() == want['input_ids'][0].tolist()
    # the un-padded route + pad_sentences = the padded call on any subset
    ids, types = tokenize_sentences(sents, tok)
    for idx in ([0, 2, 4], [1], [3, 0], list(range(5))):
        t, s, m = pad_sentences(ids, types, idx, tok.pad_token_id)
        w = tok([sents[i].strip() for i in idx], padding=True, truncation='longest_first', max_length=512, return_tensors='pt')
        assert torch.equal(t, w['input_ids']) and torch.equal(s, w['token_type_ids']) and torch.equal(m, w['attention_mask'])


def test_sentence_buckets_plan():
    from aspire_amd.batch_prep import sentence_buckets
    rng = np.random.default_rng(1)
    for n, cap in ((1, 16384), (1000, 16384), (5000, 4096), (300, 512), (50, 100)):
        lens = rng.integers(3, 513, n)
        runs = sentence_buckets(lens, cap)
        flat = np.concatenate(runs)
        assert sorted(flat.tolist()) == list(range(n))                       # a permutation
        for r in runs:
            assert len(r) >= 1
            assert len(r) * lens[r].max() <= cap or len(r) == 1            # within max_tokens (a lone long sentence excepted)
        assert all(lens[a].max() <= lens[b].min() for a, b in zip(runs, runs[1:]))     # sorted by length
    assert sentence_buckets([], 16384) == []


def test_state_dict_split():
    from aspire_amd.sentenc import split_state_dict
    w = torch.zeros(2)
    plain = {'embeddings.word_embeddings.weight': w, 'encoder.layer.0.output.dense.bias': w, 'pooler.dense.weight': w}
    assert split_state_dict(plain) == plain
    wrapped = {'sent_encoder.' + k: v for k, v in plain.items()}
    assert split_state_dict(wrapped) == plain
    ict = dict(wrapped, **{'context_encoder.' + k: v for k, v in plain.items()})
    assert split_state_dict(ict) == plain                                   # the context tower is dropped
    with pytest.raises(KeyError):
        split_state_dict(dict(wrapped, criterion_w=w))
    with pytest.raises(KeyError):
        split_state_dict(dict(plain, bert_layer_weights=w))


def test_dotmax_entry_points_refuse_bad_arguments():
    from aspire_amd import _lib
    L = _lib.lib
    fake = 1 << 20                                                          # never dereferenced: every call fails its checks first
    q = _lib.RepSet(fake, fake, fake, 2, 0, 8)
    c = _lib.RepSet(fake, fake, fake, 3, 0, 8)
    big = _lib.RepSet(fake, fake, fake, 3, 0, 129)
    s = ctypes.c_void_p(fake)
    INV, UNS = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED
    B = ctypes.byref
    # aspire_dotmax_scores_f32
    assert L.aspire_dotmax_scores_f32(None, B(c), 768, _lib.PAIR_CROSS, _lib.SIM_COSINE, s, None) == INV
    assert L.aspire_dotmax_scores_f32(B(q), B(c), 768, _lib.PAIR_CROSS, _lib.SIM_COSINE, None, None) == INV
    assert L.aspire_dotmax_scores_f32(B(q), B(c), 512, _lib.PAIR_CROSS, _lib.SIM_COSINE, s, None) == UNS
    assert b'768' in L.aspire_last_error()
    assert L.aspire_dotmax_scores_f32(B(q), B(c), 768, _lib.PAIR_CROSS, 2, s, None) == INV
    assert L.aspire_dotmax_scores_f32(B(q), B(c), 768, _lib.PAIR_PAIRED, _lib.SIM_DOT, s, None) == INV    # 2 vs 3 documents
    assert L.aspire_dotmax_scores_f32(B(q), B(big), 768, _lib.PAIR_CROSS, _lib.SIM_COSINE, s, None) == UNS
    assert b'128' in L.aspire_last_error()
    nul = _lib.RepSet(0, fake, fake, 3, 0, 8)
    assert L.aspire_dotmax_scores_f32(B(q), B(nul), 768, _lib.PAIR_CROSS, _lib.SIM_COSINE, s, None) == INV
    # aspire_dotmax_rank_batch_f32 / _workspace_bytes
    C = 5000
    cc = _lib.RepSet(fake, fake, fake, C, 0, 8)
    assert L.aspire_dotmax_rank_batch_workspace_bytes(B(q), B(cc), C, 0) == 0
    need = L.aspire_dotmax_rank_batch_workspace_bytes(B(q), B(cc), C, 10)
    assert need > 0 and need == L.aspire_topk_workspace_bytes(2, C, 10)
    ts, ti = ctypes.c_void_p(fake), ctypes.c_void_p(fake)

    def rank(qs, cs, D=768, job_off=s, max_job=C, sim=_lib.SIM_COSINE, scores=s, k=10, ws=s, ws_bytes=need):
        return L.aspire_dotmax_rank_batch_f32(qs, cs, D, job_off, max_job, sim, scores, k, None, ts, ti, None, ws, ws_bytes, None)
    assert rank(None, B(cc)) == INV
    assert rank(B(q), B(cc), D=1024) == UNS
    assert rank(B(q), B(cc), sim=-1) == INV
    assert rank(B(q), B(_lib.RepSet(fake, fake, fake, C, 0, 200))) == UNS
    assert rank(B(q), B(cc), job_off=None) == INV
    assert rank(B(q), B(cc), scores=None) == INV
    assert rank(B(q), B(cc), ws_bytes=need - 8) == INV
    assert b'workspace too small' in L.aspire_last_error()
    assert rank(B(q), B(cc), ws=None) == INV
    assert rank(B(q), B(_lib.RepSet(fake, fake, fake, C, 4, 8))) == INV      # batched jobs take CSR rep sets
    assert L.aspire_dotmax_rank_batch_f32(B(q), B(cc), 768, s, C, 0, s, 5, None, None, None, None, s, need, None) == INV
