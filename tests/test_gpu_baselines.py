"""GPU parity of the SPECTER / SimCSE baselines (aspire_amd/baselines.py) and of the pooler kernel under them
(aspire_bert_pooler_f32): the kernel against float64, HipBertEncoder.forward_pooled against HuggingFace BertModel's two read-outs,
the three classes against a restatement with HF of src/evaluation/utils/models.py:300-317, :326-357, :368-376, the two ranking
routes against float64 + Python's stable sorted, and the torch op."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_encoder import _batch, _bert

pytestmark = pytest.mark.gpu
ENC_TOL = 1e-4           # the encoder suite's bar


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', [0.02, 0.2])
@pytest.mark.parametrize('B', [1, 3, 16, 17, 65])
def test_pooler_kernel_against_float64(B, s):
    """tanh(x W^T + b) against float64: the kernel's max error is at most max(4 e_ref, 1e-6), e_ref the error of torch's fp32 CPU
    tanh(x @ W.T + b) on the same inputs (both are fp32 sums of 768 terms in different orders: the 4 is the allowance for the
    order).  s = 0.02 is BERT's init (no output saturates); with s = 0.2 about half the outputs lie beyond +-0.999.  The output
    buffer has one more row, a sentinel, which must come back unchanged: a partial row tile stores nothing past row B - 1."""
    from aspire_amd import _lib, ops
    g = torch.Generator().manual_seed(1000 * B + int(100 * s))
    x = torch.randn(B, 768, generator=g)
    w = s * torch.randn(768, 768, generator=g)
    b = 0.1 * torch.randn(768, generator=g)
    want = torch.tanh(x.double() @ w.double().T + b.double())
    if s == 0.2:
        assert 0.35 < float((want.abs() > 0.999).double().mean()) < 0.65
    else:
        assert float(want.abs().max()) < 0.999
    e_ref = float((torch.tanh(x @ w.T + b).double() - want).abs().max())
    out = torch.full((B + 1, 768), -7.25, device='cuda')
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    _lib.check(_lib.lib.aspire_bert_pooler_f32(ops._ptr(xd), B, 768, ops._ptr(wd), ops._ptr(bd), ops._ptr(out), ops._stream()))
    out = out.cpu()
    assert bool((out[B] == -7.25).all()), 'the row behind the output was written'
    e_kernel = float((out[:B].double() - want).abs().max())
    print(f'pooler B={B} s={s}: kernel {e_kernel:.3e}  torch fp32 CPU {e_ref:.3e}  ratio {e_kernel / e_ref:.2f}')
    assert e_kernel <= max(4 * e_ref, 1e-6), (e_kernel, e_ref)
    # the host layer's call is the same launch
    assert torch.equal(ops.bert_pooler(xd, wd, bd).cpu(), out[:B])


# ---- 2. end to end against HuggingFace ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pooled_bert(n_layers, seed=0):
    """tests/test_gpu_encoder.py's _bert with the pooler: random init, LayerNorms and biases (the pooler's too) perturbed."""
    from transformers import BertConfig, BertModel
    torch.manual_seed(seed)
    cfg = BertConfig(vocab_size=3000, hidden_size=768, num_hidden_layers=n_layers, num_attention_heads=12, intermediate_size=3072,
                     max_position_embeddings=512)
    m = BertModel(cfg, add_pooling_layer=True).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'LayerNorm' in n or n.endswith('.bias'):
                p.add_(0.1 * torch.randn_like(p))
    return m


@pytest.mark.parametrize('n_layers', [2, 12])
def test_forward_pooled_matches_transformers(n_layers):
    from aspire_amd.encoder import HipBertEncoder
    m = _pooled_bert(n_layers)
    enc = HipBertEncoder(m)
    # 5 x 37 ragged: the forms below 1024 token rows; 9 x 128 = 1152 token rows: the fp16-plane forms
    for b, l in ((5, 37), (9, 128)):
        tok, seg, mask, _ = _batch(b, l, 3000, seed=10 * b + n_layers)
        with torch.no_grad():
            want = m(tok, token_type_ids=seg, attention_mask=mask)
        cls, pooled = enc.forward_pooled(tok, seg, mask)
        assert cls.shape == pooled.shape == (b, 768) and cls.is_cuda and pooled.dtype == torch.float32
        e_cls = float((cls.cpu() - want.last_hidden_state[:, 0]).abs().max())
        e_pool = float((pooled.cpu() - want.pooler_output).abs().max())
        print(f'forward_pooled layers={n_layers} {b}x{l}: cls {e_cls:.3e} pooled {e_pool:.3e}')
        assert e_cls < ENC_TOL and e_pool < ENC_TOL, (b, l, e_cls, e_pool)


def test_forward_pooled_needs_a_pooler():
    from aspire_amd.encoder import HipBertEncoder
    enc = HipBertEncoder(_bert(2))                      # add_pooling_layer=False
    tok, seg, mask, _ = _batch(2, 16, 3000, seed=1)
    with pytest.raises(ValueError, match='pooler'):
        enc.forward_pooled(tok, seg, mask)
    assert enc.forward_cls(tok, seg, mask)[0].shape == (2, 768)       # the model loads and runs as before


def test_simcse_falls_back_on_the_cls_rows():
    """tests/test_gpu_bienc.py's model whose fp16-plane path overflows, with a pooler: tanh would turn an overflowed activation
    into +-1, so the fall-back rule has to look at the CLS rows -- the 'non-finite' warning, then the pooler of the full-range
    kernels' CLS rows."""
    from transformers import BertModel
    from test_gpu_bienc import _outlier_bert
    from aspire_amd._lib import pinned
    from aspire_amd.baselines import SimCSE
    from aspire_amd.encoder import HipBertEncoder
    m0, tok, seg, mask = _outlier_bert()
    torch.manual_seed(21)
    m = BertModel(m0.config, add_pooling_layer=True).eval()
    m.load_state_dict(m0.state_dict(), strict=False)
    model = SimCSE.__new__(SimCSE)                       # (no tokenizer: the sentences arrive as ids)
    model.bert_encoder = enc = HipBertEncoder(m)
    assert not bool(torch.isfinite(enc.forward_pooled(tok, seg, mask)[0]).all())
    with pinned(GEMM='bf16x3', ATTN='f32'):
        want = enc.forward_pooled(tok, seg, mask)[1]
    assert bool(torch.isfinite(want).all())
    with pytest.warns(UserWarning, match='non-finite'):
        got = model._pooled_checked(tok, seg, mask)
    assert torch.equal(got, want)


# ---- 3. the three classes against the reference path restated with HF ----------------------------------------------------------
def _tokenizer(tmp_path):
    from transformers import BertTokenizer
    vocab = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'bienc_prep.json')))['vocab']
    p = tmp_path / 'vocab.txt'
    p.write_text('\n'.join(vocab) + '\n')
    return BertTokenizer(str(p), do_lower_case=True), [w for w in vocab if not w.startswith(('[', '#'))]


def _papers(words, sent_words, seed):
    """One paper per entry of sent_words (the word count of every sentence); entities on every other sentence."""
    rng = np.random.default_rng(seed)
    out = []
    for i, counts in enumerate(sent_words):
        sents = [' '.join(rng.choice(words, size=n)) + ' .' for n in counts]
        ents = [[' '.join(rng.choice(words, size=2)), str(rng.choice(words))] if j % 2 == 0 else [] for j in range(len(sents))]
        out.append({'TITLE': ' '.join(rng.choice(words, size=3 + i)), 'ABSTRACT': sents, 'ENTITIES': ents})
    return out


def _hf_prepare(tok, texts):
    """BertMLM._prepare_batch (models.py:259-293) restated: 500 word pieces, [CLS] ids [SEP], right-padded with the pad id."""
    ids = []
    for t in texts:
        x = tok.convert_tokens_to_ids(tok.tokenize(t)[:500])
        ids.append([tok.cls_token_id] + x + [tok.sep_token_id])
    L = max(len(x) for x in ids)
    pad = tok.pad_token_id
    tokid = torch.tensor([x + [pad] * (L - len(x)) for x in ids])
    seg = torch.tensor([[0] * len(x) + [pad] * (L - len(x)) for x in ids])
    att = torch.tensor([[1] * len(x) + [pad] * (L - len(x)) for x in ids])
    return tokid, seg, att


def _hf_run(m, tok, texts):
    tokid, seg, att = _hf_prepare(tok, texts)
    with torch.no_grad():
        return m(tokid, token_type_ids=seg, attention_mask=att)


def test_classes_match_the_reference_path(tmp_path):
    from aspire_amd.baselines import BertMLM, BertNER, SimCSE
    tok, words = _tokenizer(tmp_path)
    m = _pooled_bert(2, seed=7)
    # sentence counts 1, 3, 0, 6; the last paper is beyond 500 pieces as a whole, and one of its sentences on its own
    papers = _papers(words, [[9], [4, 12, 7], [], [30, 510, 2, 17, 60, 5]], seed=5)
    three = [papers[0], papers[1], papers[3]]
    texts = [p['TITLE'] + ' [SEP] ' + ' '.join(p['ABSTRACT']) for p in three]
    assert len(tok.tokenize(texts[2])) > 500

    specter = BertMLM(name='specter', bert_model=m, tokenizer=tok)
    assert specter.name == 'specter' and specter.encoding_type == 'abstract'
    got = specter.encode(three)
    assert isinstance(got, torch.Tensor) and got.shape == (3, 768) and got.dtype == torch.float32 and not got.is_cuda
    want = _hf_run(m, tok, texts).last_hidden_state[:, 0]
    assert float((got - want).abs().max()) < ENC_TOL
    assert specter.get_faceted_encoding(got, 'method', three[0]) is got

    ner = BertNER(name='specter_ner', bert_model=m, tokenizer=tok)
    assert ner.name == 'specter_ner' and ner.encoding_type == 'abstract'
    ner_texts = [t + ' ' + '. '.join(e for sent in p['ENTITIES'] for e in sent) + '.' for t, p in zip(texts, three)]
    got_ner = ner.encode(three)
    assert got_ner.shape == (3, 768) and got_ner.dtype == torch.float32
    want_ner = _hf_run(m, tok, ner_texts).last_hidden_state[:, 0]
    assert float((got_ner - want_ner).abs().max()) < ENC_TOL
    assert float((want_ner[:2] - want[:2]).abs().max()) > 1e-2          # the entities changed the text (not behind the cut)

    from aspire_amd import get_model
    for name in ('supsimcse', 'unsupsimcse'):
        simcse = get_model(name, bert_model=m, tokenizer=tok)
        assert type(simcse) is SimCSE and simcse.name == name
    sents = [s for p in papers for s in p['ABSTRACT']]
    want_pool = np.split(_hf_run(m, tok, sents).pooler_output.numpy(), np.cumsum([len(p['ABSTRACT']) for p in papers])[:-1])
    got_pool = simcse.encode(papers)
    assert [r.shape for r in got_pool] == [(1, 768), (3, 768), (0, 768), (6, 768)]
    assert all(isinstance(r, np.ndarray) and r.dtype == np.float32 for r in got_pool)
    for r, w in zip(got_pool, want_pool):
        assert r.shape == w.shape and (r.size == 0 or float(np.abs(r - w).max()) < ENC_TOL)
    # several encoder calls (the 502-row sentence alone) give the same reps: a sentence does not depend on its batch mates
    few = simcse._encode_sentences(sents, max_tokens=600)
    assert float(np.abs(few - np.concatenate(want_pool)).max()) < ENC_TOL


# ---- 4. the ranking routes --------------------------------------------------------------------------------------------------
def _written_order(tmp_path, store, pids, method):
    from aspire_amd import evaluate
    got = evaluate.score(str(tmp_path / method), {pids[0]: {'cands': pids[1:]}}, store, method=method)
    written = got[pids[0]]
    assert sorted(c for c, _ in written) == sorted(pids[1:])          # every candidate, once
    return [c for c, _ in written], {c: -s for c, s in written}


def test_ranking_routes(tmp_path):
    """One query against six candidates: BertMLM's store through method='l2max' ranks by -euclidean, SimCSE's through
    method='cosine' by the max cosine over the sentence pairs; the written order is Python's stable sorted(reverse=True) over
    float64 scores of the store's own rows."""
    from aspire_amd.baselines import BertMLM, SimCSE
    tok, words = _tokenizer(tmp_path)
    m = _pooled_bert(2, seed=7)
    papers = _papers(words, [[8, 5], [3], [12, 4, 9], [6, 6], [20], [5, 7, 3, 11], [9, 2]], seed=13)
    pids = [f'p{i}' for i in range(7)]

    store = BertMLM(bert_model=m, tokenizer=tok).encode_to_store(papers, pids, batch_size=4)
    assert all(store.get(p).shape == (1, 768) and store.get(p).dtype == np.float32 for p in pids)
    q = store.get(pids[0])[0].astype(np.float64)
    sims = [-float(np.linalg.norm(q - store.get(c)[0].astype(np.float64))) for c in pids[1:]]
    order, by_pid = _written_order(tmp_path, store, pids, 'l2max')
    assert order == [pids[1:][i] for i in sorted(range(6), key=lambda i: sims[i], reverse=True)]
    for c, s in zip(pids[1:], sims):
        assert abs(by_pid[c] - s) < 1e-4, (c, by_pid[c], s)           # smoke()'s bar for the l2max scores

    simcse = SimCSE(bert_model=m, tokenizer=tok)
    store = simcse.encode_to_store(papers, pids)
    assert [store.get(p).shape[0] for p in pids] == [len(x['ABSTRACT']) for x in papers]

    def unit(x):
        x = x.astype(np.float64)
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    sims = [float((unit(store.get(pids[0])) @ unit(store.get(c)).T).max()) for c in pids[1:]]
    order, by_pid = _written_order(tmp_path, store, pids, 'cosine')
    assert order == [pids[1:][i] for i in sorted(range(6), key=lambda i: sims[i], reverse=True)]
    for c, s in zip(pids[1:], sims):
        assert abs(by_pid[c] - s) < 4e-6, (c, by_pid[c], s)           # tests/test_gpu_sentenc.py's bar for the cosine kernel


# ---- 5. the torch op --------------------------------------------------------------------------------------------------------------
def test_bert_pooler_op_equals_ops():
    import aspire_amd.torch_ops  # noqa: F401
    from aspire_amd import ops
    g = torch.Generator().manual_seed(4)
    x, w, b = torch.randn(19, 768, generator=g).cuda(), (0.05 * torch.randn(768, 768, generator=g)).cuda(), torch.randn(768, generator=g).cuda()
    got = torch.ops.aspire.bert_pooler(x, w, b)
    assert torch.equal(got, ops.bert_pooler(x, w, b))
    torch.library.opcheck(torch.ops.aspire.bert_pooler, (x, w, b), test_utils=('test_schema', 'test_faketensor'))
