"""GPU parity of the cosentbert / ictsentbert sentence encoder (aspire_amd/sentenc.py) and of the dot-product max-sim kernels
(aspire_dotmax_scores_f32, aspire_dotmax_rank_batch_f32).  The reference arithmetic is restated with HuggingFace BertModel
(last_hidden_state[:, 0], batch by batch as SentenceTransformer.encode runs it), sklearn's cosine_similarity + np.max
(TrainedSentModel.get_similarity, models.py:602-604), float64 numpy and Python's stable sorted (rank_pool_sent, evaluate.py:76)."""
import json
import os

import numpy as np
import pytest
import torch
from sklearn.metrics.pairwise import cosine_similarity

from test_gpu_encoder import _bert

pytestmark = pytest.mark.gpu
ENC_TOL = 1e-4           # the encoder suite's bar
SK_TOL = 4e-6            # against sklearn's float32 path
F64_TOL = 3e-6           # against float64
EPS10 = np.float32(10) * np.finfo(np.float32).eps


def _tokenizer(tmp_path):
    from transformers import BertTokenizer
    vocab = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'bienc_prep.json')))['vocab']
    p = tmp_path / 'vocab.txt'
    p.write_text('\n'.join(vocab) + '\n')
    return BertTokenizer(str(p), do_lower_case=True), [w for w in vocab if not w.startswith('[')]


def _sentences(words, n_words, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(n_words):
        s = ' '.join(rng.choice(words, size=n))
        out.append(('   ' + s + ' \n') if i % 5 == 0 else s)       # whitespace that .strip() removes
    return out


def _st_encode(m, tok, sents, batch_size=32):
    """SentenceTransformer.encode as recalled: texts sorted by length (longest first), batches of 32, each tokenised with
    padding=True, truncation='longest_first', max_length=512, the CLS row of last_hidden_state, back in input order."""
    order = np.argsort([-len(s) for s in sents], kind='stable')
    out = np.zeros((len(sents), 768), np.float32)
    for lo in range(0, len(sents), batch_size):
        idx = order[lo:lo + batch_size]
        bb = tok([sents[i].strip() for i in idx], padding=True, truncation='longest_first', max_length=512, return_tensors='pt')
        with torch.no_grad():
            h = m(bb['input_ids'], token_type_ids=bb['token_type_ids'], attention_mask=bb['attention_mask']).last_hidden_state
        out[idx] = h[:, 0].numpy()
    return out


@pytest.mark.parametrize('n_layers', [2, 12])
def test_encode_matches_sentence_transformers(n_layers, tmp_path):
    from aspire_amd.sentenc import AspireSentEnc
    tok, words = _tokenizer(tmp_path)
    # word counts -> padded L = words + 2: 7, 33, 61 (odd), 1 word, 509 and 600 (truncated to 512), a spread in between
    n_words = [5, 31, 59, 1, 509, 600, 5, 31, 59, 12, 100, 3, 250, 40, 8, 77, 31, 2, 160, 45] * (2 if n_layers == 2 else 1)
    sents = _sentences(words, n_words, seed=n_layers)
    m = _bert(n_layers, seed=40 + n_layers)
    model = AspireSentEnc(bert_model=m, tokenizer=tok)
    got = model.encode(sents, max_tokens=2048)                 # several buckets: the 512-row ones alone, short ones together
    assert got.shape == (len(sents), 768) and got.dtype == np.float32
    want = _st_encode(m, tok, sents)
    err = np.abs(got - want).max(axis=1)
    assert err.max() < ENC_TOL, (err.max(), int(err.argmax()))
    one = model.encode(sents[4])
    assert one.shape == (768,) and np.abs(one - want[4]).max() < ENC_TOL
    # SentBERTWrapper.sent_reps_bert on an HF dict
    bb = tok([s.strip() for s in sents[:3]], padding=True, return_tensors='pt')
    r = AspireSentEnc.sent_reps_bert(bb, model).cpu().numpy()
    assert r.shape == (3, 768) and np.abs(r - want[:3]).max() < ENC_TOL


def test_forward_device_falls_back_on_an_activation_beyond_fp16():
    """forward_device on tests/test_gpu_bienc.py's model whose fp16-plane path overflows: the 'non-finite' warning, then the
    full-range kernels' CLS rows, which match HF."""
    from test_gpu_bienc import _outlier_bert
    from aspire_amd.sentenc import AspireSentEnc
    m, tok, seg, mask = _outlier_bert()
    with torch.no_grad():
        want = m(tok, token_type_ids=seg, attention_mask=mask).last_hidden_state
    model = AspireSentEnc(bert_model=m)
    with pytest.warns(UserWarning, match='non-finite'):
        got = model.forward_device(tok, seg, mask).cpu()
    assert torch.isfinite(got).all()
    np.testing.assert_allclose(got.numpy(), want[:, 0].numpy(), atol=2e-5 * float(want.abs().max()), rtol=0)


def _rows(rng, n, kind):
    if kind == 'normal':
        return rng.standard_normal((n, 768)).astype(np.float32)
    return (3.0 * _COMMON + rng.standard_normal((n, 768))).astype(np.float32)      # mean cosine ~0.9


_COMMON = np.random.default_rng(99).standard_normal(768)


def _f64_cos_max(x, y, dot=False):
    x, y = x.astype(np.float64), y.astype(np.float64)
    if not dot:
        nx = np.sqrt((x.astype(np.float32) ** 2).sum(1, dtype=np.float32)).astype(np.float64)
        ny = np.sqrt((y.astype(np.float32) ** 2).sum(1, dtype=np.float32)).astype(np.float64)
        nx[nx < EPS10] = 1.0
        ny[ny < EPS10] = 1.0
        x, y = x / nx[:, None], y / ny[:, None]
    return float((x @ y.T).max())


def _check_pair(got, x, y):
    want_sk = float(np.max(cosine_similarity(x, y)))
    want_64 = _f64_cos_max(x, y)
    assert abs(got - want_sk) <= SK_TOL, (got, want_sk)
    assert abs(got - want_64) <= F64_TOL, (got, want_64)


@pytest.mark.parametrize('kind', ['normal', 'aniso'])
@pytest.mark.parametrize('layout', ['csr', 'padded'])
def test_cosine_scores_match_sklearn(kind, layout):
    from aspire_amd import _lib, ops
    rng = np.random.default_rng(7 if kind == 'normal' else 8)
    for max_rows in (8, 16, 40, 128):        # <= 16: the cross kernel; longer documents: one wave per pair
        q_docs = [_rows(rng, int(n), kind) for n in rng.integers(1, max_rows + 1, 5)]
        c_docs = [_rows(rng, int(n), kind) for n in rng.integers(1, max_rows + 1, 37)]
        q_docs[0] = _rows(rng, max_rows, kind)
        c_docs[3] = _rows(rng, max_rows, kind)

        def repset(docs):
            if layout == 'csr':
                return ops.DeviceRepSet.from_list(docs)
            s = max(len(d) for d in docs)
            pad = np.zeros((len(docs), s, 768), np.float32)
            for i, d in enumerate(docs):
                pad[i, :len(d)] = d
                pad[i, len(d):] = 1e3                          # padding rows must not be read
            return ops.DeviceRepSet.from_padded(torch.from_numpy(pad), [len(d) for d in docs])
        q, c = repset(q_docs), repset(c_docs)
        cross = ops.dotmax_scores(q, c, pairing=_lib.PAIR_CROSS).cpu().numpy().reshape(len(q_docs), len(c_docs))
        for qi, x in enumerate(q_docs):
            for ci, y in enumerate(c_docs):
                _check_pair(float(cross[qi, ci]), x, y)
        # PAIRED: the same pairs one wave each -- the same bits as the cross form
        pq = repset([q_docs[i % len(q_docs)] for i in range(len(c_docs))])
        paired = ops.dotmax_scores(pq, c, pairing=_lib.PAIR_PAIRED).cpu().numpy()
        np.testing.assert_array_equal(paired, cross[np.arange(len(c_docs)) % len(q_docs), np.arange(len(c_docs))])


def test_cosine_edge_rows():
    """sklearn's float32 edges: zero rows and rows below 10 eps keep their raw dot (norm -> 1), rows whose sum of squares
    overflows divide to zeros and score 0 against everything -- also when the raw dot overflows too.  Never NaN."""
    from aspire_amd import _lib, ops
    rng = np.random.default_rng(3)
    zero = np.zeros((1, 768), np.float32)
    tiny = (rng.standard_normal((2, 768)) * 1e-25).astype(np.float32)       # sum of squares underflows to 0
    small = (rng.standard_normal((1, 768)) * 2e-8).astype(np.float32)       # norm ~5e-7 < 10 eps: raw dot
    huge = np.full((1, 768), 1e20, np.float32)                             # sum of squares -> inf
    huge2 = np.full((2, 768), -3e19, np.float32)
    normal = rng.standard_normal((3, 768)).astype(np.float32)
    docs = [zero, tiny, small, huge, huge2, normal, np.vstack([huge, zero]), np.vstack([huge, -normal[:1]]), np.vstack([small, tiny])]
    q = ops.DeviceRepSet.from_list(docs)
    got = ops.dotmax_scores(q, q, pairing=_lib.PAIR_CROSS).cpu().numpy().reshape(len(docs), len(docs))
    assert np.isfinite(got).all()
    with np.errstate(all='ignore'):
        for i, x in enumerate(docs):
            for j, y in enumerate(docs):
                want = float(np.max(cosine_similarity(x, y)))
                assert np.isfinite(want)
                assert abs(got[i, j] - want) <= SK_TOL, (i, j, got[i, j], want)
    assert got[3, 3] == 0 and got[3, 4] == 0 and got[4, 4] == 0 and got[0, 5] == 0     # both sides overflow: 0, not NaN
    assert got[2, 2] > 0                                                          # the raw dot of a sub-10-eps row


def test_dot_form_matches_matmul():
    from aspire_amd import _lib, ops
    rng = np.random.default_rng(11)
    q_docs = [rng.standard_normal((int(n), 768)).astype(np.float32) for n in (1, 8, 16, 30, 128)]
    c_docs = [rng.standard_normal((int(n), 768)).astype(np.float32) for n in rng.integers(1, 40, 25)]
    got = ops.dotmax_scores(ops.DeviceRepSet.from_list(q_docs), ops.DeviceRepSet.from_list(c_docs), pairing=_lib.PAIR_CROSS,
                            sim=_lib.SIM_DOT).cpu().numpy().reshape(len(q_docs), len(c_docs))
    for qi, x in enumerate(q_docs):
        for ci, y in enumerate(c_docs):
            want = float(np.matmul(x, y.T).max())
            want64 = float(np.matmul(x.astype(np.float64), y.T.astype(np.float64)).max())
            assert abs(got[qi, ci] - want) <= 1e-6 * max(1.0, abs(want64)) * 4, (got[qi, ci], want)
            assert abs(got[qi, ci] - want64) <= 1e-6 * abs(want64) + 1e-5, (got[qi, ci], want64)


def test_host_layer_rejects_non_finite_and_empty():
    from aspire_amd import ops
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 768)).astype(np.float32)
    bad = x.copy()
    bad[1, 5] = np.inf
    with pytest.raises(ValueError):
        ops.dotmax_scores(ops.DeviceRepSet.from_list([x]), ops.DeviceRepSet.from_list([bad]))
    bad[1, 5] = np.nan
    with pytest.raises(ValueError):
        ops.dotmax_scores(ops.DeviceRepSet.from_list([bad]), ops.DeviceRepSet.from_list([x]))
    with pytest.raises(ValueError):
        ops.dotmax_scores(ops.DeviceRepSet.from_list([x]), ops.DeviceRepSet.from_list([x, np.zeros((0, 768), np.float32)]))


@pytest.mark.parametrize('k', [0, 10, 'all'])
def test_rank_batch_order_and_scores(k):
    from aspire_amd import _lib, ops
    rng = np.random.default_rng(5)
    sizes = [1, 7, 1000, 125, 3, 64]
    queries = [_rows(rng, int(rng.integers(1, 20)), 'aniso' if j % 2 else 'normal') for j in range(len(sizes))]
    bank = [_rows(rng, int(n), 'aniso') for n in rng.integers(1, 33, 300)]
    pools = []
    for n in sizes:
        idx = list(rng.integers(0, len(bank), n))
        if n >= 7:
            idx[3] = idx[1]                                    # a duplicated candidate: equal scores, pool order kept
        pools.append(idx)
    flat = [bank[i] for p in pools for i in p]
    c = ops.DeviceRepSet.from_list(flat)
    q = ops.DeviceRepSet.from_list(queries)
    job_off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32).cuda()
    max_job = max(sizes)
    kk = max_job if k == 'all' else k
    scores, top_s, top_i = ops.dotmax_rank_batch(q, c, job_off, max_job, kk)
    scores = scores.cpu().numpy()
    off = 0
    for j, p in enumerate(pools):
        mine = scores[off:off + len(p)]
        for t in range(0, len(p), max(1, len(p) // 40)):          # a sample of the big pool, every candidate of the small ones
            _check_pair(float(mine[t]), queries[j], bank[p[t]])
        if len(p) >= 7:
            assert mine[3] == mine[1]
        if kk:
            want = sorted(range(len(p)), key=lambda i: mine[i], reverse=True)[:kk]
            ti, ts = top_i[j].cpu().numpy(), top_s[j].cpu().numpy()
            n = min(kk, len(p))
            assert ti[:n].tolist() == want, j
            np.testing.assert_array_equal(ts[:n], mine[want])
            assert (ti[n:] == -1).all() and np.isneginf(ts[n:]).all()
        off += len(p)


def test_evaluate_score_cosine_end_to_end(tmp_path):
    from aspire_amd import evaluate
    from aspire_amd.sentenc import AspireSentEnc
    tok, words = _tokenizer(tmp_path)
    rng = np.random.default_rng(17)
    papers, pids = [], []
    for i in range(60):
        n_sents = int(rng.integers(1, 9))
        papers.append({'TITLE': f't{i}', 'ABSTRACT': _sentences(words, rng.integers(2, 40, n_sents), seed=1000 + i)})
        pids.append(f'p{i}')
    model = AspireSentEnc(bert_model=_bert(2, seed=9), tokenizer=tok)
    store = model.encode_to_store(papers, pids)
    reps = model.encode_papers(papers)
    for pid, r in zip(pids, reps):
        np.testing.assert_array_equal(store.get(pid), r)
    test_pool = {pids[q]: {'cands': [pids[c] for c in rng.permutation(60)[:int(rng.integers(5, 45))] if c != q]}
                 for q in range(0, 60, 4)}
    got = evaluate.score(str(tmp_path / 'res'), test_pool, store, method='cosine')
    for qid, pool in test_pool.items():
        # rank_pool_sent restated: sklearn cosine + np.max per candidate, stable sorted, -sim written (evaluate.py:77)
        sims = [float(np.max(cosine_similarity(store.get(qid), store.get(c)))) for c in pool['cands']]
        order = sorted(range(len(sims)), key=lambda i: sims[i], reverse=True)
        written = got[qid]
        assert len(written) == len(order)
        by_pid = {c: -s for c, s in written}
        for c, s in zip(pool['cands'], sims):
            assert abs(by_pid[c] - s) <= SK_TOL
        want_ids = [pool['cands'][i] for i in order]
        got_ids = [c for c, _ in written]
        for a in range(len(order) - 1):
            if sims[order[a]] - sims[order[a + 1]] > 8e-6:       # order fixed wherever neighbours differ by more than 8e-6
                assert set(got_ids[:a + 1]) == set(want_ids[:a + 1]), (qid, a)


def test_dotmax_op_opcheck():
    import aspire_amd.torch_ops  # noqa: F401
    rng = np.random.default_rng(1)
    q = torch.from_numpy(rng.standard_normal((3, 5, 768)).astype(np.float32)).cuda()
    c = torch.from_numpy(rng.standard_normal((4, 9, 768)).astype(np.float32)).cuda()
    ql = torch.tensor([5, 1, 3], dtype=torch.int32).cuda()
    cl = torch.tensor([9, 2, 4, 7], dtype=torch.int32).cuda()
    for cosine in (True, False):
        torch.library.opcheck(torch.ops.aspire.dotmax_scores, (q, ql, c, cl, False, cosine), test_utils=('test_schema', 'test_faketensor'))
        out = torch.ops.aspire.dotmax_scores(q, ql, c, cl, False, cosine).cpu().numpy().reshape(3, 4)
        x = q.cpu().numpy()[0, :5]
        y = c.cpu().numpy()[1, :2]
        want = float(np.max(cosine_similarity(x, y))) if cosine else float(np.matmul(x, y.T).max())
        assert abs(out[0, 1] - want) <= 1e-5 * max(1.0, abs(want))
    pq = c[:3].contiguous()
    torch.library.opcheck(torch.ops.aspire.dotmax_scores, (q, ql, pq, cl[:3].contiguous(), True, True),
                          test_utils=('test_schema', 'test_faketensor'))
