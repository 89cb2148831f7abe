"""GPU parity of the SPECTER-CoCite bi-encoder (aspire_amd/bienc.py, aspire_bert_forward_cls_f32).  The reference's arithmetic is
restated with HuggingFace BertModel(output_hidden_states=True) + torch.softmax / linear (examples/ex_aspire_bienc.py:23-58,
disent_models.py:183-205): the CLS row of every hidden state at 1e-4 (the encoder suite's bar) on every forward form, the layer mix
against float64, the CLS-only last layer against the full forward's row 0, checkpoint-like weights, MySPECTER's methods and the
evaluate route's ranking."""
import numpy as np
import pytest
import torch

from test_gpu_encoder import _batch, _bert

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _hidden_states(m, tok, seg, mask, double=False):
    with torch.no_grad():
        if double:
            m = m.double()
        hs = m(tok, token_type_ids=seg, attention_mask=mask, output_hidden_states=True).hidden_states
        if double:
            m.float()
    return torch.stack([h[:, 0] for h in hs])            # [n_layers + 1, B, 768]


# (n_layers, B, L, pins): 2 x 16 the round-2 GEMMs; 8 x 128 the plane path with the separate LayerNorm (and the fp32-qkv attention
# forms); 64 x 128 = 64 row tiles: the LayerNorm in the GEMM epilogue, hidden states only as fp16 planes; 2 x 512; 0- and 1-layer
_FORMS = [(2, 2, 16, {}), (2, 8, 128, {}), (2, 8, 128, {'ATTN': 'f32'}), (2, 8, 128, {'ATTN': 'gemm'}), (2, 64, 128, {}),
          (2, 64, 128, {'GEMM_LN': 'off'}), (1, 2, 512, {}), (0, 2, 16, {}), (1, 3, 37, {}), (12, 2, 64, {})]


@pytest.mark.parametrize('n_layers,b,l,pins', _FORMS)
def test_cls_taps_match_every_hidden_state(n_layers, b, l, pins):
    from aspire_amd._lib import pinned
    from aspire_amd.bienc import AspireBiEnc
    m = _bert(n_layers, seed=n_layers + 1)
    tok, seg, mask, _ = _batch(b, l, 3000, seed=b * 1000 + l)            # ragged masks, row 0 full length
    want = _hidden_states(m, tok, seg, mask)
    model = AspireBiEnc(bert_model=m)
    with pinned(**pins):
        cls, layers = model.forward_device(tok, seg, mask, want_layers=True)
    assert model.bert_encoder.status() == 0
    layers, cls = layers.cpu(), cls.cpu()
    assert layers.shape == (n_layers + 1, b, 768)
    for i in range(n_layers + 1):
        err = (layers[i] - want[i]).abs().max().item()
        assert err < TOL, (i, err)
    assert torch.equal(cls, layers[-1])                                   # no mix: the last hidden state's CLS row


@pytest.mark.parametrize('kind', ['zero', 'peaked', 'normal'])
@pytest.mark.parametrize('b,l', [(3, 40), (64, 128)])
def test_layer_mix_matches_float64(kind, b, l):
    from aspire_amd.bienc import AspireBiEnc
    n_layers = 4
    m = _bert(n_layers, seed=21)
    tok, seg, mask, _ = _batch(b, l, 3000, seed=77 + l)
    g = torch.Generator().manual_seed(5)
    W = {'zero': torch.zeros(1, n_layers + 1), 'peaked': torch.tensor([[0., 0., 9., 0., 1.]]),
         'normal': 2.0 * torch.randn(1, n_layers + 1, generator=g)}[kind]
    hs64 = _hidden_states(m, tok, seg, mask, double=True)
    want = torch.nn.functional.linear(hs64.permute(1, 2, 0), torch.softmax(W.double(), dim=1))[..., 0]   # SoftmaxMixLayers on [B, 768, 13]
    got = AspireBiEnc(bert_model=m, layer_weights=W).forward({'tokid_tt': tok, 'seg_tt': seg, 'attnmask_tt': mask})
    assert got.device.type == 'cpu' and got.shape == (b, 768)
    err = (got.double() - want).abs().max().item()
    assert err < TOL, err


@pytest.mark.parametrize('b,l', [(4, 96), (8, 128), (64, 128)])
def test_cls_only_last_layer_no_worse_than_the_full_forward(b, l):
    from aspire_amd.bienc import AspireBiEnc
    m = _bert(3, seed=31)
    tok, seg, mask, _ = _batch(b, l, 3000, seed=13 + b)
    want = _hidden_states(m, tok, seg, mask, double=True)[-1]
    model = AspireBiEnc(bert_model=m)
    cls = model.forward_device(tok, seg, mask)[0].cpu().double()
    full = model.bert_encoder.forward_hidden(tok, seg, mask)[:, 0].cpu().double()
    err, err_full = (cls - want).abs().max().item(), (full - want).abs().max().item()
    assert err <= TOL
    assert err <= 1.5 * err_full + 1e-6, (err, err_full)


def test_heavy_checkpoint_like_weights():
    """tests/heavy_bert.py's statistics (outlier dimensions at 30 - 100, logits of +-50) at 1024 token rows (the fp16-plane path), and
    its model with an FFN activation beyond fp16: the bar of tests/test_gpu_encoder_heavy.py, max(1e-4, 1.5 x fp32 HF's own error)."""
    from heavy_bert import heavy_tailed_bert
    from aspire_amd.bienc import AspireBiEnc
    for m, seed in ((heavy_tailed_bert(12, seed=3), 17), (heavy_tailed_bert(2, seed=5, ffn_overflow=True), 29)):
        tok, seg, mask, _ = _batch(8, 128, 3000, seed=seed)
        W = torch.randn(1, m.config.num_hidden_layers + 1, generator=torch.Generator().manual_seed(seed))
        hs32, hs64 = _hidden_states(m, tok, seg, mask), _hidden_states(m, tok, seg, mask, double=True)
        model = AspireBiEnc(bert_model=m, layer_weights=W)
        assert model.bert_encoder._w.planes
        mix = torch.softmax(W.double(), dim=1)[0]
        for got, w32, w64 in ((model.forward_device(tok, seg, mask)[0], (hs32.double() * mix[:, None, None]).sum(0),
                               (hs64 * mix[:, None, None]).sum(0)),):
            got = got.cpu().double()
            ref_err = (w32 - w64).abs().max().item()
            assert torch.isfinite(got).all()
            assert (got - w64).abs().max().item() <= max(1e-4, 1.5 * ref_err), ref_err
        model.set_layer_weights(torch.full_like(W, -1e4).index_fill_(1, torch.tensor([W.shape[1] - 1]), 0.))   # the last state only
        got = model.forward_device(tok, seg, mask)[0].cpu().double()
        ref_err = (hs32[-1].double() - hs64[-1]).abs().max().item()
        assert (got - hs64[-1]).abs().max().item() <= max(1e-4, 1.5 * ref_err), ref_err


def _outlier_bert():
    """tests/test_gpu_encoder.py's model with an activation beyond fp16 (one channel of the embedding LayerNorm scaled by 2e5, its input
    weights in layer 0 scaled down), with two layers: layer 0 runs on every token row in the CLS forward too."""
    from transformers import BertConfig, BertModel
    torch.manual_seed(11)
    cfg = BertConfig(vocab_size=400, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072,
                     max_position_embeddings=128)
    m = BertModel(cfg, add_pooling_layer=False).eval()
    ch = 5
    with torch.no_grad():
        m.embeddings.LayerNorm.weight[ch] = 2e5
        lyr = m.encoder.layer[0]
        for lin in (lyr.attention.self.query, lyr.attention.self.key, lyr.attention.self.value, lyr.intermediate.dense):
            lin.weight[:, ch] *= 1e-5
    tok = torch.randint(0, 400, (8, 128), generator=torch.Generator().manual_seed(12))      # 1024 token rows: the fp16-plane GEMMs
    return m, tok, torch.zeros_like(tok), torch.ones_like(tok)


def test_activation_beyond_fp16_falls_back_to_the_full_range_kernels():
    """forward_device on a model whose fp16-plane path overflows (asserted): the 'non-finite' warning, then the full-range kernels'
    reps, which match HF (tests/test_gpu_encoder.py's bar for this model)."""
    from aspire_amd.bienc import AspireBiEnc
    m, tok, seg, mask = _outlier_bert()
    want = _hidden_states(m, tok, seg, mask)[-1]
    model = AspireBiEnc(bert_model=m)
    assert not bool(torch.isfinite(model.bert_encoder.forward_cls(tok, seg, mask)[0]).all())
    with pytest.warns(UserWarning, match='non-finite'):
        cls, layers = model.forward_device(tok, seg, mask, want_layers=True)
    assert torch.isfinite(cls).all() and torch.isfinite(layers).all() and torch.equal(cls, layers[-1])
    np.testing.assert_allclose(cls.cpu().numpy(), want.numpy(), atol=2e-5 * float(want.abs().max()), rtol=0)


def test_readme_dict_and_myspecter_methods():
    from aspire_amd.bienc import AspireBiEnc
    m = _bert(2, seed=41)
    tok, seg, mask, _ = _batch(5, 48, 3000, seed=3)
    W = torch.randn(1, 3, generator=torch.Generator().manual_seed(1))
    model = AspireBiEnc(bert_model=m, layer_weights=W)
    a = model.forward({'input_ids': tok, 'token_type_ids': seg, 'attention_mask': mask})
    b = model({'tokid_tt': tok, 'seg_tt': seg, 'attnmask_tt': mask, 'seq_lens': [48] * 5})
    assert a.shape == (5, 768) and torch.equal(a, b)
    hs64 = _hidden_states(m, tok, seg, mask, double=True)
    want = (hs64 * torch.softmax(W.double(), 1)[0][:, None, None]).sum(0)
    assert (a.double() - want).abs().max().item() < TOL
    bb = {'bert_batch': {'tokid_tt': tok, 'seg_tt': seg, 'attnmask_tt': mask, 'seq_lens': [48] * 5}}
    enc = model.encode(bb)
    assert set(enc) == {'doc_reps'} and isinstance(enc['doc_reps'], np.ndarray) and enc['doc_reps'].shape == (5, 768)
    cached = model.caching_encode(bb)
    assert len(cached) == 5 and all(set(d) == {'doc_cls_reps'} and d['doc_cls_reps'].shape == (768,) for d in cached)
    np.testing.assert_array_equal(np.stack([d['doc_cls_reps'] for d in cached]), a.numpy())
    one = model.encode({'bert_batch': {'tokid_tt': tok[:1], 'seg_tt': seg[:1], 'attnmask_tt': mask[:1], 'seq_lens': [48]}})
    assert one['doc_reps'].shape == (1, 768)
    # no mix weights: the README's plain AutoModel read-out; load_state_dict with the reference's keys brings the mix back
    plain = AspireBiEnc(bert_model=m)
    assert (plain.forward({'input_ids': tok, 'attention_mask': mask}).double() - hs64[-1]).abs().max().item() < TOL
    sd = {'bert_encoder.' + k: v for k, v in m.state_dict().items()}
    sd['bert_layer_weights.weight'] = W
    plain.load_state_dict(sd)
    assert torch.equal(plain.forward({'input_ids': tok, 'token_type_ids': seg, 'attention_mask': mask}), a)


def test_caching_score_and_evaluate_ranking(tmp_path):
    from aspire_amd import evaluate as ev
    from aspire_amd.bienc import AspireBiEnc
    m = _bert(2, seed=51)
    model = AspireBiEnc(bert_model=m, layer_weights=torch.randn(1, 3, generator=torch.Generator().manual_seed(2)))
    n = 40
    batches = []
    for i in range(0, n, 16):
        tok, seg, mask, lens = _batch(min(16, n - i), 64, 3000, seed=500 + i)
        batches.append({'tokid_tt': tok, 'seg_tt': seg, 'attnmask_tt': mask, 'seq_lens': lens})
    pids = [f'p{i}' for i in range(n)]
    store = model.encode_to_store(batches, pids)
    assert len(store) == n and store.get('p3').shape == (1, 768)
    reps = np.concatenate([store.get(p) for p in pids])
    # caching_score: -pairwise_distance(p=2, eps=1e-6) of the query against every candidate
    q = {'doc_cls_reps': reps[0]}
    cands = [{'doc_cls_reps': reps[i]} for i in range(1, n)]
    sc = model.caching_score(q, cands)
    want = -torch.nn.functional.pairwise_distance(torch.from_numpy(reps[:1]).double().expand(n - 1, -1), torch.from_numpy(reps[1:]).double(),
                                                   p=2.0, eps=1e-6).numpy()
    assert sc['batch_scores'].shape == (n - 1,) and sc['pair_scores'] is sc['batch_scores']
    np.testing.assert_allclose(sc['batch_scores'], want, rtol=1e-5, atol=0)
    assert np.ndim(model.caching_score(q, cands[:1])['batch_scores']) == 0      # the reference's squeeze
    # evaluate.score(method='l2max') on one-row documents: -euclidean, TrainedAbstractModel.get_similarity
    from scipy.spatial.distance import euclidean
    test_pool = {'p0': {'cands': pids[1:]}, 'p7': {'cands': pids[:7] + pids[8:]}}
    res = ev.score(str(tmp_path), test_pool, store, method='l2max')
    for qid, pool in test_pool.items():
        sims = np.array([-euclidean(store.get(qid)[0].astype(np.float64), store.get(c)[0].astype(np.float64)) for c in pool['cands']])
        order = sorted(range(len(sims)), key=lambda i: -sims[i])
        ranked = [c for c, _ in res[qid]]
        assert sorted(ranked) == sorted(pool['cands'])
        expect = [pool['cands'][i] for i in order]
        s_sorted = sims[order]
        for j in range(len(order)):
            # positions whose neighbours are more than 1e-5 away are fixed
            if (j == 0 or s_sorted[j - 1] - s_sorted[j] > 1e-5) and (j == len(order) - 1 or s_sorted[j] - s_sorted[j + 1] > 1e-5):
                assert ranked[j] == expect[j], (qid, j)
        np.testing.assert_allclose([-s for _, s in res[qid]], s_sorted, rtol=1e-5, atol=1e-5)


def test_bert_cls_forward_op():
    import aspire_amd.torch_ops  # noqa: F401
    from aspire_amd.bienc import AspireBiEnc
    m = _bert(2, seed=61)
    tok, seg, mask, _ = _batch(3, 40, 3000, seed=9)
    sd = m.state_dict()
    w = [sd['embeddings.word_embeddings.weight'], sd['embeddings.position_embeddings.weight'], sd['embeddings.token_type_embeddings.weight'],
         sd['embeddings.LayerNorm.weight'], sd['embeddings.LayerNorm.bias']]
    for i in range(2):
        p = f'encoder.layer.{i}.'
        a = p + 'attention.self.'
        w += [torch.cat([sd[a + 'query.weight'], sd[a + 'key.weight'], sd[a + 'value.weight']], 0),
              torch.cat([sd[a + 'query.bias'], sd[a + 'key.bias'], sd[a + 'value.bias']], 0),
              sd[p + 'attention.output.dense.weight'], sd[p + 'attention.output.dense.bias'],
              sd[p + 'attention.output.LayerNorm.weight'], sd[p + 'attention.output.LayerNorm.bias'],
              sd[p + 'intermediate.dense.weight'], sd[p + 'intermediate.dense.bias'],
              sd[p + 'output.dense.weight'], sd[p + 'output.dense.bias'],
              sd[p + 'output.LayerNorm.weight'], sd[p + 'output.LayerNorm.bias']]
    w = [t.detach().float().cuda().contiguous() for t in w]
    W = torch.randn(1, 3, generator=torch.Generator().manual_seed(4))
    mix = torch.softmax(W, 1)[0].tolist()
    args = (tok.cuda(), seg.cuda(), mask.cuda(), w, 12, 1e-12, mix)
    torch.library.opcheck(torch.ops.aspire.bert_cls_forward, args, test_utils=('test_schema', 'test_faketensor'))
    got = torch.ops.aspire.bert_cls_forward(*args).cpu()
    want = AspireBiEnc(bert_model=m, layer_weights=W).forward({'input_ids': tok, 'token_type_ids': seg, 'attention_mask': mask})
    assert (got - want).abs().max().item() < 2e-5
    plain = torch.ops.aspire.bert_cls_forward(*args[:-1], []).cpu()
    assert (plain - _hidden_states(m, tok, seg, mask)[-1]).abs().max().item() < TOL
