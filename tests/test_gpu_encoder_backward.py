"""GPU: the encoder under training -- aspire_amd.HipBertTrainEncoder (torch.ops.aspire.bert_layers_train / bert_layers_backward over
aspire_bert_layers_forward_train_f32 / aspire_bert_layers_backward_f32) against HuggingFace BertModel under torch autograd.

Models are random-init from BertConfig at test time (hidden 768, 12 heads, intermediate_size 128, vocab 50, layer_norm_eps 1e-12,
dropout 0, eager attention), LayerNorms and biases perturbed so that every parameter matters.  Yardstick: the same model in float64 on
the CPU; loss = (hidden * G).sum() with a seeded G.  Bound per tensor: trainside_inputs.bound(ref_err, max|grad|) = max(4 ref_err,
4 * 2^-23 max|grad|), ref_err the deviation of the same model's fp32 CPU autograd from float64, computed here.  The key bias, whose
gradient is zero in exact arithmetic (the reference returns rounding noise), is held to max(4 ref_err, 4 * 2^-23 max|grad of the
query bias|).

Largest |kernel - float64| on an MI355X per tensor group, the case where error / bound is largest (n_layers x (B, L), or the RankLoss
aggregation); every comparison prints its figures before it asserts (pytest -s shows them):

    group                                  error       bound       case
    hidden                                 5.632e-07   2.154e-06   0 x (2, 5)
    tables                                 7.838e-06   2.318e-05   l2wasserstein
    emb LayerNorm                          1.983e-05   4.788e-05   2 x (2, 130)
    attention.self.query.weight            3.064e-06   6.020e-06   2 x (3, 37)
    attention.self.query.bias              1.175e-06   1.609e-06   2 x (3, 37)
    attention.self.key.weight              4.351e-06   8.861e-06   2 x (2, 130)
    attention.self.key.bias                1.788e-07   5.527e-07   1 x (2, 5)
    attention.self.value.weight            3.919e-05   8.229e-05   2 x (2, 130)
    attention.self.value.bias              5.314e-08   1.020e-07   l2max
    attention.output.dense.weight          5.353e-06   7.595e-06   1 x (1, 1)
    attention.output.dense.bias            8.215e-08   1.380e-07   l2max
    attention.output.LayerNorm.weight      1.694e-06   3.777e-06   1 x (1, 1)
    attention.output.LayerNorm.bias        1.247e-05   3.857e-05   2 x (2, 130)
    intermediate.dense.weight              2.763e-05   6.202e-05   2 x (2, 130)
    intermediate.dense.bias                6.788e-06   1.535e-05   2 x (3, 37)
    output.dense.weight                    5.326e-05   7.923e-05   2 x (2, 130)
    output.dense.bias                      6.686e-08   1.151e-07   l2max
    output.LayerNorm.weight                3.026e-07   7.076e-07   l2wasserstein
    output.LayerNorm.bias                  2.124e-07   6.636e-07   l2wasserstein
    RankLoss loss, l2wasserstein           9.537e-06   1.144e-05

At 1 x (1, 1) the soft-max has one key: the query / key gradients are exact zeros on every side (error 0, bound 0).  No product needed
the launch rule changed: every tensor is inside its bound with the forms DESIGN.md section 3 names."""
import copy
import ctypes
import functools
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from trainside_inputs import bound  # noqa: E402
import readout_inputs as ri  # noqa: E402

pytestmark = pytest.mark.gpu
VOCAB = 50


def _bert(n_layers, seed=0, dropout=0.0, intermediate_size=128):
    from transformers import BertConfig, BertModel
    torch.manual_seed(seed)
    cfg = BertConfig(vocab_size=VOCAB, hidden_size=768, num_hidden_layers=n_layers, num_attention_heads=12,
                     intermediate_size=intermediate_size, max_position_embeddings=512, layer_norm_eps=1e-12, hidden_dropout_prob=dropout,
                     attention_probs_dropout_prob=dropout, attn_implementation='eager')
    m = BertModel(cfg, add_pooling_layer=False).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'LayerNorm' in n or n.endswith('.bias'):
                p.add_(0.1 * torch.randn_like(p))
    return m


def _mask(b, l):
    """full / ragged right padding / left padding / a hole / (3, 37): one document whose mask is all zero"""
    m = torch.ones(b, l, dtype=torch.int64)
    if (b, l) == (2, 5):
        m[1, 3:] = 0
    elif (b, l) == (3, 37):
        m[0, :4] = 0
        m[0, 20] = 0
        m[1, 29:] = 0
        m[2] = 0
    elif (b, l) == (2, 130):
        m[1, 129:] = 0
        m[1, 64:70] = 0
        m[1, :2] = 0
    return m


CASES = [(0, 2, 5), (1, 1, 1), (1, 2, 5), (2, 3, 37), (2, 2, 130)]


@functools.lru_cache(maxsize=None)
def _case(n_layers, b, l):
    """the model, its inputs and both CPU reference runs (float64 the yardstick, fp32 the reference's own error) -- computed once per
    case, never written to"""
    m = _bert(n_layers, seed=10 * n_layers + b)
    g = torch.Generator().manual_seed(100 + l)
    tok = torch.randint(0, VOCAB, (b, l), generator=g)
    typ = torch.randint(0, 2, (b, l), generator=g)
    mask = _mask(b, l)
    G = torch.randn(b, l, 768, generator=g)
    runs = {}
    for dt in (torch.float64, torch.float32):
        mm = copy.deepcopy(m).to(dt)
        hidden = mm(tok, token_type_ids=typ, attention_mask=mask).last_hidden_state
        (hidden * G.to(dt)).sum().backward()
        runs[dt] = (hidden.detach(), {n: p.grad for n, p in mm.named_parameters()})
    return m, tok, typ, mask, G, runs


def _group(name):
    if name.startswith('embeddings.'):
        return 'tables' if 'LayerNorm' not in name else 'emb LayerNorm'
    return name.split('.', 3)[3]


def _compare(got, runs, tag):
    """every parameter's gradient against float64 within bound; prints the largest error / bound per tensor group first"""
    (_, g64), (_, g32) = runs[torch.float64], runs[torch.float32]
    worst, fails = {}, []
    for n, want in g64.items():
        ref_err = float((g32[n].double() - want).abs().max())
        scale = float(want.abs().max())
        if n.endswith('attention.self.key.bias'):
            scale = float(g64[n.replace('key.bias', 'query.bias')].abs().max())
        tol = bound(ref_err, scale)
        err = float((got[n].double().cpu() - want).abs().max())
        k = _group(n)
        if k not in worst or err / tol > worst[k][0] / worst[k][1]:
            worst[k] = (err, tol)
        if not err <= tol:
            fails.append((n, err, tol))
    for k, (err, tol) in worst.items():
        print(f'[{tag}] {k:42s} |kernel - float64| {err:.3e}  bound {tol:.3e}')
    assert not fails, fails


@pytest.mark.parametrize('n_layers,b,l', CASES)
def test_gradients_match_float64(n_layers, b, l):
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, runs = _case(n_layers, b, l)
    enc = HipBertTrainEncoder(copy.deepcopy(m)).train()
    hidden = enc(tok, token_type_ids=typ, attention_mask=mask)
    assert hidden.is_cuda and hidden.shape == (b, l, 768) and hidden.requires_grad
    (hidden * G.cuda()).sum().backward()
    h64, h32 = runs[torch.float64][0], runs[torch.float32][0]
    tol = bound(float((h32.double() - h64).abs().max()), float(h64.abs().max()))
    err = float((hidden.detach().double().cpu() - h64).abs().max())
    print(f'[{n_layers} x ({b}, {l})] hidden |kernel - float64| {err:.3e}  bound {tol:.3e}')
    got = {n: p.grad for n, p in enc.bert.named_parameters()}
    assert all(g is not None and torch.isfinite(g).all() for g in got.values())
    _compare(got, runs, f'{n_layers} x ({b}, {l})')
    assert err <= tol


def _op_inputs(n_layers=2, b=3, l=37):
    from aspire_amd import HipBertTrainEncoder
    import aspire_amd.torch_ops  # noqa: F401
    m, tok, typ, mask, G, _ = _case(n_layers, b, l)
    enc = HipBertTrainEncoder(copy.deepcopy(m))
    with torch.no_grad():
        emb = enc.bert.embeddings
        emb_sum = (emb.word_embeddings(tok.cuda()) + emb.token_type_embeddings(typ.cuda())) + emb.position_embeddings.weight[:l]
        weights = [w.detach().clone() for w in enc.layer_weights()]
    return emb_sum, mask.cuda(), weights, G.cuda()


def test_backward_gives_the_same_bits_twice():
    emb_sum, mask, weights, G = _op_inputs()
    hidden, tape = torch.ops.aspire.bert_layers_train(emb_sum, mask, weights, 12, 1e-12)
    hidden2, tape2 = torch.ops.aspire.bert_layers_train(emb_sum, mask, weights, 12, 1e-12)
    assert torch.equal(hidden, hidden2) and tape.numel() == tape2.numel()       # (the tape is opaque: the gaps between its slots are unwritten)
    a = torch.ops.aspire.bert_layers_backward(G, tape, mask, weights, 12, 1e-12)
    b = torch.ops.aspire.bert_layers_backward(G, tape, mask, weights, 12, 1e-12)
    assert torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) == len(weights)
    for x, y in zip(a[1], b[1]):
        assert torch.isfinite(x).all() and torch.equal(x, y)


def test_backward_writes_every_gradient_buffer():
    """buffers pre-filled with NaN come back finite and equal to the operator's (which allocates its own)"""
    from aspire_amd import _lib, ops
    from aspire_amd.encoder import pack_layer_stack
    emb_sum, mask, weights, G = _op_inputs()
    hidden, tape = torch.ops.aspire.bert_layers_train(emb_sum, mask, weights, 12, 1e-12)
    want_emb, want = torch.ops.aspire.bert_layers_backward(G, tape, mask, weights, 12, 1e-12)
    bw = pack_layer_stack(weights, 12, 1e-12)
    nan = float('nan')
    grads = [torch.full_like(w, nan) for w in weights]
    grad_emb = torch.full_like(emb_sum, nan)
    n_layers = (len(weights) - 2) // 12
    layers = (_lib.BertLayerGrads * n_layers)()
    for i in range(n_layers):
        for (f, _), t in zip(_lib.BertLayerGrads._fields_, grads[2 + 12 * i:14 + 12 * i]):
            setattr(layers[i], f, ctypes.c_void_p(t.data_ptr()))
    bg = _lib.BertGrads(ctypes.c_void_p(grads[0].data_ptr()), ctypes.c_void_p(grads[1].data_ptr()), layers)
    b, l, _ = emb_sum.shape
    ws = torch.full((_lib.lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), b, l),), 0xFF, device='cuda', dtype=torch.uint8)   # NaN bits
    for ge in (grad_emb, None):           # grad_emb_sum may be NULL: the parameter gradients are the same
        _lib.check(_lib.lib.aspire_bert_layers_backward_f32(ctypes.byref(bw), ops._ptr(mask), b, l, ops._ptr(G), ops._ptr(tape), tape.numel(),
                                                            ops._ptr(ge), ctypes.byref(bg), ops._ptr(ws), ws.numel(), ops._stream()))
        assert torch.isfinite(grad_emb).all() and torch.equal(grad_emb, want_emb)
        for x, y in zip(grads, want):
            assert torch.isfinite(x).all() and torch.equal(x, y)


# ---- through RankLoss ----------------------------------------------------------------------------------------------------------------
WORDS = ['alpha', 'beta', 'gamma', 'delta', 'kappa', 'sigma', 'omega', 'theta', 'lambda', 'zeta', 'rho', 'tau', 'phi', 'chi', 'psi', 'mu',
         'nu', 'xi', 'pi', 'eta', 'iota', 'upsilon', 'omicron', 'epsilon']


def _abstracts(seed, n=3):
    g = torch.Generator().manual_seed(seed)

    def sent():
        return ' '.join(WORDS[int(i)] for i in torch.randint(0, len(WORDS), (int(torch.randint(3, 7, (1,), generator=g)),), generator=g)) + '.'

    return [{'TITLE': sent(), 'ABSTRACT': [sent() for _ in range(int(torch.randint(2, 5, (1,), generator=g)))]} for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _rank_batch(tmp):
    from transformers import BertTokenizer
    from aspire_amd import prepare_abstracts
    vocab = ['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]', '.'] + WORDS
    assert len(vocab) <= VOCAB
    path = os.path.join(tmp, 'vocab.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(vocab) + '\n')
    tok = BertTokenizer(path, do_lower_case=True)
    batch = {}
    for key, seed in (('query', 1), ('pos', 2)):
        bert_batch, abs_lens, idxs = prepare_abstracts(_abstracts(seed), tok)
        batch.update({key + '_bert_batch': bert_batch, key + '_abs_lens': abs_lens, key + '_senttok_idxs': idxs})
    return batch


@pytest.mark.parametrize('agg', ['l2max', 'l2wasserstein'])
def test_rank_loss_trains_the_hip_encoder(agg, tmp_path_factory):
    from aspire_amd import HipBertTrainEncoder, RankLoss
    batch = _rank_batch(str(tmp_path_factory.getbasetemp()))
    perm = torch.tensor([1, 2, 0])
    m = _bert(2, seed=7)
    rank = RankLoss(ri.hparams(agg, 0.0))

    def hf_side(dtype):
        mm = copy.deepcopy(m).to(device='cuda', dtype=dtype).train()         # dropout 0: train() changes nothing

        def encoder(bb):
            return mm(bb['tokid_tt'].cuda(), token_type_ids=bb['seg_tt'].cuda(),
                      attention_mask=bb['attnmask_tt'].cuda()).last_hidden_state.to(torch.float32)

        loss = rank.forward_rank(batch, encoder, random_idxs=perm)
        loss.backward()
        return float(loss), {n: p.grad.double().cpu() for n, p in mm.named_parameters()}

    loss64, g64 = hf_side(torch.float64)
    loss32, g32 = hf_side(torch.float32)
    enc = HipBertTrainEncoder(copy.deepcopy(m)).train()
    loss = rank.forward_rank(batch, enc, random_idxs=perm)
    assert loss.is_cuda and loss.requires_grad and loss64 > 0
    loss.backward()
    tol = bound(abs(loss32 - loss64), abs(loss64))
    print(f'[{agg}] loss {float(loss):.6f} |kernel - float64| {abs(float(loss) - loss64):.3e}  bound {tol:.3e} (torch fp32 {loss32:.6f})')
    got = {n: p.grad for n, p in enc.bert.named_parameters()}
    _compare(got, {torch.float64: (None, g64), torch.float32: (None, g32)}, agg)
    assert abs(float(loss) - loss64) <= tol
    # one optimizer step changes the hidden states
    bb = batch['query_bert_batch']
    before = enc(bb).detach().clone()
    opt = torch.optim.SGD(enc.parameters(), lr=0.1)
    opt.step()
    after = enc(bb).detach()
    assert torch.isfinite(after).all() and not torch.equal(before, after)


def test_trained_weights_load_into_the_inference_encoder():
    from aspire_amd import HipBertTrainEncoder
    from aspire_amd.encoder import HipBertEncoder
    m, tok, typ, mask, G, _ = _case(2, 3, 37)
    enc = HipBertTrainEncoder(copy.deepcopy(m)).train()
    (enc(tok, token_type_ids=typ, attention_mask=mask) * G.cuda()).sum().backward()
    torch.optim.SGD(enc.parameters(), lr=0.05).step()
    sd = enc.state_dict()
    assert set(sd) == set(m.state_dict())                              # HuggingFace's names
    inf = HipBertEncoder.from_state_dict(enc.config, {k: v.cpu() for k, v in sd.items()})
    want = inf(tok, token_type_ids=typ, attention_mask=mask).last_hidden_state
    got = enc(tok, token_type_ids=typ, attention_mask=mask).detach()
    assert float((got - want).abs().max()) <= 1e-4
    assert float((got.cpu() - _case(2, 3, 37)[5][torch.float32][0]).abs().max()) > 1e-4        # ... and they did move
    other = HipBertTrainEncoder(_bert(2, seed=99))
    other.load_state_dict(sd)
    assert torch.equal(other.train()(tok, token_type_ids=typ, attention_mask=mask).detach(), got)


def test_no_tape_without_grad(monkeypatch):
    from aspire_amd import HipBertTrainEncoder, _lib
    m, tok, typ, mask, G, runs = _case(1, 2, 5)
    enc = HipBertTrainEncoder(copy.deepcopy(m)).train()
    with_tape = enc(tok, token_type_ids=typ, attention_mask=mask)
    assert with_tape.grad_fn is not None

    def no_training_forward(*args):
        raise AssertionError('the training forward ran: a tape was written')

    monkeypatch.setattr(_lib.lib, 'aspire_bert_layers_forward_train_f32', no_training_forward)
    with torch.no_grad():
        plain = enc(tok, token_type_ids=typ, attention_mask=mask)
    assert plain.grad_fn is None and not plain.requires_grad
    assert float((plain - with_tape.detach()).abs().max()) <= 1e-4
    evald = enc.eval()(tok, token_type_ids=typ, attention_mask=mask)              # eval(): the inference forward as well
    assert evald.grad_fn is None and torch.equal(evald, plain)
    with pytest.raises(AssertionError, match='a tape was written'):
        enc.train()(tok, token_type_ids=typ, attention_mask=mask)


def test_roberta_is_refused_and_dropout_warns_once():
    from transformers import RobertaConfig, RobertaModel
    from aspire_amd import HipBertTrainEncoder
    rob = RobertaModel(RobertaConfig(vocab_size=VOCAB, hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=128,
                                     max_position_embeddings=64), add_pooling_layer=False)
    with pytest.raises(NotImplementedError, match='BertModel'):
        HipBertTrainEncoder(rob)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        enc = HipBertTrainEncoder(_bert(1, dropout=0.1))
        tok = torch.randint(0, VOCAB, (1, 4))
        enc.train()(tok)
        enc(tok)
    assert len([w for w in caught if issubclass(w.category, UserWarning) and 'dropout is not built' in str(w.message)]) == 1
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        HipBertTrainEncoder(_bert(1))                  # dropout 0: no warning
    assert not [w for w in caught if 'dropout' in str(w.message)]
