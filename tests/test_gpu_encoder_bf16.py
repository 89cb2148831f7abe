"""GPU: the training encoder's bf16 matmul mode -- aspire_amd.HipBertTrainEncoder(bert, matmul='bf16') (torch.ops.aspire.
bert_layers_train_prec / bert_layers_train_cls_prec over aspire_bert_layers_forward_train_prec_f32 / aspire_bert_layers_backward_prec_f32).

Yardstick: the EXACT float64 CPU model (no rounding to bf16 anywhere), on the cases 1 x (2, 5), 2 x (3, 37), 2 x (2, 130) of
tests/test_gpu_encoder_backward.py.  Bound per tensor: trainside_inputs.bound(ref_err, max|grad|) = max(4 ref_err, 4 * 2^-23 max|grad|),
ref_err the deviation from the exact model of the mode's arithmetic emulated on the CPU with fp32 accumulation
(tests/bf16_matmul_ref.py: both operands of every forward and backward product rounded to bf16); the key bias scaled by the query bias,
as the fp32 test does.  What the bound checks: the kernels round what the mode says is rounded, once, and nothing else -- an operand
rounded twice, left unrounded or truncated, or a product that stayed on the fp32 pipe, moves a tensor by about ref_err itself.

Largest |kernel - float64| / bound per tensor group on an MI355X, the case where the ratio is largest (every comparison prints its
figures before it asserts; also DESIGN.md section 7, "bf16 matrix products"):

    group                                  error       bound       ratio  case
    hidden                                 3.407e-03   1.363e-02   0.25   1 x (2, 5)
    tables                                 1.090e+00   3.818e+00   0.29   2 x (3, 37)
    emb LayerNorm                          5.628e-02   2.174e-01   0.26   2 x (3, 37)
    attention.self.query.weight            2.045e-02   7.252e-02   0.28   2 x (3, 37)
    attention.self.query.bias              3.957e-03   1.583e-02   0.25   1 x (2, 5)
    attention.self.key.weight              2.267e-02   7.705e-02   0.29   2 x (3, 37)
    attention.self.key.bias                2.229e-03   8.127e-03   0.27   2 x (3, 37)
    attention.self.value.weight            1.458e-01   5.167e-01   0.28   2 x (2, 130)
    attention.self.value.bias              9.754e-02   3.583e-01   0.27   2 x (2, 130)
    attention.output.dense.weight          1.498e-01   5.868e-01   0.26   2 x (2, 130)
    attention.output.dense.bias            3.964e-02   1.399e-01   0.28   2 x (3, 37)
    attention.output.LayerNorm.weight      4.703e-02   1.842e-01   0.26   2 x (3, 37)
    attention.output.LayerNorm.bias        3.675e-02   1.386e-01   0.27   2 x (3, 37)
    intermediate.dense.weight              1.129e-01   4.206e-01   0.27   2 x (3, 37)
    intermediate.dense.bias                5.862e-02   2.191e-01   0.27   2 x (2, 130)
    output.dense.weight                    1.389e-01   4.672e-01   0.30   2 x (2, 130)
    output.dense.bias                      1.869e-03   6.717e-03   0.28   2 x (3, 37)
    output.LayerNorm.weight                6.412e-02   1.987e-01   0.32   2 x (2, 130)
    output.LayerNorm.bias                  3.502e-02   1.470e-01   0.24   2 x (3, 37)
    cls, learned mix                       2.196e-03   9.637e-03   0.23   2 x (3, 37)
    mix logits' gradient                   6.851e-04   7.019e-03   0.10   2 x (3, 37)

A ratio of 0.25 is the emulation's own error: the bound is four times it.  Every tensor sits at 0.23 - 0.32, so the kernels' error IS
the mode's rounding, and what is left of the factor 4 is the room for the summation order.  The parameter gradients of the CLS case
(largest ratio 0.43, the key bias) are printed by the test.
"""
import copy
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import bf16_matmul_ref as br  # noqa: E402
import readout_inputs as ri  # noqa: E402
from trainside_inputs import bound  # noqa: E402

pytestmark = pytest.mark.gpu


def _step(enc, tok, typ, mask, G):
    """one training forward + backward -> (hidden, {name: grad})"""
    enc.zero_grad(set_to_none=True)
    hidden = enc(tok, token_type_ids=typ, attention_mask=mask)
    (hidden * G.cuda()).sum().backward()
    return hidden.detach(), {n: p.grad.clone() for n, p in enc.bert.named_parameters()}


@functools.lru_cache(maxsize=None)
def _gpu_run(n_layers, b, l, matmul):
    """the mode's step on a case, computed once and shared (never written to); matmul None: the default-constructed encoder"""
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, _ = br.case(n_layers, b, l)
    enc = (HipBertTrainEncoder(copy.deepcopy(m)) if matmul is None else HipBertTrainEncoder(copy.deepcopy(m), matmul=matmul)).train()
    return _step(enc, tok, typ, mask, G)


@pytest.mark.parametrize('n_layers,b,l', br.CASES)
def test_parity_with_the_exact_float64_model(n_layers, b, l):
    m, tok, typ, mask, G, runs = br.case(n_layers, b, l)
    hidden, got = _gpu_run(n_layers, b, l, 'bf16')
    assert hidden.is_cuda and hidden.shape == (b, l, 768)
    assert all(g is not None and torch.isfinite(g).all() for g in got.values())
    (h, g, _), (h32, g32, _) = runs['exact'], runs['emu32']
    tag = f'{n_layers} x ({b}, {l})'
    tol = bound(float((h32.double() - h).abs().max()), float(h.abs().max()))
    err = float((hidden.double().cpu() - h).abs().max())
    print(f'[{tag}] hidden |kernel - float64| {err:.3e}  bound {tol:.3e}  ratio {err / tol:.2f}')
    br.compare_grads(got, g, g32, bound, tag)
    assert err <= tol


def test_the_default_path_is_untouched():
    """HipBertTrainEncoder(m) and HipBertTrainEncoder(m, matmul='fp32'): the same bits for hidden and every gradient"""
    h0, g0 = _gpu_run(2, 3, 37, None)
    h1, g1 = _gpu_run(2, 3, 37, 'fp32')
    assert torch.equal(h0, h1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_fp32_mode_of_the_prec_operators_gives_the_siblings_bits():
    """the _prec_ operators with matmul = 0 are the dropout / CLS operators, bit for bit (the C entries' ASPIRE_MATMUL_FP32)"""
    from aspire_amd import HipBertTrainEncoder
    import aspire_amd.torch_ops  # noqa: F401
    m, tok, typ, mask, G, _ = br.case(2, 3, 37)
    enc = HipBertTrainEncoder(copy.deepcopy(m))
    with torch.no_grad():
        emb = enc.bert.embeddings
        emb_sum = (emb.word_embeddings(tok.cuda()) + emb.token_type_embeddings(typ.cuda())) + emb.position_embeddings.weight[:37]
        weights = [w.detach().clone() for w in enc.layer_weights()]
    drop = (0.1, 0.1, 12345, 3)
    h0, t0 = torch.ops.aspire.bert_layers_train_dropout(emb_sum, mask.cuda(), weights, 12, 1e-12, *drop)
    h1, t1 = torch.ops.aspire.bert_layers_train_prec(emb_sum, mask.cuda(), weights, 12, 1e-12, *drop, 0)
    assert torch.equal(h0, h1)
    a = torch.ops.aspire.bert_layers_backward_dropout(G.cuda(), t0, mask.cuda(), weights, 12, 1e-12, *drop)
    c = torch.ops.aspire.bert_layers_backward_prec(G.cuda(), t1, mask.cuda(), weights, 12, 1e-12, *drop, 0)
    assert torch.equal(a[0], c[0]) and all(torch.equal(x, y) for x, y in zip(a[1], c[1]))
    with pytest.raises(AssertionError):                    # ASPIRE_ERR_INVALID_ARG: an unknown mode, before any launch
        torch.ops.aspire.bert_layers_train_prec(emb_sum, mask.cuda(), weights, 12, 1e-12, *drop, 2)


def test_the_mode_does_something():
    """a switch that is silently ignored would give the fp32 mode's hidden"""
    h_bf16, _ = _gpu_run(2, 2, 130, 'bf16')
    h_fp32, _ = _gpu_run(2, 2, 130, 'fp32')
    diff = float((h_bf16 - h_fp32).abs().max())
    print(f'max |hidden bf16 - hidden fp32| at 2 x (2, 130): {diff:.3e}')
    assert not torch.equal(h_bf16, h_fp32) and diff > 1e-4
    # two steps of the mode: the same bits
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, _ = br.case(2, 2, 130)
    h2, g2 = _step(HipBertTrainEncoder(copy.deepcopy(m), matmul='bf16').train(), tok, typ, mask, G)
    h1, g1 = _gpu_run(2, 2, 130, 'bf16')
    assert torch.equal(h1, h2) and all(torch.equal(g1[n], g2[n]) for n in g1)


def test_eval_and_no_grad_forwards_work_in_the_mode():
    """eval() and no_grad stay on the inference path in fp32 (no tape, not differentiable), in either mode"""
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, runs = br.case(1, 2, 5)
    enc = HipBertTrainEncoder(copy.deepcopy(m), matmul='bf16').train()
    ref = HipBertTrainEncoder(copy.deepcopy(m)).eval()(tok, token_type_ids=typ, attention_mask=mask)
    with torch.no_grad():
        plain = enc(tok, token_type_ids=typ, attention_mask=mask)
    assert plain.grad_fn is None and torch.equal(plain, ref)
    assert torch.equal(enc.eval()(tok, token_type_ids=typ, attention_mask=mask), ref)
    assert float((enc.forward_cls((tok, typ, mask)) - ref[:, 0, :]).abs().max()) <= 1e-4        # (the CLS forward: inference kernels of its own)
    assert float((plain.double().cpu() - runs['exact'][0]).abs().max()) <= 1e-4


def test_dropout_in_the_mode():
    """the same (seed, step) gives the same bits twice; p = 0 gives the no-dropout bits of the mode"""
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, _ = br.case(2, 3, 37)

    def run(p, state):
        mm = copy.deepcopy(m)
        mm.config.hidden_dropout_prob = mm.config.attention_probs_dropout_prob = p
        enc = HipBertTrainEncoder(mm, dropout=True, seed=77, matmul='bf16').train()
        enc.set_dropout_state(*state)
        out = _step(enc, tok, typ, mask, G)
        assert enc.dropout_state() == (state[0], state[1] + 1)
        return out

    h1, g1 = run(0.1, (77, 5))
    h2, g2 = run(0.1, (77, 5))
    assert torch.equal(h1, h2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    h3, _ = run(0.1, (77, 6))
    assert not torch.equal(h1, h3)
    h0, g0 = run(0.0, (77, 5))
    hn, gn = _gpu_run(2, 3, 37, 'bf16')
    assert not torch.equal(h1, h0)
    assert torch.equal(h0, hn) and all(torch.equal(g0[n], gn[n]) for n in g0)


def test_cls_readout_with_a_learned_mix():
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, logits, runs = br.cls_case()
    enc = HipBertTrainEncoder(copy.deepcopy(m), matmul='bf16').train()
    lg = logits.clone().cuda().requires_grad_(True)
    cls = enc.forward_cls((tok, typ, mask), mix=torch.softmax(lg, 0))
    assert cls.shape == (3, 768) and cls.requires_grad
    (cls * G.cuda()).sum().backward()
    (c, g, gl), (c32, g32, gl32) = runs['exact'], runs['emu32']
    tol = bound(float((c32.double() - c).abs().max()), float(c.abs().max()))
    err = float((cls.detach().double().cpu() - c).abs().max())
    print(f'[cls 2 x (3, 37)] cls |kernel - float64| {err:.3e}  bound {tol:.3e}  ratio {err / tol:.2f}')
    tol_l = bound(float((gl32.double() - gl).abs().max()), float(gl.abs().max()))
    err_l = float((lg.grad.double().cpu() - gl).abs().max())
    print(f'[cls 2 x (3, 37)] mix logits\' gradient |kernel - float64| {err_l:.3e}  bound {tol_l:.3e}  ratio {err_l / tol_l:.2f}')
    br.compare_grads({n: p.grad for n, p in enc.bert.named_parameters()}, g, g32, bound, 'cls 2 x (3, 37)')
    assert err <= tol and err_l <= tol_l
    # without a mix: the CLS rows of the mode's last hidden state
    enc2 = HipBertTrainEncoder(copy.deepcopy(m), matmul='bf16').train()
    assert torch.equal(enc2.forward_cls((tok, typ, mask)).detach(), _gpu_run(2, 3, 37, 'bf16')[0][:, 0, :])


# ---- the trainer (the pattern of tests/test_gpu_trainer.py) -----------------------------------------------------------------------------
VOCAB = 300
WORDS = ['alpha', 'beta', 'gamma', 'delta', 'kappa', 'sigma', 'omega', 'theta', 'lambda', 'zeta', 'rho', 'tau', 'phi', 'chi', 'psi', 'mu',
         'nu', 'xi', 'pi', 'eta', 'iota', 'upsilon', 'omicron', 'epsilon']
TABLES = ('embeddings.word_embeddings.weight', 'embeddings.position_embeddings.weight', 'embeddings.token_type_embeddings.weight')


def _trainer_bert(seed, dropout=0.1):
    from transformers import BertConfig, BertModel
    torch.manual_seed(seed)
    cfg = BertConfig(vocab_size=VOCAB, hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=256,
                     max_position_embeddings=64, layer_norm_eps=1e-12, hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout,
                     attn_implementation='eager')
    return BertModel(cfg, add_pooling_layer=True)


def _abstracts(seed):
    g = torch.Generator().manual_seed(seed)

    def sent():
        return ' '.join(WORDS[int(i)] for i in torch.randint(0, len(WORDS), (int(torch.randint(3, 7, (1,), generator=g)),), generator=g)) + '.'

    return [{'TITLE': sent(), 'ABSTRACT': [sent() for _ in range(int(torch.randint(1, 4, (1,), generator=g)))]} for _ in range(3)]


def _batches(tmp):
    from transformers import BertTokenizer
    from aspire_amd import prepare_abstracts
    path = os.path.join(tmp, 'bf16_trainer_vocab.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]', '.'] + WORDS) + '\n')
    tok = BertTokenizer(path, do_lower_case=True)
    out = []
    for base in (10, 20):
        batch = {}
        for key, seed in (('query', base + 1), ('pos', base + 2), ('neg', base + 3)):
            bert_batch, abs_lens, idxs = prepare_abstracts(_abstracts(seed), tok)
            batch.update({key + '_bert_batch': bert_batch, key + '_abs_lens': abs_lens, key + '_senttok_idxs': idxs})
        out.append(batch)
    return out


def test_trainer_resumes_on_the_straight_runs_bits(tmp_path):
    """RankTrainer in bf16 mode with dropout, the tables frozen (their scatter gradient is torch's): four iterations straight, and two +
    a checkpoint + two, end on the same bits; the checkpoint names its mode and an fp32-mode encoder refuses it"""
    from aspire_amd import HipBertTrainEncoder, RankTrainer
    batches = _batches(str(tmp_path))
    hparams = ri.hparams('l2wasserstein', 0.0)
    train_hparams = dict(es_check_every=1000, train_size=6, dev_size=3, batch_size=3, num_epochs=2, update_rule='adam', learning_rate=1e-3,
                         lr_decay_method='exponential', decay_lr_by=0.7, decay_lr_every=1)

    def make(seed, tag, matmul='bf16'):
        model = _trainer_bert(seed)
        for n, p in model.named_parameters():
            if n in TABLES:
                p.requires_grad_(False)
        enc = HipBertTrainEncoder(model, dropout=True, seed=0x9E3779B97F4A7C15, matmul=matmul)
        return RankTrainer(enc, hparams, train_hparams, str(tmp_path / tag), lambda epoch: batches)

    straight = make(5, 'straight')
    straight.train(max_iterations=4)
    first = make(5, 'first')
    first.train(max_iterations=2)
    first.save_checkpoint(tmp_path / 'ck.pt')
    assert torch.load(tmp_path / 'ck.pt', weights_only=True)['matmul'] == 'bf16'
    second = make(99, 'second')
    second.load_checkpoint(tmp_path / 'ck.pt')
    second.train(max_iterations=2)
    assert second.iteration == straight.iteration == 4
    trained = 0
    for (n, a), (_, b) in zip(second.encoder.bert.named_parameters(), straight.encoder.bert.named_parameters()):
        assert torch.isfinite(a).all() and torch.equal(a, b), n
        sa, sb = second.optimizer.state.get(a, {}), straight.optimizer.state.get(b, {})
        assert set(sa) == set(sb), n
        for key in sa:
            assert torch.equal(sa[key], sb[key]), (n, key)
        trained += bool(sa)
    assert trained >= 16
    # the run was the mode's: the fp32 mode ends elsewhere
    other = make(5, 'other', matmul='fp32')
    with pytest.raises(ValueError, match="'bf16'.*'fp32'"):
        other.load_checkpoint(tmp_path / 'ck.pt')
    other.train(max_iterations=4)
    name, a = next((n, p) for n, p in other.encoder.bert.named_parameters() if n.endswith('output.dense.weight'))
    assert not torch.equal(a, dict(straight.encoder.bert.named_parameters())[name])
