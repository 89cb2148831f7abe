"""GPU: aspire_amd.RankTrainer over HipBertTrainEncoder + RankLoss + HipAdam -- the full training step on this project's kernels.

A random-init one-layer BertModel WITH its pooler (hidden 768, 12 heads, a vocabulary of 300), B = 3 abstracts of a title and at most
three sentences (L <= 48), explicit negatives (so no permutation is drawn).  The parity bound is tests/optim_ref.bound.
"""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import optim_ref as orf  # noqa: E402
import readout_inputs as ri  # noqa: E402

pytestmark = pytest.mark.gpu
VOCAB = 300
WORDS = ['alpha', 'beta', 'gamma', 'delta', 'kappa', 'sigma', 'omega', 'theta', 'lambda', 'zeta', 'rho', 'tau', 'phi', 'chi', 'psi', 'mu',
         'nu', 'xi', 'pi', 'eta', 'iota', 'upsilon', 'omicron', 'epsilon']
TABLES = ('embeddings.word_embeddings.weight', 'embeddings.position_embeddings.weight', 'embeddings.token_type_embeddings.weight')


def _bert(seed, dropout=0.0):
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


@functools.lru_cache(maxsize=None)
def _batches(tmp):
    """two rank batches with explicit negatives"""
    from transformers import BertTokenizer
    from aspire_amd import prepare_abstracts
    path = os.path.join(tmp, 'trainer_vocab.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]', '.'] + WORDS) + '\n')
    tok = BertTokenizer(path, do_lower_case=True)
    out = []
    for base in (10, 20):
        batch = {}
        for key, seed in (('query', base + 1), ('pos', base + 2), ('neg', base + 3)):
            bert_batch, abs_lens, idxs = prepare_abstracts(_abstracts(seed), tok)
            assert bert_batch['tokid_tt'].shape[1] <= 48
            batch.update({key + '_bert_batch': bert_batch, key + '_abs_lens': abs_lens, key + '_senttok_idxs': idxs})
        out.append(batch)
    return out


def _train_hparams(**over):
    hp = dict(es_check_every=1000, train_size=6, dev_size=3, batch_size=3, num_epochs=2, update_rule='adam', learning_rate=1e-3,
              lr_decay_method='exponential', decay_lr_by=0.7, decay_lr_every=1)
    hp.update(over)
    return hp


@pytest.mark.parametrize('agg,prop', [('l2wasserstein', 0.0), ('l2max', 0.5)])
def test_four_iterations_train_and_the_result_loads_for_inference(agg, prop, tmp_path, tmp_path_factory):
    from aspire_amd import HipAdam, HipBertTrainEncoder, RankTrainer
    from aspire_amd.encoder import HipBertEncoder
    batches = _batches(str(tmp_path_factory.getbasetemp()))
    enc = HipBertTrainEncoder(_bert(3))
    before = {n: p.detach().clone() for n, p in enc.bert.named_parameters()}
    tr = RankTrainer(enc, ri.hparams(agg, prop), _train_hparams(), str(tmp_path), lambda epoch: batches)
    assert isinstance(tr.optimizer, HipAdam) and tr.num_batches == 2 and tr.total_iters == 4
    assert tr.train() is True and tr.iteration == 4
    assert tr.loss_checked_iters == [0] and np.isfinite(tr.loss_history['loss'][0]) and tr.loss_history['loss'][0] > 0
    moved = 0
    for n, p in enc.bert.named_parameters():
        if n.startswith('pooler.'):
            assert p.grad is None and p not in tr.optimizer.state and torch.equal(p.detach(), before[n]), n      # never part of the loss
            continue
        assert torch.isfinite(p).all(), n
        assert int(tr.optimizer.state[p]['step']) == 4, n
        # (exp_avg != 0: some iteration's gradient was not zero; the hinge may be inactive by the last one)
        if bool(tr.optimizer.state[p]['exp_avg'].abs().max() > 0):
            assert not torch.equal(p.detach(), before[n]), n
            moved += 1
    assert moved >= 15                      # all of a layer's sixteen tensors but (possibly) the key bias, the embedding LayerNorm, tables
    assert tr.optimizer.param_groups[0]['lr'] == pytest.approx(1e-3 * 0.7 ** 3)
    # model_final.pt holds HuggingFace's names and loads into the inference encoder
    sd = torch.load(tmp_path / 'model_final.pt', weights_only=True)
    assert set(sd) == set(enc.bert.state_dict())
    inf = HipBertEncoder.from_state_dict(enc.config, {k: v.cpu() for k, v in sd.items()})
    bb = batches[0]['query_bert_batch']
    want = inf(bb['tokid_tt'], token_type_ids=bb['seg_tt'], attention_mask=bb['attnmask_tt']).last_hidden_state
    got = enc.eval()(bb)
    diff = float((got - want).abs().max())
    print(f'[{agg}] trained eval() forward vs the inference encoder on model_final.pt: max |diff| {diff:.3e}')
    assert torch.isfinite(got).all() and diff <= 1e-4


def test_accumulated_gradients_make_one_adam_step(tmp_path, tmp_path_factory):
    """two iterations at update_params_every = 2: the parameters are within the bound of ONE float64 Adam step on the summed gradients,
    which are captured from .grad before the step; the sum itself is checked against the two batches' separate gradients"""
    from aspire_amd import HipBertTrainEncoder, RankLoss, RankTrainer
    batches = _batches(str(tmp_path_factory.getbasetemp()))
    model = _bert(4)
    hparams = ri.hparams('l2wasserstein', 0.0)
    # the two gradients separately, at the initial parameters
    separate = []
    for batch in batches:
        e = HipBertTrainEncoder(copy.deepcopy(model)).train()
        RankLoss(hparams).forward_rank(batch, e).backward()
        separate.append({n: p.grad.clone() for n, p in e.bert.named_parameters() if p.grad is not None})
    enc = HipBertTrainEncoder(copy.deepcopy(model))
    start = {n: p.detach().cpu().numpy().copy() for n, p in enc.bert.named_parameters()}
    tr = RankTrainer(enc, hparams, _train_hparams(accumulated_batch_size=6, num_epochs=1, decay_lr_every=1000), str(tmp_path),
                     lambda epoch: batches)
    captured, step = {}, tr.optimizer.step

    def spy(*a, **k):
        assert not captured
        captured.update({n: p.grad.detach().clone() for n, p in enc.bert.named_parameters() if p.grad is not None})
        return step(*a, **k)

    tr.optimizer.step = spy
    tr.train()
    assert tr.iteration == 2 and captured and all(p.grad is None for p in enc.parameters())       # one step, then zero_grad
    worst = 0.0
    for n, p in enc.bert.named_parameters():
        if n not in captured:
            assert n.startswith('pooler.') and np.array_equal(p.detach().cpu().numpy(), start[n])
            continue
        if n not in TABLES:        # (the tables' scatter gradient is torch's, with atomics: not the same bits run to run)
            assert torch.equal(captured[n], separate[0][n] + separate[1][n]), n
        g = captured[n].cpu().numpy()
        p64, _, _ = orf.adam_update(start[n].astype(np.float64), np.zeros(g.shape), np.zeros(g.shape), g.astype(np.float64), 1, 1e-3)
        cpu = torch.nn.Parameter(torch.from_numpy(start[n].copy()))
        cpu.grad = torch.from_numpy(g.copy())
        torch.optim.Adam([cpu], lr=1e-3, foreach=False).step()
        err = float(np.abs(p.detach().cpu().numpy().astype(np.float64) - p64).max())
        tol = orf.bound(np.abs(cpu.detach().numpy().astype(np.float64) - p64).max(), np.abs(p64).max())
        print(f'{n:60s} |kernel - float64| {err:.3e}  bound {tol:.3e}')
        worst = max(worst, err / tol)
        assert err <= tol, n
        assert float(np.abs(p64 - start[n]).max()) > 100 * tol or not g.any(), n        # the step is far larger than the bound
    print(f'largest error / bound: {worst:.3f}')


def test_resume_gives_the_bits_of_the_straight_run(tmp_path, tmp_path_factory):
    """The three embedding tables are frozen: every gradient then comes from kernels documented as same-bits (the tables' scatter
    gradient is torch's).  The encoder runs WITH dropout, whose (seed, step) the checkpoint carries."""
    from aspire_amd import HipBertTrainEncoder, RankLoss, RankTrainer
    batches = _batches(str(tmp_path_factory.getbasetemp()))
    hparams = ri.hparams('l2wasserstein', 0.0)

    def make(seed, tag):
        model = _bert(seed, dropout=0.1)
        for n, p in model.named_parameters():
            if n in TABLES:
                p.requires_grad_(False)
        enc = HipBertTrainEncoder(model, dropout=True, seed=0x9E3779B97F4A7C15)
        return RankTrainer(enc, hparams, _train_hparams(), str(tmp_path / tag), lambda epoch: batches)

    straight = make(5, 'straight')
    straight.train(max_iterations=4)
    first = make(5, 'first')
    first.train(max_iterations=2)
    first.save_checkpoint(tmp_path / 'ck.pt')
    second = make(99, 'second')                    # other weights: everything must come from the checkpoint
    second.encoder.set_dropout_state(1, 0)
    second.load_checkpoint(tmp_path / 'ck.pt')
    assert (second.iteration, second.epoch, second.batch_in_epoch) == (2, 1, 0)
    second.train(max_iterations=2)
    assert second.iteration == straight.iteration == 4
    assert second.encoder.dropout_state() == straight.encoder.dropout_state() == (0x9E3779B97F4A7C15, 12)   # three forwards a step
    assert second.optimizer.param_groups[0]['lr'] == straight.optimizer.param_groups[0]['lr'] != 1e-3
    assert second.scheduler.state_dict() == straight.scheduler.state_dict()
    trained = 0
    for (n, a), (_, b) in zip(second.encoder.bert.named_parameters(), straight.encoder.bert.named_parameters()):
        assert torch.equal(a, b), n
        sa, sb = second.optimizer.state.get(a, {}), straight.optimizer.state.get(b, {})
        assert set(sa) == set(sb), n
        for key in sa:
            assert torch.equal(sa[key], sb[key]), (n, key)
        trained += bool(sa)
    assert trained >= 16
    # ... and the run did train under dropout: another seed gives other parameters
    other = make(5, 'other')
    other.encoder.set_dropout_state(7, 0)
    other.train(max_iterations=4)
    name, a = next((n, p) for n, p in other.encoder.bert.named_parameters() if n.endswith('output.dense.weight'))
    assert not torch.equal(a, dict(straight.encoder.bert.named_parameters())[name])
