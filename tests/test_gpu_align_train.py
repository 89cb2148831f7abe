"""GPU: the alignment data path end to end on a tiny corpus -- 8 papers of 2 .. 5 sentences and 3 co-cited sets with 2 .. 4 contexts
are encoded by alignment_encoder('cosentbert') (AspireSentEnc over a random 2-layer BertModel and the golden vocab) into a resident RepStore, write_aligned_examples
writes the train and dev files through ops.dot_argmax, write_shuffled_copies / rank_batch_sources stream them into RankTrainer with
an 'sbalisentbienc' / 'l2wasserstein' hparams dict for 2 epochs of 2 iterations and one dev check.  The alignments in the files are
the numpy loop's on the same rows (pre_proc_cocits.py:487-494), the loss sees the written alignments, and a second run from the same
seeds writes the same bytes and gives the same losses."""
import itertools
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import supalign_inputs as si  # noqa: E402

pytestmark = pytest.mark.gpu

N_SENTS = (3, 2, 5, 4, 2, 3, 5, 2)
TRAIN_SETS, DEV_SETS = [('p0', 'p1', 'p2'), ('p3', 'p4')], [('p5', 'p6', 'p7')]
N_CONTEXTS = {'train': (3, 2), 'dev': (4,)}


def _tokenizer(tmp_path):
    from transformers import BertTokenizer
    vocab = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'bienc_prep.json')))['vocab']
    p = tmp_path / 'vocab.txt'
    p.write_text('\n'.join(vocab) + '\n')
    return BertTokenizer(str(p), do_lower_case=True), [w for w in vocab if not w.startswith(('[', '#')) and w.isalpha()], len(vocab)


def _bert(seed, vocab_size):
    from transformers import BertConfig, BertModel
    torch.manual_seed(seed)
    cfg = BertConfig(vocab_size=vocab_size, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=256,
                     max_position_embeddings=128, layer_norm_eps=1e-12, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                     attn_implementation='eager')
    return BertModel(cfg, add_pooling_layer=True).eval()


def _corpus(words):
    rng = np.random.default_rng(21)
    sent = lambda: ' '.join(rng.choice(words, size=int(rng.integers(3, 8)))) + ' .'
    pid2abstract = {f'p{k}': {'title': sent(), 'abstract': [sent() for _ in range(n)]} for k, n in enumerate(N_SENTS)}
    contexts = {split: [[(f'{split}-c{s}-{k}', sent()) for k in range(n)] for s, n in enumerate(ns)] for split, ns in N_CONTEXTS.items()}
    return pid2abstract, contexts


def _numpy_alignments(abs_store, ctx_set, sets):
    """the reference's loop on the rows the store holds; asserts on the way that no product is a near tie"""
    ctx_rows, c_start, c_len = ctx_set.rows.cpu().numpy(), ctx_set.start.cpu().numpy(), ctx_set.len.cpu().numpy()
    worst = 0.0

    def pick(x, y):
        nonlocal worst
        s64 = x.astype(np.float64) @ y.astype(np.float64).T
        tol = max(4 * np.abs(np.matmul(x, y.T) - s64).max(), 4 * 2.0 ** -23 * np.abs(s64).max())
        top = np.sort(s64, axis=None)[::-1]
        worst = max(worst, tol / (top[0] - top[1]))
        return np.unravel_index(s64.argmax(), s64.shape)

    out = []
    for s, pids in enumerate(sets):
        ctx = ctx_rows[c_start[s]:c_start[s] + c_len[s]]
        for i, j in itertools.combinations(range(len(pids)), 2):
            q, p = abs_store.get(pids[i]), abs_store.get(pids[j])
            a2p = pick(q, p)
            out.append(([int(pick(q, ctx)[0]), int(pick(p, ctx)[0])], [int(a2p[0]), int(a2p[1])]))
    assert worst < 0.25, worst            # generic rows: every gap is far above the fp32 error
    return out


def _run(root, tok, words, vocab_size):
    from aspire_amd import (HipBertTrainEncoder, RankTrainer, SupAlignRankLoss, alignment_encoder, context_set, random_neg_sampler,
                            rank_batch_sources, write_aligned_examples, write_shuffled_copies)
    from aspire_amd.sentenc import AspireSentEnc
    pid2abstract, contexts = _corpus(words)
    data, model_path = os.path.join(root, 'data'), os.path.join(root, 'run')
    os.makedirs(data)
    # encode: every abstract once into a resident store, every set's contexts as one document
    enc = alignment_encoder('cosentbert', bert_model=_bert(31, vocab_size), tokenizer=tok)
    assert isinstance(enc, AspireSentEnc) and enc.max_seq_length == 512
    pids = list(pid2abstract)
    abs_store = enc.encode_to_store([{'TITLE': a['title'], 'ABSTRACT': a['abstract']} for a in pid2abstract.values()], pids).to_device()
    want = {}
    for split, sets, sampler in (('train', TRAIN_SETS, None), ('dev', DEV_SETS, random_neg_sampler(pid2abstract, random.Random(7)))):
        ctx_set = context_set(enc, contexts[split])
        assert ctx_set.n == len(sets) and ctx_set.host_lens() == list(N_CONTEXTS[split])
        n = write_aligned_examples(os.path.join(data, f'{split}-cocitabsalign.jsonl'), sets, contexts[split], pid2abstract, abs_store,
                                   ctx_set, neg_sampler=sampler)
        want[split] = _numpy_alignments(abs_store, ctx_set, sets)
        assert n == len(want[split])
    files = {}
    for split in ('train', 'dev'):
        with open(os.path.join(data, f'{split}-cocitabsalign.jsonl'), 'rb') as fp:
            files[split] = fp.read()
        exs = [json.loads(x) for x in files[split].decode('utf-8').splitlines()]
        assert [(e['pos_context']['cc_align'], e['pos_context']['abs_align']) for e in exs] == want[split]
        assert all(('neg_context' in e) == (split == 'dev') for e in exs)
    assert len(want['train']) == 4 and len(want['dev']) == 3
    # stream the files into the trainer
    train_hparams = dict(train_suffix='cocitabsalign', es_check_every=2, train_size=4, dev_size=3, batch_size=2, num_epochs=2,
                         update_rule='adam', learning_rate=1e-3, lr_decay_method='exponential', decay_lr_by=0.7, decay_lr_every=1)
    names = write_shuffled_copies(data, model_path, train_hparams, seed=13)
    for n in names:
        with open(n, 'rb') as fp:
            files[os.path.basename(n)] = fp.read()
    train_batches, dev_batches = rank_batch_sources(data, model_path, train_hparams, tok)
    train_enc = HipBertTrainEncoder(_bert(32, vocab_size))
    torch.manual_seed(5)             # the in-batch negatives' torch.randperm
    trainer = RankTrainer(train_enc, dict(si.CASES['ot_train'][2]), train_hparams, model_path, train_batches, dev_batches)
    assert isinstance(trainer.loss_fn.__self__, SupAlignRankLoss) and trainer.num_batches == 2 and trainer.total_iters == 4
    seen, loss_fn = [], trainer.loss_fn

    def listening(batch, encoder):
        loss = loss_fn(batch, encoder)
        seen.append(('neg_bert_batch' in batch, batch['pos_align_idxs'], float(loss.detach())))
        return loss

    trainer.loss_fn = listening
    assert trainer.train() is True and trainer.iteration == 4
    assert os.path.exists(os.path.join(model_path, 'model_final.pt'))
    assert trainer.dev_checked_iters == [2] and len(trainer.dev_score_history) == 1
    # what the loss saw: per epoch the shuffled file's alignments, two lines at a time; the dev pass (two batches) after iteration 2
    shuffled = [[json.loads(x)['pos_context']['cc_align'] for x in files[os.path.basename(n)].decode('utf-8').splitlines()] for n in names]
    train_seen = [a for dev, a, _ in seen if not dev]
    assert train_seen == [shuffled[0][:2], shuffled[0][2:], shuffled[1][:2], shuffled[1][2:]]
    assert [dev for dev, _, _ in seen] == [False, False, False, True, True, False]
    assert [a for dev, a, _ in seen if dev] == [[w[0] for w in want['dev'][:2]], [w[0] for w in want['dev'][2:]]]
    losses = [x for _, _, x in seen]
    assert np.isfinite(losses).all() and np.isfinite(trainer.loss_history['loss']).all() and np.isfinite(trainer.dev_score_history).all()
    return files, losses, list(trainer.loss_history['loss']), list(trainer.dev_score_history)


def test_files_to_trainer_and_back_again(tmp_path):
    tok, words, vocab_size = _tokenizer(tmp_path)
    first = _run(str(tmp_path / 'a'), tok, words, vocab_size)
    again = _run(str(tmp_path / 'b'), tok, words, vocab_size)
    assert first[0] == again[0]                  # byte-identical example files and shuffled copies
    assert first[1:] == again[1:]                # the same losses, iteration by iteration, and the same dev score
    assert len(first[2]) == 2                    # recorded at iteration 0 and at the dev check


def test_alignment_encoder_builds_the_three_encoders_from_handed_in_models(tmp_path):
    """pre_proc_cocits.py:401-416 over a handed-in model and tokenizer (nothing is downloaded): the class, the pooling, the
    normalisation and max_seq_length of each, the checkpoint of 'cosentbert', and rows out of each."""
    from transformers import MPNetConfig, MPNetModel
    from aspire_amd import alignment_encoder
    from aspire_amd.sbert import SentenceModel
    from aspire_amd.sentenc import AspireSentEnc
    tok, words, vocab_size = _tokenizer(tmp_path)
    sents = ['we propose a graph model .', 'the score is similar .', 'rank the set .']
    # 'cosentbert': CLS rows; sent_encoder_cur_best.pt under trained_model_path replaces the handed-in weights
    trained = _bert(41, vocab_size)
    torch.save(trained.state_dict(), tmp_path / 'sent_encoder_cur_best.pt')
    enc = alignment_encoder('cosentbert', trained_model_path=str(tmp_path), bert_model=_bert(42, vocab_size), tokenizer=tok)
    assert type(enc) is AspireSentEnc and enc.max_seq_length == 512
    want = alignment_encoder('cosentbert', bert_model=trained, tokenizer=tok).encode(sents)
    other = alignment_encoder('cosentbert', bert_model=_bert(42, vocab_size), tokenizer=tok).encode(sents)
    got = enc.encode(sents)
    assert got.shape == (3, 768) and np.abs(got - want).max() < 1e-4 and np.abs(got - other).max() > 1e-2      # the checkpoint's weights
    bb = tok(sents, padding=True, return_tensors='pt')
    with torch.no_grad():
        cls = trained(**bb).last_hidden_state[:, 0].numpy()
    assert np.abs(got - cls).max() < 1e-4                      # the CLS row, the encoder suite's bar
    # 'specter': SentenceModel over a BertModel, mean pooling, not normalised, 512 tokens
    spec = alignment_encoder('specter', model=_bert(43, vocab_size), tokenizer=tok)
    assert type(spec) is SentenceModel and spec.name == 'specter' and spec.normalize is False and spec.max_seq_length == 512
    rows = spec.encode([{'ABSTRACT': sents}])[0]
    with torch.no_grad():
        hid = _bert(43, vocab_size)(**bb).last_hidden_state
    mask = bb['attention_mask'][:, :, None].float()
    mean = ((hid * mask).sum(1) / mask.sum(1)).numpy()
    assert rows.shape == (3, 768) and np.abs(rows - mean).max() < 1e-4
    assert np.abs(np.linalg.norm(rows, axis=1) - 1.0).min() > 0.5          # far from unit rows: no normalisation
    # 'sbmpnet1B': SentenceModel over an MPNetModel, its defaults (384 tokens, normalised)
    torch.manual_seed(44)
    mpnet = MPNetModel(MPNetConfig(vocab_size=vocab_size, hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=3072,
                                   max_position_embeddings=514, layer_norm_eps=1e-5, pad_token_id=0), add_pooling_layer=False).eval()
    sb = alignment_encoder('sbmpnet1B', model=mpnet, tokenizer=tok)
    assert type(sb) is SentenceModel and sb.name == 'sbmpnet1B' and sb.normalize is True and sb.max_seq_length == 384
    rows = sb.encode([{'ABSTRACT': sents}])[0]
    assert rows.shape == (3, 768) and np.abs(np.linalg.norm(rows, axis=1) - 1.0).max() < 1e-5
