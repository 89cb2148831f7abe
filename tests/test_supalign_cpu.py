"""CPU: the host side of the sup-alignment training path -- aspire_amd.SupAlignRankLoss's hyper-parameters and refusals, the rule for
the in-batch negatives' alignment indices held against what the reference's two calls left in its lists (tests/golden/supalign.npz),
batch_prep.make_batch against the reference's batchers (supalign_prep.json), the C ABI and operator surface of the cross-document
distance matrix, and RankTrainer's choice of the loss by model_name.  No kernel runs."""
import ctypes
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import readout_inputs as ri  # noqa: E402
import supalign_inputs as si  # noqa: E402


def _fixture():
    return np.load(os.path.join(GOLDEN, 'supalign.npz'))


def test_hyper_parameter_defaults_and_refusals():
    from aspire_amd import RankLoss, SupAlignRankLoss, pair_distances as pd
    with pytest.raises(KeyError, match='sentsup_loss_prop'):
        SupAlignRankLoss({'score_aggregation': 'l2max'})
    with pytest.raises(KeyError, match='score_aggregation'):
        SupAlignRankLoss({'sentsup_loss_prop': 1.0})
    with pytest.raises(ValueError, match='Unknown aggregation'):
        SupAlignRankLoss({'score_aggregation': 'cosine', 'sentsup_loss_prop': 1.0})
    loss = SupAlignRankLoss({'score_aggregation': 'l2max', 'sentsup_loss_prop': '0.5'})
    assert (loss.sentsup_loss_prop, loss.sent_loss_prop, loss.abs_loss_prop, loss.cd_svalue_l1_prop) == (0.5, 0.0, 0.0, 0.0)
    assert loss.sup_dist_function is pd.allpair_masked_dist_l2sup and loss.dist_function is pd.allpair_masked_dist_l2max
    loss = SupAlignRankLoss({'score_aggregation': 'l2wasserstein', 'sentsup_loss_prop': 1.0, 'weighted_sup': True, 'sent_loss_prop': 1,
                             'abs_loss_prop': 0.25, 'cd_svalue_l1_prop': 0.1, 'geoml_blur': 0.1})
    assert loss.sup_dist_function is pd.allpair_masked_dist_l2sup_weighted
    assert (loss.sent_loss_prop, loss.abs_loss_prop, loss.cd_svalue_l1_prop) == (1.0, 0.25, 0.1)
    assert loss.dist_function.__self__.geoml_blur == 0.1
    assert list(inspect.signature(loss.forward_rank).parameters) == list(inspect.signature(RankLoss.forward_rank).parameters)[1:]
    # RankLoss is as it was: sent_loss_prop defaults to 1 and both regularisers are refused
    assert RankLoss({'score_aggregation': 'l2max'}).sent_loss_prop == 1.0
    for key in ('cd_l1_prop', 'cd_svalue_l1_prop'):
        with pytest.raises(NotImplementedError, match=key):
            RankLoss({'score_aggregation': 'l2max', key: 0.1})


def test_negative_alignment_rule_gives_the_lists_the_reference_left():
    from aspire_amd.rank_loss import negative_align_idxs
    fx = _fixture()
    cond = json.loads(str(fx['conditions']))
    assert cond == dict(clip=True, quirk=True, weighted=True, dev=True)
    seen_quirk = False
    for name in (str(n) for n in fx['cases']):
        size, dev, hp = si.CASES[name]
        active = json.loads(str(fx[f'{name}_active']))
        assert active and all(share >= 0.5 for share in active.values()), (name, active)
        assert set(active) == ({'sup'} if not dev else {'sent'}) | ({'sent'} if hp['sent_loss_prop'] > 0 and not dev else set()) \
            | ({'doc'} if hp['abs_loss_prop'] > 0 else set())
        if dev:
            assert f'{name}_neg_align' not in fx
            continue
        spec = ri.SIZES[size]
        align = [list(a) for a in si.ALIGN[size]]
        perm = [int(i) for i in fx[f'{name}_perm']]
        got = negative_align_idxs(align, perm, spec['q_lens'], spec['p_lens'])
        assert got == fx[f'{name}_neg_align'].tolist(), name
        assert align == si.ALIGN[size], 'the caller\'s lists were written to'
        assert all(got[i] is not align[j] for i, j in enumerate(perm))
        plain = [[min(align[j][0], spec['q_lens'][i] - 1), min(align[j][1], spec['p_lens'][j] - 1)] for i, j in enumerate(perm)]
        seen_quirk |= plain != got
    assert seen_quirk, 'no case in which the write-back changes the negative\'s sentence'
    # tensors and numpy integers as indices, an identity permutation
    assert negative_align_idxs(torch.tensor([[4, 4], [0, 1]]), [0, 1], [2, 3], [5, 1]) == [[1, 4], [0, 0]]


def test_a_negative_alignment_index_survives_the_host_rule_and_is_refused():
    """the negatives' index rule only takes minima, so a negative index of a positive stays negative in the negative that inherits it,
    and the distance SupAlignRankLoss chose refuses it on the host, in front of the device check: it shows without a GPU"""
    from aspire_amd import SupAlignRankLoss, pair_distances as pd
    from aspire_amd.rank_loss import negative_align_idxs
    neg = negative_align_idxs([[1, 0], [-1, 1], [0, -2]], [1, 2, 0], [2, 2, 2], [2, 2, 2])
    assert neg == [[-1, 1], [0, -2], [1, 0]]
    q = pd.rep_len_tup(embed=torch.zeros(3, 768, 2), abs_lens=[2, 2, 2])
    for weighted in (False, True):
        loss = SupAlignRankLoss({'score_aggregation': 'l2max', 'sentsup_loss_prop': 1.0, 'weighted_sup': weighted})
        with pytest.raises(ValueError, match='negative'):
            loss.sup_dist_function(q, pd.rep_len_ali_tup(embed=torch.zeros(3, 768, 2), abs_lens=[2, 2, 2], align_idxs=neg))


def _tokenizer(tmp_path, vocab):
    from transformers import BertTokenizer
    path = os.path.join(str(tmp_path), 'vocab.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(vocab) + '\n')
    return BertTokenizer(path, do_lower_case=True)


def test_make_batch_equals_the_reference_batchers(tmp_path):
    from aspire_amd.batch_prep import ALIGN_TYPES, make_batch
    with open(os.path.join(GOLDEN, 'prep.json')) as f:
        prep = json.load(f)
    with open(os.path.join(GOLDEN, 'supalign_prep.json')) as f:
        want = json.load(f)['cases']
    tok = _tokenizer(tmp_path, prep['vocab'])
    assert ALIGN_TYPES == ('cc_align', 'abs_align') and set(want) == set(si.PREP_FEEDS)
    for name, spec in si.PREP_FEEDS.items():
        feed = si.prep_feed(prep['docs'], spec)
        got = make_batch(feed, tok, align_type=spec['align_type'])
        assert set(got) == set(want[name]), name
        for key, w in want[name].items():
            if isinstance(w, dict):     # a bert batch
                assert set(got[key]) == set(w)
                for k, v in w.items():
                    g = got[key][k]
                    assert (g.tolist() if torch.is_tensor(g) else g) == v, (name, key, k)
                    assert not torch.is_tensor(g) or g.dtype == torch.int64
            else:
                assert got[key] == w, (name, key)
        assert ('pos_align_idxs' in got) == ('pos_align' in spec) and ('neg_align_idxs' in got) == ('neg_align' in spec)
        if 'pos_align' in spec:         # copies: clipping them later cannot reach the examples
            assert all(a is not ex[spec['align_type']] for a, ex in zip(got['pos_align_idxs'], feed['pos_texts']))
    # the key under the other align_type is not read; an unknown one is refused
    train = si.prep_feed(prep['docs'], si.PREP_FEEDS['train'])
    assert 'pos_align_idxs' not in make_batch(train, tok, align_type='cc_align')
    assert 'pos_align_idxs' in make_batch(train, tok, align_type='abs_align')
    with pytest.raises(ValueError, match='align_type'):
        make_batch(train, tok, align_type='title_align')
    # only some examples carry the key: the reference's assertion; an alignment that is no pair: its other one
    del train['pos_texts'][1]['abs_align']
    with pytest.raises(AssertionError):
        make_batch(train, tok, align_type='abs_align')
    train['pos_texts'][1]['abs_align'] = [1, 2, 3]
    with pytest.raises(AssertionError):
        make_batch(train, tok, align_type='abs_align')


def test_sent_cdist_abi_and_operator_surface():
    from aspire_amd import _lib, cross_doc_l1, pair_distances as pd
    import aspire_amd.torch_ops as to
    ptr, rs = ctypes.c_void_p, ctypes.POINTER(_lib.RepSet)
    assert _lib.SIGNATURES['aspire_sent_cdist_f32'] == (ctypes.c_int, [rs, rs, ctypes.c_int64, ptr, ptr])
    assert _lib.SIGNATURES['aspire_sent_cdist_backward_f32'] == (ctypes.c_int, [rs, rs, ctypes.c_int64, ptr, ptr, ptr, ptr])
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'aspire_hip.h')).read()
    for name in ('aspire_sent_cdist_f32', 'aspire_sent_cdist_backward_f32'):
        assert name in header and hasattr(_lib.lib, name)
    assert 'disent_models.py:653-659' in header and ':826-835' in header
    for name in ('sent_cdist', 'sent_cdist_backward'):
        assert name in to.OPS and hasattr(torch.ops.aspire, name) and f'torch.ops.aspire.{name}(' in to.__doc__
    assert len(set(to.OPS)) == len(to.OPS)
    assert str(torch.ops.aspire.sent_cdist.default._schema) == 'aspire::sent_cdist(Tensor q, Tensor q_lens, Tensor c, Tensor c_lens) -> Tensor'
    assert str(torch.ops.aspire.sent_cdist_backward.default._schema) == \
        'aspire::sent_cdist_backward(Tensor grad_dist, Tensor q, Tensor q_lens, Tensor c, Tensor c_lens) -> (Tensor, Tensor)'
    # argument checks that need no device: unequal batch sizes, CSR sets, another encoding dim, too many rows
    q, c = _lib.RepSet(0, 0, 0, 2, 4, 4), _lib.RepSet(0, 0, 0, 3, 4, 4)
    call = lambda a, b, d=768, p=None: _lib.lib.aspire_sent_cdist_f32(ctypes.byref(a), ctypes.byref(b), d, p, None)
    back = lambda a, b, d=768, p=None: _lib.lib.aspire_sent_cdist_backward_f32(ctypes.byref(a), ctypes.byref(b), d, p, p, p, None)
    for fn in (call, back):
        assert fn(q, c) == _lib.ASPIRE_ERR_INVALID_ARG
        assert fn(q, q, 512) == _lib.ASPIRE_ERR_UNSUPPORTED
        assert fn(q, _lib.RepSet(0, 0, 0, 2, 0, 4)) == _lib.ASPIRE_ERR_INVALID_ARG and b'padded' in _lib.lib.aspire_last_error()
        assert fn(q, q) == _lib.ASPIRE_ERR_INVALID_ARG and b'null' in _lib.lib.aspire_last_error()
        assert fn(_lib.RepSet(0, 0, 0, 2, 129, 129), q, p=16) == _lib.ASPIRE_ERR_UNSUPPORTED and b'128' in _lib.lib.aspire_last_error()   # (refused before any launch)
        empty = _lib.RepSet(0, 0, 0, 0, 4, 4)
        assert fn(empty, empty) == _lib.ASPIRE_OK
    # shapes propagate without a device; CPU tensors are refused by the dispatcher, the host layer asks for a GPU
    q, c = torch.empty(3, 5, 768, device='meta'), torch.empty(3, 2, 768, device='meta')
    lens = torch.empty(3, dtype=torch.int32, device='meta')
    assert torch.ops.aspire.sent_cdist(q, lens, c, lens).shape == (3, 5, 2)
    gq, gc = torch.ops.aspire.sent_cdist_backward(torch.empty(3, 5, 2, device='meta'), q, lens, c, lens)
    assert gq.shape == q.shape and gc.shape == c.shape
    with pytest.raises(NotImplementedError):
        torch.ops.aspire.sent_cdist(torch.zeros(1, 2, 768), torch.ones(1, dtype=torch.int32), torch.zeros(1, 2, 768), torch.ones(1, dtype=torch.int32))
    if not torch.cuda.is_available():
        reps = pd.rep_len_tup(embed=torch.zeros(1, 768, 2), abs_lens=[2])
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            cross_doc_l1(reps, reps)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            pd.sent_cdist(reps, reps)


def _train_hparams():
    return dict(es_check_every=1000, train_size=6, batch_size=3, num_epochs=1, update_rule='adam', learning_rate=1e-3,
                lr_decay_method='exponential', decay_lr_by=0.7, decay_lr_every=1)


def test_rank_trainer_picks_the_loss_by_model_name(tmp_path):
    from aspire_amd import RankLoss, RankTrainer, SupAlignRankLoss
    enc = torch.nn.Linear(3, 1)

    def trainer(model_hparams, **kw):
        return RankTrainer(enc, model_hparams, _train_hparams(), str(tmp_path), lambda epoch: [],
                           optimizer=torch.optim.SGD(enc.parameters(), lr=0.1), **kw)

    sup = trainer(dict(si.CASES['ot_train'][2]))
    assert isinstance(sup.loss_fn.__self__, SupAlignRankLoss) and sup.loss_fn.__func__ is SupAlignRankLoss.forward_rank
    assert sup.loss_fn.__self__.sentsup_loss_prop == 1.0 and sup.loss_fn.__self__.score_agg_type == 'l2wasserstein'
    with pytest.raises(KeyError, match='sentsup_loss_prop'):
        trainer({'model_name': 'sbalisentbienc', 'score_aggregation': 'l2max'})
    for hp in ({'score_aggregation': 'l2max'}, {'score_aggregation': 'l2max', 'model_name': 'miswordbienc', 'sentsup_loss_prop': 1.0}):
        plain = trainer(hp)
        assert type(plain.loss_fn.__self__) is RankLoss
    stub = lambda batch, encoder: None
    assert trainer({'model_name': 'sbalisentbienc'}, loss_fn=stub).loss_fn is stub        # a caller's loss is never replaced
