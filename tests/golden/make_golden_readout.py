"""Generate tests/golden/readout.npz by RUNNING THE REFERENCE'S OWN CODE under fp32 autograd on the CPU: the read-out
(WordSentAlignBiEnc.sent_reps_bert) and the rank loss (WordSentAbsAlignBiEnc.forward_rank), from last_hidden_state to the loss and back.

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_readout.py
The fixture is data (losses, the permutation used, errors, a few gradients); no reference source is copied.

What executes from the reference:
  src/learning/facetid_models/disent_models.py    WordSentAlignBiEnc.sent_reps_bert (:487-535), partial_forward (:470-485),
                                                  WordSentAbsAlignBiEnc.forward_rank (:587-660); __init__ is bypassed and bert_encoder
                                                  replaced by a stub that hands out leaf last_hidden_state tensors
  src/learning/facetid_models/pair_distances.py   allpair_masked_dist_l2max, allpair_masked_dist_l2topk, AllPairMaskedAttention,
                                                  allpair_joint_sm_negscore -- the dist_function of the run

(criterion_sent is nn.TripletMarginWithDistanceLoss's arithmetic spelled out -- clamp_min(margin + d(a, p) - d(a, n), 0).sum() --
since the installed torch's module reads .ndim of its inputs and refuses the reference's RepLen tuples.)

Inputs are regenerated from seeds (readout_inputs), here and in the tests.  Per case the fixture holds `loss` (the reference's fp32
value), `loss_err` = |loss - float64 yardstick| with `max_loss`, `ref_err` = the largest absolute deviation of the reference's fp32
hidden-state gradients from float64 autograd over the restatement (readout_inputs.rank_loss64) with `max_grad`, the permutation of the
in-batch cases, and for the small cases the gradients themselves.  'l2wasserstein' has no reference here (geomloss is absent): its
dist_function in the reference's forward_rank is the fp32 run of the restatement the OT backward's tests use (distances from direct
differences), so its ref_err is that restatement's fp32 error, as in tests/test_gpu_ot_backward.py; 'jointsm' runs the reference's
allpair_joint_sm_negscore against the float64 closed form of trainside_inputs.py.

Asserted about the inputs: every hinge has an active and an inactive triple, no triple lies within 1e-3 of the kink, no arg-max /
top-2 pick within 1e-3 of a tie.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference on sys.path, stubs geomloss)
import readout_inputs as ri  # noqa: E402
import ot_backward_ref  # noqa: E402

ref_pd = importlib.import_module('src.learning.facetid_models.pair_distances')
ref_dm = importlib.import_module('src.learning.facetid_models.disent_models')


class _Encoder:
    """bert_encoder's stand-in: tokid_tt carries the batch's number, the answer is that batch's leaf"""

    def __init__(self):
        self.leaves = []

    def batch(self, hidden):
        leaf = torch.from_numpy(hidden).clone().requires_grad_(True)
        self.leaves.append(leaf)
        b, l, _ = hidden.shape
        ids = torch.full((b, l), len(self.leaves) - 1, dtype=torch.long)
        return {'tokid_tt': ids, 'seg_tt': torch.zeros_like(ids), 'attnmask_tt': torch.ones_like(ids), 'seq_lens': [l] * b}

    def __call__(self, tokid_tt, token_type_ids=None, attention_mask=None):
        return types.SimpleNamespace(last_hidden_state=self.leaves[int(tokid_tt[0, 0])])


def _model(agg, prop, enc):
    model = ref_dm.WordSentAbsAlignBiEnc.__new__(ref_dm.WordSentAbsAlignBiEnc)
    torch.nn.Module.__init__(model)
    model.bert_encoding_dim = ri.D
    model.bert_encoder = enc
    hp = ri.hparams(agg, prop)
    if agg == 'l2wasserstein':
        def dist(query, cand):
            return ot_backward_ref.restated_distance(query.embed.permute(0, 2, 1), cand.embed.permute(0, 2, 1), query.abs_lens, cand.abs_lens,
                                                     blur=hp['geoml_blur'], scaling=hp['geoml_scaling'], temp=hp['sent_sm_temp'], direct=True)
    else:
        dist = {'l2max': ref_pd.allpair_masked_dist_l2max, 'l2top2': ref_pd.allpair_masked_dist_l2topk,
                'l2attention': ref_pd.AllPairMaskedAttention(hp).compute_distance, 'jointsm': ref_pd.allpair_joint_sm_negscore}[agg]
    model.dist_function = dist
    # nn.TripletMarginWithDistanceLoss(distance_function=dist, margin=1.0, reduction='sum') of the torch the reference pins; this
    # torch's reads .ndim of its inputs and so no longer takes the reference's RepLen tuples: its arithmetic, spelled out
    model.criterion_sent = lambda a, p, n: torch.clamp_min(1.0 + dist(a, p) - dist(a, n), 0).sum()
    model.criterion_abs = torch.nn.TripletMarginLoss(margin=1, p=2, reduction='sum')
    model.abs_loss_prop, model.sent_loss_prop, model.cd_l1_prop = float(prop), 1.0, 0.0
    return model


def make_rank(out):
    for name, (size, agg, neg, prop) in ri.RANK_CASES.items():
        inp = ri.rank_inputs(size)
        enc = _Encoder()
        batch = {}
        for w, key in (('q', 'query'), ('p', 'pos'), ('n', 'neg'))[:3 if neg else 2]:
            batch[key + '_bert_batch'] = enc.batch(inp[w + '_hidden'])
            batch[key + '_abs_lens'] = list(inp[w + '_lens'])
            batch[key + '_senttok_idxs'] = inp[w + '_idxs']
        real_randperm = torch.randperm
        torch.randperm = lambda n, *a, **k: torch.tensor(inp['perm'], dtype=torch.long)     # the permutation of the fixture
        try:
            loss = _model(agg, prop, enc).forward_rank(batch)
        finally:
            torch.randperm = real_randperm
        loss.backward()
        grads = [t.grad.numpy() for t in enc.leaves]
        want_loss, want, parts = ri.rank_loss64(inp, agg, neg, prop)
        hinges = [parts['sent']] + ([parts['doc']] if prop > 0 else [])
        for h in hinges:
            assert (h > 0).any() and (h < 0).any(), (name, h)
            assert np.abs(h).min() > 1e-3, (name, h)
        gap = ri.pick_margin(inp, neg)
        assert gap > 1e-3, (name, gap)
        for g, w, key in zip(grads, want, 'qpn'):       # tokens of no span, position 0 aside: the reference's gradient is exact zeros
            for b, doc in enumerate(inp[key + '_idxs']):
                free = sorted(set(range(1, inp['L'])) - {t for span in doc for t in span})
                assert not g[b, free].any() and not w[b, free].any(), name
        err = max(float(np.abs(g - w).max()) for g, w in zip(grads, want))
        top = max(float(np.abs(w).max()) for w in want)
        out[f'{name}_loss'] = np.float32(loss.item())
        out[f'{name}_loss_err'] = np.float64(abs(float(loss.item()) - want_loss))
        out[f'{name}_max_loss'] = np.float64(abs(want_loss))
        out[f'{name}_ref_err'] = np.float64(err)
        out[f'{name}_max_grad'] = np.float64(top)
        out[f'{name}_perm'] = np.array(inp['perm'], dtype=np.int64)
        if name in ri.SMALL_CASES:
            for g, key in zip(grads, 'qpn'):
                out[f'{name}_grad_{key}'] = g
        print(f'{name:26s} loss {loss.item():10.5f} err {abs(loss.item() - want_loss):.2e}  grad ref err {err:.3e} max {top:.3e} '
              f'bound {ri.bound(err, top):.3e}  hinge {np.round(parts["sent"], 3)}  pick gap {gap:.3g}')


def make_pool(out):
    """the reference's sent_reps_bert under fp32 autograd on the cases in its own span layout (disjoint runs; 'c' lists positions
    twice, which its mask cannot express: that case is held to the stated order bit for bit instead)"""
    model = _model('l2max', 0.0, None)
    for name in ('a', 'b', 'd'):
        case = ri.pool_case(name)
        enc = _Encoder()
        model.bert_encoder = enc
        hidden = np.random.RandomState(900).standard_normal((case['B'], case['L'], ri.D)).astype(np.float32)
        lens = [len(doc) for doc in case['spans']]
        cls, sent = model.sent_reps_bert(enc.batch(hidden), case['spans'], lens)
        sent = sent.reshape(case['B'], -1, ri.D)
        ((sent * torch.from_numpy(case['gs'][:, :sent.shape[1]])).sum() + (cls.reshape(case['B'], ri.D) * torch.from_numpy(case['gc'])).sum()).backward()
        got, want = enc.leaves[0].grad.numpy(), ri.pool_grad64(case)
        out[f'pool_{name}_ref_err'] = np.float64(np.abs(got - want).max())
        out[f'pool_{name}_max_grad'] = np.float64(np.abs(want).max())
        print(f'pool {name}: ref err {float(out[f"pool_{name}_ref_err"]):.3e} max grad {float(out[f"pool_{name}_max_grad"]):.3e}')


def make_cls(out):
    for name in ('b5', 'same', 'b1'):
        q, c, g = ri.cls_case(name)
        d32, q32, c32 = ri.cls_ref(q, c, g, torch.float32)
        d64, q64, c64 = ri.cls_ref(q, c, g, torch.float64)
        out[f'cls_{name}_ref_err'] = np.float64(max(np.abs(q32 - q64).max(), np.abs(c32 - c64).max()))
        out[f'cls_{name}_max_grad'] = np.float64(np.abs(q64).max())
        print(f'cls {name}: dist {d64.min():.4g} .. {d64.max():.4g}  ref err {float(out[f"cls_{name}_ref_err"]):.3e}')


if __name__ == '__main__':
    torch.set_num_threads(4)
    out = {}
    make_pool(out)
    make_cls(out)
    make_rank(out)
    out['rank_cases'] = np.array(list(ri.RANK_CASES))
    path = os.path.join(HERE, 'readout.npz')
    np.savez_compressed(path, **out)
    print('readout.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000 * 1000
