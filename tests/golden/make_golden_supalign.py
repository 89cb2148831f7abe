"""Generate tests/golden/supalign.npz and supalign_prep.json by RUNNING THE REFERENCE'S OWN CODE on the CPU: the sup-alignment rank loss
(WordSentAbsSupAlignBiEnc.forward_rank) under fp32 autograd from last_hidden_state to the loss and back, and the pre-aligned batcher.

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_supalign.py
The fixtures are data (losses, the permutation used, the alignment lists as the reference left them, errors, a few gradients; the
batcher's outputs); no reference source is copied.

What executes from the reference:
  src/learning/facetid_models/disent_models.py    WordSentAbsSupAlignBiEnc.forward_rank (:750-837) with partial_forward / sent_reps_bert of
                                                  its parents; __init__ is bypassed and bert_encoder replaced by a stub that hands out
                                                  leaf last_hidden_state tensors (make_golden_readout._Encoder)
  src/learning/facetid_models/pair_distances.py   allpair_masked_dist_l2sup, allpair_masked_dist_l2sup_weighted (with their in-place
                                                  clipping of the alignment lists), allpair_masked_dist_l2max
  src/learning/batchers.py                        AbsSentTokBatcherPreAlign.make_batch (:642-746) and, for a feed without alignments,
                                                  AbsSentTokBatcher.make_batch (:462-523), over make_golden.make_tokenizer's tokenizer

(criterion_sent / criterion_sentsup are nn.TripletMarginWithDistanceLoss's arithmetic spelled out, as in make_golden_readout.py: the
installed torch's module refuses the reference's RepLen tuples.  It calls the distance of the positive first, then of the negative.)

'l2wasserstein' has no reference here (geomloss is absent): its dist_function in the reference's forward_rank is the fp32 run of the
restatement the OT backward's tests use (ot_backward_ref.restated_distance, distances from direct differences), as in
make_golden_readout.py; the sentsup, abstract and singular-value terms of those cases are the reference's own all the same.

Per case the fixture holds `loss` (the reference's fp32 value), `loss_err` = |loss - float64 yardstick| with `max_loss`, `ref_err` = the
largest absolute deviation of the reference's fp32 hidden-state gradients from float64 autograd over the restatement
(supalign_inputs.supalign_loss64) with `max_grad`, `perm`, for the train cases `neg_align` (the negatives' alignment lists after the
reference's two calls) and `active` (the share of triples with an active hinge, per term), and for the small cases the gradients.

Asserted here, and recorded as `conditions`: in every case at least half of the triples have an active hinge in each term that is
switched on, and no hinge argument lies within 1e-3 of the kink; a train case has an alignment index beyond a document's length; a
train case has a negative whose query index is at or beyond q_lens[perm[i]] with a longer query of its own (the write-back quirk
changes what is read); a case has weighted_sup; there is a dev case; the float64 yardstick's own negative-index rule gives the lists
the reference left.
"""
import importlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference on sys.path, stubs geomloss)
import make_golden_readout as mgr  # noqa: E402
import readout_inputs as ri  # noqa: E402
import supalign_inputs as si  # noqa: E402
import ot_backward_ref  # noqa: E402

ref_pd = importlib.import_module('src.learning.facetid_models.pair_distances')
ref_dm = importlib.import_module('src.learning.facetid_models.disent_models')


def _model(hp, enc):
    cls = ref_dm.WordSentAbsSupAlignBiEnc
    model = cls.__new__(cls)
    torch.nn.Module.__init__(model)
    model.bert_encoding_dim = ri.D
    model.bert_encoder = enc
    if hp['score_aggregation'] == 'l2wasserstein':
        def dist(query, cand):
            return ot_backward_ref.restated_distance(query.embed.permute(0, 2, 1), cand.embed.permute(0, 2, 1), query.abs_lens, cand.abs_lens,
                                                     blur=hp['geoml_blur'], scaling=hp['geoml_scaling'], temp=hp['sent_sm_temp'], direct=True)
    else:
        dist = {'l2max': ref_pd.allpair_masked_dist_l2max}[hp['score_aggregation']]
    sup = ref_pd.allpair_masked_dist_l2sup_weighted if hp.get('weighted_sup', False) else ref_pd.allpair_masked_dist_l2sup
    model.dist_function = dist
    model.criterion_sent = lambda a, p, n: torch.clamp_min(1.0 + dist(a, p) - dist(a, n), 0).sum()
    model.criterion_sentsup = lambda a, p, n: torch.clamp_min(1.0 + sup(a, p) - sup(a, n), 0).sum()
    model.criterion_abs = torch.nn.TripletMarginLoss(margin=1, p=2, reduction='sum')
    # the reads of WordSentAbsSupAlignBiEnc.__init__ (:714-717)
    model.abs_loss_prop = float(hp.get('abs_loss_prop', 0.0))
    model.sent_loss_prop = float(hp.get('sent_loss_prop', 0.0))
    model.sentsup_loss_prop = float(hp['sentsup_loss_prop'])
    model.cd_svalue_l1_prop = float(hp.get('cd_svalue_l1_prop', 0.0))
    return model


def make_rank(out):
    cond = dict(clip=False, quirk=False, weighted=False, dev=False)
    for name, (size, dev, hp) in si.CASES.items():
        inp = si.rank_inputs(size)
        enc = mgr._Encoder()
        batch = {}
        for w, key in (('q', 'query'), ('p', 'pos'), ('n', 'neg'))[:3 if dev else 2]:
            batch[key + '_bert_batch'] = enc.batch(inp[w + '_hidden'])
            batch[key + '_abs_lens'] = list(inp[w + '_lens'])
            batch[key + '_senttok_idxs'] = inp[w + '_idxs']
        batch['pos_align_idxs'] = [list(a) for a in inp['align']]       # the reference clips these in place
        real_randperm = torch.randperm
        torch.randperm = lambda n, *a, **k: torch.tensor(inp['perm'], dtype=torch.long)     # the permutation of the fixture
        try:
            loss = _model(hp, enc).forward_rank(batch)
        finally:
            torch.randperm = real_randperm
        loss.backward()
        grads = [t.grad.numpy() for t in enc.leaves]
        want_loss, want, parts = si.supalign_loss64(inp, dev, hp)
        active = {}
        for term, h in parts.items():
            assert np.abs(h).min() > 1e-3, (name, term, h)
            active[term] = float((h > 0).mean())
            assert active[term] >= 0.5, (name, term, h)
        q_lens, p_lens, perm, align = inp['q_lens'], inp['p_lens'], inp['perm'], inp['align']
        if dev:
            cond['dev'] = True
            assert batch['pos_align_idxs'] == align, 'the dev branch does not touch the alignments'
        else:
            left = [batch['pos_align_idxs'][j] for j in perm]      # neg_align_idxs: the same inner lists, after both calls
            assert left == si.negative_align(align, perm, q_lens, p_lens), (name, left)
            out[f'{name}_neg_align'] = np.array(left, dtype=np.int64)
            cond['clip'] |= any(a[0] > q_lens[b] - 1 or a[1] > p_lens[b] - 1 for b, a in enumerate(align))
            cond['quirk'] |= any(align[j][0] >= q_lens[j] and min(align[j][0], q_lens[i] - 1) != left[i][0] for i, j in enumerate(perm))
            cond['weighted'] |= bool(hp.get('weighted_sup', False))
        err = max(float(np.abs(g - w).max()) for g, w in zip(grads, want))
        top = max(float(np.abs(w).max()) for w in want)
        assert abs(float(loss.item()) - want_loss) <= 1e-4 * max(1.0, abs(want_loss)), (name, loss.item(), want_loss)
        assert err <= 1e-4 * top, (name, err, top)
        out[f'{name}_loss'] = np.float32(loss.item())
        out[f'{name}_loss_err'] = np.float64(abs(float(loss.item()) - want_loss))
        out[f'{name}_max_loss'] = np.float64(abs(want_loss))
        out[f'{name}_ref_err'] = np.float64(err)
        out[f'{name}_max_grad'] = np.float64(top)
        out[f'{name}_perm'] = np.array(perm, dtype=np.int64)
        out[f'{name}_active'] = np.array(json.dumps(active))
        if name in si.SMALL_CASES:
            for g, key in zip(grads, 'qpn'):
                out[f'{name}_grad_{key}'] = g
        print(f'{name:24s} loss {loss.item():10.5f} err {abs(loss.item() - want_loss):.2e}  grad ref err {err:.3e} max {top:.3e} '
              f'bound {ri.bound(err, top):.3e}  active {active}')
    assert all(cond.values()), cond
    out['conditions'] = np.array(json.dumps(cond))
    # the quirk changes the loss: without the write-back the negative of some triple reads another sentence
    assert any(si.negative_align(si.ALIGN[s], ri.SIZES[s]['perm'], ri.SIZES[s]['q_lens'], ri.SIZES[s]['p_lens'])
               != [[min(si.ALIGN[s][j][0], ri.SIZES[s]['q_lens'][i] - 1), min(si.ALIGN[s][j][1], ri.SIZES[s]['p_lens'][j] - 1)]
                   for i, j in enumerate(ri.SIZES[s]['perm'])] for s in si.ALIGN)


def make_prep():
    ref_b = importlib.import_module('src.learning.batchers')
    with open(os.path.join(HERE, 'prep.json')) as f:
        docs = json.load(f)['docs']
    cases = {}
    with tempfile.TemporaryDirectory() as td:
        tok = mg.make_tokenizer(td)
        for name, spec in si.PREP_FEEDS.items():
            feed = si.prep_feed(docs, spec)
            carries = any(spec['align_type'] in ex for exs in feed.values() for ex in exs)
            batcher = ref_b.AbsSentTokBatcherPreAlign if carries or 'pos_texts' not in feed else ref_b.AbsSentTokBatcher
            ref_b.AbsSentTokBatcherPreAlign.align_type = spec['align_type']
            got = batcher.make_batch(feed, tok)
            cases[name] = {k: ({kk: (vv.tolist() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} if isinstance(v, dict) else v)
                           for k, v in got.items()}
            print('prep', name, sorted(cases[name]))
    with open(os.path.join(HERE, 'supalign_prep.json'), 'w') as f:
        json.dump({'cases': cases}, f)
    print('supalign_prep.json', os.path.getsize(os.path.join(HERE, 'supalign_prep.json')), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(4)
    out = {}
    make_rank(out)
    out['cases'] = np.array(list(si.CASES))
    path = os.path.join(HERE, 'supalign.npz')
    np.savez_compressed(path, **out)
    print('supalign.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000 * 1000
    make_prep()
