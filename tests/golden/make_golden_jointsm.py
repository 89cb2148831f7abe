"""Generate tests/golden/jointsm.npz by RUNNING THE REFERENCE'S OWN CODE: the joint soft-max alignment score.

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_jointsm.py
The fixture is data (seeds + expected outputs); no reference source is copied.

What executes from the reference:
  src/learning/facetid_models/pair_distances.py   allpair_joint_sm_negscore (:348-402)
  src/learning/models_common/activations.py       masked_2d_softmax (:35-61)
  src/learning/facetid_models/disent_models.py    WordSentAlignPolyEnc.score (:877-925)

To keep the fixture small it holds SEEDS AND OUTPUTS, not inputs: jointsm_inputs.py (beside this file) regenerates a case's rows from
numpy.random.RandomState(seed), here and in the tests.  Per case the fixture holds the reference's fp32 scores (similarities: minus
what allpair_joint_sm_negscore returns), its pair_sm for the small cases, and the reference's OWN error against the float64 closed
form 2 sum_ij p_ij d_ij on the same fp32 inputs (max relative score error, relative to max(|score|, 1); max absolute pair_sm error):
the tests hold the kernels to twice that.  For the pools (WordSentAlignPolyEnc.score's outputs) it also checks, here on the CPU,
that the reference's own fp32 ranking leaves the float64 ranking only between candidates closer than its own error -- and in no
more than POOL_SWAP_CAP of the adjacent pairs: the cap the end-to-end test applies to the kernels.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference on sys.path, stubs geomloss)
from jointsm_inputs import CASES, POOLS, POOL_SWAP_CAP, case_inputs, closed_form, pool_inputs  # noqa: E402

ref_pd = importlib.import_module('src.learning.facetid_models.pair_distances')
ref_dm = importlib.import_module('src.learning.facetid_models.disent_models')


def make_jointsm():
    out = {}
    for name, spec in CASES.items():
        q, c, qlens, clens = case_inputs(spec)
        qt = mg.RepLen(embed=torch.from_numpy(q).permute(0, 2, 1), abs_lens=qlens)
        ct = mg.RepLen(embed=torch.from_numpy(c).permute(0, 2, 1), abs_lens=clens)
        neg = ref_pd.allpair_joint_sm_negscore(query=qt, cand=ct)
        neg2, pair_sm = ref_pd.allpair_joint_sm_negscore(query=qt, cand=ct, return_pair_sims=True)
        assert torch.equal(neg, neg2)
        scores, pair_sm = (-neg).numpy(), pair_sm.numpy()
        want, want_sm = closed_form(q, c, qlens, clens)
        err = float(np.max(np.abs(scores - want) / np.maximum(np.abs(want), 1.0)))
        err_sm = float(np.max(np.abs(pair_sm - want_sm)))
        assert all(np.all(pair_sm[b, ql:, :] == 0.0) and np.all(pair_sm[b, :, cl:] == 0.0) for b, (ql, cl) in enumerate(zip(qlens, clens)))
        for k in ('seed', 'shape', 'qlens', 'clens', 'scale', 'dup'):
            out[f'{name}_{k}'] = np.asarray(spec[k] if k not in ('qlens', 'clens') else {'qlens': qlens, 'clens': clens}[k])
        out[f'{name}_scores'] = scores
        out[f'{name}_ref_err'] = np.float64(err)
        out[f'{name}_ref_err_sm'] = np.float64(err_sm)
        if q.shape[1] * c.shape[1] <= 64:
            out[f'{name}_pair_sm'] = pair_sm
        print(f'{name:8s} scores {scores.min():9.2f} .. {scores.max():9.2f}  ref err {err:.2e}  pair_sm err {err_sm:.2e}  '
              f'max p {max(want_sm[b].max() for b in range(len(qlens))):.3f}')
    for name, spec in POOLS.items():
        query, cands = pool_inputs(spec)
        ret = ref_dm.WordSentAlignPolyEnc.score(query_reps=query, cand_reps=cands)
        scores = np.asarray(ret['batch_scores'], dtype=np.float32)
        want = np.array([closed_form(query[None], cd[None], [len(query)], [len(cd)])[0][0] for cd in cands])
        err = float(np.max(np.abs(scores - want) / np.maximum(np.abs(want), 1.0)))
        # the reference's own ranking against the float64 one: a swap only between candidates its error cannot tell apart
        order64 = sorted(range(len(want)), key=lambda i: want[i], reverse=True)
        order32 = sorted(range(len(scores)), key=lambda i: scores[i], reverse=True)
        close = sum(1 for a, b in zip(order64[:-1], order64[1:]) if abs(want[a] - want[b]) < 2 * err * max(abs(want[a]), 1.0))
        for a, b in zip(order32[:-1], order32[1:]):
            assert want[a] >= want[b] or abs(want[a] - want[b]) < 2 * err * max(abs(want[a]), 1.0), (name, a, b)
        assert close <= POOL_SWAP_CAP * (len(want) - 1), (name, close)
        for k in ('seed', 'qlen', 'clens', 'scale'):
            out[f'{name}_{k}'] = np.asarray(spec[k])
        out[f'{name}_scores'] = scores
        out[f'{name}_ref_err'] = np.float64(err)
        for i in spec['keep_pair_scores']:
            out[f'{name}_pair_scores_{i}'] = np.asarray(ret['pair_scores'][i], dtype=np.float32)
        print(f'{name:8s} {len(cands)} candidates  scores {scores.min():9.2f} .. {scores.max():9.2f}  ref err {err:.2e}  '
              f'indistinguishable neighbours {close}  fp32 order == fp64 order: {order32 == order64}')
    out['cases'] = np.array(list(CASES))
    out['pools'] = np.array(list(POOLS))
    np.savez_compressed(os.path.join(HERE, 'jointsm.npz'), **out)
    print('jointsm.npz', os.path.getsize(os.path.join(HERE, 'jointsm.npz')), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(4)
    make_jointsm()
