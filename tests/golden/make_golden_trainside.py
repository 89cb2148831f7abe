"""Generate tests/golden/trainside.npz by RUNNING THE REFERENCE'S OWN CODE under fp32 autograd: the gradient of the joint soft-max
alignment score, and the supervised-alignment distances l2sup / l2sup_weighted with their gradients.

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_trainside.py
The fixture is data (seeds' outputs, errors, a few gradients); no reference source is copied.

What executes from the reference:
  src/learning/facetid_models/pair_distances.py   allpair_joint_sm_negscore (:348-402), allpair_masked_dist_l2sup (:189-235),
                                                  allpair_masked_dist_l2sup_weighted (:238-292)
  src/learning/models_common/activations.py       masked_2d_softmax (:35-61)

Inputs are regenerated from seeds (jointsm_inputs.case_inputs, trainside_inputs.l2sup_inputs), here and in the tests.  Per case the
fixture holds the upstream gradient gs [B] (loss = sum_b gs[b] * similarity_b: the reference returns distances, so its loss here is
sum_b gs[b] * -distance_b), `ref_err`: the largest absolute deviation of the reference's fp32 gradient from float64 autograd over the
closed form (trainside_inputs.jointsm_grad64 / l2sup_ref64) over valid rows, and `max_grad`: the largest absolute float64 gradient
entry; for the l2sup cases also the reference's fp32 distances with `dist_err` / `max_dist` made the same way.  The reference's
gradients themselves are kept for the small cases only.  Pad-row gradients of the reference are asserted to be exactly 0.
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference on sys.path, stubs geomloss)
import trainside_inputs as ti  # noqa: E402

ref_pd = importlib.import_module('src.learning.facetid_models.pair_distances')
ref_dm = importlib.import_module('src.learning.facetid_models.disent_models')


def _leaf(x):
    """[B, S, 768] float32 -> a leaf in the reference's [B, 768, S] layout."""
    return torch.from_numpy(x).permute(0, 2, 1).contiguous().requires_grad_(True)


def _rows(t):
    return t.grad.permute(0, 2, 1).contiguous().numpy()


def _valid_err(got, want, lens):
    return max(float(np.max(np.abs(got[b, :n] - want[b, :n]))) for b, n in enumerate(lens))


def _pads_zero(g, lens):
    return all(np.all(g[b, n:] == 0.0) for b, n in enumerate(lens))


def make_jointsm(out):
    for name, spec in ti.CASES.items():
        q, c, qlens, clens = ti.case_inputs(spec)
        gs = ti.jointsm_upstream(name, spec)
        qt, ct = _leaf(q), _leaf(c)
        neg = ref_pd.allpair_joint_sm_negscore(query=mg.RepLen(embed=qt, abs_lens=qlens), cand=mg.RepLen(embed=ct, abs_lens=clens))
        (-neg * torch.from_numpy(gs)).sum().backward()
        gq, gc = _rows(qt), _rows(ct)
        assert _pads_zero(gq, qlens) and _pads_zero(gc, clens), name
        wq, wc = ti.jointsm_grad64(q, c, qlens, clens, gs)
        err = max(_valid_err(gq, wq, qlens), _valid_err(gc, wc, clens))
        top = max(float(np.abs(wq).max()), float(np.abs(wc).max()))
        out[f'jointsm_{name}_gs'] = gs
        out[f'jointsm_{name}_ref_err'] = np.float64(err)
        out[f'jointsm_{name}_max_grad'] = np.float64(top)
        if name in ti.STORE_JOINTSM_GRADS:
            out[f'jointsm_{name}_grad_q'] = gq
            out[f'jointsm_{name}_grad_c'] = gc
        print(f'jointsm {name:6s} ref err {err:.3e}  max grad {top:.3e}  relative {err / top:.2e}  bound {ti.bound(err, top):.3e}')


def make_l2sup(out):
    ali = ref_dm.rep_len_ali_tup
    for name, spec in ti.L2SUP_CASES.items():
        q, c, qlens, clens, align, gs = ti.l2sup_inputs(spec)
        for weighted, fn in ((0, ref_pd.allpair_masked_dist_l2sup), (1, ref_pd.allpair_masked_dist_l2sup_weighted)):
            qt, ct = _leaf(q), _leaf(c)
            # (the reference writes the clipped indices back into the list it is given: a copy)
            dist = fn(query=mg.RepLen(embed=qt, abs_lens=qlens), cand=ali(embed=ct, abs_lens=clens, align_idxs=copy.deepcopy(align)))
            (-dist * torch.from_numpy(gs)).sum().backward()
            gq, gc = _rows(qt), _rows(ct)
            assert _pads_zero(gq, qlens) and _pads_zero(gc, clens), name
            wd, wq, wc = ti.l2sup_ref64(q, c, qlens, clens, align, weighted, gs)
            dist = dist.detach().numpy()
            err = max(_valid_err(gq, wq, qlens), _valid_err(gc, wc, clens))
            top = max(float(np.abs(wq).max()), float(np.abs(wc).max()))
            key = f'l2sup_{name}_w{weighted}'
            out[f'{key}_dist'] = dist
            out[f'{key}_dist_err'] = np.float64(np.max(np.abs(dist - wd)))
            out[f'{key}_max_dist'] = np.float64(np.max(np.abs(wd)))
            out[f'{key}_ref_err'] = np.float64(err)
            out[f'{key}_max_grad'] = np.float64(top)
            if name in ti.STORE_L2SUP_GRADS:
                out[f'{key}_grad_q'] = gq
                out[f'{key}_grad_c'] = gc
            print(f'l2sup {name:6s} w{weighted} dist {dist.min():.4g} .. {dist.max():.4g} err {float(out[key + "_dist_err"]):.2e}  '
                  f'grad ref err {err:.3e}  max grad {top:.3e}  bound {ti.bound(err, top):.3e}')
        out[f'l2sup_{name}_gs'] = gs


if __name__ == '__main__':
    torch.set_num_threads(4)
    out = {}
    make_jointsm(out)
    make_l2sup(out)
    out['jointsm_cases'] = np.array(list(ti.CASES))
    out['l2sup_cases'] = np.array(list(ti.L2SUP_CASES))
    path = os.path.join(HERE, 'trainside.npz')
    np.savez_compressed(path, **out)
    print('trainside.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000 * 1000
