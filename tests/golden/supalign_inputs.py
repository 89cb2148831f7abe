"""Inputs and float64 yardsticks of the sup-alignment fixture (tests/golden/supalign.npz, supalign_prep.json): the rank loss of
WordSentAbsSupAlignBiEnc.forward_rank (disent_models.py:750-837) from last_hidden_state to the loss and back, the cross-document
distance matrix behind its regularisers, and the raw feeds of the pre-aligned batcher.  Shared by make_golden_supalign.py (which runs
the reference on these inputs and records its own fp32 error against the yardsticks) and by the tests (which hold the kernels to a
bound made of that error: trainside_inputs.bound).  Everything is regenerated from seeds.

The hidden states, sentence spans and permutations are readout_inputs.rank_inputs' (the 'std' and 'small' sizes, whose seeds were
chosen for pick gaps above 1e-3); what is added are the pre-computed alignments [query sentence, positive sentence] per triple:

  std    q_lens [4, 2, 3, 2], p_lens [3, 4, 2, 2], perm [2, 0, 1, 3]
         align  [[1, 2], [5, 1], [2, 7], [0, 0]]
           triple 1: query index 5 beyond its 2 sentences (the clip); triple 2: positive index 7 beyond its 2 sentences (the clip)
           the negative of triple 2 is the positive of triple perm[2] = 1: its query index 5 was clipped IN PLACE to q_lens[1] - 1 = 1 by
           the reference's positive call, so the negative reads sentence 1 of query 2 although query 2 has sentence 2 (the write-back quirk:
           min(5, q_lens[2] - 1) alone would be 2)
  small  q_lens [2, 2], p_lens [2, 2], perm [1, 0], align [[3, 0], [0, 5]] (both clipped)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import readout_inputs as ri  # noqa: E402
from readout_inputs import D, bound  # noqa: E402,F401  (bound re-exported)
from trainside_inputs import l2sup_dists  # noqa: E402

ALIGN = {'std': [[1, 2], [5, 1], [2, 7], [0, 0]], 'small': [[3, 0], [0, 5]]}


def _hp(agg, sentsup=1.0, sent=0.0, prop=0.0, weighted=False, svalue=0.0):
    hp = dict(ri.HPARAMS, model_name='sbalisentbienc', score_aggregation=agg, sentsup_loss_prop=sentsup, sent_loss_prop=sent,
              abs_loss_prop=prop, weighted_sup=weighted)
    if svalue > 0:
        hp['cd_svalue_l1_prop'] = svalue
    return hp


# name -> (size, dev branch (explicit negatives), model_hparams); the small ones keep the reference's gradients in the fixture
CASES = {
    'l2max_train_sup': ('std', False, _hp('l2max')),                                          # the sentsup term alone (the defaults)
    'l2max_train_all': ('std', False, _hp('l2max', sentsup=0.5, sent=1.0, prop=0.5)),
    'l2max_train_w': ('std', False, _hp('l2max', sent=1.0, weighted=True)),
    'ot_train': ('std', False, _hp('l2wasserstein', sent=1.0)),                               # sbalisentbienc-misup-ot.json
    'ot_train_w_a5': ('std', False, _hp('l2wasserstein', sent=1.0, prop=0.5, weighted=True)),
    'l2max_dev_a0': ('std', True, _hp('l2max', sent=0.25)),                                   # (sent_loss_prop is not applied on the dev set)
    'l2max_dev_a5': ('std', True, _hp('l2max', sent=0.25, prop=0.5)),
    'ot_dev_a5': ('std', True, _hp('l2wasserstein', sent=1.0, prop=0.5)),
    'small_l2max_train_all': ('small', False, _hp('l2max', sentsup=0.5, sent=1.0, prop=0.5)),
    'small_l2max_train_w': ('small', False, _hp('l2max', weighted=True)),
    'small_svalue': ('small', False, _hp('l2max', sent=1.0, svalue=0.1)),
}
SMALL_CASES = tuple(n for n in CASES if n.startswith('small_'))
SVALUE_CASES = tuple(n for n, (_, _, hp) in CASES.items() if hp.get('cd_svalue_l1_prop', 0.0) > 0)


def rank_inputs(size):
    """readout_inputs.rank_inputs(size) plus 'align': the pre-computed alignments (fresh lists on every call)."""
    inp = dict(ri.rank_inputs(size))
    inp['align'] = [list(a) for a in ALIGN[size]]
    return inp


def negative_align(align, perm, q_lens, p_lens):
    """What the reference's negative call reads (the module docstring's quirk), written out on its own for the yardstick:
    -> list([q_idx, c_idx]), already clipped."""
    return [[min(align[j][0], q_lens[j] - 1, q_lens[i] - 1), min(align[j][1], p_lens[j] - 1)] for i, j in enumerate(perm)]


def svalue_reg(q, p):
    """disent_models.py:829-834 on torch tensors [B, S, 768] in their dtype (cdist from direct differences)"""
    pair_sims = -1 * torch.cdist(q, p, compute_mode='donot_use_mm_for_euclid_dist')
    return torch.linalg.svdvals(pair_sims).sum()


def supalign_loss64(inp, dev, hp, dtype=torch.float64, direct=False):
    """The loss restated with torch in `dtype` -> (loss, [grad of the query, positive(, negative) hidden states], parts): parts = the
    hinge arguments [B] of the terms that are switched on ('sup', 'sent', 'doc')."""
    hid = {w: torch.tensor(inp[w + '_hidden'], dtype=dtype, requires_grad=True) for w in (('q', 'p', 'n') if dev else ('q', 'p'))}
    reps = {w: ri.pool64(h, inp[w + '_idxs'], max(inp[w + '_lens'])) for w, h in hid.items()}
    cls = {w: h[:, 0] for w, h in hid.items()}
    lens = {w: inp[w + '_lens'] for w in ('q', 'p', 'n')}
    agg = hp['score_aggregation']
    if not dev:
        perm = torch.tensor(inp['perm'], dtype=torch.long)
        reps['n'], cls['n'], lens['n'] = reps['p'][perm], cls['p'][perm], [inp['p_lens'][i] for i in inp['perm']]
    sent = 1.0 + ri.dist64(agg, reps['q'], reps['p'], lens['q'], lens['p'], direct) - ri.dist64(agg, reps['q'], reps['n'], lens['q'], lens['n'], direct)
    pd = torch.nn.functional.pairwise_distance
    doc = 1.0 + pd(cls['q'], cls['p'], p=2.0, eps=1e-6) - pd(cls['q'], cls['n'], p=2.0, eps=1e-6)
    parts = {}
    if dev:
        loss = torch.clamp_min(sent, 0).sum()
        parts['sent'] = sent
    else:
        w = bool(hp.get('weighted_sup', False))
        neg_align = negative_align(inp['align'], inp['perm'], inp['q_lens'], inp['p_lens'])
        sup = 1.0 + l2sup_dists(reps['q'], reps['p'], lens['q'], lens['p'], inp['align'], w) \
            - l2sup_dists(reps['q'], reps['n'], lens['q'], lens['n'], neg_align, w)
        loss = hp['sentsup_loss_prop'] * torch.clamp_min(sup, 0).sum()
        parts['sup'] = sup
        if hp['sent_loss_prop'] > 0:
            loss = loss + hp['sent_loss_prop'] * torch.clamp_min(sent, 0).sum()
            parts['sent'] = sent
    if hp['abs_loss_prop'] > 0:
        loss = loss + hp['abs_loss_prop'] * torch.clamp_min(doc, 0).sum()
        parts['doc'] = doc
    if not dev and hp.get('cd_svalue_l1_prop', 0.0) > 0:
        loss = loss + hp['cd_svalue_l1_prop'] * svalue_reg(reps['q'], reps['p'])
    loss.backward()
    return loss.item(), [h.grad.numpy() for h in hid.values()], {k: v.detach().numpy() for k, v in parts.items()}


# ---- the cross-document distance matrix -------------------------------------------------------------------------------------------------
# (Sq, Sc, (q_len, c_len) of every pair or None = full): the smallest sizes at which the kernel can go wrong -- one entry; one row or
# one column; one row per wave and one over; real-against-pad and pad-against-pad entries; more rows than a wave's share with two
# columns; the 128-row limit (64 KiB of LDS)
CDIST_SHAPES = {'1x1': (1, 1, None), '1x5': (1, 5, None), '5x1': (5, 1, None), '4x4': (4, 4, None), '5x3': (5, 3, None),
                '9x7': (9, 7, (6, 4)), '33x2': (33, 2, None), '128x128': (128, 128, None)}


def cdist_case(shape, b):
    """-> q [b, Sq, 768], c [b, Sc, 768] float32 with zero pad rows, qlens, clens, G [b, Sq, Sc] float32 of mixed sign.  Rows are
    independent standard normals: distinct rows are about sqrt(2 * 768) = 39 apart.  With lens given, pair 0 has them and every
    further pair one row less on each side."""
    sq, sc, lens = CDIST_SHAPES[shape]
    rng = np.random.RandomState(4000 + 131 * sq + 7 * sc + b)
    q = rng.standard_normal((b, sq, D)).astype(np.float32)
    c = rng.standard_normal((b, sc, D)).astype(np.float32)
    qlens = [sq if lens is None else max(lens[0] - k, 1) for k in range(b)]
    clens = [sc if lens is None else max(lens[1] - k, 1) for k in range(b)]
    for k in range(b):
        q[k, qlens[k]:] = 0
        c[k, clens[k]:] = 0
    return q, c, qlens, clens, rng.standard_normal((b, sq, sc)).astype(np.float32)


def cdist_ref(q, c, g, dtype, qlens, clens):
    """autograd of torch.cdist (direct differences) in `dtype`, loss = sum(G * dist) -> dist, grad_q, grad_c (numpy).  The pad rows
    are constants, as in the reference (its read-out writes zeros there, no leaf stands behind them): their gradient is zero."""
    qt = torch.tensor(q, dtype=dtype, requires_grad=True)
    ct = torch.tensor(c, dtype=dtype, requires_grad=True)
    keep_q = torch.tensor([[float(i < n)] for n in qlens for i in range(q.shape[1])], dtype=dtype).view(q.shape[0], q.shape[1], 1)
    keep_c = torch.tensor([[float(j < n)] for n in clens for j in range(c.shape[1])], dtype=dtype).view(c.shape[0], c.shape[1], 1)
    dist = torch.cdist(qt * keep_q, ct * keep_c, compute_mode='donot_use_mm_for_euclid_dist')
    (dist * torch.tensor(g, dtype=dtype)).sum().backward()
    return dist.detach().numpy(), qt.grad.numpy(), ct.grad.numpy()


# ---- the pre-aligned batcher's raw feeds (documents: prep.json's, by index) ---------------------------------------------------------------
PREP_FEEDS = {
    'dev': dict(align_type='cc_align', query=[0, 1], pos=[4, 0], neg=[1, 4], pos_align=[[1, 4], [0, 2]], neg_align=[[0, 0], [2, 1]]),
    'train': dict(align_type='abs_align', query=[0, 1, 4], pos=[4, 0, 1], pos_align=[[2, 1], [0, 0], [9, 3]]),
    'train_plain': dict(align_type='cc_align', query=[0, 1], pos=[4, 0]),                 # no example carries the key
    'encode': dict(align_type='cc_align', query=[0, 4, 1]),
}


def prep_feed(docs, spec):
    """-> raw_feed: 'query_texts' [, 'pos_texts' [, 'neg_texts']], the examples of a side carrying spec['align_type'] where given"""
    feed = {}
    for side in ('query', 'pos', 'neg'):
        if side in spec:
            exs = [dict(docs[i]) for i in spec[side]]
            for ex, a in zip(exs, spec.get(side + '_align', [])):
                ex[spec['align_type']] = list(a)
            feed[side + '_texts'] = exs
    return feed
