"""Inputs and float64 yardsticks of the read-out fixture (tests/golden/readout.npz): the backward of the span mean pool and of the CLS
distance, and the reference's rank loss (WordSentAbsAlignBiEnc.forward_rank) from last_hidden_state to the loss and back.  Shared by
make_golden_readout.py (which runs the reference on these inputs and records its own fp32 error against the yardsticks) and by the
tests (which hold the kernels to a bound made of that error: trainside_inputs.bound).  Everything is regenerated from seeds."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):       # tests/ (ot_backward_ref), the root (oracle)
    if _p not in sys.path:
        sys.path.append(_p)

from trainside_inputs import D, bound, jointsm_sims  # noqa: E402,F401  (bound re-exported)

AGGS = ('l2max', 'l2top2', 'l2attention', 'l2wasserstein', 'jointsm')
REF_AGGS = ('l2max', 'l2top2', 'l2attention')            # held against the reference's own functions
HPARAMS = dict(cdatt_sm_temp=2.0, geoml_blur=0.05, geoml_scaling=0.9, sent_sm_temp=1.0)


# ---- the pool backward's cases --------------------------------------------------------------------------------------------------
def _reference_layout(rng, n_sents, seq_len, lo=3, hi=8, title=2):
    """[CLS] title [SEP] sentence [SEP] sentence [SEP] ... pads: disjoint ascending runs that never contain position 0"""
    spans, pos = [], 1 + title + 1
    for _ in range(n_sents):
        n = int(rng.randint(lo, hi))
        spans.append(list(range(pos, pos + n)))
        pos += n + 1
    assert pos - 1 <= seq_len, (pos, seq_len)
    return spans


def pool_case(name):
    """-> dict(B, L, S, spans [B][<= S][positions], gs [B, S, 768] float32, gc [B, 768] float32)"""
    seed = {'a': 501, 'b': 502, 'c': 503, 'd': 504}[name]
    rng = np.random.RandomState(seed)
    if name == 'a':      # 4 / 2 / 1 sentences: empty slots; one span ends at the last row; L a multiple of no tile
        b, l, s = 3, 37, 4
        spans = [[list(range(4, 9)), list(range(10, 17)), list(range(18, 22)), list(range(23, 37))],
                 [list(range(3, 20)), list(range(21, 30))], [list(range(5, 11))]]
    elif name == 'b':    # one row: the span term and the CLS term land on it
        b, l, s, spans = 1, 1, 1, [[[0]]]
    elif name == 'c':    # a position twice in a slot, a position shared by two slots, an unsorted slot, position 0 in a span
        b, l, s = 2, 33, 3
        spans = [[[5, 6, 6, 7], [7, 8, 9], [20, 3, 32, 11, 0]], [[1, 2, 3], [16, 15, 15, 2, 31], [8, 9, 10, 8]]]
    else:                # the reference's layout, ragged; most rows in no span
        b, l, s = 2, 502, 20
        spans = [_reference_layout(rng, 20, l), _reference_layout(rng, 7, l)]
    gs = rng.standard_normal((b, s, D)).astype(np.float32)
    gc = rng.standard_normal((b, D)).astype(np.float32)
    return dict(B=b, L=l, S=s, spans=spans, gs=gs, gc=gc)


def pool64(hidden, spans, max_sents):
    """The span mean pool on a torch tensor [B, L, 768], in its dtype, differentiable: every listed position counts (twice when listed
    twice, as the kernel's forward), sum / max(count, 1) -> sent [B, max_sents, 768]."""
    out = []
    for b, doc in enumerate(spans):
        rows = []
        for s in range(max_sents):
            idx = doc[s] if s < len(doc) else []
            if idx:
                rows.append(hidden[b, torch.tensor(idx, dtype=torch.long)].sum(0) / float(len(idx)))
            else:
                rows.append(hidden.new_zeros(hidden.shape[2]))
        out.append(torch.stack(rows))
    return torch.stack(out)


def pool_grad64(case, use_gs=True, use_gc=True):
    """float64 autograd: the gradient of sum(gs * sent) + sum(gc * hidden[:, 0]) with respect to hidden -> [B, L, 768] float64"""
    h = torch.zeros(case['B'], case['L'], D, dtype=torch.float64, requires_grad=True)
    loss = h.sum() * 0.0
    if use_gs:
        loss = loss + (pool64(h, case['spans'], case['S']) * torch.tensor(case['gs'], dtype=torch.float64)).sum()
    if use_gc:
        loss = loss + (h[:, 0] * torch.tensor(case['gc'], dtype=torch.float64)).sum()
    loss.backward()
    return h.grad.numpy()


def pool_grad32_ordered(case, use_gs=True, use_gc=True):
    """The stated order in fp32 numpy: slots ascending, within a slot its positions ascending in the list, each match adds
    gs / max(count, 1) (one division per slot); the CLS gradient last.  What the kernel must give bit for bit."""
    out = np.zeros((case['B'], case['L'], D), dtype=np.float32)
    for b, doc in enumerate(case['spans']):
        if use_gs:
            for s, idx in enumerate(doc):
                g = case['gs'][b, s] / np.float32(max(len(idx), 1))
                for t in idx:
                    if 0 <= t < case['L']:
                        out[b, t] = out[b, t] + g
        if use_gc:
            out[b, 0] = out[b, 0] + case['gc'][b]
    return out


# ---- the CLS distance ---------------------------------------------------------------------------------------------------------------
def cls_case(name):
    """-> q, c [B, 768] float32, g [B] float32.  'same': pair 1 has q == c (dist = eps * sqrt(768))."""
    rng = np.random.RandomState({'b5': 601, 'same': 602, 'b1': 603}[name])
    b = {'b5': 5, 'same': 3, 'b1': 1}[name]
    q = rng.standard_normal((b, D)).astype(np.float32)
    c = rng.standard_normal((b, D)).astype(np.float32)
    if name == 'same':
        c[1] = q[1]
    return q, c, rng.standard_normal(b).astype(np.float32)


def cls_ref(q, c, g, dtype, eps=1e-6):
    """autograd of F.pairwise_distance in `dtype` -> dist, grad_q, grad_c (numpy)"""
    qt = torch.tensor(q, dtype=dtype, requires_grad=True)
    ct = torch.tensor(c, dtype=dtype, requires_grad=True)
    dist = torch.nn.functional.pairwise_distance(qt, ct, p=2.0, eps=eps)
    (dist * torch.tensor(g, dtype=dtype)).sum().backward()
    return dist.detach().numpy(), qt.grad.numpy(), ct.grad.numpy()


# ---- the rank loss -------------------------------------------------------------------------------------------------------------------
SIZES = {'std': dict(B=4, L=40, q_lens=[4, 2, 3, 2], p_lens=[3, 4, 2, 2], n_lens=[2, 3, 4, 3], perm=[2, 0, 1, 3], seed=821),
         'small': dict(B=2, L=10, q_lens=[2, 2], p_lens=[2, 2], n_lens=[2, 2], perm=[1, 0], seed=701, lo=2, hi=3, title=0)}
# (the seeds were chosen, before any kernel ran, for pick gaps above 1e-3: readout_inputs.pick_margin)
# (size, aggregation, explicit negatives, abs_loss_prop); the small ones keep the reference's gradients in the fixture
RANK_CASES = {f'{agg}_{"neg" if neg else "inb"}_a{int(10 * prop)}': ('std', agg, neg, prop)
              for agg in AGGS for neg in (True, False) for prop in (0.0, 0.5)}
SMALL_CASES = {'small_l2max_neg_a5': ('small', 'l2max', True, 0.5), 'small_l2top2_inb_a0': ('small', 'l2top2', False, 0.0),
               'small_l2attention_inb_a5': ('small', 'l2attention', False, 0.5)}
RANK_CASES.update(SMALL_CASES)


def rank_inputs(size):
    """-> dict: hidden of the query / positive / negative batch [B, L, 768] float32, their abs_lens and senttok_idxs, perm.
    A document's rows are one topic vector plus noise; a positive shares its query's topic in the even documents, a negative in the
    odd ones: the hinge of the even triples is inactive, of the odd ones active (the generator asserts both, and the margins)."""
    spec = SIZES[size]
    rng = np.random.RandomState(spec['seed'])
    b, l = spec['B'], spec['L']
    kw = {k: spec[k] for k in ('lo', 'hi', 'title') if k in spec}
    topics = 0.1 * rng.standard_normal((3, b, D))
    out = dict(B=b, L=l, perm=list(spec['perm']))
    for which, lens in (('q', spec['q_lens']), ('p', spec['p_lens']), ('n', spec['n_lens'])):
        own = topics[0].copy()
        if which == 'p':
            own[1::2] = topics[1][1::2]
        if which == 'n':
            own[0::2] = topics[2][0::2]
        out[which + '_hidden'] = (own[:, None, :] + 0.05 * rng.standard_normal((b, l, D))).astype(np.float32)
        out[which + '_lens'] = list(lens)
        out[which + '_idxs'] = [_reference_layout(rng, n, l, **kw) for n in lens]
    return out


def hparams(agg, prop):
    return dict(HPARAMS, score_aggregation=agg, abs_loss_prop=prop, sent_loss_prop=1.0)


def pair_sims64(q, c, ql, cl):
    """s = -cdist (direct differences) of one pair's valid block, flattened"""
    return (-torch.cdist(q[:ql][None], c[:cl][None], compute_mode='donot_use_mm_for_euclid_dist')[0]).reshape(-1)


def dist64(agg, q, c, qlens, clens, direct=False):
    """The distance of every pair on torch tensors [B, S, 768], in their dtype, differentiable -> [B]: the closed forms of the three
    L2 aggregations, trainside_inputs.jointsm_sims, and for 'l2wasserstein' ot_backward_ref.restated_distance (the yardstick of the
    OT backward's tests; direct: distances from direct differences, the fp32 run's formula)."""
    if agg == 'l2wasserstein':
        import ot_backward_ref
        return ot_backward_ref.restated_distance(q, c, qlens, clens, blur=HPARAMS['geoml_blur'], scaling=HPARAMS['geoml_scaling'],
                                                 temp=HPARAMS['sent_sm_temp'], direct=direct)
    if agg == 'jointsm':
        return -jointsm_sims(q, c, qlens, clens)
    out = []
    for b, (ql, cl) in enumerate(zip(qlens, clens)):
        s = pair_sims64(q[b], c[b], ql, cl)
        if agg == 'l2max':
            out.append(-s.max())
        elif agg == 'l2top2':
            out.append(-torch.topk(s, 2)[0].sum())
        else:
            out.append(-(torch.softmax(s / HPARAMS['cdatt_sm_temp'], dim=0) * s).sum())
    return torch.stack(out)


def rank_loss64(inp, agg, neg, prop, dtype=torch.float64, direct=False):
    """The rank loss restated with torch in `dtype` -> (loss, [grad of the query, positive(, negative) hidden states], parts):
    parts = the hinge arguments of the sentence term and of the abstract term [B] each."""
    hid = {w: torch.tensor(inp[w + '_hidden'], dtype=dtype, requires_grad=True) for w in (('q', 'p', 'n') if neg else ('q', 'p'))}
    reps = {w: pool64(h, inp[w + '_idxs'], max(inp[w + '_lens'])) for w, h in hid.items()}
    cls = {w: h[:, 0] for w, h in hid.items()}
    lens = {w: inp[w + '_lens'] for w in ('q', 'p', 'n')}
    if not neg:
        perm = torch.tensor(inp['perm'], dtype=torch.long)
        reps['n'], cls['n'], lens['n'] = reps['p'][perm], cls['p'][perm], [inp['p_lens'][i] for i in inp['perm']]
    sent = 1.0 + dist64(agg, reps['q'], reps['p'], lens['q'], lens['p'], direct) - dist64(agg, reps['q'], reps['n'], lens['q'], lens['n'], direct)
    pd = torch.nn.functional.pairwise_distance
    doc = 1.0 + pd(cls['q'], cls['p'], p=2.0, eps=1e-6) - pd(cls['q'], cls['n'], p=2.0, eps=1e-6)
    loss = torch.clamp_min(sent, 0).sum()
    if prop > 0:
        loss = loss + prop * torch.clamp_min(doc, 0).sum()
    loss.backward()
    return loss.item(), [h.grad.numpy() for h in hid.values()], dict(sent=sent.detach().numpy(), doc=doc.detach().numpy())


def pick_margin(inp, neg):
    """float64: the smallest gap the arg-max / top-2 picks of any pair of the case have -- between the best and the second, and the
    second and the third, entry of s = -cdist, and (ot_backward_ref.pick_margins) within every row and column."""
    import ot_backward_ref
    reps = {w: pool64(torch.tensor(inp[w + '_hidden'], dtype=torch.float64), inp[w + '_idxs'], max(inp[w + '_lens'])) for w in 'qpn'}
    lens = {w: inp[w + '_lens'] for w in 'qpn'}
    if not neg:
        reps['n'], lens['n'] = reps['p'][inp['perm']], [inp['p_lens'][i] for i in inp['perm']]
    gap = float('inf')
    for w in 'pn':
        gap = min(gap, ot_backward_ref.pick_margins(reps['q'], reps[w], lens['q'], lens[w]))
        for b, (ql, cl) in enumerate(zip(lens['q'], lens[w])):
            s = torch.sort(pair_sims64(reps['q'][b], reps[w][b], ql, cl), descending=True)[0]
            gap = min(gap, float((s[:-1] - s[1:])[:2].min()))
    return gap
