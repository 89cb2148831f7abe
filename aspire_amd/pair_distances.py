"""Drop-in replacements for the reference's sentence-set distance functions, same names, argument
meaning and error behaviour; the arithmetic runs in libaspire_hip.so on the GPU.

Reference: src/learning/facetid_models/pair_distances.py (AllPairMaskedWasserstein :14-92,
allpair_masked_dist_l2max :138-186, allpair_masked_dist_l2sup / _weighted :189-292, allpair_joint_sm_negscore :348-402); copy at examples/ex_aspire_consent_multimatch.py:111-189.

Inputs may live on the CPU (as in the reference's examples) or on the GPU; outputs come back on the
device of ``query.embed``.  There is no CPU code path: without a GPU these raise.

The three L2 aggregations (allpair_masked_dist_l2max, allpair_masked_dist_l2topk, AllPairMaskedAttention) are differentiable
with respect to the sentence reps, as the reference's are under its triplet loss: with grad mode on and ``query.embed`` or
``cand.embed`` requiring grad, the returned distance (or ``sims``) is attached to the graph and ``backward()`` leaves the gradient
in the caller's [batch_size, encoding_dim, max_sents] layout on the caller's device.  So is the OT distance,
AllPairMaskedWasserstein.compute_distance with ``return_pair_sims=False`` (the distance function of the reference's flagship triplet
loss, disent_models.py:241-250): its gradient is a restatement of what geomloss 0.2.4 does for SamplesLoss("sinkhorn", p=1,
debias=False) -- the epsilon-scaling loop without grad, the last extrapolation with grad on detached arguments, the soft-max marginals
not detached (include/aspire_hip.h, aspire_ot_backward_f32) -- since geomloss itself is not available to hold it against; with
``return_pair_sims=True`` its outputs stay detached (the reference marks that branch "only used at test time").  Differentiable too are
allpair_joint_sm_negscore, the dist_function of WordSentAlignPolyEnc (aspire_jointsm_backward_f32; ``pair_sm`` stays detached), and the
supervised-alignment distances allpair_masked_dist_l2sup / allpair_masked_dist_l2sup_weighted, the criterion_sentsup of
WordSentAbsSupAlignBiEnc (aspire_l2sup_backward_f32), and ``sent_cdist``, the cross-document distance matrix of the zero-padded
blocks that the reference's L1 regularisers read (aspire_sent_cdist_backward_f32).  The cosine and dot scores have no backward: the reference does not train with
them.  For the L2 aggregations and jointsm, with ``return_pair_sims=True`` and a rep requiring grad the forward runs
twice -- once for the (detached) pair matrices, once through the differentiable operator for ``sims`` -- and the inputs are copied to
the GPU for each: correct and the same bits, twice the work; the train-time branch (``return_pair_sims=False``) runs it once.
"""
import collections

import torch

from . import _lib, ops

rep_len_tup = collections.namedtuple('RepLen', ['embed', 'abs_lens'])
rep_len_ali_tup = collections.namedtuple('RepLenAli', ['embed', 'abs_lens', 'align_idxs'])      # disent_models.py:17


def _to_repsets(query, cand):
    query_reps, cand_reps = query.embed, cand.embed
    qef_batch_size, _, qmax_sents = query_reps.size()
    cef_batch_size, encoding_dim, cmax_sents = cand_reps.size()
    assert (qef_batch_size == cef_batch_size)   # pair_distances.py:46
    # inputs are batch_size x encoding_dim x max_sents, as in the reference; kernels want rows of 768.
    q = ops.DeviceRepSet.from_padded(query_reps.permute(0, 2, 1), query.abs_lens)
    c = ops.DeviceRepSet.from_padded(cand_reps.permute(0, 2, 1), cand.abs_lens)
    return q, c, query_reps.device


def _wants_grad(query, cand):
    return torch.is_grad_enabled() and (query.embed.requires_grad or cand.embed.requires_grad)


def _differentiable_sims(query, cand, op):
    """sims [batch_size] of the pairs, attached to the graph of query.embed / cand.embed: op(q, q_lens, c, c_lens) -> sims, one of
    the differentiable torch.ops.aspire.*_pair_scores operators (the same bits as the plain scoring calls give), on the GPU between
    differentiable moves and permutes.  (sent_cdist sends torch.ops.aspire.sent_cdist through it: then the result is that operator's
    [batch_size, q_max_sents, c_max_sents] matrix.)"""
    from . import torch_ops  # noqa: F401  (registers the operators)
    dev = ops.require_gpu()
    assert (query.embed.size(0) == cand.embed.size(0))   # pair_distances.py:46
    lens = []
    for rep in (query, cand):
        host = [int(n) for n in rep.abs_lens]
        assert len(host) == rep.embed.size(0), 'abs_lens must have one entry per batch element'
        if any(n <= 0 for n in host):       # (ops.DeviceRepSet's rule)
            raise ValueError('a document without sentence rows cannot be scored (the reference raises on it: '
                             'pair_distances.py:57); drop it from the pool')
        lens.append(torch.as_tensor(host, dtype=torch.int32).to(dev))
    q = query.embed.permute(0, 2, 1).to(device=dev, dtype=torch.float32)
    c = cand.embed.permute(0, 2, 1).to(device=dev, dtype=torch.float32)
    return op(q, lens[0], c, lens[1]).to(query.embed.device)


def _l2agg_pair_op(agg, temp=1.0):
    return lambda q, ql, c, cl: torch.ops.aspire.l2agg_pair_scores(q, ql, c, cl, agg, float(temp))


def ot_kwargs(hparams):
    """Model hyper-parameters -> the blur / scaling / sent_sm_temp keyword arguments of ops.ot_sinkhorn, ot_rank and ot_rank_batch,
    with the reference's defaults (pair_distances.py:16-19).  Every otAspire caller of the host layer reads them here."""
    if hparams.get('geoml_reach', None) is not None:
        # No reference config sets it (config/models_config/**: geoml_reach absent everywhere).
        raise NotImplementedError('unbalanced OT (geoml_reach) is not built')
    return dict(blur=hparams.get('geoml_blur', 0.05), scaling=hparams.get('geoml_scaling', 0.9),
                sent_sm_temp=hparams.get('sent_sm_temp', 1.0))


class AllPairMaskedWasserstein:
    def __init__(self, model_hparams):
        kw = ot_kwargs(model_hparams)
        self.geoml_blur = kw['blur']
        self.geoml_scaling = kw['scaling']
        self.geoml_reach = None
        self.sent_sm_temp = kw['sent_sm_temp']

    def compute_distance(self, query, cand, return_pair_sims=False):
        """
        :param query: namedtuple(embed: batch_size x encoding_dim x q_max_sents; abs_lens: list(int))
        :param cand: namedtuple(embed: batch_size x encoding_dim x c_max_sents; abs_lens: list(int))
        :return: wasserstein distances [batch_size]; with return_pair_sims the plan-weighted similarity and
            [query_distr, cand_distr, pair_sims, transport_plan, masked_sims] (pair_distances.py:86).
        With grad mode on, an embed requiring grad and return_pair_sims=False the distance is attached to the graph (the train-time
        branch, pair_distances.py:88-92; the same bits as without).  With return_pair_sims=True everything stays detached: the
        reference marks that branch "only used at test time", and the plan-weighted similarity has no backward here.
        """
        if _wants_grad(query, cand) and not return_pair_sims:
            # geomloss derives ONE epsilon schedule from the bounding box of the whole batch, pads included: group = batch size
            return _differentiable_sims(query, cand, lambda q, ql, c, cl: torch.ops.aspire.ot_pair_scores(
                q, ql, c, cl, float(self.geoml_blur), float(self.geoml_scaling), float(self.sent_sm_temp), max(q.size(0), 1),
                _lib.OT_DISTANCE))
        q, c, out_dev = _to_repsets(query, cand)
        # geomloss derives ONE epsilon schedule from the bounding box of the whole batch, pads included.
        diam = ops.group_diameter(q, c, _lib.PAIR_PAIRED, group=max(q.n, 1))
        kw = dict(pairing=_lib.PAIR_PAIRED, blur=self.geoml_blur, scaling=self.geoml_scaling,
                  sent_sm_temp=self.sent_sm_temp, diameter=diam, diam_group=max(q.n, 1))
        if return_pair_sims:
            sims, (qd, cd, pair_sims, plan) = ops.ot_sinkhorn(q, c, want=_lib.OT_PLAN_SIM, want_extras=True, **kw)
            masked_sims = plan * pair_sims
            return sims.to(out_dev), [t.to(out_dev) for t in (qd, cd, pair_sims, plan, masked_sims)]
        return ops.ot_sinkhorn(q, c, want=_lib.OT_DISTANCE, **kw).to(out_dev)


def allpair_masked_dist_l2max(query, cand, return_pair_sims=False):
    """
    :return: positive distances [batch_size] (the smallest sentence-pair L2), or with return_pair_sims
        (sims [batch_size], pair_sims [batch_size, q_max_sents, c_max_sents]).
    """
    if _wants_grad(query, cand) and not return_pair_sims:       # "Happens at train time" (pair_distances.py:184-186)
        return -1 * _differentiable_sims(query, cand, _l2agg_pair_op(_lib.AGG_MAX))
    q, c, out_dev = _to_repsets(query, cand)
    if return_pair_sims:
        sims, pair = ops.l2max_scores(q, c, pairing=_lib.PAIR_PAIRED, want_pair_sims=True)
        if _wants_grad(query, cand):        # the pair matrix stays detached
            sims = _differentiable_sims(query, cand, _l2agg_pair_op(_lib.AGG_MAX))
        return sims.to(out_dev), pair.to(out_dev)
    return (-1 * ops.l2max_scores(q, c, pairing=_lib.PAIR_PAIRED)).to(out_dev)


def allpair_masked_dist_l2topk(query, cand, return_pair_sims=False):
    """pair_distances.py:295-345 (score_agg_type 'l2top2').
    :return: positive distances [batch_size] (minus the sum of the two largest -cdist entries), or with
        return_pair_sims (sims [batch_size], pair_sims [batch_size, q_max_sents, c_max_sents])."""
    if query.embed.shape[-1] * cand.embed.shape[-1] < 2:
        # torch.topk(k=2) over the [batch, q_max_sents * c_max_sents] view raises for a single entry (pair_distances.py:333)
        raise RuntimeError('selected index k out of range')
    if _wants_grad(query, cand) and not return_pair_sims:
        return -1 * _differentiable_sims(query, cand, _l2agg_pair_op(_lib.AGG_TOP2))
    q, c, out_dev = _to_repsets(query, cand)
    if return_pair_sims:
        sims, pair = ops.l2agg_scores(q, c, _lib.AGG_TOP2, pairing=_lib.PAIR_PAIRED, want_pair_sims=True)
        if _wants_grad(query, cand):
            sims = _differentiable_sims(query, cand, _l2agg_pair_op(_lib.AGG_TOP2))
        return sims.to(out_dev), pair.to(out_dev)
    return (-1 * ops.l2agg_scores(q, c, _lib.AGG_TOP2, pairing=_lib.PAIR_PAIRED)).to(out_dev)


class AllPairMaskedAttention:
    """pair_distances.py:95-135 (score_agg_type 'l2attention'): -cdist weighted by its masked 2-D soft-max."""

    def __init__(self, model_hparams):
        self.cdatt_sm_temp = model_hparams.get('cdatt_sm_temp', 1.0)

    def compute_distance(self, query, cand, return_pair_sims=False):
        """:return: doc_dists [batch_size]; with return_pair_sims (doc_sims, [pair_sims, pair_softmax, masked_sims])."""
        if _wants_grad(query, cand) and not return_pair_sims:
            return -1 * _differentiable_sims(query, cand, _l2agg_pair_op(_lib.AGG_ATTENTION, self.cdatt_sm_temp))
        q, c, out_dev = _to_repsets(query, cand)
        kw = dict(temp=self.cdatt_sm_temp, pairing=_lib.PAIR_PAIRED)
        if return_pair_sims:
            sims, pair, soft = ops.l2agg_scores(q, c, _lib.AGG_ATTENTION, want_pair_sims=True, **kw)
            if _wants_grad(query, cand):
                sims = _differentiable_sims(query, cand, _l2agg_pair_op(_lib.AGG_ATTENTION, self.cdatt_sm_temp))
            return sims.to(out_dev), [t.to(out_dev) for t in (pair, soft, soft * pair)]
        return (-1 * ops.l2agg_scores(q, c, _lib.AGG_ATTENTION, **kw)).to(out_dev)


def allpair_joint_sm_negscore(query, cand, return_pair_sims=False):
    """pair_distances.py:348-402 (score_aggregation 'jointsm'): the query's and the candidate's sentences re-expressed through the
    joint soft-max of their scaled dot products, the dot similarities to the aligned reps summed -- 2 sum_ij p_ij <q_i, c_j>.
    :return: a distance [batch_size] (minus that sum: "because the optimizer calls for it"), or with return_pair_sims
        (distance, pair_sm [batch_size, q_max_sents, c_max_sents]: the soft-max, 0.0 outside a pair's valid block).
    With grad mode on and an embed requiring grad the distance is attached to the graph (pair_sm never is); without, today's bits."""
    if _wants_grad(query, cand) and not return_pair_sims:       # the triplet loss of WordSentAlignPolyEnc (disent_models.py:868-875)
        return -1.0 * _differentiable_sims(query, cand, _jointsm_pair_op)
    q, c, out_dev = _to_repsets(query, cand)
    if return_pair_sims:
        sims, pair_sm = ops.jointsm_scores(q, c, pairing=_lib.PAIR_PAIRED, want_pair_softmax=True)
        if _wants_grad(query, cand):        # pair_sm stays detached
            sims = _differentiable_sims(query, cand, _jointsm_pair_op)
        return (-1.0 * sims).to(out_dev), pair_sm.to(out_dev)
    return (-1.0 * ops.jointsm_scores(q, c, pairing=_lib.PAIR_PAIRED)).to(out_dev)


def _jointsm_pair_op(q, q_lens, c, c_lens):
    return torch.ops.aspire.jointsm_pair_scores(q, q_lens, c, c_lens)


def _l2sup_dist(query, cand, weighted):
    """The distance ||q_i - c_j|| of every pair's pre-aligned sentences (i, j) = cand.align_idxs[p], each index clipped to its
    document's last row (pair_distances.py:214-215; unlike the reference the clipped values are NOT written back into the caller's
    list), divided by q_len * c_len when `weighted`.  One code path with and without grad: torch.ops.aspire.l2sup_pair_scores."""
    from . import torch_ops  # noqa: F401  (registers the operator)
    align = [[int(a) for a in pair] for pair in cand.align_idxs]
    assert len(align) == query.embed.size(0) and all(len(pair) == 2 for pair in align), \
        'align_idxs: one (query sentence, candidate sentence) per batch element'
    if any(a < 0 for pair in align for a in pair):
        raise ValueError('align_idxs must not be negative (the reference would index from the end of the padded block)')
    align = torch.as_tensor(align, dtype=torch.int32).reshape(-1, 2).to(ops.require_gpu())
    sims = _differentiable_sims(query, cand, lambda q, ql, c, cl: torch.ops.aspire.l2sup_pair_scores(q, ql, c, cl, align, weighted))
    return -1 * sims


def allpair_masked_dist_l2sup(query, cand):
    """pair_distances.py:189-235: the L2 distance of the (pre) aligned pair of sentences.
    :param cand: namedtuple(embed, abs_lens, align_idxs: list([int, int]); alignment from query to cand) -- rep_len_ali_tup
    :return: positive distances [batch_size], attached to the graph when an embed requires grad."""
    return _l2sup_dist(query, cand, False)


def allpair_masked_dist_l2sup_weighted(query, cand):
    """pair_distances.py:238-292: allpair_masked_dist_l2sup divided by the number of entries q_len * c_len of the pair's cross-document
    block ("for use in multi tasking with the OT loss")."""
    return _l2sup_dist(query, cand, True)


def sent_cdist(query, cand):
    """disent_models.py:655 / :829 without the sign: torch.cdist(query.embed.permute(0, 2, 1), cand.embed.permute(0, 2, 1)) over the
    whole zero-padded blocks -> [batch_size, q_max_sents, c_max_sents], with a row at or beyond its document's abs_lens entry taken as
    zeros (what the read-out leaves there).  Distances from direct differences; attached to the graph when an embed requires grad
    (torch.ops.aspire.sent_cdist, aspire_sent_cdist_backward_f32)."""
    return _differentiable_sims(query, cand, lambda q, ql, c, cl: torch.ops.aspire.sent_cdist(q, ql, c, cl))
