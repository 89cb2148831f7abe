"""The reference's training loss on this project's kernels: from an encoder's ``last_hidden_state`` to the triplet rank loss of
WordSentAbsAlignBiEnc.forward_rank (disent_models.py:587-660), differentiable down to the hidden states.

    encoder(bert_batch) -> last_hidden_state [B, L, 768] (fp32, GPU; under torch autograd when it is to be trained)
        -> torch.ops.aspire.span_mean_pool: the CLS rows and the span mean pool        (backward: aspire_span_mean_pool_backward_f32)
        -> dist_function of aspire_amd.pair_distances over (query, positive) and (query, negative)    (backward: their HIP kernels)
        -> clamp_min(d(q, p) - d(q, n) + 1, 0).sum()        [+ the same hinge over torch.ops.aspire.cls_l2_pair of the CLS rows]

The hinge and the sum are torch ops on [B] tensors.  The encoder's own backward is whatever the caller's encoder brings: with
aspire_amd.HipBertTrainEncoder(bert_model) as the `encoder` argument (an instance takes the reference's batch dict as it stands) the
twelve layers and the embedding LayerNorm run forward and backward on this project's kernels (encoder_bwd.hip) and only the embedding
table lookup is torch's; a HuggingFace model called under torch autograd brings torch's.  Dropout is that encoder's (dropout=True), the
parameter update aspire_amd.HipAdam / HipAdagrad, the loop around all three aspire_amd.RankTrainer; the batch dicts come from
aspire_amd.batch_prep.make_batch, streamed from the jsonl files by aspire_amd.batchers (data-parallel training: aspire_amd/ddp.py).

SupAlignRankLoss is the same for WordSentAbsSupAlignBiEnc.forward_rank (disent_models.py:750-837, model_name 'sbalisentbienc'): the
hinge over the supervised-alignment distance of the batch's pre-aligned sentences (torch.ops.aspire.l2sup_pair_scores) in front of the
sentence and abstract terms, and the singular-value regulariser cd_svalue_l1_prop over torch.ops.aspire.sent_cdist (the distance
matrix in HIP, forward and backward; the SVD of the B small matrices is torch's).  cross_doc_l1 is the value of the parent class's
cd_l1_prop regulariser for callers; RankLoss itself keeps refusing both keys.  Not built: double backward.
"""
import torch

from . import ops, pair_distances as pair_dist
from .batch_prep import spans_to_csr
from .pair_distances import rep_len_ali_tup, rep_len_tup

MARGIN = 1.0            # nn.TripletMarginWithDistanceLoss(margin=1.0) / nn.TripletMarginLoss(margin=1) (disent_models.py:580-582)
CLS_EPS = 1e-6          # nn.TripletMarginLoss's eps, F.pairwise_distance's


def sent_reps_from_hidden(hidden, abs_lens, sent_tok_idxs):
    """partial_forward (disent_models.py:470-485) behind the encoder call: hidden [B, L, 768] fp32 on the GPU ->
    (doc_cls_reps [B, 768], sent_reps [B, 768, max_sents]), max_sents = max(abs_lens); a slot a document does not have is zeros.
    Differentiable with respect to hidden.  A token position outside [0, L) raises IndexError, as the reference's mask indexing."""
    from . import torch_ops  # noqa: F401  (registers the operators)
    assert hidden.dim() == 3 and hidden.shape[0] == len(abs_lens) == len(sent_tok_idxs), 'hidden [B, L, 768], one entry per document'
    max_sents, seq_len = max(abs_lens), hidden.shape[1]
    for doc in sent_tok_idxs:
        for span in doc:
            if span and (min(span) < 0 or max(span) >= seq_len):
                raise IndexError('sentence token index out of range')   # numpy fancy indexing raises too
    tok_idx, span_off = (t.to(hidden.device) for t in spans_to_csr(sent_tok_idxs, max_sents))
    doc_cls_reps, sent_reps = torch.ops.aspire.span_mean_pool(hidden, tok_idx, span_off, max_sents)
    return doc_cls_reps, sent_reps.permute(0, 2, 1)


def _dist_function(model_hparams):
    agg = model_hparams['score_aggregation']
    if agg == 'l2max':
        return pair_dist.allpair_masked_dist_l2max
    if agg == 'l2top2':
        return pair_dist.allpair_masked_dist_l2topk
    if agg == 'l2attention':
        return pair_dist.AllPairMaskedAttention(model_hparams).compute_distance
    if agg == 'l2wasserstein':
        return pair_dist.AllPairMaskedWasserstein(model_hparams).compute_distance
    if agg == 'jointsm':        # this project's name for the dist_function of WordSentAlignPolyEnc (disent_models.py:868)
        return pair_dist.allpair_joint_sm_negscore
    raise ValueError(f'Unknown aggregation: {agg}')


def _hinge(dist_pos, dist_neg):
    """What both of torch's triplet losses compute with reduction='sum': clamp_min(margin + d(a, p) - d(a, n), 0).sum()."""
    return torch.clamp_min(MARGIN + dist_pos - dist_neg, 0).sum()


def _triple_reps(batch_rank, encoder, random_idxs):
    """The three read-outs of forward_rank: (q, p, n), each (cls_reps [B, 768], sent_reps [B, 768, max_sents], abs_lens), and the
    permutation (a list) that made the negatives out of the positives, None with explicit negatives."""
    qabs_lens, pabs_lens = batch_rank['query_abs_lens'], batch_rank['pos_abs_lens']
    q_cls_rep, q_sent_reps = sent_reps_from_hidden(encoder(batch_rank['query_bert_batch']), qabs_lens, batch_rank['query_senttok_idxs'])
    p_cls_rep, p_sent_reps = sent_reps_from_hidden(encoder(batch_rank['pos_bert_batch']), pabs_lens, batch_rank['pos_senttok_idxs'])
    perm = None
    if 'neg_bert_batch' in batch_rank:
        nabs_lens = batch_rank['neg_abs_lens']
        n_cls_reps, n_sent_reps = sent_reps_from_hidden(encoder(batch_rank['neg_bert_batch']), nabs_lens,
                                                        batch_rank['neg_senttok_idxs'])
    else:
        # Use a shuffled set of positives as the negatives. -- in-batch negatives.
        if random_idxs is None:
            random_idxs = torch.randperm(p_sent_reps.size()[0])
        random_idxs = torch.as_tensor(random_idxs, dtype=torch.long)
        n_sent_reps = p_sent_reps[random_idxs.to(p_sent_reps.device)]
        n_cls_reps = p_cls_rep[random_idxs.to(p_cls_rep.device)]
        perm = random_idxs.tolist()
        nabs_lens = [pabs_lens[i] for i in perm]
    return (q_cls_rep, q_sent_reps, qabs_lens), (p_cls_rep, p_sent_reps, pabs_lens), (n_cls_reps, n_sent_reps, nabs_lens), perm


def _abs_hinge(q_cls_rep, p_cls_rep, n_cls_reps):
    """criterion_abs: nn.TripletMarginLoss(margin=1, p=2, reduction='sum') on the CLS rows"""
    return _hinge(torch.ops.aspire.cls_l2_pair(q_cls_rep, p_cls_rep, CLS_EPS), torch.ops.aspire.cls_l2_pair(q_cls_rep, n_cls_reps, CLS_EPS))


class RankLoss:
    """WordSentAbsAlignBiEnc.forward_rank restated over a caller's encoder.  model_hparams: 'score_aggregation' ('l2max', 'l2top2',
    'l2attention', 'l2wasserstein' -- the reference's values, with its hparams keys cdatt_sm_temp / geoml_blur / geoml_scaling /
    sent_sm_temp -- or 'jointsm'), 'sent_loss_prop' (default 1) and 'abs_loss_prop' (default 0: WordSentAlignBiEnc's and
    WordSentAlignPolyEnc's loss, the sentence term alone).

    At the hinge's kink (margin + d(q, p) - d(q, n) == 0 exactly) the sub-gradient is torch.clamp_min's: 1, the triple still sends
    its gradients back (clamp_min's backward passes grad where input >= min)."""

    def __init__(self, model_hparams):
        self.score_agg_type = model_hparams['score_aggregation']
        self.dist_function = _dist_function(model_hparams)
        self.abs_loss_prop = float(model_hparams.get('abs_loss_prop', 0.0))
        self.sent_loss_prop = float(model_hparams.get('sent_loss_prop', 1.0))
        for key in ('cd_l1_prop', 'cd_svalue_l1_prop'):
            if float(model_hparams.get(key, 0.0)) > 0:
                raise NotImplementedError(f'the L1 regulariser {key} is not built')

    def forward_rank(self, batch_rank, encoder, random_idxs=None):
        """batch_rank: the reference's dict -- 'query_bert_batch', 'query_abs_lens', 'query_senttok_idxs', the same for 'pos' and, for
        explicit negatives, 'neg'.  encoder(bert_batch) -> last_hidden_state [B, L, 768] fp32 on the GPU; called for the query, the
        positive and (when 'neg_bert_batch' is present) the negative batch.  Without negatives the positives shuffled by random_idxs
        (default torch.randperm(B)) are the negatives, and autograd adds the two gradients a positive then gets.
        :return: loss_val; a scalar on the GPU, attached to the graph of the encoder's outputs."""
        ops.require_gpu()
        (q_cls_rep, q_sent_reps, qabs_lens), (p_cls_rep, p_sent_reps, pabs_lens), (n_cls_reps, n_sent_reps, nabs_lens), _ = \
            _triple_reps(batch_rank, encoder, random_idxs)
        query_sents = rep_len_tup(embed=q_sent_reps, abs_lens=qabs_lens)
        pos_sents = rep_len_tup(embed=p_sent_reps, abs_lens=pabs_lens)
        neg_sents = rep_len_tup(embed=n_sent_reps, abs_lens=nabs_lens)
        loss_val = self.sent_loss_prop * _hinge(self.dist_function(query_sents, pos_sents), self.dist_function(query_sents, neg_sents))
        if self.abs_loss_prop > 0:
            loss_val = loss_val + self.abs_loss_prop * _abs_hinge(q_cls_rep, p_cls_rep, n_cls_reps)
        return loss_val


def negative_align_idxs(pos_align_idxs, perm, qabs_lens, pabs_lens):
    """The alignment indices the reference's in-batch negatives are scored at (disent_models.py:808-818), as new lists.
    neg_align_idxs[i] is the SAME inner list as pos_align_idxs[perm[i]], and allpair_masked_dist_l2sup clips its indices IN PLACE
    (pair_distances.py:214-215); the positive call runs first, so the negative of triple i reads the indices of triple perm[i]
    already clipped to that triple's documents and clips them again to its own:
        q_idx = min(q_idx, qabs_lens[perm[i]] - 1, qabs_lens[i] - 1)        c_idx = min(c_idx, pabs_lens[perm[i]] - 1)
    This project's l2sup does not write back, so that result is formed here, on the host; the caller's lists are not touched."""
    out = []
    for i, src in enumerate(perm):
        q_idx, c_idx = (int(a) for a in pos_align_idxs[src])
        out.append([min(q_idx, qabs_lens[src] - 1, qabs_lens[i] - 1), min(c_idx, pabs_lens[src] - 1)])
    return out


def cross_doc_l1(query_sents, pos_sents):
    """The value of WordSentAbsAlignBiEnc's cd_l1_prop regulariser (disent_models.py:653-659): the L1 norm of every pair's flattened
    -cdist block over the zero-padded sentence reps, summed over the batch -- |-d| = d, so the sum of torch.ops.aspire.sent_cdist.
    query_sents / pos_sents: RepLen tuples (embed [B, 768, max_sents], abs_lens).  A scalar on the device of query_sents.embed,
    attached to the graph when an embed requires grad.  For callers: RankLoss does not add it (it refuses cd_l1_prop)."""
    return pair_dist.sent_cdist(query_sents, pos_sents).sum()


class SupAlignRankLoss:
    """WordSentAbsSupAlignBiEnc.__init__ + .forward_rank (disent_models.py:673-717, :750-837) restated over a caller's encoder.
    model_hparams: 'score_aggregation' and its keys as RankLoss; 'sentsup_loss_prop' (required: KeyError when absent, as in the
    reference); 'sent_loss_prop' and 'abs_loss_prop' (both default 0.0 -- RankLoss's sent_loss_prop defaults to 1); 'weighted_sup'
    (default False: allpair_masked_dist_l2sup, else allpair_masked_dist_l2sup_weighted); 'cd_svalue_l1_prop' (default 0.0).

    The negatives' alignment indices reproduce the reference's in-place clipping (negative_align_idxs) without mutating the batch's
    lists; a negative index raises ValueError, as l2sup does.  The hinge's kink: as RankLoss."""

    def __init__(self, model_hparams):
        self.score_agg_type = model_hparams['score_aggregation']
        self.dist_function = _dist_function(model_hparams)
        self.sup_dist_function = (pair_dist.allpair_masked_dist_l2sup_weighted if model_hparams.get('weighted_sup', False)
                                  else pair_dist.allpair_masked_dist_l2sup)
        self.abs_loss_prop = float(model_hparams.get('abs_loss_prop', 0.0))
        self.sent_loss_prop = float(model_hparams.get('sent_loss_prop', 0.0))
        self.sentsup_loss_prop = float(model_hparams['sentsup_loss_prop'])
        self.cd_svalue_l1_prop = float(model_hparams.get('cd_svalue_l1_prop', 0.0))

    def forward_rank(self, batch_rank, encoder, random_idxs=None):
        """batch_rank: RankLoss's dict plus 'pos_align_idxs' (list([query sentence, positive sentence]), read by the train branch only).
        Train branch (no 'neg_bert_batch'): sentsup_loss_prop * the hinge over the supervised-alignment distance, + sent_loss_prop *
        the sentence term, + abs_loss_prop * the abstract term, + cd_svalue_l1_prop * the summed singular values of every pair's
        -cdist block, each only when its prop is above 0.  Dev branch ('neg_bert_batch' present): the sentence term UNSCALED
        (disent_models.py:797: "Dev set based on predictions not the pre-alignments"), + abs_loss_prop * the abstract term; alignment
        indices are ignored.  :return: loss_val; a scalar on the GPU, attached to the graph of the encoder's outputs."""
        ops.require_gpu()
        (q_cls_rep, q_sent_reps, qabs_lens), (p_cls_rep, p_sent_reps, pabs_lens), (n_cls_reps, n_sent_reps, nabs_lens), perm = \
            _triple_reps(batch_rank, encoder, random_idxs)
        query_sents = rep_len_tup(embed=q_sent_reps, abs_lens=qabs_lens)
        pos_sents = rep_len_tup(embed=p_sent_reps, abs_lens=pabs_lens)
        neg_sents = rep_len_tup(embed=n_sent_reps, abs_lens=nabs_lens)
        if perm is None:        # Happens when running on the dev set.
            loss_val = _hinge(self.dist_function(query_sents, pos_sents), self.dist_function(query_sents, neg_sents))
            if self.abs_loss_prop > 0:
                loss_val = loss_val + self.abs_loss_prop * _abs_hinge(q_cls_rep, p_cls_rep, n_cls_reps)
            return loss_val
        pos_align_idxs = batch_rank['pos_align_idxs']
        neg_align_idxs = negative_align_idxs(pos_align_idxs, perm, qabs_lens, pabs_lens)
        pos_sents_ali = rep_len_ali_tup(embed=p_sent_reps, abs_lens=pabs_lens, align_idxs=pos_align_idxs)
        neg_sents_ali = rep_len_ali_tup(embed=n_sent_reps, abs_lens=nabs_lens, align_idxs=neg_align_idxs)
        loss_val = self.sentsup_loss_prop * _hinge(self.sup_dist_function(query_sents, pos_sents_ali),
                                                   self.sup_dist_function(query_sents, neg_sents_ali))
        if self.sent_loss_prop > 0:
            loss_val = loss_val + self.sent_loss_prop * _hinge(self.dist_function(query_sents, pos_sents),
                                                               self.dist_function(query_sents, neg_sents))
        if self.abs_loss_prop > 0:
            loss_val = loss_val + self.abs_loss_prop * _abs_hinge(q_cls_rep, p_cls_rep, n_cls_reps)
        # If asked to regularize the cross doc singular values, do so to make them more sparse.
        if self.cd_svalue_l1_prop > 0:
            svalues = torch.linalg.svdvals(-1 * pair_dist.sent_cdist(query_sents, pos_sents))       # [B, min(Sq, Sc)], all >= 0
            loss_val = loss_val + self.cd_svalue_l1_prop * svalues.sum()
        return loss_val
