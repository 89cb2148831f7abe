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
parameter update aspire_amd.HipAdam / HipAdagrad, the loop around all three aspire_amd.RankTrainer; no batcher or DDP is built.  Not
built either: the `sentsup` term of WordSentAbsSupAlignBiEnc, the two L1 regularisers (cd_l1_prop, cd_svalue_l1_prop), double
backward.
"""
import torch

from . import ops, pair_distances as pair_dist
from .batch_prep import spans_to_csr
from .pair_distances import rep_len_tup

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
        qabs_lens, pabs_lens = batch_rank['query_abs_lens'], batch_rank['pos_abs_lens']
        q_cls_rep, q_sent_reps = sent_reps_from_hidden(encoder(batch_rank['query_bert_batch']), qabs_lens, batch_rank['query_senttok_idxs'])
        p_cls_rep, p_sent_reps = sent_reps_from_hidden(encoder(batch_rank['pos_bert_batch']), pabs_lens, batch_rank['pos_senttok_idxs'])
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
            nabs_lens = [pabs_lens[i] for i in random_idxs.tolist()]
        query_sents = rep_len_tup(embed=q_sent_reps, abs_lens=qabs_lens)
        pos_sents = rep_len_tup(embed=p_sent_reps, abs_lens=pabs_lens)
        neg_sents = rep_len_tup(embed=n_sent_reps, abs_lens=nabs_lens)
        loss_val = self.sent_loss_prop * _hinge(self.dist_function(query_sents, pos_sents), self.dist_function(query_sents, neg_sents))
        if self.abs_loss_prop > 0:
            abs_loss_val = _hinge(torch.ops.aspire.cls_l2_pair(q_cls_rep, p_cls_rep, CLS_EPS),
                                  torch.ops.aspire.cls_l2_pair(q_cls_rep, n_cls_reps, CLS_EPS))
            loss_val = loss_val + self.abs_loss_prop * abs_loss_val
        return loss_val
