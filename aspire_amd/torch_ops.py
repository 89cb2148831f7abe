"""PyTorch-ROCm custom ops over the C ABI ("what the build's extension must export").

``import aspire_amd.torch_ops`` registers the operators below in the ``aspire`` namespace with ``torch.library``; every
one is a thin shim over one entry point of include/aspire_hip.h (no arithmetic here), has a GPU ("cuda" = HIP on ROCm)
implementation ONLY -- calling one with CPU tensors fails in the dispatcher, there is no CPU kernel -- and a fake (meta)
implementation so that shapes propagate under FakeTensor / torch.compile tracing.

    torch.ops.aspire.span_mean_pool(hidden, tok_idx, span_off, max_sents) -> (cls, sent)         A2/A3  ex_aspire_consent.py:75-100
    torch.ops.aspire.span_pool_ranges(hidden, row_doc, row_start, row_len) -> (cls, rows [R, 768])  A2r  models.py:437-477
    torch.ops.aspire.bert_encoder_forward(ids, type_ids, mask, weights, n_heads, ln_eps) -> hidden  A1   ex_aspire_consent.py:72-73
    torch.ops.aspire.bert_cls_forward(ids, type_ids, mask, weights, n_heads, ln_eps, layer_mix) -> cls [B, 768]
                                                                                   A1b  ex_aspire_bienc.py:23-58
    torch.ops.aspire.bert_pooler(cls, weight, bias) -> pooled [B, 768]                             A1c  models.py:350
    torch.ops.aspire.token_mean_pool(hidden, mask, normalize) -> reps [B, 768]                     A1d  models.py:402
    torch.ops.aspire.l2max_scores(q, q_lens, c, c_lens, paired) -> scores                          A9   pair_distances.py:138-186
    torch.ops.aspire.ot_sinkhorn_scores(q, q_lens, c, c_lens, blur, scaling, temp, group, want, paired, extras)
                                         -> (scores, q_distr, c_distr, pair_sims, plan)           A5-A8 pair_distances.py:21-92
    torch.ops.aspire.dotmax_scores(q, q_lens, c, c_lens, paired, cosine) -> scores                A13  models.py:602-604
    torch.ops.aspire.jointsm_scores(q, q_lens, c, c_lens, paired) -> scores                       A14  pair_distances.py:348-402
    torch.ops.aspire.topk_desc(scores, k, idx_base) -> (top_scores, top_idx)                       A12  evaluate.py:76
    torch.ops.aspire.topk_keys(scores, k, idx_base) -> keys          } the shard merge of section 8(e): local top-k in key
    torch.ops.aspire.topk_merge(gathered_keys, k) -> (top_scores, top_idx)  } form, (all-gather by the caller), merge
  differentiable (padded pairs, pair p = query p with candidate p; agg 0 max-sim / 1 top-2 / 2 attention):
    torch.ops.aspire.l2agg_pair_scores(q, q_lens, c, c_lens, agg, temp) -> scores [B]              pair_distances.py:138-186, :295-345,
                                         (autograd registered: the gradient with respect to q and c)                       :95-135
    torch.ops.aspire.l2agg_pair_backward(grad_scores, q, q_lens, c, c_lens, agg, temp) -> (grad_q, grad_c)   its formula
    torch.ops.aspire.ot_pair_scores(q, q_lens, c, c_lens, blur, scaling, temp, group, want) -> scores [B]   pair_distances.py:21-92
                                         (autograd registered; want 0 distance / 2 -distance; group as ot_sinkhorn_scores)
    torch.ops.aspire.ot_pair_backward(grad_scores, q, q_lens, c, c_lens, blur, scaling, temp, group, want) -> (grad_q, grad_c)
    torch.ops.aspire.jointsm_pair_scores(q, q_lens, c, c_lens) -> scores [B]                       pair_distances.py:348-402
                                         (autograd registered; the bits of jointsm_scores(..., paired=True))
    torch.ops.aspire.jointsm_pair_backward(grad_scores, q, q_lens, c, c_lens) -> (grad_q, grad_c)
    torch.ops.aspire.l2sup_pair_scores(q, q_lens, c, c_lens, align, weighted) -> scores [B]        pair_distances.py:189-292
                                         (autograd registered; align int32 [B, 2]: the pre-aligned (query row, candidate row))
    torch.ops.aspire.l2sup_pair_backward(grad_scores, q, q_lens, c, c_lens, align, weighted) -> (grad_q, grad_c)
    torch.ops.aspire.sent_cdist(q, q_lens, c, c_lens) -> dist [B, Sq, Sc]                          disent_models.py:655, :829
                                         (autograd registered; ||q_i - c_j|| over the whole zero-padded blocks, pad rows as zeros)
    torch.ops.aspire.sent_cdist_backward(grad_dist, q, q_lens, c, c_lens) -> (grad_q, grad_c)      torch.cdist's rule
  the read-out under autograd (span_mean_pool above has its autograd registered: the gradient with respect to hidden):
    torch.ops.aspire.span_mean_pool_backward(grad_sent | None, grad_cls | None, tok_idx, span_off, B, L, max_sents) -> grad_hidden [B, L, 768]
    torch.ops.aspire.cls_l2_pair(q_cls, c_cls, eps) -> dist [B]                                    disent_models.py:582, :634
                                         (autograd registered; F.pairwise_distance on paired CLS rows, the bits of ops.cls_l2)
    torch.ops.aspire.cls_l2_pair_backward(grad, q_cls, c_cls, eps) -> (grad_q, grad_c)
  the encoder under autograd (behind the embedding lookup; weights = [emb_ln_g, emb_ln_b] + the twelve tensors per layer below):
    torch.ops.aspire.bert_layers_train(emb_sum, mask, weights, n_heads, ln_eps) -> (hidden [B, L, 768], tape uint8)      A1t
                                         (autograd registered: the gradient with respect to emb_sum and every tensor of weights)
    torch.ops.aspire.bert_layers_backward(grad_hidden, tape, mask, weights, n_heads, ln_eps) -> (grad_emb_sum, grads)    its formula
    torch.ops.aspire.bert_layers_train_dropout(emb_sum, mask, weights, n_heads, ln_eps, p_hidden, p_attn, seed, step)     A1t with dropout
    torch.ops.aspire.bert_layers_backward_dropout(grad_hidden, tape, mask, weights, n_heads, ln_eps, p_hidden, p_attn, seed, step)
    torch.ops.aspire.bert_dropout_mask(seed, step, site, p, first, n) -> uint8 [n]                          a site's keep mask
    torch.ops.aspire.bert_layers_train_cls(emb_sum, mask, weights, mix | None, n_heads, ln_eps, p_hidden, p_attn, seed, step)
                                         -> (cls [B, 768], layer_cls, tape)      disent_models.py:178-205, sentsim_models.py:62-78
                                         (autograd registered: emb_sum, every tensor of weights and mix, from the gradient of cls)
    torch.ops.aspire.bert_layers_backward_cls(grad_cls, layer_cls, tape, mask, weights, mix | None, n_heads, ln_eps, p_hidden, p_attn,
                                         seed, step) -> (grad_emb_sum, grads, grad_mix)                                 its formula
    torch.ops.aspire.bert_layers_train_prec(..., p_hidden, p_attn, seed, step, matmul) / bert_layers_backward_prec(..., matmul)
    torch.ops.aspire.bert_layers_train_cls_prec(..., seed, step, matmul) / bert_layers_backward_cls_prec(..., matmul)
                                         the dropout pair and the CLS pair with the matmul mode (0 fp32, 1 bf16 matrix products, 3 bf16x3:
                                         HipBertTrainEncoder(matmul='bf16' | 'bf16x3')); autograd registered like their siblings
    torch.ops.aspire.bert_layers_train_attn(..., matmul, attention) / bert_layers_backward_attn / bert_layers_train_cls_attn /
    bert_layers_backward_cls_attn        the _prec operators with the attention mode (0 the three-kernel form, 1 the fused training
                                         attention, with matmul 1 alone: HipBertTrainEncoder(matmul='bf16', attention='flash'))
    torch.ops.aspire.bert_layers_train_packed(emb_sum, doc_start, row_src, row_dst, max_len, prefix, weights, n_heads, ln_eps, p_hidden,
        p_attn, seed, step) / bert_layers_backward_packed / bert_layers_train_cls_packed / bert_layers_backward_cls_packed
                                         the _attn operators of (matmul 1, attention 1) over the valid token rows alone, the row lists
                                         of aspire_amd.packed_rows where the mask was: HipBertTrainEncoder(..., packed=True)
    torch.ops.aspire.inbatch_xent(q, c) -> (loss [1], row_lse [B])                                 sentsim_models.py:81-126
                                         (autograd registered: the gradient of loss with respect to q and c)
    torch.ops.aspire.inbatch_xent_backward(grad_loss, q, c, row_lse) -> (grad_q, grad_c)
  the embedding lookup in front of the encoder (HipBertTrainEncoder(hip_embeddings=True)):
    torch.ops.aspire.bert_embed_sum(tok, typ | None, word, pos, type_emb, padding_idx) -> emb_sum [B, L, 768]     BertEmbeddings' sum
                                         (autograd registered: the three tables' gradients, written in a fixed order, no atomics)
    torch.ops.aspire.bert_embed_backward(grad, tok, typ | None, vocab, max_pos, n_types, padding_idx, want_word, want_pos, want_type)
                                         -> (grad_word, grad_pos, grad_type), an empty tensor for a table that is not wanted
  resident CSR pools (rows + start + len, struct aspire_repset):
    torch.ops.aspire.l2max_scores_csr / ot_scores_csr(q_rows, q_start, q_len, q_max, c_rows, c_start, c_len, c_max, ...) -> [Q * C]
    torch.ops.aspire.ot_rank_batch(q_rows, q_start, q_len, q_max, c_rows, c_start, c_len, c_max, job_off, max_job, k, ...)
                                         -> (scores [C], top_scores [J, k], top_idx [J, k])        evaluate.py:58-76, batched
    torch.ops.aspire.dot_argmax(q_rows, q_start, q_len, c_rows, c_start, c_len, q_bound, c_bound)
                                         -> (arg int32 [P, 2], best [P])                           A16  pre_proc_cocits.py:487-494
                                         (a data-preparation op: it reads min(q_len) and min(c_len) back before the launch -- two
                                         blocking device syncs -- to raise ValueError on a document without rows, as numpy does)
  one resident [N, 768] matrix of whole-document reps, jobs as row-index lists:
    torch.ops.aspire.dense_rank_batch(rows, q_idx, cand_idx, job_off, max_job, k, metric)
                                         -> (scores [C], top_scores [J, k], top_idx [J, k])        A15  pp_gen_nearest.py:683-717

Padded inputs are [n, S, 768] fp32 with int32 lens [n] (the reference's RepLen after its permute, disent_models.py:15);
``paired`` False scores every query against every candidate ([Q * C], query-major), True scores pair p (Q == C).
"""
import ctypes
from typing import List, Optional, Tuple

import torch

from . import _lib, ops
from ._lib import lib, check
from .encoder import fill_layers, pack_layer_stack, pack_weights

Tensor = torch.Tensor
_D = 768


def _padded_repset(t, lens):
    assert t.dim() == 3 and t.shape[-1] == _D, 'padded reps must be [n, S, 768]'
    n, s, _ = t.shape
    t = t.contiguous()
    start = torch.arange(n, device=t.device, dtype=torch.int32) * s
    return ops.DeviceRepSet(t.view(n * s, _D), start, lens.to(torch.int32).contiguous(), ext=s)


def _csr_repset(rows, start, lens, max_len):
    return ops.DeviceRepSet(rows, start, lens, ext=0, max_len=max_len)


def _scratch(query, bw, b, l, device):
    """uint8 [what the library's size query asks for, at least 16]: a call's workspace or tape"""
    return torch.empty(max(query(ctypes.byref(bw), b, l), 16), device=device, dtype=torch.uint8)


def _int64(*tensors):
    return [t.to(torch.int64).contiguous() for t in tensors]


# ---------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('aspire::span_mean_pool', mutates_args=(), device_types='cuda')
def span_mean_pool(hidden: Tensor, tok_idx: Tensor, span_off: Tensor, max_sents: int) -> Tuple[Tensor, Tensor]:
    cls, sent = ops.span_mean_pool(hidden.contiguous(), tok_idx, span_off, max_sents)
    return cls, sent


@span_mean_pool.register_fake
def _(hidden, tok_idx, span_off, max_sents):
    b, _, d = hidden.shape
    return hidden.new_empty(b, d), hidden.new_empty(b, max_sents, d)


# its gradient with respect to hidden (aspire_span_mean_pool_backward_f32); a gradient that is None is passed as NULL: that output
# took no part in the loss
@torch.library.custom_op('aspire::span_mean_pool_backward', mutates_args=(), device_types='cuda')
def span_mean_pool_backward(grad_sent: Optional[Tensor], grad_cls: Optional[Tensor], tok_idx: Tensor, span_off: Tensor, B: int, L: int,
                            max_sents: int) -> Tensor:
    grad_sent, grad_cls = (None if g is None else g.to(torch.float32).contiguous() for g in (grad_sent, grad_cls))
    return ops.span_mean_pool_backward(grad_sent, grad_cls, tok_idx, span_off, B, L, max_sents)


@span_mean_pool_backward.register_fake
def _(grad_sent, grad_cls, tok_idx, span_off, B, L, max_sents):
    return span_off.new_empty(B, L, _D, dtype=torch.float32)


def _span_mean_pool_setup(ctx, inputs, output):
    hidden, tok_idx, span_off, max_sents = inputs
    ctx.save_for_backward(tok_idx, span_off)
    ctx.dims = (hidden.shape[0], hidden.shape[1], max_sents)
    ctx.set_materialize_grads(False)        # an output the loss does not read arrives as None, not as a block of zeros


def _span_mean_pool_grad(ctx, grad_cls, grad_sent):
    tok_idx, span_off = ctx.saved_tensors
    return torch.ops.aspire.span_mean_pool_backward(grad_sent, grad_cls, tok_idx, span_off, *ctx.dims), None, None, None


span_mean_pool.register_autograd(_span_mean_pool_grad, setup_context=_span_mean_pool_setup)


# ragged span pooling (aspire_span_pool_ranges_f32): row r = mean of hidden[row_doc[r], row_start[r] : row_start[r] + row_len[r]]
@torch.library.custom_op('aspire::span_pool_ranges', mutates_args=(), device_types='cuda')
def span_pool_ranges(hidden: Tensor, row_doc: Tensor, row_start: Tensor, row_len: Tensor) -> Tuple[Tensor, Tensor]:
    hidden = hidden.contiguous()
    cls = torch.empty(hidden.shape[0], hidden.shape[2], device=hidden.device, dtype=torch.float32)
    rows = ops.span_pool_ranges(hidden, row_doc, row_start, row_len, cls=cls)
    return cls, rows


@span_pool_ranges.register_fake
def _(hidden, row_doc, row_start, row_len):
    b, _, d = hidden.shape
    return hidden.new_empty(b, d), hidden.new_empty(row_doc.shape[0], d)


# weights: [word_emb, pos_emb, type_emb, emb_ln_g, emb_ln_b] + per layer [w_qkv, b_qkv, w_o, b_o, ln1_g, ln1_b, w_ffn1,
# b_ffn1, w_ffn2, b_ffn2, ln2_g, ln2_b] (struct aspire_bert_layer, nn.Linear layout)
@torch.library.custom_op('aspire::bert_encoder_forward', mutates_args=(), device_types='cuda')
def bert_encoder_forward(ids: Tensor, type_ids: Tensor, mask: Tensor, weights: List[Tensor], n_heads: int, ln_eps: float) -> Tensor:
    bw = pack_weights(weights, n_heads, ln_eps)
    ids, type_ids, mask = _int64(ids, type_ids, mask)
    b, l = ids.shape
    out = torch.empty(b, l, bw.hidden, device=ids.device, dtype=torch.float32)
    ws = _scratch(lib.aspire_bert_workspace_bytes, bw, b, l, ids.device)
    check(lib.aspire_bert_forward_f32(ctypes.byref(bw), ops._ptr(ids), ops._ptr(type_ids), ops._ptr(mask), b, l, ops._ptr(out), ops._ptr(ws),
                                      ws.numel(), ops._stream()))
    return out


@bert_encoder_forward.register_fake
def _(ids, type_ids, mask, weights, n_heads, ln_eps):
    return weights[0].new_empty(ids.shape[0], ids.shape[1], weights[0].shape[1])


# the bi-encoder read-out (aspire_bert_forward_cls_f32): the same weights list; layer_mix = the softmaxed mix of the n_layers + 1 hidden
# states' CLS rows (ex_aspire_bienc.py:23-58), or [] for the last hidden state's CLS row alone
@torch.library.custom_op('aspire::bert_cls_forward', mutates_args=(), device_types='cuda')
def bert_cls_forward(ids: Tensor, type_ids: Tensor, mask: Tensor, weights: List[Tensor], n_heads: int, ln_eps: float,
                     layer_mix: List[float]) -> Tensor:
    bw = pack_weights(weights, n_heads, ln_eps)
    assert len(layer_mix) in (0, bw.n_layers + 1), 'layer_mix: n_layers + 1 weights, or none'
    ids, type_ids, mask = _int64(ids, type_ids, mask)
    b, l = ids.shape
    out = torch.empty(b, bw.hidden, device=ids.device, dtype=torch.float32)
    mix = ctypes.cast((ctypes.c_float * len(layer_mix))(*layer_mix), ctypes.c_void_p) if layer_mix else None
    ws = _scratch(lib.aspire_bert_cls_workspace_bytes, bw, b, l, ids.device)
    check(lib.aspire_bert_forward_cls_f32(ctypes.byref(bw), ops._ptr(ids), ops._ptr(type_ids), ops._ptr(mask), b, l, mix, ops._ptr(out), None,
                                          ops._ptr(ws), ws.numel(), ops._stream()))
    return out


@bert_cls_forward.register_fake
def _(ids, type_ids, mask, weights, n_heads, ln_eps, layer_mix):
    return weights[0].new_empty(ids.shape[0], weights[0].shape[1])


# HF BertPooler on the CLS rows (aspire_bert_pooler_f32): tanh(cls @ weight.T + bias), the SimCSE baselines' pooler_output
@torch.library.custom_op('aspire::bert_pooler', mutates_args=(), device_types='cuda')
def bert_pooler(cls: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    return ops.bert_pooler(cls.contiguous(), weight.contiguous(), bias.contiguous())


@bert_pooler.register_fake
def _(cls, weight, bias):
    return cls.new_empty(cls.shape[0], weight.shape[0])


# sentence-transformers' Pooling(mean) [+ Normalize] on a forward's hidden states (aspire_token_mean_pool_f32): the mean of the token
# rows with mask != 0, then with normalize x / max(||x||, 1e-12); the SentenceTransformer baselines' rep
@torch.library.custom_op('aspire::token_mean_pool', mutates_args=(), device_types='cuda')
def token_mean_pool(hidden: Tensor, mask: Tensor, normalize: bool) -> Tensor:
    return ops.token_mean_pool(hidden.contiguous(), mask, normalize)


@token_mean_pool.register_fake
def _(hidden, mask, normalize):
    return hidden.new_empty(hidden.shape[0], hidden.shape[2])


def _npairs(qn, cn, paired):
    if paired:
        assert qn == cn, 'paired scoring needs equal batch sizes'      # pair_distances.py:46
        return qn
    return qn * cn


@torch.library.custom_op('aspire::l2max_scores', mutates_args=(), device_types='cuda')
def l2max_scores(q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor, paired: bool) -> Tensor:
    return ops.l2max_scores(_padded_repset(q, q_lens), _padded_repset(c, c_lens),
                            pairing=_lib.PAIR_PAIRED if paired else _lib.PAIR_CROSS)


@l2max_scores.register_fake
def _(q, q_lens, c, c_lens, paired):
    return q.new_empty(_npairs(q.shape[0], c.shape[0], paired))


# cosine: max over the sentence pairs of sklearn's cosine similarity (TrainedSentModel.get_similarity); False: of the raw dot
@torch.library.custom_op('aspire::dotmax_scores', mutates_args=(), device_types='cuda')
def dotmax_scores(q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor, paired: bool, cosine: bool) -> Tensor:
    return ops.dotmax_scores(_padded_repset(q, q_lens), _padded_repset(c, c_lens),
                             pairing=_lib.PAIR_PAIRED if paired else _lib.PAIR_CROSS,
                             sim=_lib.SIM_COSINE if cosine else _lib.SIM_DOT)


@dotmax_scores.register_fake
def _(q, q_lens, c, c_lens, paired, cosine):
    return q.new_empty(_npairs(q.shape[0], c.shape[0], paired))


# the joint soft-max alignment similarity (WordSentAlignPolyEnc.score's batch_scores: minus allpair_joint_sm_negscore)
@torch.library.custom_op('aspire::jointsm_scores', mutates_args=(), device_types='cuda')
def jointsm_scores(q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor, paired: bool) -> Tensor:
    return ops.jointsm_scores(_padded_repset(q, q_lens), _padded_repset(c, c_lens),
                              pairing=_lib.PAIR_PAIRED if paired else _lib.PAIR_CROSS)


@jointsm_scores.register_fake
def _(q, q_lens, c, c_lens, paired):
    return q.new_empty(_npairs(q.shape[0], c.shape[0], paired))


# group: 0 = one epsilon schedule per pair (models.py:190-197); n > 0 = one per consecutive group of n candidates
# (caching_score's padded batches, pp_gen_nearest.py:182-196; paired: one per n pairs).  want: 0 distance, 1 plan-weighted
# similarity, 2 -distance.  extras: also return query_distr, cand_distr, pair_sims, transport plan (else empty tensors).
@torch.library.custom_op('aspire::ot_sinkhorn_scores', mutates_args=(), device_types='cuda')
def ot_sinkhorn_scores(q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor, blur: float, scaling: float, temp: float,
                       group: int, want: int, paired: bool, extras: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    qs, cs = _padded_repset(q, q_lens), _padded_repset(c, c_lens)
    pairing = _lib.PAIR_PAIRED if paired else _lib.PAIR_CROSS
    diam = ops.group_diameter(qs, cs, pairing, group) if group > 0 else None
    out = ops.ot_sinkhorn(qs, cs, pairing=pairing, blur=blur, scaling=scaling, sent_sm_temp=temp, diameter=diam,
                          diam_group=group, want=want, want_extras=extras)
    if extras:
        scores, (qd, cd, ps, plan) = out
        return scores, qd, cd, ps, plan
    e = q.new_empty(0)
    return out, e, e.clone(), e.clone(), e.clone()


@ot_sinkhorn_scores.register_fake
def _(q, q_lens, c, c_lens, blur, scaling, temp, group, want, paired, extras):
    p = _npairs(q.shape[0], c.shape[0], paired)
    if not extras:
        return q.new_empty(p), q.new_empty(0), q.new_empty(0), q.new_empty(0), q.new_empty(0)
    sq, sc = q.shape[1], c.shape[1]
    return q.new_empty(p), q.new_empty(p, sq), q.new_empty(p, sc), q.new_empty(p, sq, sc), q.new_empty(p, sq, sc)


@torch.library.custom_op('aspire::topk_desc', mutates_args=(), device_types='cuda')
def topk_desc(scores: Tensor, k: int, idx_base: int) -> Tuple[Tensor, Tensor]:
    return ops.topk_desc(scores.contiguous(), k, idx_base)


@topk_desc.register_fake
def _(scores, k, idx_base):
    return scores.new_empty(scores.shape[0], k), scores.new_empty(scores.shape[0], k, dtype=torch.int64)


@torch.library.custom_op('aspire::topk_keys', mutates_args=(), device_types='cuda')
def topk_keys(scores: Tensor, k: int, idx_base: int) -> Tensor:
    return ops.topk_keys(scores.contiguous(), k, idx_base)


@topk_keys.register_fake
def _(scores, k, idx_base):
    return scores.new_empty(scores.shape[0], k, dtype=torch.int64)


@torch.library.custom_op('aspire::topk_merge', mutates_args=(), device_types='cuda')
def topk_merge(gathered_keys: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    return ops.topk_merge_keys(gathered_keys.contiguous(), k)


@topk_merge.register_fake
def _(gathered_keys, k):
    qn = gathered_keys.shape[1]
    return gathered_keys.new_empty(qn, k, dtype=torch.float32), gathered_keys.new_empty(qn, k, dtype=torch.int64)


# ---- resident CSR pools -------------------------------------------------------------------------------------------------
@torch.library.custom_op('aspire::l2max_scores_csr', mutates_args=(), device_types='cuda')
def l2max_scores_csr(q_rows: Tensor, q_start: Tensor, q_len: Tensor, q_max: int, c_rows: Tensor, c_start: Tensor,
                     c_len: Tensor, c_max: int) -> Tensor:
    return ops.l2max_scores(_csr_repset(q_rows, q_start, q_len, q_max), _csr_repset(c_rows, c_start, c_len, c_max))


@l2max_scores_csr.register_fake
def _(q_rows, q_start, q_len, q_max, c_rows, c_start, c_len, c_max):
    return q_rows.new_empty(q_start.shape[0] * c_start.shape[0])


@torch.library.custom_op('aspire::ot_scores_csr', mutates_args=(), device_types='cuda')
def ot_scores_csr(q_rows: Tensor, q_start: Tensor, q_len: Tensor, q_max: int, c_rows: Tensor, c_start: Tensor, c_len: Tensor,
                  c_max: int, blur: float, scaling: float, temp: float, group: int, want: int) -> Tensor:
    qs, cs = _csr_repset(q_rows, q_start, q_len, q_max), _csr_repset(c_rows, c_start, c_len, c_max)
    diam = ops.group_diameter(qs, cs, _lib.PAIR_CROSS, group) if group > 0 else None
    return ops.ot_sinkhorn(qs, cs, pairing=_lib.PAIR_CROSS, blur=blur, scaling=scaling, sent_sm_temp=temp, diameter=diam,
                           diam_group=group, want=want)


@ot_scores_csr.register_fake
def _(q_rows, q_start, q_len, q_max, c_rows, c_start, c_len, c_max, blur, scaling, temp, group, want):
    return q_rows.new_empty(q_start.shape[0] * c_start.shape[0])


@torch.library.custom_op('aspire::ot_rank_batch', mutates_args=(), device_types='cuda')
def ot_rank_batch(q_rows: Tensor, q_start: Tensor, q_len: Tensor, q_max: int, c_rows: Tensor, c_start: Tensor, c_len: Tensor,
                  c_max: int, job_off: Tensor, max_job: int, k: int, blur: float, scaling: float, temp: float,
                  want: int) -> Tuple[Tensor, Tensor, Tensor]:
    qs, cs = _csr_repset(q_rows, q_start, q_len, q_max), _csr_repset(c_rows, c_start, c_len, c_max)
    return ops.ot_rank_batch(qs, cs, job_off, max_job, k, blur=blur, scaling=scaling, sent_sm_temp=temp, want=want)


@ot_rank_batch.register_fake
def _(q_rows, q_start, q_len, q_max, c_rows, c_start, c_len, c_max, job_off, max_job, k, blur, scaling, temp, want):
    j = q_start.shape[0]
    return (q_rows.new_empty(c_start.shape[0]), q_rows.new_empty(j, k), q_rows.new_empty(j, k, dtype=torch.int64))


@torch.library.custom_op('aspire::dot_argmax', mutates_args=(), device_types='cuda')
def dot_argmax(q_rows: Tensor, q_start: Tensor, q_len: Tensor, c_rows: Tensor, c_start: Tensor, c_len: Tensor, q_bound: int,
               c_bound: int) -> Tuple[Tensor, Tensor]:
    return ops.dot_argmax(_csr_repset(q_rows, q_start, q_len, q_bound), _csr_repset(c_rows, c_start, c_len, c_bound))


@dot_argmax.register_fake
def _(q_rows, q_start, q_len, c_rows, c_start, c_len, q_bound, c_bound):
    p = q_start.shape[0]
    return q_rows.new_empty(p, 2, dtype=torch.int32), q_rows.new_empty(p)


@torch.library.custom_op('aspire::dense_rank_batch', mutates_args=(), device_types='cuda')
def dense_rank_batch(rows: Tensor, q_idx: Tensor, cand_idx: Tensor, job_off: Tensor, max_job: int, k: int,
                     metric: int) -> Tuple[Tensor, Tensor, Tensor]:
    assert k > 0, 'the op returns the ranked lists: k > 0 (ops.dense_rank_batch takes k = 0 for scores only)'
    return ops.dense_rank_batch(rows, q_idx, cand_idx, job_off, max_job, k, metric=metric)


@dense_rank_batch.register_fake
def _(rows, q_idx, cand_idx, job_off, max_job, k, metric):
    j = q_idx.shape[0]
    return (rows.new_empty(cand_idx.shape[0]), rows.new_empty(j, k), rows.new_empty(j, k, dtype=torch.int64))


# ---- the differentiable pair scores -------------------------------------------------------------------------------------
# Four operator pairs of one shape: X_pair_scores(q, q_lens, c, c_lens, ...) -> scores [B], pair p = query p with candidate p, is an
# existing PAIRED scoring entry (the same bits); its autograd formula is X_pair_backward(grad_scores, the same inputs) ->
# (grad_q, grad_c), which recomputes what it needs from the inputs -- nothing else is saved.
def _pair_scores_fake(q, q_lens, c, c_lens, *rest):
    return q.new_empty(_npairs(q.shape[0], c.shape[0], True))


def _pair_backward(backward, grad_scores, q, q_lens, c, c_lens):
    """(grad_q, grad_c) shaped like q / c: backward(qs, cs, grad_scores, out) is the ops.*_backward call on the padded sets."""
    qs, cs = _padded_repset(q, q_lens), _padded_repset(c, c_lens)
    gq, gc = backward(qs, cs, grad_scores.to(torch.float32).contiguous(),
                      (torch.empty_like(qs.rows), torch.empty_like(cs.rows)))     # padded: every row has its writer
    return gq.view(q.shape), gc.view(c.shape)


def _pair_backward_fake(grad_scores, q, q_lens, c, c_lens, *rest):
    return q.new_empty(q.shape), c.new_empty(c.shape)


def _register_pair_autograd(forward_op, backward_op, forward_fake=_pair_scores_fake):
    """The two operators' fakes and the forward's autograd: the tensor inputs (they lead in every schema) are saved, the others kept
    on ctx; backward_op gives the gradients of q (position 0) and c (position 2), no other input has one."""
    forward_op.register_fake(forward_fake)
    backward_op.register_fake(_pair_backward_fake)

    def setup(ctx, inputs, output):
        n = sum(isinstance(x, Tensor) for x in inputs)
        assert all(isinstance(x, Tensor) for x in inputs[:n])
        ctx.save_for_backward(*inputs[:n])
        ctx.rest = tuple(inputs[n:])

    def grad(ctx, grad_scores):
        inputs = (*ctx.saved_tensors, *ctx.rest)
        gq, gc = backward_op(grad_scores, *inputs)
        return (gq, None, gc) + (None,) * (len(inputs) - 3)

    forward_op.register_autograd(grad, setup_context=setup)


# agg: 0 max-sim, 1 top-2, 2 attention (temp = cdatt_sm_temp; read by attention only).  The forward is aspire_l2max_scores_f32 for
# agg 0, aspire_l2agg_scores_f32 else: the bits of l2max_scores / ops.l2agg_scores; the backward aspire_l2agg_backward_f32.
@torch.library.custom_op('aspire::l2agg_pair_scores', mutates_args=(), device_types='cuda')
def l2agg_pair_scores(q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor, agg: int, temp: float) -> Tensor:
    qs, cs = _padded_repset(q, q_lens), _padded_repset(c, c_lens)
    if agg == _lib.AGG_MAX:
        return ops.l2max_scores(qs, cs, pairing=_lib.PAIR_PAIRED)
    return ops.l2agg_scores(qs, cs, agg, temp=temp, pairing=_lib.PAIR_PAIRED)


@torch.library.custom_op('aspire::l2agg_pair_backward', mutates_args=(), device_types='cuda')
def l2agg_pair_backward(grad_scores: Tensor, q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor, agg: int,
                        temp: float) -> Tuple[Tensor, Tensor]:
    return _pair_backward(lambda qs, cs, g, out: ops.l2agg_backward(qs, cs, agg, g, temp=temp, out=out), grad_scores, q, q_lens, c, c_lens)


_register_pair_autograd(l2agg_pair_scores, l2agg_pair_backward)


# The otAspire distance.  group / want as ot_sinkhorn_scores (want: 0 distance, 2 -distance; 1, the plan-weighted similarity, has no
# backward): the bits of ot_sinkhorn_scores(..., paired=True, extras=False).  The backward (aspire_ot_backward_f32: a restatement of
# geomloss's detach pattern, include/aspire_hip.h) repeats the solve and forms the group diameters again from the inputs, so that
# forward and backward see one epsilon schedule.
def _ot_pair_diameter(qs, cs, group):
    return ops.group_diameter(qs, cs, _lib.PAIR_PAIRED, group) if group > 0 else None


@torch.library.custom_op('aspire::ot_pair_scores', mutates_args=(), device_types='cuda')
def ot_pair_scores(q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor, blur: float, scaling: float, temp: float, group: int,
                   want: int) -> Tensor:
    qs, cs = _padded_repset(q, q_lens), _padded_repset(c, c_lens)
    return ops.ot_sinkhorn(qs, cs, pairing=_lib.PAIR_PAIRED, blur=blur, scaling=scaling, sent_sm_temp=temp,
                           diameter=_ot_pair_diameter(qs, cs, group), diam_group=group, want=want)


@torch.library.custom_op('aspire::ot_pair_backward', mutates_args=(), device_types='cuda')
def ot_pair_backward(grad_scores: Tensor, q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor, blur: float, scaling: float,
                     temp: float, group: int, want: int) -> Tuple[Tensor, Tensor]:
    return _pair_backward(lambda qs, cs, g, out: ops.ot_backward(qs, cs, g, blur=blur, scaling=scaling, sent_sm_temp=temp,
                                                                 diameter=_ot_pair_diameter(qs, cs, group), diam_group=group,
                                                                 want=want, out=out), grad_scores, q, q_lens, c, c_lens)


_register_pair_autograd(ot_pair_scores, ot_pair_backward)


# The joint soft-max alignment score: the bits of jointsm_scores(..., paired=True); the backward aspire_jointsm_backward_f32.
@torch.library.custom_op('aspire::jointsm_pair_scores', mutates_args=(), device_types='cuda')
def jointsm_pair_scores(q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor) -> Tensor:
    return ops.jointsm_scores(_padded_repset(q, q_lens), _padded_repset(c, c_lens), pairing=_lib.PAIR_PAIRED)


@torch.library.custom_op('aspire::jointsm_pair_backward', mutates_args=(), device_types='cuda')
def jointsm_pair_backward(grad_scores: Tensor, q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor) -> Tuple[Tensor, Tensor]:
    return _pair_backward(ops.jointsm_backward, grad_scores, q, q_lens, c, c_lens)


_register_pair_autograd(jointsm_pair_scores, jointsm_pair_backward)


# The supervised-alignment distance.  align int32 [B, 2]: (query row, candidate row) of each pair's pre-aligned sentences, clipped on
# the device to the documents' last rows; weighted: the similarity divided by q_len * c_len.  scores = the SIMILARITY -||q_i - c_j||
# (aspire_l2sup_scores_f32); the backward aspire_l2sup_backward_f32.
@torch.library.custom_op('aspire::l2sup_pair_scores', mutates_args=(), device_types='cuda')
def l2sup_pair_scores(q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor, align: Tensor, weighted: bool) -> Tensor:
    return ops.l2sup_scores(_padded_repset(q, q_lens), _padded_repset(c, c_lens), align.to(torch.int32).contiguous(), weighted)


@torch.library.custom_op('aspire::l2sup_pair_backward', mutates_args=(), device_types='cuda')
def l2sup_pair_backward(grad_scores: Tensor, q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor, align: Tensor,
                        weighted: bool) -> Tuple[Tensor, Tensor]:
    align = align.to(torch.int32).contiguous()
    return _pair_backward(lambda qs, cs, g, out: ops.l2sup_backward(qs, cs, align, g, weighted, out=out), grad_scores, q, q_lens, c, c_lens)


_register_pair_autograd(l2sup_pair_scores, l2sup_pair_backward)


# The distance matrix of the pairs' whole zero-padded blocks, [B, Sq, Sc] instead of a score per pair (aspire_sent_cdist_f32): what the
# reference's L1 regularisers take the norm / the singular values of.  q_lens / c_lens say which rows are pads: those count as zeros
# and are not read.  The backward (aspire_sent_cdist_backward_f32) forms the distances again from the rows.
@torch.library.custom_op('aspire::sent_cdist', mutates_args=(), device_types='cuda')
def sent_cdist(q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor) -> Tensor:
    return ops.sent_cdist(_padded_repset(q, q_lens), _padded_repset(c, c_lens))


@torch.library.custom_op('aspire::sent_cdist_backward', mutates_args=(), device_types='cuda')
def sent_cdist_backward(grad_dist: Tensor, q: Tensor, q_lens: Tensor, c: Tensor, c_lens: Tensor) -> Tuple[Tensor, Tensor]:
    return _pair_backward(lambda qs, cs, g, out: ops.sent_cdist_backward(qs, cs, g, out=out), grad_dist, q, q_lens, c, c_lens)


_register_pair_autograd(sent_cdist, sent_cdist_backward,
                        forward_fake=lambda q, q_lens, c, c_lens: q.new_empty(_npairs(q.shape[0], c.shape[0], True), q.shape[1], c.shape[1]))


# The document-level distance of the rank loss's abstract term: functional.pairwise_distance(q_cls, c_cls, p=2, eps) on paired CLS rows
# [B, 768] -> [B], the bits of ops.cls_l2; the backward aspire_cls_l2_backward_f32.  (Two row matrices and no lens: not the shape
# _register_pair_autograd serves.)
@torch.library.custom_op('aspire::cls_l2_pair', mutates_args=(), device_types='cuda')
def cls_l2_pair(q_cls: Tensor, c_cls: Tensor, eps: float) -> Tensor:
    return ops.cls_l2(q_cls.contiguous(), c_cls.contiguous(), pairing=_lib.PAIR_PAIRED, eps=eps)


@torch.library.custom_op('aspire::cls_l2_pair_backward', mutates_args=(), device_types='cuda')
def cls_l2_pair_backward(grad: Tensor, q_cls: Tensor, c_cls: Tensor, eps: float) -> Tuple[Tensor, Tensor]:
    return ops.cls_l2_backward(q_cls.contiguous(), c_cls.contiguous(), grad.to(torch.float32).contiguous(), eps=eps)


@cls_l2_pair.register_fake
def _(q_cls, c_cls, eps):
    return q_cls.new_empty(_npairs(q_cls.shape[0], c_cls.shape[0], True))


@cls_l2_pair_backward.register_fake
def _(grad, q_cls, c_cls, eps):
    return q_cls.new_empty(q_cls.shape), c_cls.new_empty(c_cls.shape)


def _cls_l2_pair_setup(ctx, inputs, output):
    q_cls, c_cls, ctx.eps = inputs
    ctx.save_for_backward(q_cls, c_cls)


def _cls_l2_pair_grad(ctx, grad):
    gq, gc = torch.ops.aspire.cls_l2_pair_backward(grad, *ctx.saved_tensors, ctx.eps)
    return gq, gc, None


cls_l2_pair.register_autograd(_cls_l2_pair_grad, setup_context=_cls_l2_pair_setup)


# ---- the encoder under autograd (aspire_bert_layers_forward_train_f32 / aspire_bert_layers_backward_f32) -------------------------------
# emb_sum [B, L, 768]: word + position + type rows before the embedding LayerNorm; weights: [emb_ln_g, emb_ln_b] + per layer the twelve
# tensors of bert_encoder_forward's list.  tape: what the backward reads (opaque bytes, aspire_bert_tape_bytes).
def _train_workspace(bw, b, l, device, attention=None):
    if attention is not None:
        return _scratch(lambda w, b_, l_: lib.aspire_bert_train_workspace_bytes_attn(w, b_, l_, attention), bw, b, l, device)
    return _scratch(lib.aspire_bert_train_workspace_bytes, bw, b, l, device)


def _check_attention(matmul, attention):
    """the _attn operators' modes, before a size query could answer 0 for them (the C entries refuse the same)"""
    if attention not in (_lib.ATTENTION_GEMM, _lib.ATTENTION_FLASH):
        raise AssertionError(f'attention mode {attention}: ASPIRE_ATTENTION_GEMM (0) or ASPIRE_ATTENTION_FLASH (1)')
    if attention == _lib.ATTENTION_FLASH and matmul != 1:
        raise NotImplementedError(f'ASPIRE_ATTENTION_FLASH is built for ASPIRE_MATMUL_BF16 alone (matmul mode {matmul})')


# drop: a _lib.BertDropout for the _dropout_ entry points, None for the plain ones (the body of both operator pairs)
# matmul: None for those entries, or ASPIRE_MATMUL_* for the _prec_ entry points (drop may then be None as well)
# attention: None for those, or ASPIRE_ATTENTION_* for the _attn_ entry points (with a matmul mode), whose tape and workspace have sizes of their own
def _layers_forward(emb_sum, mask, weights, n_heads, ln_eps, drop=None, matmul=None, attention=None):
    if attention is not None:
        _check_attention(matmul, attention)
    bw = pack_layer_stack(weights, n_heads, ln_eps)
    emb_sum = emb_sum.to(torch.float32).contiguous()
    b, l, _ = emb_sum.shape
    mask, = _int64(mask)
    out = torch.empty_like(emb_sum)
    if attention is not None:
        tape = _scratch(lambda w, b_, l_: lib.aspire_bert_tape_bytes_attn(w, b_, l_, attention), bw, b, l, emb_sum.device)
    else:
        tape = _scratch(lib.aspire_bert_tape_bytes, bw, b, l, emb_sum.device)
    ws = _train_workspace(bw, b, l, emb_sum.device, attention)
    args = (ctypes.byref(bw), ops._ptr(emb_sum), ops._ptr(mask), b, l, ops._ptr(out), ops._ptr(tape), tape.numel(), ops._ptr(ws), ws.numel())
    if attention is not None:
        check(lib.aspire_bert_layers_forward_train_attn_f32(*args, ctypes.byref(drop) if drop is not None else None, matmul, attention,
                                                            ops._stream()))
    elif matmul is not None:
        check(lib.aspire_bert_layers_forward_train_prec_f32(*args, ctypes.byref(drop) if drop is not None else None, matmul, ops._stream()))
    elif drop is None:
        check(lib.aspire_bert_layers_forward_train_f32(*args, ops._stream()))
    else:
        check(lib.aspire_bert_layers_forward_train_dropout_f32(*args, ctypes.byref(drop), ops._stream()))
    return out, tape


def _layers_backward(grad_hidden, tape, mask, weights, n_heads, ln_eps, drop=None, matmul=None, attention=None):
    if attention is not None:
        _check_attention(matmul, attention)
    bw = pack_layer_stack(weights, n_heads, ln_eps)
    grad_hidden = grad_hidden.to(torch.float32).contiguous()
    b, l, _ = grad_hidden.shape
    mask, = _int64(mask)
    grads = [torch.empty_like(t, memory_format=torch.contiguous_format) for t in weights]
    grad_emb = torch.empty_like(grad_hidden)
    layers = fill_layers(_lib.BertLayerGrads, grads[2:])
    bg = _lib.BertGrads(ctypes.c_void_p(grads[0].data_ptr()), ctypes.c_void_p(grads[1].data_ptr()), layers)
    ws = _train_workspace(bw, b, l, grad_hidden.device, attention)
    args = (ctypes.byref(bw), ops._ptr(mask), b, l, ops._ptr(grad_hidden), ops._ptr(tape), tape.numel(), ops._ptr(grad_emb), ctypes.byref(bg),
            ops._ptr(ws), ws.numel())
    if matmul is not None:
        head, tail = args[:5], args[5:]     # (the _prec_ backward is the CLS one: grad_cls, mix, layer_cls behind grad_hidden; grad_mix behind grads)
        if attention is not None:
            check(lib.aspire_bert_layers_backward_attn_f32(*head, None, None, None, *tail[:4], None, *tail[4:],
                                                           ctypes.byref(drop) if drop is not None else None, matmul, attention, ops._stream()))
            return grad_emb, grads
        check(lib.aspire_bert_layers_backward_prec_f32(*head, None, None, None, *tail[:4], None, *tail[4:],
                                                       ctypes.byref(drop) if drop is not None else None, matmul, ops._stream()))
    elif drop is None:
        check(lib.aspire_bert_layers_backward_f32(*args, ops._stream()))
    else:
        check(lib.aspire_bert_layers_backward_dropout_f32(*args, ctypes.byref(drop), ops._stream()))
    return grad_emb, grads


@torch.library.custom_op('aspire::bert_layers_train', mutates_args=(), device_types='cuda')
def bert_layers_train(emb_sum: Tensor, mask: Tensor, weights: List[Tensor], n_heads: int, ln_eps: float) -> Tuple[Tensor, Tensor]:
    return _layers_forward(emb_sum, mask, weights, n_heads, ln_eps)


@torch.library.custom_op('aspire::bert_layers_backward', mutates_args=(), device_types='cuda')
def bert_layers_backward(grad_hidden: Tensor, tape: Tensor, mask: Tensor, weights: List[Tensor], n_heads: int,
                         ln_eps: float) -> Tuple[Tensor, List[Tensor]]:
    return _layers_backward(grad_hidden, tape, mask, weights, n_heads, ln_eps)


@bert_layers_train.register_fake
def _(emb_sum, mask, weights, n_heads, ln_eps):
    # (the tape's size is the library's to say: one byte per element of an unbacked length would need a GPU-free query of the struct;
    # shapes downstream never depend on it)
    return emb_sum.new_empty(emb_sum.shape, dtype=torch.float32), emb_sum.new_empty(_fake_tape_bytes(emb_sum, weights, n_heads, ln_eps),
                                                                                     dtype=torch.uint8)


def _fake_tape_bytes(emb_sum, weights, n_heads, ln_eps, attention=0):
    """aspire_bert_tape_bytes(_attn) from shapes alone (a host-only query: it reads the struct's geometry, no pointer)."""
    n_layers = (len(weights) - 2) // 12
    bw = _lib.BertWeights(None, None, None, None, None, None, n_layers, n_heads, emb_sum.shape[2],
                          weights[2 + 6].shape[0] if n_layers else 4 * emb_sum.shape[2], 0, 0, 0, float(ln_eps), None)
    return max(lib.aspire_bert_tape_bytes_attn(ctypes.byref(bw), emb_sum.shape[0], emb_sum.shape[1], attention), 16)


@bert_layers_backward.register_fake
def _(grad_hidden, tape, mask, weights, n_heads, ln_eps):
    return grad_hidden.new_empty(grad_hidden.shape, dtype=torch.float32), [t.new_empty(t.shape) for t in weights]


def _bert_layers_train_setup(ctx, inputs, output):
    emb_sum, mask, weights, ctx.n_heads, ctx.ln_eps = inputs
    ctx.save_for_backward(output[1], mask, *weights)


def _bert_layers_train_grad(ctx, grad_hidden, grad_tape):
    tape, mask, *weights = ctx.saved_tensors
    grad_emb, grads = torch.ops.aspire.bert_layers_backward(grad_hidden, tape, mask, weights, ctx.n_heads, ctx.ln_eps)
    return grad_emb, None, grads, None, None


bert_layers_train.register_autograd(_bert_layers_train_grad, setup_context=_bert_layers_train_setup)


# ---- the same with dropout (aspire_bert_layers_forward_train_dropout_f32 / aspire_bert_layers_backward_dropout_f32) ----------------------
# p_hidden, p_attn: BertConfig's hidden_dropout_prob / attention_probs_dropout_prob; (seed, step): the masks' key (include/aspire_hip.h:
# the generator, the sites, the keep rule).  seed is taken modulo 2^64 and step modulo 2^32 (an operator's int is signed).  The backward
# forms the forward's masks again from the same four numbers; no mask is saved.
def _dropout(p_hidden, p_attn, seed, step):
    return _lib.BertDropout(p_hidden, p_attn, seed & 0xFFFFFFFFFFFFFFFF, step & 0xFFFFFFFF)


@torch.library.custom_op('aspire::bert_layers_train_dropout', mutates_args=(), device_types='cuda')
def bert_layers_train_dropout(emb_sum: Tensor, mask: Tensor, weights: List[Tensor], n_heads: int, ln_eps: float, p_hidden: float,
                              p_attn: float, seed: int, step: int) -> Tuple[Tensor, Tensor]:
    return _layers_forward(emb_sum, mask, weights, n_heads, ln_eps, _dropout(p_hidden, p_attn, seed, step))


@torch.library.custom_op('aspire::bert_layers_backward_dropout', mutates_args=(), device_types='cuda')
def bert_layers_backward_dropout(grad_hidden: Tensor, tape: Tensor, mask: Tensor, weights: List[Tensor], n_heads: int, ln_eps: float,
                                 p_hidden: float, p_attn: float, seed: int, step: int) -> Tuple[Tensor, List[Tensor]]:
    return _layers_backward(grad_hidden, tape, mask, weights, n_heads, ln_eps, _dropout(p_hidden, p_attn, seed, step))


@bert_layers_train_dropout.register_fake
def _(emb_sum, mask, weights, n_heads, ln_eps, p_hidden, p_attn, seed, step):
    return emb_sum.new_empty(emb_sum.shape, dtype=torch.float32), emb_sum.new_empty(_fake_tape_bytes(emb_sum, weights, n_heads, ln_eps),
                                                                                     dtype=torch.uint8)


@bert_layers_backward_dropout.register_fake
def _(grad_hidden, tape, mask, weights, n_heads, ln_eps, p_hidden, p_attn, seed, step):
    return grad_hidden.new_empty(grad_hidden.shape, dtype=torch.float32), [t.new_empty(t.shape) for t in weights]


def _bert_layers_train_dropout_setup(ctx, inputs, output):
    emb_sum, mask, weights, ctx.n_heads, ctx.ln_eps, *ctx.dropout = inputs
    ctx.save_for_backward(output[1], mask, *weights)


def _bert_layers_train_dropout_grad(ctx, grad_hidden, grad_tape):
    tape, mask, *weights = ctx.saved_tensors
    grad_emb, grads = torch.ops.aspire.bert_layers_backward_dropout(grad_hidden, tape, mask, weights, ctx.n_heads, ctx.ln_eps, *ctx.dropout)
    return grad_emb, None, grads, None, None, None, None, None, None


bert_layers_train_dropout.register_autograd(_bert_layers_train_dropout_grad, setup_context=_bert_layers_train_dropout_setup)


# ---- the CLS read-out under autograd (aspire_bert_cls_mix_train_f32 / aspire_bert_layers_backward_cls_f32) --------------------------------
# The training forward with the CLS rows of the (optionally mix-weighted) hidden states as its differentiable output: MySPECTER's
# doc_reps_bert (disent_models.py:178-205) and SentBERTWrapper.sent_reps_bert (sentsim_models.py:62-78).  mix: post-soft-max weights
# [n_layers + 1] on the device, or None (the last hidden state's rows); both probabilities 0: the launches without dropout.  layer_cls
# [n_layers + 1, B, 768] (with a mix; else [0]) and the tape are what the backward reads; neither is differentiable.  No [B, L, 768]
# gradient crosses the operator: the backward forms the top gradient in its workspace.
def _drop_or_none(p_hidden, p_attn, seed, step):
    return _dropout(p_hidden, p_attn, seed, step) if (p_hidden > 0 or p_attn > 0) else None


# matmul: None for the entries above, or ASPIRE_MATMUL_* for the _prec_ ones (the body of both operator pairs)
def _train_cls(emb_sum, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul=None, attention=None):
    hidden, tape = _layers_forward(emb_sum, mask, weights, n_heads, ln_eps, _drop_or_none(p_hidden, p_attn, seed, step), matmul, attention)
    bw = pack_layer_stack(weights, n_heads, ln_eps)
    b, l, d = hidden.shape
    cls = hidden.new_empty(b, d)
    layer_cls = hidden.new_empty(((len(weights) - 2) // 12 + 1, b, d) if mix is not None else (0,))
    if mix is not None:
        mix = mix.to(torch.float32).contiguous()
    cls_args = (ctypes.byref(bw), b, l, ops._ptr(tape), tape.numel(), ops._ptr(hidden), ops._ptr(mix), ops._ptr(cls),
                ops._ptr(layer_cls if mix is not None else None))
    if attention is not None:       # (a tape of that mode: the layer inputs sit at other offsets)
        check(lib.aspire_bert_cls_mix_train_attn_f32(*cls_args, attention, ops._stream()))
    else:
        check(lib.aspire_bert_cls_mix_train_f32(*cls_args, ops._stream()))
    return cls, layer_cls, tape


@torch.library.custom_op('aspire::bert_layers_train_cls', mutates_args=(), device_types='cuda')
def bert_layers_train_cls(emb_sum: Tensor, mask: Tensor, weights: List[Tensor], mix: Optional[Tensor], n_heads: int, ln_eps: float,
                          p_hidden: float, p_attn: float, seed: int, step: int) -> Tuple[Tensor, Tensor, Tensor]:
    return _train_cls(emb_sum, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step)


@torch.library.custom_op('aspire::bert_layers_backward_cls', mutates_args=(), device_types='cuda')
def bert_layers_backward_cls(grad_cls: Tensor, layer_cls: Tensor, tape: Tensor, mask: Tensor, weights: List[Tensor], mix: Optional[Tensor],
                             n_heads: int, ln_eps: float, p_hidden: float, p_attn: float, seed: int,
                             step: int) -> Tuple[Tensor, List[Tensor], Tensor]:
    return _backward_cls(grad_cls, layer_cls, tape, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step)


def _backward_cls(grad_cls, layer_cls, tape, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul=None, attention=None):
    if attention is not None:
        _check_attention(matmul, attention)
    bw = pack_layer_stack(weights, n_heads, ln_eps)
    grad_cls = grad_cls.to(torch.float32).contiguous()
    mask, = _int64(mask)
    b, l = mask.shape
    grads = [torch.empty_like(t, memory_format=torch.contiguous_format) for t in weights]
    grad_emb = grad_cls.new_empty(b, l, grad_cls.shape[1])
    grad_mix = grad_cls.new_empty(mix.numel() if mix is not None else 0)
    if mix is not None:
        mix = mix.to(torch.float32).contiguous()
    layers = fill_layers(_lib.BertLayerGrads, grads[2:])
    bg = _lib.BertGrads(ctypes.c_void_p(grads[0].data_ptr()), ctypes.c_void_p(grads[1].data_ptr()), layers)
    ws = _train_workspace(bw, b, l, grad_cls.device, attention)
    drop = _drop_or_none(p_hidden, p_attn, seed, step)
    with_mix = mix is not None
    args = (ctypes.byref(bw), ops._ptr(mask), b, l, None, ops._ptr(grad_cls), ops._ptr(mix),
            ops._ptr(layer_cls.contiguous() if with_mix else None), ops._ptr(tape), tape.numel(), ops._ptr(grad_emb), ctypes.byref(bg),
            ops._ptr(grad_mix if with_mix else None), ops._ptr(ws), ws.numel(), ctypes.byref(drop) if drop is not None else None)
    if attention is not None:
        check(lib.aspire_bert_layers_backward_attn_f32(*args, matmul, attention, ops._stream()))
    elif matmul is not None:
        check(lib.aspire_bert_layers_backward_prec_f32(*args, matmul, ops._stream()))
    else:
        check(lib.aspire_bert_layers_backward_cls_f32(*args, ops._stream()))
    return grad_emb, grads, grad_mix


@bert_layers_train_cls.register_fake
def _(emb_sum, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step):
    b, _, d = emb_sum.shape
    return (emb_sum.new_empty((b, d), dtype=torch.float32),
            emb_sum.new_empty(((len(weights) - 2) // 12 + 1, b, d) if mix is not None else (0,), dtype=torch.float32),
            emb_sum.new_empty(_fake_tape_bytes(emb_sum, weights, n_heads, ln_eps), dtype=torch.uint8))


@bert_layers_backward_cls.register_fake
def _(grad_cls, layer_cls, tape, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step):
    b, l = mask.shape
    return (grad_cls.new_empty((b, l, grad_cls.shape[1]), dtype=torch.float32), [t.new_empty(t.shape) for t in weights],
            grad_cls.new_empty(mix.numel() if mix is not None else 0, dtype=torch.float32))


def _bert_layers_train_cls_setup(ctx, inputs, output):
    emb_sum, mask, weights, mix, ctx.n_heads, ctx.ln_eps, *ctx.dropout = inputs
    ctx.with_mix = mix is not None
    ctx.save_for_backward(output[1], output[2], mask, *([mix] if ctx.with_mix else []), *weights)
    ctx.mark_non_differentiable(output[1])          # (the tape's bytes are no floating-point tensor: not differentiable as they are)


def _bert_layers_train_cls_grad(ctx, grad_cls, grad_layer_cls, grad_tape):
    layer_cls, tape, mask, *rest = ctx.saved_tensors
    mix, weights = (rest[0], rest[1:]) if ctx.with_mix else (None, rest)
    grad_emb, grads, grad_mix = torch.ops.aspire.bert_layers_backward_cls(grad_cls, layer_cls, tape, mask, weights, mix, ctx.n_heads,
                                                                          ctx.ln_eps, *ctx.dropout)
    return grad_emb, None, grads, grad_mix if ctx.with_mix else None, None, None, None, None, None, None


bert_layers_train_cls.register_autograd(_bert_layers_train_cls_grad, setup_context=_bert_layers_train_cls_setup)


# ---- the matmul mode (aspire_bert_layers_forward_train_prec_f32 / aspire_bert_layers_backward_prec_f32) -------------------------------------
# The dropout pair and the CLS pair with a trailing matmul: int (include/aspire_hip.h: ASPIRE_MATMUL_FP32 0, ASPIRE_MATMUL_BF16 1 -- every
# matrix product of the layer stack with both operands rounded to bf16 once, fp32 accumulators; ASPIRE_MATMUL_BF16X3 3 -- the products
# with a k-major operand on the bf16 matrix cores at fp32 accuracy, the others as in mode 0; everything else, the tape and every
# gradient fp32; any other integer, 2 among them, is refused).  HipBertTrainEncoder takes these only with matmul != 'fp32'; with 0 they give the bits of their siblings above.  Both
# probabilities 0: the launches without dropout.
@torch.library.custom_op('aspire::bert_layers_train_prec', mutates_args=(), device_types='cuda')
def bert_layers_train_prec(emb_sum: Tensor, mask: Tensor, weights: List[Tensor], n_heads: int, ln_eps: float, p_hidden: float, p_attn: float,
                           seed: int, step: int, matmul: int) -> Tuple[Tensor, Tensor]:
    return _layers_forward(emb_sum, mask, weights, n_heads, ln_eps, _drop_or_none(p_hidden, p_attn, seed, step), matmul)


@torch.library.custom_op('aspire::bert_layers_backward_prec', mutates_args=(), device_types='cuda')
def bert_layers_backward_prec(grad_hidden: Tensor, tape: Tensor, mask: Tensor, weights: List[Tensor], n_heads: int, ln_eps: float,
                              p_hidden: float, p_attn: float, seed: int, step: int, matmul: int) -> Tuple[Tensor, List[Tensor]]:
    return _layers_backward(grad_hidden, tape, mask, weights, n_heads, ln_eps, _drop_or_none(p_hidden, p_attn, seed, step), matmul)


@bert_layers_train_prec.register_fake
def _(emb_sum, mask, weights, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul):
    return emb_sum.new_empty(emb_sum.shape, dtype=torch.float32), emb_sum.new_empty(_fake_tape_bytes(emb_sum, weights, n_heads, ln_eps),
                                                                                     dtype=torch.uint8)


@bert_layers_backward_prec.register_fake
def _(grad_hidden, tape, mask, weights, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul):
    return grad_hidden.new_empty(grad_hidden.shape, dtype=torch.float32), [t.new_empty(t.shape) for t in weights]


def _bert_layers_train_prec_setup(ctx, inputs, output):
    emb_sum, mask, weights, ctx.n_heads, ctx.ln_eps, *ctx.mode = inputs         # mode: p_hidden, p_attn, seed, step, matmul
    ctx.save_for_backward(output[1], mask, *weights)


def _bert_layers_train_prec_grad(ctx, grad_hidden, grad_tape):
    tape, mask, *weights = ctx.saved_tensors
    grad_emb, grads = torch.ops.aspire.bert_layers_backward_prec(grad_hidden, tape, mask, weights, ctx.n_heads, ctx.ln_eps, *ctx.mode)
    return grad_emb, None, grads, None, None, None, None, None, None, None


bert_layers_train_prec.register_autograd(_bert_layers_train_prec_grad, setup_context=_bert_layers_train_prec_setup)


@torch.library.custom_op('aspire::bert_layers_train_cls_prec', mutates_args=(), device_types='cuda')
def bert_layers_train_cls_prec(emb_sum: Tensor, mask: Tensor, weights: List[Tensor], mix: Optional[Tensor], n_heads: int, ln_eps: float,
                               p_hidden: float, p_attn: float, seed: int, step: int, matmul: int) -> Tuple[Tensor, Tensor, Tensor]:
    return _train_cls(emb_sum, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul)


@torch.library.custom_op('aspire::bert_layers_backward_cls_prec', mutates_args=(), device_types='cuda')
def bert_layers_backward_cls_prec(grad_cls: Tensor, layer_cls: Tensor, tape: Tensor, mask: Tensor, weights: List[Tensor],
                                  mix: Optional[Tensor], n_heads: int, ln_eps: float, p_hidden: float, p_attn: float, seed: int, step: int,
                                  matmul: int) -> Tuple[Tensor, List[Tensor], Tensor]:
    return _backward_cls(grad_cls, layer_cls, tape, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul)


@bert_layers_train_cls_prec.register_fake
def _(emb_sum, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul):
    b, _, d = emb_sum.shape
    return (emb_sum.new_empty((b, d), dtype=torch.float32),
            emb_sum.new_empty(((len(weights) - 2) // 12 + 1, b, d) if mix is not None else (0,), dtype=torch.float32),
            emb_sum.new_empty(_fake_tape_bytes(emb_sum, weights, n_heads, ln_eps), dtype=torch.uint8))


@bert_layers_backward_cls_prec.register_fake
def _(grad_cls, layer_cls, tape, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul):
    b, l = mask.shape
    return (grad_cls.new_empty((b, l, grad_cls.shape[1]), dtype=torch.float32), [t.new_empty(t.shape) for t in weights],
            grad_cls.new_empty(mix.numel() if mix is not None else 0, dtype=torch.float32))


def _bert_layers_train_cls_prec_setup(ctx, inputs, output):
    emb_sum, mask, weights, mix, ctx.n_heads, ctx.ln_eps, *ctx.mode = inputs
    ctx.with_mix = mix is not None
    ctx.save_for_backward(output[1], output[2], mask, *([mix] if ctx.with_mix else []), *weights)
    ctx.mark_non_differentiable(output[1])


def _bert_layers_train_cls_prec_grad(ctx, grad_cls, grad_layer_cls, grad_tape):
    layer_cls, tape, mask, *rest = ctx.saved_tensors
    mix, weights = (rest[0], rest[1:]) if ctx.with_mix else (None, rest)
    grad_emb, grads, grad_mix = torch.ops.aspire.bert_layers_backward_cls_prec(grad_cls, layer_cls, tape, mask, weights, mix, ctx.n_heads,
                                                                               ctx.ln_eps, *ctx.mode)
    return grad_emb, None, grads, grad_mix if ctx.with_mix else None, None, None, None, None, None, None, None


bert_layers_train_cls_prec.register_autograd(_bert_layers_train_cls_prec_grad, setup_context=_bert_layers_train_cls_prec_setup)


# ---- the attention mode (aspire_bert_layers_forward_train_attn_f32 / aspire_bert_layers_backward_attn_f32) ---------------------------------
# The _prec operators with a trailing attention: int (include/aspire_hip.h: ASPIRE_ATTENTION_GEMM 0 -- the _prec operators' launches and
# bits; ASPIRE_ATTENTION_FLASH 1 -- the fused attention, with matmul = 1 alone: any other matmul mode raises NotImplementedError; any
# other integer is refused).  The tape is the mode's own (aspire_bert_tape_bytes_attn): with 1 it holds two statistics per (document,
# head, query) where the probabilities were.  HipBertTrainEncoder takes these only with attention != 'gemm'.
@torch.library.custom_op('aspire::bert_layers_train_attn', mutates_args=(), device_types='cuda')
def bert_layers_train_attn(emb_sum: Tensor, mask: Tensor, weights: List[Tensor], n_heads: int, ln_eps: float, p_hidden: float, p_attn: float,
                           seed: int, step: int, matmul: int, attention: int) -> Tuple[Tensor, Tensor]:
    return _layers_forward(emb_sum, mask, weights, n_heads, ln_eps, _drop_or_none(p_hidden, p_attn, seed, step), matmul, attention)


@torch.library.custom_op('aspire::bert_layers_backward_attn', mutates_args=(), device_types='cuda')
def bert_layers_backward_attn(grad_hidden: Tensor, tape: Tensor, mask: Tensor, weights: List[Tensor], n_heads: int, ln_eps: float,
                              p_hidden: float, p_attn: float, seed: int, step: int, matmul: int,
                              attention: int) -> Tuple[Tensor, List[Tensor]]:
    return _layers_backward(grad_hidden, tape, mask, weights, n_heads, ln_eps, _drop_or_none(p_hidden, p_attn, seed, step), matmul, attention)


@bert_layers_train_attn.register_fake
def _(emb_sum, mask, weights, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul, attention):
    return emb_sum.new_empty(emb_sum.shape, dtype=torch.float32), emb_sum.new_empty(
        _fake_tape_bytes(emb_sum, weights, n_heads, ln_eps, attention), dtype=torch.uint8)


@bert_layers_backward_attn.register_fake
def _(grad_hidden, tape, mask, weights, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul, attention):
    return grad_hidden.new_empty(grad_hidden.shape, dtype=torch.float32), [t.new_empty(t.shape) for t in weights]


def _bert_layers_train_attn_setup(ctx, inputs, output):
    emb_sum, mask, weights, ctx.n_heads, ctx.ln_eps, *ctx.mode = inputs         # mode: p_hidden, p_attn, seed, step, matmul, attention
    ctx.save_for_backward(output[1], mask, *weights)


def _bert_layers_train_attn_grad(ctx, grad_hidden, grad_tape):
    tape, mask, *weights = ctx.saved_tensors
    grad_emb, grads = torch.ops.aspire.bert_layers_backward_attn(grad_hidden, tape, mask, weights, ctx.n_heads, ctx.ln_eps, *ctx.mode)
    return grad_emb, None, grads, None, None, None, None, None, None, None, None


bert_layers_train_attn.register_autograd(_bert_layers_train_attn_grad, setup_context=_bert_layers_train_attn_setup)


@torch.library.custom_op('aspire::bert_layers_train_cls_attn', mutates_args=(), device_types='cuda')
def bert_layers_train_cls_attn(emb_sum: Tensor, mask: Tensor, weights: List[Tensor], mix: Optional[Tensor], n_heads: int, ln_eps: float,
                               p_hidden: float, p_attn: float, seed: int, step: int, matmul: int,
                               attention: int) -> Tuple[Tensor, Tensor, Tensor]:
    return _train_cls(emb_sum, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul, attention)


@torch.library.custom_op('aspire::bert_layers_backward_cls_attn', mutates_args=(), device_types='cuda')
def bert_layers_backward_cls_attn(grad_cls: Tensor, layer_cls: Tensor, tape: Tensor, mask: Tensor, weights: List[Tensor],
                                  mix: Optional[Tensor], n_heads: int, ln_eps: float, p_hidden: float, p_attn: float, seed: int, step: int,
                                  matmul: int, attention: int) -> Tuple[Tensor, List[Tensor], Tensor]:
    return _backward_cls(grad_cls, layer_cls, tape, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul, attention)


@bert_layers_train_cls_attn.register_fake
def _(emb_sum, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul, attention):
    b, _, d = emb_sum.shape
    return (emb_sum.new_empty((b, d), dtype=torch.float32),
            emb_sum.new_empty(((len(weights) - 2) // 12 + 1, b, d) if mix is not None else (0,), dtype=torch.float32),
            emb_sum.new_empty(_fake_tape_bytes(emb_sum, weights, n_heads, ln_eps, attention), dtype=torch.uint8))


@bert_layers_backward_cls_attn.register_fake
def _(grad_cls, layer_cls, tape, mask, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step, matmul, attention):
    b, l = mask.shape
    return (grad_cls.new_empty((b, l, grad_cls.shape[1]), dtype=torch.float32), [t.new_empty(t.shape) for t in weights],
            grad_cls.new_empty(mix.numel() if mix is not None else 0, dtype=torch.float32))


def _bert_layers_train_cls_attn_setup(ctx, inputs, output):
    emb_sum, mask, weights, mix, ctx.n_heads, ctx.ln_eps, *ctx.mode = inputs
    ctx.with_mix = mix is not None
    ctx.save_for_backward(output[1], output[2], mask, *([mix] if ctx.with_mix else []), *weights)
    ctx.mark_non_differentiable(output[1])


def _bert_layers_train_cls_attn_grad(ctx, grad_cls, grad_layer_cls, grad_tape):
    layer_cls, tape, mask, *rest = ctx.saved_tensors
    mix, weights = (rest[0], rest[1:]) if ctx.with_mix else (None, rest)
    grad_emb, grads, grad_mix = torch.ops.aspire.bert_layers_backward_cls_attn(grad_cls, layer_cls, tape, mask, weights, mix, ctx.n_heads,
                                                                               ctx.ln_eps, *ctx.mode)
    return grad_emb, None, grads, grad_mix if ctx.with_mix else None, None, None, None, None, None, None, None, None


bert_layers_train_cls_attn.register_autograd(_bert_layers_train_cls_attn_grad, setup_context=_bert_layers_train_cls_attn_setup)


# ---- the padding-free mode (aspire_bert_layers_forward_train_packed_f32 / aspire_bert_layers_backward_packed_f32) --------------------------
# The _attn operators of (matmul 1, attention 1) with the row lists of aspire_amd.packed_rows(mask) where the mask was: doc_start int32
# [B + 1], row_src int32 [R], row_dst int32 [B L], max_len, prefix.  The layer stack, the tape (aspire_bert_tape_bytes_packed: sized by
# R = row_src.shape[0], a shape, so the fake registrations know it) and the workspace hold the R valid token rows alone; emb_sum,
# hidden and both [B, L, 768] gradients keep the padded layout, with exact zeros on masked rows.  R == 0: zeros, no launch.
_PACKED_MODES = (1, _lib.ATTENTION_FLASH)       # ASPIRE_MATMUL_BF16, ASPIRE_ATTENTION_FLASH: the mode's only form


def _packing(doc_start, row_src, row_dst, max_len, prefix):
    """-> (struct aspire_bert_packing, the int32 tensors it points into: keep them alive), B, L"""
    lists = [t.to(torch.int32).contiguous() for t in (doc_start, row_src, row_dst)]
    b = lists[0].numel() - 1
    assert b >= 0 and (lists[2].numel() % b == 0 if b else lists[2].numel() == 0), 'doc_start [B + 1], row_dst [B L]'
    pk = _lib.BertPacking(lists[1].numel(), max_len, 1 if prefix else 0, *(ctypes.c_void_p(t.data_ptr()) for t in lists))
    return pk, lists, b, (lists[2].numel() // b if b else 0)


def _packed_scratch(query, bw, b, l, rows, device):
    return torch.empty(max(query(ctypes.byref(bw), b, l, rows), 16), device=device, dtype=torch.uint8)


def _packed_forward(emb_sum, doc_start, row_src, row_dst, max_len, prefix, weights, n_heads, ln_eps, drop):
    bw = pack_layer_stack(weights, n_heads, ln_eps)
    emb_sum = emb_sum.to(torch.float32).contiguous()
    pk, lists, b, l = _packing(doc_start, row_src, row_dst, max_len, prefix)
    assert emb_sum.shape[:2] == (b, l), 'emb_sum [B, L, 768] and the row lists disagree'
    out = torch.empty_like(emb_sum)
    tape = _packed_scratch(lib.aspire_bert_tape_bytes_packed, bw, b, l, pk.rows, emb_sum.device)
    ws = _packed_scratch(lib.aspire_bert_train_workspace_bytes_packed, bw, b, l, pk.rows, emb_sum.device)
    check(lib.aspire_bert_layers_forward_train_packed_f32(ctypes.byref(bw), ops._ptr(emb_sum), ctypes.byref(pk), b, l, ops._ptr(out), ops._ptr(tape),
                                                          tape.numel(), ops._ptr(ws), ws.numel(),
                                                          ctypes.byref(drop) if drop is not None else None, *_PACKED_MODES, ops._stream()))
    return out, tape


def _packed_backward(grad_hidden, grad_cls, layer_cls, tape, doc_start, row_src, row_dst, max_len, prefix, weights, mix, n_heads, ln_eps, drop):
    bw = pack_layer_stack(weights, n_heads, ln_eps)
    pk, lists, b, l = _packing(doc_start, row_src, row_dst, max_len, prefix)
    src = grad_hidden if grad_hidden is not None else grad_cls
    grads = [torch.empty_like(t, memory_format=torch.contiguous_format) for t in weights]
    grad_emb = src.new_empty((b, l, src.shape[-1]), dtype=torch.float32)
    with_mix = mix is not None
    grad_mix = src.new_empty(mix.numel() if with_mix else 0, dtype=torch.float32)
    if with_mix:
        mix = mix.to(torch.float32).contiguous()
    layers = fill_layers(_lib.BertLayerGrads, grads[2:])
    bg = _lib.BertGrads(ctypes.c_void_p(grads[0].data_ptr()), ctypes.c_void_p(grads[1].data_ptr()), layers)
    ws = _packed_scratch(lib.aspire_bert_train_workspace_bytes_packed, bw, b, l, pk.rows, src.device)
    check(lib.aspire_bert_layers_backward_packed_f32(ctypes.byref(bw), ctypes.byref(pk), b, l, ops._ptr(grad_hidden), ops._ptr(grad_cls),
                                                     ops._ptr(mix), ops._ptr(layer_cls.contiguous() if with_mix else None), ops._ptr(tape),
                                                     tape.numel(), ops._ptr(grad_emb), ctypes.byref(bg),
                                                     ops._ptr(grad_mix if with_mix else None), ops._ptr(ws), ws.numel(),
                                                     ctypes.byref(drop) if drop is not None else None, *_PACKED_MODES, ops._stream()))
    return grad_emb, grads, grad_mix


def _fake_packed_tape(emb_sum, row_src, weights, n_heads, ln_eps):
    n_layers = (len(weights) - 2) // 12
    bw = _lib.BertWeights(None, None, None, None, None, None, n_layers, n_heads, emb_sum.shape[2],
                          weights[2 + 6].shape[0] if n_layers else 4 * emb_sum.shape[2], 0, 0, 0, float(ln_eps), None)
    return emb_sum.new_empty(max(lib.aspire_bert_tape_bytes_packed(ctypes.byref(bw), emb_sum.shape[0], emb_sum.shape[1], row_src.shape[0]), 16),
                             dtype=torch.uint8)


@torch.library.custom_op('aspire::bert_layers_train_packed', mutates_args=(), device_types='cuda')
def bert_layers_train_packed(emb_sum: Tensor, doc_start: Tensor, row_src: Tensor, row_dst: Tensor, max_len: int, prefix: bool,
                             weights: List[Tensor], n_heads: int, ln_eps: float, p_hidden: float, p_attn: float, seed: int,
                             step: int) -> Tuple[Tensor, Tensor]:
    return _packed_forward(emb_sum, doc_start, row_src, row_dst, max_len, prefix, weights, n_heads, ln_eps,
                           _drop_or_none(p_hidden, p_attn, seed, step))


@torch.library.custom_op('aspire::bert_layers_backward_packed', mutates_args=(), device_types='cuda')
def bert_layers_backward_packed(grad_hidden: Tensor, tape: Tensor, doc_start: Tensor, row_src: Tensor, row_dst: Tensor, max_len: int,
                                prefix: bool, weights: List[Tensor], n_heads: int, ln_eps: float, p_hidden: float, p_attn: float, seed: int,
                                step: int) -> Tuple[Tensor, List[Tensor]]:
    grad_hidden = grad_hidden.to(torch.float32).contiguous()
    return _packed_backward(grad_hidden, None, None, tape, doc_start, row_src, row_dst, max_len, prefix, weights, None, n_heads, ln_eps,
                            _drop_or_none(p_hidden, p_attn, seed, step))[:2]


@bert_layers_train_packed.register_fake
def _(emb_sum, doc_start, row_src, row_dst, max_len, prefix, weights, n_heads, ln_eps, p_hidden, p_attn, seed, step):
    return emb_sum.new_empty(emb_sum.shape, dtype=torch.float32), _fake_packed_tape(emb_sum, row_src, weights, n_heads, ln_eps)


@bert_layers_backward_packed.register_fake
def _(grad_hidden, tape, doc_start, row_src, row_dst, max_len, prefix, weights, n_heads, ln_eps, p_hidden, p_attn, seed, step):
    return grad_hidden.new_empty(grad_hidden.shape, dtype=torch.float32), [t.new_empty(t.shape) for t in weights]


def _bert_layers_train_packed_setup(ctx, inputs, output):
    emb_sum, doc_start, row_src, row_dst, ctx.max_len, ctx.prefix, weights, ctx.n_heads, ctx.ln_eps, *ctx.dropout = inputs
    ctx.save_for_backward(output[1], doc_start, row_src, row_dst, *weights)


def _bert_layers_train_packed_grad(ctx, grad_hidden, grad_tape):
    tape, doc_start, row_src, row_dst, *weights = ctx.saved_tensors
    grad_emb, grads = torch.ops.aspire.bert_layers_backward_packed(grad_hidden, tape, doc_start, row_src, row_dst, ctx.max_len, ctx.prefix,
                                                                   weights, ctx.n_heads, ctx.ln_eps, *ctx.dropout)
    return grad_emb, None, None, None, None, None, grads, None, None, None, None, None, None


bert_layers_train_packed.register_autograd(_bert_layers_train_packed_grad, setup_context=_bert_layers_train_packed_setup)


@torch.library.custom_op('aspire::bert_layers_train_cls_packed', mutates_args=(), device_types='cuda')
def bert_layers_train_cls_packed(emb_sum: Tensor, doc_start: Tensor, row_src: Tensor, row_dst: Tensor, max_len: int, prefix: bool,
                                 weights: List[Tensor], mix: Optional[Tensor], n_heads: int, ln_eps: float, p_hidden: float, p_attn: float,
                                 seed: int, step: int) -> Tuple[Tensor, Tensor, Tensor]:
    hidden, tape = _packed_forward(emb_sum, doc_start, row_src, row_dst, max_len, prefix, weights, n_heads, ln_eps,
                                   _drop_or_none(p_hidden, p_attn, seed, step))
    bw = pack_layer_stack(weights, n_heads, ln_eps)
    pk, lists, b, l = _packing(doc_start, row_src, row_dst, max_len, prefix)
    d = hidden.shape[2]
    cls = hidden.new_empty(b, d)
    layer_cls = hidden.new_empty(((len(weights) - 2) // 12 + 1, b, d) if mix is not None else (0,))
    if mix is not None:
        mix = mix.to(torch.float32).contiguous()
    check(lib.aspire_bert_cls_mix_train_packed_f32(ctypes.byref(bw), ctypes.byref(pk), b, l, ops._ptr(tape), tape.numel(), ops._ptr(hidden),
                                                   ops._ptr(mix), ops._ptr(cls), ops._ptr(layer_cls if mix is not None else None),
                                                   ops._stream()))
    return cls, layer_cls, tape


@torch.library.custom_op('aspire::bert_layers_backward_cls_packed', mutates_args=(), device_types='cuda')
def bert_layers_backward_cls_packed(grad_cls: Tensor, layer_cls: Tensor, tape: Tensor, doc_start: Tensor, row_src: Tensor, row_dst: Tensor,
                                    max_len: int, prefix: bool, weights: List[Tensor], mix: Optional[Tensor], n_heads: int, ln_eps: float,
                                    p_hidden: float, p_attn: float, seed: int, step: int) -> Tuple[Tensor, List[Tensor], Tensor]:
    grad_cls = grad_cls.to(torch.float32).contiguous()
    return _packed_backward(None, grad_cls, layer_cls, tape, doc_start, row_src, row_dst, max_len, prefix, weights, mix, n_heads, ln_eps,
                            _drop_or_none(p_hidden, p_attn, seed, step))


@bert_layers_train_cls_packed.register_fake
def _(emb_sum, doc_start, row_src, row_dst, max_len, prefix, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step):
    b, _, d = emb_sum.shape
    return (emb_sum.new_empty((b, d), dtype=torch.float32),
            emb_sum.new_empty(((len(weights) - 2) // 12 + 1, b, d) if mix is not None else (0,), dtype=torch.float32),
            _fake_packed_tape(emb_sum, row_src, weights, n_heads, ln_eps))


@bert_layers_backward_cls_packed.register_fake
def _(grad_cls, layer_cls, tape, doc_start, row_src, row_dst, max_len, prefix, weights, mix, n_heads, ln_eps, p_hidden, p_attn, seed, step):
    b = doc_start.shape[0] - 1
    return (grad_cls.new_empty((b, row_dst.shape[0] // b, grad_cls.shape[1]), dtype=torch.float32), [t.new_empty(t.shape) for t in weights],
            grad_cls.new_empty(mix.numel() if mix is not None else 0, dtype=torch.float32))


def _bert_layers_train_cls_packed_setup(ctx, inputs, output):
    emb_sum, doc_start, row_src, row_dst, ctx.max_len, ctx.prefix, weights, mix, ctx.n_heads, ctx.ln_eps, *ctx.dropout = inputs
    ctx.with_mix = mix is not None
    ctx.save_for_backward(output[1], output[2], doc_start, row_src, row_dst, *([mix] if ctx.with_mix else []), *weights)
    ctx.mark_non_differentiable(output[1])


def _bert_layers_train_cls_packed_grad(ctx, grad_cls, grad_layer_cls, grad_tape):
    layer_cls, tape, doc_start, row_src, row_dst, *rest = ctx.saved_tensors
    mix, weights = (rest[0], rest[1:]) if ctx.with_mix else (None, rest)
    grad_emb, grads, grad_mix = torch.ops.aspire.bert_layers_backward_cls_packed(grad_cls, layer_cls, tape, doc_start, row_src, row_dst,
                                                                                 ctx.max_len, ctx.prefix, weights, mix, ctx.n_heads, ctx.ln_eps,
                                                                                 *ctx.dropout)
    return grad_emb, None, None, None, None, None, grads, grad_mix if ctx.with_mix else None, None, None, None, None, None, None


bert_layers_train_cls_packed.register_autograd(_bert_layers_train_cls_packed_grad, setup_context=_bert_layers_train_cls_packed_setup)


# ---- the in-batch cross-entropy (aspire_inbatch_xent_f32 / aspire_inbatch_xent_backward_f32) -----------------------------------------------
# ICTBERTWrapper.forward_rank's loss (sentsim_models.py:81-126) over two towers' CLS rows q, c [B, 768], B <= 128: loss [1] and the
# rows' logsumexp [B], which the backward reads.
@torch.library.custom_op('aspire::inbatch_xent', mutates_args=(), device_types='cuda')
def inbatch_xent(q: Tensor, c: Tensor) -> Tuple[Tensor, Tensor]:
    q, c = q.to(torch.float32).contiguous(), c.to(torch.float32).contiguous()
    assert q.dim() == 2 and q.shape == c.shape, 'q and c must be [B, 768] alike'
    loss, row_lse = q.new_zeros(1), q.new_empty(q.shape[0])
    check(lib.aspire_inbatch_xent_f32(ops._ptr(q), ops._ptr(c), q.shape[0], q.shape[1], ops._ptr(loss), ops._ptr(row_lse), ops._stream()))
    return loss, row_lse


@torch.library.custom_op('aspire::inbatch_xent_backward', mutates_args=(), device_types='cuda')
def inbatch_xent_backward(grad_loss: Tensor, q: Tensor, c: Tensor, row_lse: Tensor) -> Tuple[Tensor, Tensor]:
    q, c = q.to(torch.float32).contiguous(), c.to(torch.float32).contiguous()
    grad_loss = grad_loss.to(torch.float32).reshape(1).contiguous()
    grad_q, grad_c = torch.empty_like(q), torch.empty_like(c)
    check(lib.aspire_inbatch_xent_backward_f32(ops._ptr(q), ops._ptr(c), q.shape[0], q.shape[1], ops._ptr(row_lse.contiguous()),
                                               ops._ptr(grad_loss), ops._ptr(grad_q), ops._ptr(grad_c), ops._stream()))
    return grad_q, grad_c


@inbatch_xent.register_fake
def _(q, c):
    return q.new_empty(1, dtype=torch.float32), q.new_empty(q.shape[0], dtype=torch.float32)


@inbatch_xent_backward.register_fake
def _(grad_loss, q, c, row_lse):
    return q.new_empty(q.shape, dtype=torch.float32), c.new_empty(c.shape, dtype=torch.float32)


def _inbatch_xent_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs, output[1])
    ctx.mark_non_differentiable(output[1])


def _inbatch_xent_grad(ctx, grad_loss, grad_lse):
    return torch.ops.aspire.inbatch_xent_backward(grad_loss, *ctx.saved_tensors)


inbatch_xent.register_autograd(_inbatch_xent_grad, setup_context=_inbatch_xent_setup)


# ---- the embedding lookup under autograd (aspire_bert_embed_sum_f32 / aspire_bert_embed_backward_f32) ------------------------------------
# BertEmbeddings' sum (word[tok] + type_emb[typ]) + pos[:L] with torch's bits; typ None: every token of type 0.  padding_idx: the word
# table's row without a gradient (nn.Embedding's padding_idx), -1 for none; the forward does not read it.  The backward writes every row
# of every wanted table in a fixed order without atomics; a table that is not wanted comes back as an empty tensor and the autograd
# formula hands None on (the want flags are the forward's needs_input_grad).
@torch.library.custom_op('aspire::bert_embed_sum', mutates_args=(), device_types='cuda')
def bert_embed_sum(tok: Tensor, typ: Optional[Tensor], word: Tensor, pos: Tensor, type_emb: Tensor, padding_idx: int) -> Tensor:
    tok, = _int64(tok)
    if typ is not None:
        typ, = _int64(typ)
    return ops.bert_embed_sum(tok, typ, *(t.to(torch.float32).contiguous() for t in (word, pos, type_emb)))


@torch.library.custom_op('aspire::bert_embed_backward', mutates_args=(), device_types='cuda')
def bert_embed_backward(grad: Tensor, tok: Tensor, typ: Optional[Tensor], vocab: int, max_pos: int, n_types: int, padding_idx: int,
                        want_word: bool, want_pos: bool, want_type: bool) -> Tuple[Tensor, Tensor, Tensor]:
    tok, = _int64(tok)
    if typ is not None:
        typ, = _int64(typ)
    grads = ops.bert_embed_backward(grad.to(torch.float32).contiguous(), tok, typ, vocab, max_pos, n_types, padding_idx,
                                    want=(want_word, want_pos, want_type))
    return tuple(g if g is not None else grad.new_empty(0, dtype=torch.float32) for g in grads)


@bert_embed_sum.register_fake
def _(tok, typ, word, pos, type_emb, padding_idx):
    return word.new_empty((tok.shape[0], tok.shape[1], word.shape[1]), dtype=torch.float32)


@bert_embed_backward.register_fake
def _(grad, tok, typ, vocab, max_pos, n_types, padding_idx, want_word, want_pos, want_type):
    return tuple(grad.new_empty((n, grad.shape[2]) if want else (0,), dtype=torch.float32)
                 for n, want in ((vocab, want_word), (max_pos, want_pos), (n_types, want_type)))


def _bert_embed_sum_setup(ctx, inputs, output):
    tok, typ, word, pos, type_emb, ctx.padding_idx = inputs
    ctx.with_typ = typ is not None
    ctx.save_for_backward(tok, *([typ] if ctx.with_typ else []))
    ctx.rows = (word.shape[0], pos.shape[0], type_emb.shape[0])


def _bert_embed_sum_grad(ctx, grad):
    tok, *rest = ctx.saved_tensors
    want = tuple(ctx.needs_input_grad[2:5])
    gw, gp, gt = torch.ops.aspire.bert_embed_backward(grad, tok, rest[0] if ctx.with_typ else None, *ctx.rows, ctx.padding_idx, *want)
    return None, None, gw if want[0] else None, gp if want[1] else None, gt if want[2] else None, None


bert_embed_sum.register_autograd(_bert_embed_sum_grad, setup_context=_bert_embed_sum_setup)


# keep bytes (0 / 1) of elements first .. first + n - 1 of one site's mask, by the device function the training kernels use
@torch.library.custom_op('aspire::bert_dropout_mask', mutates_args=(), device_types=None)
def bert_dropout_mask(seed: int, step: int, site: int, p: float, first: int, n: int) -> Tensor:
    keep = torch.empty(max(n, 0), device=ops.require_gpu(), dtype=torch.uint8)
    if n != 0:
        check(lib.aspire_bert_dropout_mask_u8(seed & 0xFFFFFFFFFFFFFFFF, step & 0xFFFFFFFF, site, p, first, n, ops._ptr(keep), ops._stream()))
    return keep


@bert_dropout_mask.register_fake
def _(seed, step, site, p, first, n):
    return torch.empty(n, device='cuda', dtype=torch.uint8)


OPS = ('span_mean_pool', 'span_pool_ranges', 'bert_encoder_forward', 'bert_cls_forward', 'bert_pooler', 'token_mean_pool', 'l2max_scores', 'jointsm_scores', 'ot_sinkhorn_scores', 'topk_desc', 'topk_keys', 'topk_merge',
       'l2max_scores_csr', 'ot_scores_csr', 'ot_rank_batch', 'dot_argmax', 'dense_rank_batch', 'l2agg_pair_scores', 'l2agg_pair_backward',
       'ot_pair_scores', 'ot_pair_backward', 'jointsm_pair_scores', 'jointsm_pair_backward', 'l2sup_pair_scores', 'l2sup_pair_backward',
       'sent_cdist', 'sent_cdist_backward', 'span_mean_pool_backward', 'cls_l2_pair', 'cls_l2_pair_backward', 'bert_layers_train', 'bert_layers_backward',
       'bert_layers_train_dropout', 'bert_layers_backward_dropout', 'bert_dropout_mask', 'bert_layers_train_cls', 'bert_layers_backward_cls',
       'bert_layers_train_prec', 'bert_layers_backward_prec', 'bert_layers_train_cls_prec', 'bert_layers_backward_cls_prec',
       'bert_layers_train_attn', 'bert_layers_backward_attn', 'bert_layers_train_cls_attn', 'bert_layers_backward_cls_attn',
       'bert_layers_train_packed', 'bert_layers_backward_packed', 'bert_layers_train_cls_packed', 'bert_layers_backward_cls_packed',
       'inbatch_xent', 'inbatch_xent_backward', 'bert_embed_sum', 'bert_embed_backward')
