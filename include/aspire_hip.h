/*
 * aspire_hip.h -- C ABI of libaspire_hip.so: the MI355X (gfx950) implementation of Aspire's
 * query-vs-candidate scoring path.
 *
 * The reference (allenai/aspire) is pure Python and has no FFI; the drop-in boundary is the Python
 * call surface of examples/ex_aspire_consent{,_multimatch}.py.  Every entry point below replaces the
 * PyTorch-eager arithmetic of one reference function (cited per function, paths relative to the
 * reference root) and is what a ctypes binding of that function calls.
 *
 * Conventions
 *   - plain C: device pointers + sizes, no torch types.  All pointers are DEVICE pointers unless
 *     the parameter name ends in `_host`.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are asynchronous
 *     on that stream; inputs are borrowed, outputs must be pre-allocated by the caller.
 *   - every function returns an aspire_status; aspire_last_error() gives the message (thread local).
 *   - fp32 arithmetic throughout ("within 1e-4 of the reference CPU path").  D (encoding dim) must
 *     be 768 (BERT-base, `bert_encoding_dim` at ex_aspire_consent.py:31).
 *
 * Rep store layout ("rows + CSR"): sentence reps of many documents are one row-major fp32 matrix
 * rows[total_sents, D]; document k owns rows [start[k], start[k] + len[k]).  A padded reference
 * tensor [B, S, D] is the special case start[k] = k*S.
 */
#ifndef ASPIRE_HIP_H
#define ASPIRE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASPIRE_ABI_VERSION 6

typedef enum {
    ASPIRE_OK = 0,
    ASPIRE_ERR_INVALID_ARG = 1,  /* the reference would raise AssertionError / IndexError          */
    ASPIRE_ERR_UNSUPPORTED = 2,  /* shape outside what the kernels are built for (message says)    */
    ASPIRE_ERR_HIP = 3           /* a HIP runtime call failed                                      */
} aspire_status;

int aspire_abi_version(void);
const char* aspire_last_error(void);
/* number of sentence rows per document the scoring kernels accept (larger -> ASPIRE_ERR_UNSUPPORTED) */
int aspire_max_sents(void);

/* ---------------------------------------------------------------------------------------------
 * A2 + A3  CLS read-out and span mean pooling.
 * Replaces AspireConSent.consent_reps_bert's pooling loop, examples/ex_aspire_consent.py:75-100
 * (original src/learning/facetid_models/disent_models.py:487-535).
 *   hidden    [B, L, D]  final hidden states
 *   tok_idx   flat int32 token positions; slot (b, s) owns tok_idx[span_off[b*S+s] .. span_off[b*S+s+1])
 *   span_off  [B*S + 1]; an empty slot (doc has fewer than S sentences) yields exact zeros
 *   sent_reps [B, S, D]  out: sum of the slot's token rows / max(count, 1)
 *   cls_reps  [B, D]     out (may be NULL): hidden[b, 0, :]
 * ------------------------------------------------------------------------------------------- */
int aspire_span_mean_pool_f32(const float* hidden, int64_t B, int64_t L, int64_t D,
                              const int32_t* tok_idx, const int32_t* span_off, int64_t S,
                              float* sent_reps, float* cls_reps, void* stream);
/* The same pooling written straight into a resident rep store (rows + CSR, no padding rows): slot (b, s) goes to row
 * out_row[b*S+s] of `rows` (device int32 [B*S]; < 0 = document b has no sentence s, nothing is written).  This is the
 * un-padding of caching_encode (src/learning/facetid_models/disent_models.py:363-370: sent_reps[i, :, :num_sents]) and of
 * AspireModel.encode (src/evaluation/utils/models.py:208) done by the kernel's store addresses instead of a host loop,
 * so encoded documents never leave HBM on their way into the candidate pool. */
int aspire_span_mean_pool_rows_f32(const float* hidden, int64_t B, int64_t L, int64_t D,
                                   const int32_t* tok_idx, const int32_t* span_off, int64_t S,
                                   const int32_t* out_row, float* rows, float* cls_reps, void* stream);
/* Ragged span pooling: R output rows, each the mean of a RANGE of token rows of one document.  Replaces
 * AspireConSenContextual._get_sent_reps / _get_ner_reps, src/evaluation/utils/models.py:437-477 (one [B, L, 768] mask pass per
 * sentence slot, then one fancy-indexed mean per entity): sentence spans and entity spans (find_sublist_range, models.py:684-697)
 * are runs of consecutive positions, so a row is (document, first token, token count) and no token-index list is read.  The grid
 * is over the R rows that exist: no per-batch slot maximum, no padding rows.  Spans may overlap freely (an entity always overlaps
 * its sentence).
 *   hidden    [B, L, D]  final hidden states
 *   row_doc, row_start, row_len   device int32 [R]: row r = sum, in ascending token order, of
 *             hidden[row_doc[r], row_start[r] .. row_start[r] + row_len[r]) / max(row_len[r], 1); row_len 0 yields exact zeros.
 *             The caller guarantees 0 <= row_doc < B and 0 <= row_start, row_start + row_len <= L (checked where the tables are
 *             built, on the host).
 *   out_row   device int32 [R] or NULL: row r is written to rows[out_row[r]] (a rows + CSR rep store); NULL = rows[r]
 *   rows      [>= max out_row + 1, D]  out
 *   cls_reps  [B, D]     out (may be NULL): hidden[b, 0, :]; written also when R == 0
 * On the same span the result has the bits of aspire_span_mean_pool_f32 (same order of the sum, same division). */
int aspire_span_pool_ranges_f32(const float* hidden, int64_t B, int64_t L, int64_t D,
                                const int32_t* row_doc, const int32_t* row_start, const int32_t* row_len, int64_t R,
                                const int32_t* out_row, float* rows, float* cls_reps, void* stream);
/* The gradient of aspire_span_mean_pool_f32 with respect to `hidden` (the read-out of the reference's training step,
 * disent_models.py:487-535 under autograd): what reaches last_hidden_state from the sentence rows and the CLS rows.
 *   grad_sent   [B, S, D] or NULL  dLoss / dsent_reps       grad_cls  [B, D] or NULL  dLoss / dcls_reps     (NULL: the term is absent)
 *   tok_idx, span_off, S           the forward's
 *   grad_hidden [B, L, D]  out:  grad_hidden[b, t, :] = the sum, over the slots s of document b in ascending order and within a slot
 *               over its positions k in ascending order with tok_idx[k] == t, of grad_sent[b, s, :] / max(count_s, 1) (a division,
 *               formed once per slot, as torch's autograd of sum / count); then, last, + grad_cls[b, :] when t == 0.
 * Every element of grad_hidden is written exactly once, tokens of no span (pads, the title, [SEP]) with exact zeros; with both
 * gradients NULL all of it is zeros.  Any index list the forward takes: a position listed twice in a slot counts twice, a position of
 * two slots gets both terms, position 0 may sit in a span beside grad_cls; an index outside [0, L) contributes nothing and is never
 * used as an address.  The kernel is a gather (a tile of token rows looks for its slots; one writer per row): no atomics, no zero
 * fill in front, the same bits on every run and for every launch geometry.
 * D != 768 -> ASPIRE_ERR_UNSUPPORTED; B < 0, L < 0, S <= 0, grad_hidden NULL, span_off NULL beside grad_sent, or a gradient pointer
 * not 16-byte aligned -> ASPIRE_ERR_INVALID_ARG; B == 0 or L == 0 -> ASPIRE_OK without a launch.  All of it before any launch. */
int aspire_span_mean_pool_backward_f32(const float* grad_sent /* [B,S,D] or NULL */, const float* grad_cls /* [B,D] or NULL */,
                                       int64_t B, int64_t L, int64_t D, const int32_t* tok_idx, const int32_t* span_off, int64_t S,
                                       float* grad_hidden /* [B,L,D] out */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1  BERT-base encoder forward.  Replaces `self.bert_encoder(tokid_tt, token_type_ids=seg_tt,
 * attention_mask=attnmask_tt).last_hidden_state` at examples/ex_aspire_consent.py:72-73 (HuggingFace
 * BertModel: embeddings + LayerNorm, 12 x [QKV, masked softmax attention, output proj + residual +
 * LayerNorm, 768->3072 GELU(erf) 3072->768 + residual + LayerNorm]; the pooler is not part of the
 * forward: the one reference model that reads pooler_output gets it from aspire_bert_pooler_f32, A1c).
 * fp32 ACCURACY throughout (1e-4 of HuggingFace's fp32 CPU forward, also on weights with a trained
 * checkpoint's outliers: tests/test_gpu_encoder_heavy.py): with `planes` prepared and >= 1024 token rows every GEMM and the
 * attention run on the fp16 matrix pipe over operands held as two fp16 planes (three exact products per term, fp32 sums); otherwise
 * on operands split on the fly / the fp32-input matrix cores.  An activation beyond fp16's range (|x| > 65504) makes the plane path
 * return non-finite rows: check the output and run again after aspire_debug_set("GEMM", "bf16x3") + ("ATTN", "f32") (aspire_amd does).
 *   weights are borrowed device pointers in nn.Linear layout ([out, in] row-major);
 *   w_qkv is query/key/value weights concatenated along `out` ([2304, 768]), b_qkv likewise.
 *   tok_ids / type_ids / attn_mask  int64 [B, L] (type_ids may be NULL = all zero); attn_mask != 0 = real token
 *   Any 0/1 pattern is accepted (left padding, holes, real tokens behind a key tile of padding), in every attention form; a row that
 *   is all zero attends uniformly over its L keys, as HuggingFace's (1 - mask) * finfo.min does.
 *   hidden_out [B, L, 768]
 *   workspace  device scratch of aspire_bert_workspace_bytes(w, B, L) bytes
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const float *w_qkv, *b_qkv;      /* [2304, 768], [2304] */
    const float *w_o, *b_o;          /* [768, 768],  [768]  */
    const float *ln1_g, *ln1_b;      /* attention.output.LayerNorm */
    const float *w_ffn1, *b_ffn1;    /* intermediate.dense [ffn, 768], [ffn] */
    const float *w_ffn2, *b_ffn2;    /* output.dense       [768, ffn], [768] */
    const float *ln2_g, *ln2_b;      /* output.LayerNorm */
} aspire_bert_layer;

typedef struct {
    const float *word_emb, *pos_emb, *type_emb; /* [vocab,768] [max_pos,768] [n_types,768] */
    const float *emb_ln_g, *emb_ln_b;
    const aspire_bert_layer* layers;            /* HOST array of n_layers entries (device pointers inside) */
    int32_t n_layers, n_heads, hidden, ffn_dim, vocab, max_pos, n_types;
    float ln_eps;                               /* layer_norm_eps (1e-12) */
    /* NULL, or the nn.Linear weights' pre-split planes: a DEVICE buffer of aspire_bert_planes_bytes(w) bytes filled once by
     * aspire_bert_prepare_planes when the model is loaded (the weights never change; the call synchronises the stream and
     * returns ASPIRE_ERR_UNSUPPORTED for a weight beyond +-1023 or not finite).  With it the forward's GEMMs (from 1024 token
     * rows on) stream pre-split operands: every fp32 value as two fp16 planes h + l (24 significant bits, the weights scaled by
     * 2^6 first), three exact matrix-pipe products per term (h.h' + h.l' + l.h') summed in fp32 -- fp32's accuracy, measured
     * against float64 in tests/test_gpu_encoder.py -- and no conversion work in the main loop; without it every workgroup splits
     * its fp32 tiles into three bf16 planes on the fly (six products per term). */
    const void* planes;
} aspire_bert_weights;

size_t aspire_bert_planes_bytes(const aspire_bert_weights* w);
int aspire_bert_prepare_planes(const aspire_bert_weights* w, void* planes, size_t planes_bytes, void* stream);
size_t aspire_bert_workspace_bytes(const aspire_bert_weights* w, int64_t B, int64_t L);
int aspire_bert_forward_f32(const aspire_bert_weights* w, const int64_t* tok_ids, const int64_t* type_ids,
                            const int64_t* attn_mask, int64_t B, int64_t L, float* hidden_out,
                            void* workspace, size_t workspace_bytes, void* stream);
/* The encoder kernels' sticky per-device status word.  From 6144 token rows on (gfx950 in SPX mode) the two N = 768 GEMMs of a layer
 * carry the LayerNorm in their epilogue: the six column tiles of a 128-row block exchange their rows' moments through device memory
 * and a tile WAITS inside the kernel for its partners.  The wait is bounded (20 ms): a tile that gives up sets
 * ASPIRE_BERT_STATUS_LN_TIMEOUT and the outputs of the forwards in flight are invalid.  aspire_bert_status copies the word to
 * *status_host, SYNCHRONISES `stream`, and clears it; on a non-zero word run the forwards since the last check again with
 * aspire_debug_set("GEMM_LN", "off") (the separate LayerNorm pass; run_checked in aspire_amd/encoder.py is that rule, and the model
 * classes -- consent.py, bienc.py, sentenc.py, contextner.py -- apply it to what they hand out).  Never seen set outside the
 * fault-injection test (tests/test_gpu_encoder_wait.py); the bound turns a hang under a broken dispatch-order assumption (CU masking,
 * a serialising debugger) into an error. */
#define ASPIRE_BERT_STATUS_LN_TIMEOUT 1
int aspire_bert_status(int32_t* status_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1b  SPECTER-CoCite bi-encoder read-out.  Replaces `SoftmaxMixLayers(13 -> 1, bias=False)` over
 * `bert_encoder(..., output_hidden_states=True).hidden_states` at examples/ex_aspire_bienc.py:23-58
 * (linear(stack(hidden_states, dim=3), softmax(W, dim=1))[:, 0, :]) and MySPECTER.doc_reps_bert,
 * src/learning/facetid_models/disent_models.py:183-205; with layer_mix NULL the plain AutoModel read-out
 * last_hidden_state[:, 0, :] of the README (:101-164).  The encoder is aspire_bert_forward_f32's, with the
 * same weights, forms and accuracy, except that the last layer computes the CLS rows only: its QKV GEMM
 * runs over every row, then one attention query per (document, head) and the rest of the layer on the B
 * CLS rows.
 *   layer_mix   NULL, or a HOST array of n_layers + 1 weights (already softmaxed): hidden state 0 is the
 *               embedding LayerNorm output, i the output of layer i
 *   cls_out     [B, 768]  sum_i layer_mix[i] x hidden_states[i][:, 0, :]  (NULL mix: the last one's)
 *   layer_cls   NULL, or [n_layers + 1, B, 768]: the CLS row of every hidden state
 *   workspace   device scratch of aspire_bert_cls_workspace_bytes(w, B, L) bytes
 * The same argument checks as aspire_bert_forward_f32 (plus a finite layer_mix), all before any launch;
 * aspire_bert_status covers these forwards too.
 * ------------------------------------------------------------------------------------------- */
size_t aspire_bert_cls_workspace_bytes(const aspire_bert_weights* w, int64_t B, int64_t L);
int aspire_bert_forward_cls_f32(const aspire_bert_weights* w, const int64_t* tok_ids, const int64_t* type_ids,
                                const int64_t* attn_mask, int64_t B, int64_t L, const float* layer_mix, float* cls_out,
                                float* layer_cls, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1c  BERT pooler read-out.  Replaces `model_out.pooler_output` at src/evaluation/utils/models.py:350
 * (SimCSE.encode, :322-357: the 'supsimcse' / 'unsupsimcse' baselines; pre_proc_buildreps.py:105-127 writes
 * the same reps).  HuggingFace BertPooler: nn.Linear(768, 768) on last_hidden_state[:, 0], then nn.Tanh:
 *   pooled[b, n] = tanh( sum_k cls[b, k] * w_pool[n, k] + b_pool[n] )
 * fp32 throughout (exact fp32 products on the matrix cores, fp32 sums, the library's tanhf).
 *   cls     [B, 768]   the CLS rows aspire_bert_forward_cls_f32 wrote (layer_mix NULL)
 *   w_pool  [768, 768] pooler.dense.weight, nn.Linear layout;  b_pool [768] pooler.dense.bias
 *   pooled  [B, 768]   out; must not be cls
 * All four are contiguous device pointers, cls and w_pool 16-byte aligned.  Checked before any launch:
 * D != 768 -> ASPIRE_ERR_UNSUPPORTED; B < 0, a NULL pointer with B > 0, pooled == cls -> ASPIRE_ERR_INVALID_ARG;
 * B == 0 -> ASPIRE_OK without a launch.
 * ------------------------------------------------------------------------------------------- */
int aspire_bert_pooler_f32(const float* cls, int64_t B, int64_t D, const float* w_pool, const float* b_pool,
                           float* pooled, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1d  The SentenceTransformer baselines' encoders.  Replaces `self.model.encode(batch, show_progress_bar=False)` at
 * src/evaluation/utils/models.py:402 (SentenceModel.encode, :379-410: 'sbtinybertsota', 'sbrobertanli', 'sbmpnet1B'), i.e.
 * sentence-transformers' Transformer -> Pooling(mean) [-> Normalize] over HuggingFace BertModel / RobertaModel / MPNetModel.
 * All three have BERT-base geometry, erf-GELU and post-LayerNorm; what RoBERTa and MPNet add to aspire_bert_forward_f32 travels
 * in aspire_bert_extras:
 *   pos_ids   RoBERTa / MPNet number the real tokens from padding_idx + 1 and give every pad token padding_idx
 *             (create_position_ids_from_input_ids); the caller builds the table and guarantees 0 <= pos_ids < max_pos
 *             (aspire_amd checks it on the host, as it does token ids).
 *   rel_bias  MPNet's relative_attention_bias, expanded by the caller per key-minus-query distance (the bucket arithmetic of
 *             MPNetEncoder.relative_position_bucket stays on the host): scores are q.k / 8, + rel_bias, + the key-padding mask,
 *             then the soft-max, as HF MPNetSelfAttention; the same table in every layer.
 * aspire_bert_forward_var_f32 with x == NULL, or both pointers NULL, IS aspire_bert_forward_f32: the same plan, the same kernels
 * (instantiated without the bias), the same bits, the same workspace size (aspire_bert_workspace_bytes).  The same argument checks,
 * before any launch, plus rel_bias != NULL with rel_span < L -> ASPIRE_ERR_INVALID_ARG.  Every attention form carries the bias
 * except the 64-key tiles of aspire_debug_set("ATTN", "p64"): with a bias that form returns ASPIRE_ERR_UNSUPPORTED (before any
 * launch).  aspire_bert_status covers this forward too.  The CLS-only forward takes no extras.
 * MPNet has no token types: pass a type_emb of one zero row and type_ids NULL ((word + 0) + pos is exact).
 *
 * aspire_token_mean_pool_f32: the read-out behind it.
 *   out[b] = (sum over the tokens t with attn_mask[b, t] != 0, in token order, of hidden[b, t]) / max(count, 1e-9)
 *   normalize != 0: then out[b] / max(||out[b]||_2, 1e-12)                          (torch.nn.functional.normalize)
 * A row without a valid token gives zeros.  hidden [B, L, 768] and out [B, 768] contiguous, 16-byte aligned; rows of masked tokens
 * are not read.  D != 768 -> ASPIRE_ERR_UNSUPPORTED; B < 0, L <= 0, a NULL pointer with B > 0 -> ASPIRE_ERR_INVALID_ARG;
 * B == 0 -> ASPIRE_OK without a launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const int64_t* pos_ids;   /* device [B, L] or NULL: the row of pos_emb each token takes (NULL: its index, as BERT) */
    const float*   rel_bias;  /* device [n_heads, 2 * rel_span - 1] or NULL: added to the scaled score of (query i, key j):
                                 rel_bias[h][(j - i) + rel_span - 1], before the key-padding mask, in every layer */
    int32_t        rel_span;  /* >= L when rel_bias != NULL */
} aspire_bert_extras;
int aspire_bert_forward_var_f32(const aspire_bert_weights* w, const aspire_bert_extras* x, const int64_t* tok_ids,
                                const int64_t* type_ids, const int64_t* attn_mask, int64_t B, int64_t L, float* hidden_out,
                                void* workspace, size_t workspace_bytes, void* stream);
int aspire_token_mean_pool_f32(const float* hidden, const int64_t* attn_mask, int64_t B, int64_t L, int64_t D,
                               int normalize, float* out /* [B, D] */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1t  The BERT layer stack under training (fine_tune: true in the reference's configs: the encoder call of
 * disent_models.py:470-485 under autograd).  HuggingFace BertModel from the embedding sum to last_hidden_state -- the embedding
 * LayerNorm, then n_layers x [QKV, masked soft-max attention, output projection + residual + LayerNorm, GELU(erf) FFN + residual +
 * LayerNorm] -- with both dropout probabilities 0, and its backward to every parameter of that stack and to the embedding sum.
 * The table lookup (word + position + type rows) and its scatter gradient stay the caller's.  fp32 accuracy throughout.
 *
 * The forward runs the kernels aspire_bert_forward_f32 takes on fp32 operands (operands split into bf16 planes on the fly / the
 * fp32-input matrix cores, the three-kernel attention, LayerNorm as its own pass: no kernel waits on another workgroup, so
 * aspire_bert_status is not involved) and keeps on the caller's `tape`, per layer: the layer input, qkv, the soft-max probabilities
 * [B, heads, L, Lp = L rounded up to 4], the attention context, both pre-LayerNorm sums, the LN1 output and the PRE-GELU FFN1 output
 * (GELU is a pass of its own here; the backward forms GELU(u) again), and in front of layer 0 the embedding sum.  At B x L = 5 x 512,
 * 12 layers, ffn 3072: 94 MB of activations + 63 MB of probabilities per layer.
 *   emb_sum      [B, L, 768]  word + position + type embedding rows BEFORE the embedding LayerNorm
 *   w            emb_ln_g / emb_ln_b, layers, n_layers, n_heads, hidden, ffn_dim, ln_eps are read; word_emb / pos_emb / type_emb /
 *                vocab / max_pos / n_types / planes are not
 *   attn_mask    int64 [B, L], any 0/1 pattern; an all-zero row attends uniformly (as the forward above)
 *   hidden_out   [B, L, 768]  the bits of the fp32-operand forward (aspire_debug_set("GEMM", "bf16x3") + ("ATTN", "gemm"))
 *   tape         device, aspire_bert_tape_bytes(w, B, L) bytes; opaque; valid for backward calls until it is overwritten
 *   ws           device scratch, aspire_bert_train_workspace_bytes(w, B, L) bytes (one size serves both calls)
 * The backward: grad_hidden [B, L, 768] -> grad_emb_sum [B, L, 768] (may be NULL) and every pointer of `grads`, each shaped like the
 * weight of the same name.  Every gradient buffer is WRITTEN, not accumulated.  No atomics: column sums (bias and LayerNorm
 * gradients) go through per-row-block partials added in a fixed order, so two calls on one tape give the same bits.  attn_mask
 * must be the forward's (the masked keys' zeros are on the tape: it is checked, not read).
 * Checked before the first launch: a NULL pointer, L outside (0, 512], a tape or workspace smaller than the query functions say
 * -> ASPIRE_ERR_INVALID_ARG; hidden != 768, n_heads != 12, ffn_dim % 64 != 0 -> ASPIRE_ERR_UNSUPPORTED; B == 0 -> ASPIRE_OK
 * without a launch; n_layers == 0 is legal (the embedding LayerNorm alone).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float *w_qkv, *b_qkv, *w_o, *b_o, *ln1_g, *ln1_b, *w_ffn1, *b_ffn1, *w_ffn2, *b_ffn2, *ln2_g, *ln2_b;
} aspire_bert_layer_grads;

typedef struct {
    float *emb_ln_g, *emb_ln_b;
    aspire_bert_layer_grads* layers;            /* HOST array of n_layers entries (device pointers inside) */
} aspire_bert_grads;

size_t aspire_bert_tape_bytes(const aspire_bert_weights* w, int64_t B, int64_t L);
size_t aspire_bert_train_workspace_bytes(const aspire_bert_weights* w, int64_t B, int64_t L);
int aspire_bert_layers_forward_train_f32(const aspire_bert_weights* w, const float* emb_sum, const int64_t* attn_mask, int64_t B,
                                         int64_t L, float* hidden_out, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                                         void* stream);
int aspire_bert_layers_backward_f32(const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L,
                                    const float* grad_hidden, const void* tape, size_t tape_bytes, float* grad_emb_sum,
                                    const aspire_bert_grads* grads, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1t with dropout: BertModel.train() with hidden_dropout_prob / attention_probs_dropout_prob > 0.  The two calls above plus a
 * `dropout` argument; NULL, or a probability of 0, switches the sites of that probability off, and they then run exactly the
 * launches -- and give exactly the bits -- of the calls above.  Tape and workspace sizes are the same.
 *
 * No mask is stored: a mask is a function of (seed, step, site, element) that the forward and the backward each evaluate.
 *   generator  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85)
 *   key        (low word of seed, high word of seed); counter (block low, block high, site, step); block = e >> 2, and element e
 *              takes output word e & 3; e = the element's flat index in the tensor HuggingFace drops: [B, L, 768] at the hidden
 *              sites, [B, heads, L, L] for the probabilities (not the tape's padded rows)
 *   sites      0 after the embedding LayerNorm (p_hidden); layer l: 1 + 3 l the soft-max probabilities (p_attn), 2 + 3 l the
 *              output projection before the residual (p_hidden), 3 + 3 l the FFN2 output before the residual (p_hidden):
 *              HuggingFace's call order
 *   keep rule  keep iff word >= (uint32) floor((double) p * 2^32); kept elements are multiplied by 1.0f / (1.0f - p), dropped ones
 *              are 0.0f
 * The backward must be given the forward's struct.  Advance `step` once per training forward; the same (seed, step) gives the
 * same bits on every run.  A forward run again for the same step (activation checkpointing) must pass that step again: the
 * library keeps no counter.  p outside [0, 1) or NaN -> ASPIRE_ERR_INVALID_ARG (the value is in aspire_last_error()), checked
 * with the other arguments before the device is touched.
 *
 * aspire_bert_dropout_mask_u8 writes keep_out[i] = 1 if element first + i of `site` is kept, else 0, for i < n, with the device
 * function the training kernels use.  site < 0, first < 0, n < 0, keep_out NULL, p outside [0, 1) -> ASPIRE_ERR_INVALID_ARG;
 * n == 0 -> ASPIRE_OK without a launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float    p_hidden;        /* hidden_dropout_prob: sites 0, 2 + 3 l, 3 + 3 l */
    float    p_attn;          /* attention_probs_dropout_prob: sites 1 + 3 l */
    uint64_t seed;
    uint32_t step;
} aspire_bert_dropout;

int aspire_bert_layers_forward_train_dropout_f32(const aspire_bert_weights* w, const float* emb_sum, const int64_t* attn_mask,
                                                 int64_t B, int64_t L, float* hidden_out, void* tape, size_t tape_bytes, void* ws,
                                                 size_t ws_bytes, const aspire_bert_dropout* dropout, void* stream);
int aspire_bert_layers_backward_dropout_f32(const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L,
                                            const float* grad_hidden, const void* tape, size_t tape_bytes, float* grad_emb_sum,
                                            const aspire_bert_grads* grads, void* ws, size_t ws_bytes,
                                            const aspire_bert_dropout* dropout, void* stream);
int aspire_bert_dropout_mask_u8(uint64_t seed, uint32_t step, int32_t site, float p, int64_t first, int64_t n,
                                unsigned char* keep_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1t for the CLS-row models: the read-out of MySPECTER (cospecter; disent_models.py:178-205: torch.stack of hidden_states,
 * SoftmaxMixLayers, [:, 0, :]) and of SentBERTWrapper / ICTBERTWrapper (cosentbert / ictsentbert; sentsim_models.py:62-78:
 * last_hidden_state[:, 0, :]) under training, and its gradient as one more source of the backward above.
 *
 * aspire_bert_cls_mix_train_f32: call it after aspire_bert_layers_forward_train[_dropout]_f32, on that call's tape and hidden_out.
 * Hidden state l < n_layers is the tape's layer-l input (under dropout state 0 is the embedding LayerNorm output AFTER site 0's
 * dropout: HuggingFace's hidden_states[0]); state n_layers is hidden_out.  The tape stays opaque: only this entry knows where the
 * layer inputs lie.
 *   mix        device [n_layers + 1] post-soft-max weights, or NULL
 *   layer_cls  [n_layers + 1, B, 768]: the CLS rows of every state; may be NULL when mix is NULL
 *   cls_out    [B, 768] = sum_l mix[l] * state_l[b, 0, :], l ascending in fp32; mix NULL: the top state's CLS rows, bit for bit
 *
 * aspire_bert_layers_backward_cls_f32: aspire_bert_layers_backward_dropout_f32 with one more gradient source.  Row (b, 0) of the
 * gradient of hidden state l additionally receives mix[l] * grad_cls[b, :] for every l in 0 .. n_layers (mix NULL: the top state
 * alone, factor 1): below the top a B x 768 row update on the residual branch's gradient between a layer's backward and the LayerNorm
 * backward that adds the two branches; for state 0 before the backward of site 0's dropout.  grad_hidden may be NULL: the top
 * gradient is then zeros plus the CLS rows, formed in the workspace (no [B, L, 768] gradient crosses the interface).
 *   grad_mix   device [n_layers + 1] or NULL: grad_mix[l] = sum_b <grad_cls[b], layer_cls[l, b]>, one workgroup per l, fixed order
 *   dropout    NULL or the forward's struct, as above
 * Tape and workspace sizes are unchanged.  No atomics, one writer per element: two calls on one tape give the same bits.  Checked
 * before the first launch, beyond the checks above: grad_cls and grad_hidden both NULL, grad_mix with layer_cls / mix / grad_cls
 * NULL -> ASPIRE_ERR_INVALID_ARG; B == 0 -> ASPIRE_OK without a launch.
 *
 * aspire_inbatch_xent_f32 / _backward_f32: ICTBERTWrapper.forward_rank's loss (sentsim_models.py:81-126: torch.matmul(q, c.T) into
 * nn.CrossEntropyLoss(reduction='sum') against targets arange(B)) over q, c [B, 768], 16-byte aligned.
 *   s = Q C^T (exact fp32 products on the matrix cores, as aspire_dotmax_scores_f32);  row_lse[i] = max-shifted logsumexp_j s_ij
 *   loss[0] = sum_i (row_lse[i] - s_ii), a fixed order;  B == 1 gives exactly 0
 *   backward: W_ij = grad_loss[0] * (exp(s_ij - row_lse[i]) - [i == j]), grad_q[i] = sum_j W_ij c_j, grad_c[j] = sum_i W_ij q_i; the
 *   dot products are formed again on the matrix cores, and with them every row's maximum m_i and normaliser z_i, kept apart:
 *   W_ij = grad_loss[0] * (exp(s_ij - m_i) / z_i - [i == j]), so a row of weights sums to 0 to a rounding at any |s| (m_i + log z_i
 *   rounded to one float loses log z_i's low bits at |s| of several hundred, where one ulp is 6e-5).  row_lse is therefore checked
 *   for NULL but not read.  Every row is written once by the workgroup that owns it; no atomics, the same bits on every run
 * B in [1, 128] (the document-row limit); B > 128 or D != 768 -> ASPIRE_ERR_UNSUPPORTED (the value is in aspire_last_error()); a NULL
 * pointer -> ASPIRE_ERR_INVALID_ARG; B == 0 -> ASPIRE_OK without a launch.
 * ------------------------------------------------------------------------------------------- */
int aspire_bert_cls_mix_train_f32(const aspire_bert_weights* w, int64_t B, int64_t L, const void* tape, size_t tape_bytes,
                                  const float* hidden_out, const float* mix, float* cls_out, float* layer_cls, void* stream);
int aspire_bert_layers_backward_cls_f32(const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L,
                                        const float* grad_hidden, const float* grad_cls, const float* mix, const float* layer_cls,
                                        const void* tape, size_t tape_bytes, float* grad_emb_sum, const aspire_bert_grads* grads,
                                        float* grad_mix, void* ws, size_t ws_bytes, const aspire_bert_dropout* dropout, void* stream);
int aspire_inbatch_xent_f32(const float* q, const float* c, int64_t B, int64_t D, float* loss, float* row_lse, void* stream);
int aspire_inbatch_xent_backward_f32(const float* q, const float* c, int64_t B, int64_t D, const float* row_lse,
                                     const float* grad_loss, float* grad_q, float* grad_c, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1t with the matrix products in bf16 (opt-in): "matrix products in bf16, everything else in fp32", what
 * torch.autocast(dtype=torch.bfloat16) asks of a BertModel's linears and matmuls.
 *
 * aspire_bert_layers_forward_train_prec_f32 / aspire_bert_layers_backward_prec_f32 are
 * aspire_bert_layers_forward_train_dropout_f32 / aspire_bert_layers_backward_cls_f32 plus `matmul`:
 *   ASPIRE_MATMUL_FP32  those calls: the same launches, the same bits
 *   ASPIRE_MATMUL_BF16  all 16 products of a layer (QKV, out, FFN1, FFN2 projections, Q K^T, P V forward; the ten of the backward)
 *                       in the arithmetic below; LayerNorm, soft-max, GELU, column sums, dropout, the CLS mix and their backwards
 *                       stay fp32 launches.  The tape stays fp32 in the same layout (the two size queries are unchanged), the
 *                       weights stay fp32 and are rounded per use: no bf16 copy exists, nothing to refresh after an optimizer step
 *   ASPIRE_MATMUL_BF16X3  fp32 accuracy on the bf16 matrix cores (opt-in as well).  The NT products (the four projections, Q K^T, dP)
 *                       are ASPIRE_MATMUL_FP32's launches -- already that arithmetic wherever K % 16 == 0, which every NT product of
 *                       the layer stack is -- so the forward differs from ASPIRE_MATMUL_FP32 in P V alone; the B_KN products (P V,
 *                       da, dh, dctx, dx, dQ) and the TN products (every dW, dV, dK) leave the fp32-input matrix cores for the
 *                       bf16x3 arithmetic below.  Everything else as in ASPIRE_MATMUL_BF16: the same fp32 launches, tape and weights
 *   any other value     ASPIRE_ERR_INVALID_ARG before the device is touched, the value in aspire_last_error().  2 among them: the
 *                       value was a rejected mode before ASPIRE_MATMUL_BF16X3 existed and callers and tests rely on that, so the
 *                       enum skips it
 * The forward and the backward of one step take the same mode.
 *
 * The arithmetic of a bf16x3 product C = alpha A B (+ bias) (+ GELU) (+ residual), and nothing else:
 *   - every element of A and B is split ONCE, when its tile is staged from the fp32 tensor, into three bf16 values x = x1 + x2 + x3:
 *     x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2), each round to nearest even, both subtractions exact (24 mantissa bits);
 *   - a product a b is the six terms a3 b1, a1 b3, a2 b2, a2 b1, a1 b2, a1 b1, each exact in fp32, added in that order (smallest
 *     first); the three dropped terms a2 b3 + a3 b2 + a3 b3 are below 2^-23 |a| |b| (|a2| <= 2^-8 |a|, |a3| <= 2^-16 |a|):
 *     of the order of fp32's own rounding;
 *   - the sums over K are the matrix cores' fp32 accumulators in a fixed order.  In the B_KN and TN forms a1 b1 has an accumulator of
 *     its own and the five correction terms share a second one, added once at the end (the matrix cores cut addends far below the
 *     running sum toward minus infinity; kept apart, the small terms are not cut).  One level in the B_KN form; the TN form, which
 *     contracts over token rows, adds both to a further set every 256 k (the fp32 TN form's two levels);
 *   - alpha, bias, GELU and the residual are fp32;
 *   - no atomics, one writer per element of C: the same bits on every run;
 *   - a non-finite element of A or B (or one that rounds past bf16's largest finite) splits into a NaN plane (inf - inf): its output
 *     row or column is NaN, as in the NT form of the fp32 mode.
 *
 * The arithmetic of a bf16 product C = alpha A B (+ bias) (+ GELU) (+ residual), and nothing else:
 *   - every element of A and B is rounded to bf16 ONCE, round to nearest even, when its tile is staged from the fp32 tensor: the
 *     values of torch.Tensor.to(torch.bfloat16) -- +-0, ties and +-inf as torch gives them, NaN stays NaN, a magnitude that rounds past
 *     bf16's largest finite becomes inf;
 *   - a product of two bf16 values is exact in fp32;
 *   - the sum over K is the matrix cores' fp32 accumulator in a fixed order, one level in all three forms;
 *   - alpha, bias, GELU and the residual are fp32;
 *   - no atomics, one writer per element of C: the same bits on every run.
 *
 * aspire_debug_gemm_bf16_f32: one such product, for tests and tools.  Per matrix C [M, N] (row stride ldc), by `form`:
 *   ASPIRE_GEMM_NT    A [M, K] (lda), B [N, K] (ldb), both k-contiguous
 *   ASPIRE_GEMM_BKN   A [M, K] (lda), B [K, N] (ldb)
 *   ASPIRE_GEMM_TN    A [K, M] (lda), B [K, N] (ldb): C = A^T B
 * `batch` matrices, matrix z = z1 * nz2 + z2 at offsets z1 * s?1 + z2 * s?2 floats of A, B and C (attention: z1 the document, z2
 * the head); bias [N] or NULL; res [M, ldr] or NULL (not batched); gelu != 0 applies GELU before the residual.  Any M, N, K (tails
 * are zero-filled when staged, nothing is read past an operand's rows); A and B 16-byte aligned, lda, ldb and their batch strides
 * multiples of 4.  A NULL A / B / C, a negative size, an unknown form, nz2 < 1, a leading dimension shorter than its row or a
 * misaligned operand -> ASPIRE_ERR_INVALID_ARG; M, N, K or batch == 0 -> ASPIRE_OK without a launch (C is not written).
 * aspire_debug_get("GEMM_BF16_LAST") reads which kernel instantiation the latest bf16 product of this process launched, as
 * 3 * form + tile (tile 0: 128 x 128, 1: 128 x 64, 2: 64 x 64; chosen by shape, aspire_debug_set("GEMM_TILE", "128" | "64") pins),
 * -1 before the first.
 *
 * aspire_debug_gemm_bf16x3_f32: one bf16x3 product, the same arguments and checks.  ASPIRE_GEMM_BKN and ASPIRE_GEMM_TN run the
 * arithmetic above for any M, N, K; ASPIRE_GEMM_NT is what the mode launches for an NT product, the fp32 mode's GEMM (bf16x3 where
 * K % 16 == 0, else the fp32-input matrix cores), and asks K % 4 == 0 as that GEMM does.  aspire_debug_get("GEMM_BF16X3_LAST"): the
 * instantiation of the latest B_KN or TN launch of this process as 3 * form + tile (3 .. 8; the tiles and the pin as above), -1
 * before the first; an NT product does not change it.
 * ------------------------------------------------------------------------------------------- */
enum { ASPIRE_MATMUL_FP32 = 0, ASPIRE_MATMUL_BF16 = 1, ASPIRE_MATMUL_BF16X3 = 3,        /* 2 is not a mode (above) */
       ASPIRE_MATMUL_FP16 = 4 };   /* the INFERENCE forwards' mode (A1h below); the training entries refuse it like any other value */
enum { ASPIRE_GEMM_NT = 0, ASPIRE_GEMM_BKN = 1, ASPIRE_GEMM_TN = 2 };

int aspire_bert_layers_forward_train_prec_f32(const aspire_bert_weights* w, const float* emb_sum, const int64_t* attn_mask, int64_t B,
                                              int64_t L, float* hidden_out, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                                              const aspire_bert_dropout* dropout, int matmul, void* stream);
int aspire_bert_layers_backward_prec_f32(const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L,
                                         const float* grad_hidden, const float* grad_cls, const float* mix, const float* layer_cls,
                                         const void* tape, size_t tape_bytes, float* grad_emb_sum, const aspire_bert_grads* grads,
                                         float* grad_mix, void* ws, size_t ws_bytes, const aspire_bert_dropout* dropout, int matmul,
                                         void* stream);
int aspire_debug_gemm_bf16_f32(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                               int64_t ldc, int form, int64_t batch, int64_t nz2, int64_t sa1, int64_t sa2, int64_t sb1, int64_t sb2,
                               int64_t sc1, int64_t sc2, float alpha, const float* bias, const float* res, int64_t ldr, int gelu,
                               void* stream);
int aspire_debug_gemm_bf16x3_f32(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                                 int64_t ldc, int form, int64_t batch, int64_t nz2, int64_t sa1, int64_t sa2, int64_t sb1, int64_t sb2,
                                 int64_t sc1, int64_t sc2, float alpha, const float* bias, const float* res, int64_t ldr, int gelu,
                                 void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1h  The inference forwards with the matrix products in fp16 (opt-in): "matrix products in 16 bits, everything else fp32", the
 * trade a user of HuggingFace `.half()` makes, for the encoder calls of examples/ex_aspire_consent.py:72-73 (A1),
 * examples/ex_aspire_bienc.py:23-58 (A1b) and src/evaluation/utils/models.py:379-410 (A1d).  The default path holds every nn.Linear
 * operand as two fp16 planes and pays three matrix instructions per term; this mode holds ONE plane and pays one.
 *
 * aspire_bert_forward_prec_f32 is aspire_bert_forward_var_f32 (x may be NULL: aspire_bert_forward_f32) and
 * aspire_bert_forward_cls_prec_f32 is aspire_bert_forward_cls_f32, plus `hplanes` and `matmul`:
 *   ASPIRE_MATMUL_FP32  those calls: the same launches, the same bits; hplanes is not read
 *   ASPIRE_MATMUL_FP16  the arithmetic below, at every B x L (the mode has no row threshold); hplanes == NULL ->
 *                       ASPIRE_ERR_INVALID_ARG
 *   any other value     ASPIRE_ERR_INVALID_ARG (ASPIRE_MATMUL_BF16 and ASPIRE_MATMUL_BF16X3 are the training entries' modes)
 * All checks -- those of the plain entries, then these -- run before the first launch and touch no device.
 *
 * The mode's arithmetic, and nothing else:
 *   - in the QKV, attention output, FFN1 and FFN2 projections every operand element is rounded to fp16 ONCE, round to nearest even:
 *     activations as they are, weights as fp16(64 w) with the factor taken off exactly in the epilogue;
 *   - a product of two fp16 values is exact in fp32; the sums over K are the matrix cores' fp32 accumulators in a fixed order;
 *   - bias, residual and GELU are fp32; GELU(FFN1) is rounded to fp16 once, as the operand of FFN2 (no fp32 [B L, ffn] exists);
 *   - no atomics, no waits inside a kernel (aspire_bert_status plays no part), no device globals, one writer per output element: the
 *     same bits on every run, also from several streams at once (one workspace per stream);
 *   - the residual stream, LayerNorm, the embeddings, the attention (Q K^T, soft-max, P V: an existing attention kernel on the fp32
 *     Q / K / V the mode's QKV projection writes), the CLS forward's last-layer tail on the B CLS rows, the pooler and every read-out
 *     keep the accuracy they have in ASPIRE_MATMUL_FP32;
 *   - an activation beyond 65504 becomes inf in the operand and shows as non-finite output: check the output and run again after
 *     aspire_debug_set("GEMM", "bf16x3") + ("ATTN", "f32") (aspire_amd's run_checked does) -- a GEMM pin (aspire_debug_set("GEMM", ..)
 *     or ASPIRE_HIP_GEMM) overrides the mode: such a forward runs ASPIRE_MATMUL_FP32's plan.
 * The mode needs 64-wide heads and ffn_dim % 128 == 0 (BERT-base); otherwise, and with n_layers == 0, the forward is
 * ASPIRE_MATMUL_FP32's.
 *
 *   hplanes   a DEVICE buffer of aspire_bert_hplanes_bytes(w) bytes, filled once by aspire_bert_prepare_hplanes when the model is
 *             loaded (synchronises the stream; ASPIRE_ERR_UNSUPPORTED for a weight that is not finite or has |64 w| > 65504).  An
 *             argument, not a field: aspire_bert_weights keeps its layout.
 *   workspace aspire_bert_workspace_bytes_prec / aspire_bert_cls_workspace_bytes_prec (w, B, L, matmul) bytes (0 for a matmul value
 *             that is no mode of these entries)
 *
 * The layout of an operand ("H layout") of X [R, K], K % 32 == 0: per 32-wide k block kb and row r four 16-byte pieces q = 0 .. 3 = the
 * 8 fp16 at k = 32 kb + 8 q .. + 7, at piece index (kb R + r) 4 + (q ^ ((r >> 2) & 3)); 256 rows of slack behind the matrix:
 * (R + 256) K 2 bytes.  For tests and tools:
 *   aspire_debug_hplane_bytes(R, K)      that size
 *   aspire_debug_split_hplane            X fp32 [R, K] contiguous -> H (weight != 0: 64 X, the B side of a product)
 *   aspire_debug_gemm_hplane             one product on H operands A [M, K] and B [N, K] (split with weight != 0); any M >= 1,
 *                                        N % 64 == 0, K % 32 == 0.  epilogue 0: C [M, N] fp32 = A B^T (+ bias [N]) (+ res [M, N]);
 *                                        epilogue 1: Ch [M, N] in the H layout = GELU(A B^T + bias), res must be NULL.  Rows of A
 *                                        behind M (the slack) are read and never written to C / Ch.
 * ------------------------------------------------------------------------------------------- */
size_t aspire_bert_hplanes_bytes(const aspire_bert_weights* w);
int aspire_bert_prepare_hplanes(const aspire_bert_weights* w, void* hplanes, size_t hplanes_bytes, void* stream);
size_t aspire_bert_workspace_bytes_prec(const aspire_bert_weights* w, int64_t B, int64_t L, int matmul);
size_t aspire_bert_cls_workspace_bytes_prec(const aspire_bert_weights* w, int64_t B, int64_t L, int matmul);
int aspire_bert_forward_prec_f32(const aspire_bert_weights* w, const aspire_bert_extras* x, const void* hplanes, int matmul,
                                 const int64_t* tok_ids, const int64_t* type_ids, const int64_t* attn_mask, int64_t B, int64_t L,
                                 float* hidden_out, void* workspace, size_t workspace_bytes, void* stream);
int aspire_bert_forward_cls_prec_f32(const aspire_bert_weights* w, const void* hplanes, int matmul, const int64_t* tok_ids,
                                     const int64_t* type_ids, const int64_t* attn_mask, int64_t B, int64_t L, const float* layer_mix,
                                     float* cls_out, float* layer_cls, void* workspace, size_t workspace_bytes, void* stream);
size_t aspire_debug_hplane_bytes(int64_t R, int64_t K);
int aspire_debug_split_hplane(const float* X, int64_t R, int64_t K, void* H, int weight, void* stream);
int aspire_debug_gemm_hplane(const void* Ah, const void* Bh, float* C, void* Ch, const float* bias, const float* res, int64_t M,
                             int64_t N, int64_t K, int epilogue, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1t with a fused attention (opt-in, with ASPIRE_MATMUL_BF16 only): no [L, L] tensor on the tape or in the workspace.
 *
 * aspire_bert_layers_forward_train_attn_f32 / aspire_bert_layers_backward_attn_f32 are the _prec_ entries plus `attention`:
 *   ASPIRE_ATTENTION_GEMM   those calls (the _prec_ entries forward here with it): the same launches, the same bits
 *   ASPIRE_ATTENTION_FLASH  per layer, the forward's Q K^T, soft-max, dropout and P V launches become ONE kernel that writes ctx and, per
 *                           (document, head, query), two fp32 statistics -- the row maximum m of the scaled, masked scores in log2
 *                           units and the row sum l of exp2(s - m) over the UNdropped probabilities -- in the tape slot that held P;
 *                           the backward's launches over [B, 12, L, L] become three kernels: D = rowsum(bf16(dctx) . ctx), a key-block
 *                           kernel (dK, dV) and a query-block kernel (dQ), which form P = exp2(s - m) / l and the dropout mask again.
 *                           Valid with ASPIRE_MATMUL_BF16 alone: any other matmul mode -> ASPIRE_ERR_UNSUPPORTED
 *   any other value         ASPIRE_ERR_INVALID_ARG before the device is touched
 * The forward and the backward of one step take the same modes, and a tape and a workspace of the _attn size queries
 * (aspire_bert_tape_bytes_attn, aspire_bert_train_workspace_bytes_attn: host only; with ASPIRE_ATTENTION_GEMM the values of
 * aspire_bert_tape_bytes / aspire_bert_train_workspace_bytes, with ASPIRE_ATTENTION_FLASH linear in L; 0 for an unknown mode).
 * aspire_bert_cls_mix_train_attn_f32 is aspire_bert_cls_mix_train_f32 on a tape of that mode (the layer inputs sit at other offsets).
 *
 * The arithmetic of the fused attention, and nothing else: Q, K, V and dctx are rounded to bf16 once (round to nearest even) as their
 * tiles are staged; scores, the online exp2 soft-max, m, l and D are fp32; HuggingFace's mask semantics as in every other form (a
 * masked key adds the finite -FLT_MAX; a document without a real key attends uniformly -- which is why m and l are two values:
 * -FLT_MAX + log2(L) rounds back to -FLT_MAX); the forward rounds the UNNORMALISED probability exp2(s - m_running), times keep . scale
 * where the site drops, to bf16 on its way into the product with V and divides by l in fp32; the backward rounds
 * P_drop = keep scale exp2(s - m) / l and dS = P (keep scale (dctx V^T) - D) to bf16 as they enter dV = P_drop^T dctx,
 * dK = dS^T Q / 8 and dQ = dS K / 8 (the 1 / 8 in fp32).  Dropout: site 1 + 3 layer on the logical index ((b 12 + h) L + i) L + j
 * (aspire_bert_dropout_mask_u8's masks).  No atomics, one writer per element, fixed summation orders: the same bits on every run.
 *
 * aspire_debug_flash_attn_train_f32 / aspire_debug_flash_attn_train_backward_f32: the bare kernels, for tests and tools.  qkv
 * [B L, 2304] fp32, mask int64 [B, L], ctx / dctx [B L, 768], stats [B, 12, L, 2] = (m, l), dqkv [B L, 2304] = [dQ | dK | dV]; 12 heads
 * of 64, L in 1 .. 512.  dropout NULL or p_attn == 0: none; else p_attn, seed and step of the struct at the site of `layer` (the
 * forward entry: layer 0).  D [B, 12, L] fp32 is the backward's scratch, the caller's as in the layer stack (written, then read by the
 * two kernels behind it on the same stream): the entry allocates nothing and does not wait for the stream.
 * ------------------------------------------------------------------------------------------- */
#define ASPIRE_ATTENTION_GEMM 0
#define ASPIRE_ATTENTION_FLASH 1

size_t aspire_bert_tape_bytes_attn(const aspire_bert_weights* w, int64_t B, int64_t L, int attention);
size_t aspire_bert_train_workspace_bytes_attn(const aspire_bert_weights* w, int64_t B, int64_t L, int attention);
int aspire_bert_layers_forward_train_attn_f32(const aspire_bert_weights* w, const float* emb_sum, const int64_t* attn_mask, int64_t B,
                                              int64_t L, float* hidden_out, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                                              const aspire_bert_dropout* dropout, int matmul, int attention, void* stream);
int aspire_bert_layers_backward_attn_f32(const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L,
                                         const float* grad_hidden, const float* grad_cls, const float* mix, const float* layer_cls,
                                         const void* tape, size_t tape_bytes, float* grad_emb_sum, const aspire_bert_grads* grads,
                                         float* grad_mix, void* ws, size_t ws_bytes, const aspire_bert_dropout* dropout, int matmul,
                                         int attention, void* stream);
int aspire_bert_cls_mix_train_attn_f32(const aspire_bert_weights* w, int64_t B, int64_t L, const void* tape, size_t tape_bytes,
                                       const float* hidden_out, const float* mix, float* cls_out, float* layer_cls, int attention,
                                       void* stream);
int aspire_debug_flash_attn_train_f32(const float* qkv, const int64_t* mask, int64_t B, int64_t L, const aspire_bert_dropout* dropout,
                                      float* ctx, float* stats, void* stream);
int aspire_debug_flash_attn_train_backward_f32(const float* qkv, const int64_t* mask, const float* ctx, const float* stats,
                                               const float* dctx, int64_t B, int64_t L, const aspire_bert_dropout* dropout, int layer,
                                               float* D, float* dqkv, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1t without padding (opt-in, with ASPIRE_MATMUL_BF16 and ASPIRE_ATTENTION_FLASH only): the layer stack, its tape and its workspace hold
 * the R = sum(attention mask) valid token rows alone, where the calls above run every launch over B L rows of a batch padded to its
 * longest document -- what the reference's forward does (disent_models.py:178-205 and sentsim_models.py:62-78 call BertModel on the
 * padded tokid_tt / attnmask_tt that batchers.py:249 / :627 build).  A pad row buys nothing: no read-out reads one, a masked key has
 * probability exactly 0, so no parameter gradient depends on one.
 *
 * aspire_bert_packing describes the batch (aspire_amd.packed_rows builds it from the mask, with one host read of the totals): packed
 * rows are in document order and, inside a document, in position order; a mask with holes or left padding packs the same way.
 *   rows        R, 0 .. B L
 *   max_len     the longest document's rows (0 iff rows == 0), at most L
 *   prefix      nonzero iff every document's rows are its positions 0 .. len - 1 (right padding alone)
 *   doc_start   device int32 [B + 1]: document b's rows are doc_start[b] .. doc_start[b + 1] - 1
 *   row_src     device int32 [R]: the padded row b L + l of packed row m
 *   row_dst     device int32 [B L]: the packed row of a padded row, or -1
 * B L < 2^31.  The host checks the pointers, rows <= B L, max_len <= L and the modes before anything is read; the lists' contents are
 * the caller's, and the kernels clamp what they read from them into their tensors.
 *
 * Semantics.  emb_sum, hidden_out, grad_hidden and grad_emb_sum keep the padded layout [B, L, 768]; the entries gather and scatter
 * inside the call.  Valid rows of hidden_out are the mode's result; masked rows are EXACT ZEROS (a deliberate departure: HuggingFace
 * computes something there); a document whose mask is all zero has no rows and its output rows are zeros; rows == 0 returns zeros and
 * launches nothing.  grad_emb_sum has exact zeros on masked rows, and grad_hidden is read on valid rows only.  The CLS read-out takes
 * each document's CLS row at its FIRST packed row: the caller guarantees mask[:, 0] == 1 for every document (the Python layer raises
 * ValueError otherwise, before a launch).  Dropout is keyed by the PADDED logical index, the one the calls above use -- row b L + l for
 * the hidden sites, ((b 12 + h) L + i) L + j with i, j the tokens' original positions for the probabilities -- so with the same
 * (seed, step) a packed step draws, at valid positions, the masks a padded step draws (aspire_bert_dropout_mask_u8 serves as it
 * stands).  One draw per four keys is taken only when prefix != 0 and L % 4 == 0; the mask bits are the same either way.  No atomics:
 * every element of every output has one writer and every sum a fixed order, the same bits on every run.
 *
 * aspire_bert_tape_bytes_packed / aspire_bert_train_workspace_bytes_packed: host only, 0 for rows <= 0 or rows > B L; the tape is that
 *   of ASPIRE_ATTENTION_FLASH with M = rows (statistics [12, R, 2]), so at most aspire_bert_tape_bytes_attn's and below it as soon as one
 *   row is masked.
 * aspire_bert_layers_forward_train_packed_f32 / aspire_bert_layers_backward_packed_f32: the _attn_ entries with `packing` where the mask
 *   was (no mask is read: every key of a document is real); the backward takes the CLS source arguments of
 *   aspire_bert_layers_backward_attn_f32.  matmul must be ASPIRE_MATMUL_BF16 and attention ASPIRE_ATTENTION_FLASH: anything else
 *   -> ASPIRE_ERR_UNSUPPORTED (or ASPIRE_ERR_INVALID_ARG for an unknown mode) before the device is touched.
 * aspire_bert_cls_mix_train_packed_f32: aspire_bert_cls_mix_train_attn_f32 on a packed tape; hidden_out is the padded [B, L, 768].
 * aspire_debug_flash_attn_train_packed_f32 / _packed_backward_f32: the bare kernels over packed rows, for tests and tools: qkv / dqkv
 *   [R, 2304], ctx / dctx [R, 768], stats [12, R, 2], D [12, R]; L is the padded length, which the dropout keys are made of.
 * ------------------------------------------------------------------------------------------- */
typedef struct aspire_bert_packing {
    int64_t rows;
    int32_t max_len;
    int32_t prefix;
    const int32_t* doc_start;
    const int32_t* row_src;
    const int32_t* row_dst;
} aspire_bert_packing;

size_t aspire_bert_tape_bytes_packed(const aspire_bert_weights* w, int64_t B, int64_t L, int64_t rows);
size_t aspire_bert_train_workspace_bytes_packed(const aspire_bert_weights* w, int64_t B, int64_t L, int64_t rows);
int aspire_bert_layers_forward_train_packed_f32(const aspire_bert_weights* w, const float* emb_sum, const aspire_bert_packing* packing,
                                                int64_t B, int64_t L, float* hidden_out, void* tape, size_t tape_bytes, void* ws,
                                                size_t ws_bytes, const aspire_bert_dropout* dropout, int matmul, int attention, void* stream);
int aspire_bert_layers_backward_packed_f32(const aspire_bert_weights* w, const aspire_bert_packing* packing, int64_t B, int64_t L,
                                           const float* grad_hidden, const float* grad_cls, const float* mix, const float* layer_cls,
                                           const void* tape, size_t tape_bytes, float* grad_emb_sum, const aspire_bert_grads* grads,
                                           float* grad_mix, void* ws, size_t ws_bytes, const aspire_bert_dropout* dropout, int matmul,
                                           int attention, void* stream);
int aspire_bert_cls_mix_train_packed_f32(const aspire_bert_weights* w, const aspire_bert_packing* packing, int64_t B, int64_t L,
                                         const void* tape, size_t tape_bytes, const float* hidden_out, const float* mix, float* cls_out,
                                         float* layer_cls, void* stream);
int aspire_debug_flash_attn_train_packed_f32(const float* qkv, const aspire_bert_packing* packing, int64_t B, int64_t L,
                                             const aspire_bert_dropout* dropout, float* ctx, float* stats, void* stream);
int aspire_debug_flash_attn_train_packed_backward_f32(const float* qkv, const aspire_bert_packing* packing, const float* ctx,
                                                      const float* stats, const float* dctx, int64_t B, int64_t L,
                                                      const aspire_bert_dropout* dropout, int layer, float* D, float* dqkv, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The embedding lookup under training: BertEmbeddings' sum in front of aspire_bert_layers_forward_train_f32 and the three tables'
 * gradients behind aspire_bert_layers_backward_f32 (what nn.Embedding's forward and scatter backward do on the reference path).
 * Hidden size 768.  Token rows m = b L + l, M = B L.  word [vocab, 768], pos [max_pos, 768], type [n_types, 768]; tok, typ int64
 * [B, L] on the device, typ may be NULL (every token of type 0).  Tables, out and the gradients are 16-byte aligned.
 *
 * aspire_bert_embed_sum_f32:  out[b, l, :] = (word[tok[b, l]] + type[typ[b, l]]) + pos[l], plain fp32 adds in BertEmbeddings'
 *   order (torch's bits).  One wave per token row.  A row whose id lies outside [0, vocab) or whose type lies outside [0, n_types)
 *   is never turned into an address: that row of out is NaN.
 *
 * aspire_bert_embed_backward_f32:  grad_emb_sum [B, L, 768] -> grad_word [vocab, 768], grad_pos [max_pos, 768], grad_type
 *   [n_types, 768].  Each output pointer may be NULL: that table is not wanted and nothing is launched for it.  Every row of every
 *   wanted table is WRITTEN (the buffers need no zero-fill; rows that no token names are exact zeros), every element by one writer,
 *   no atomics: the same bits on every run.  All sums are plain fp32 adds in these orders:
 *     grad_word[v]   the rows grad_emb_sum[m] with tok[m] == v, added one after the other in ascending m, starting from the first
 *                    row; zeros for v == padding_idx (nn.Embedding's padding row has no gradient; padding_idx = -1: there is no such
 *                    row) and for an id no token has.  A token whose id lies outside [0, vocab) contributes to no row.
 *     grad_pos[l]    grad_emb_sum[0, l] + grad_emb_sum[1, l] + ... in ascending b, for l < L; zeros for l >= L.
 *     grad_type[t]   two stages whose order depends on M alone.  R = ceil(M / 64) rows per block; partial_j, j = 0 .. 63, starts at
 *                    0 and adds, in ascending m, the rows m in [j R, min((j + 1) R, M)) with typ[m] == t (a block without such a
 *                    row, or beyond M, stays 0); grad_type[t] starts at 0 and adds partial_0 .. partial_63 in ascending j.  A
 *                    type outside [0, n_types) contributes to no row.
 *   The word table: the keys (tok[m], m) are ranked by counting -- every token counts the keys below its own, M^2 integer compares,
 *   no data-dependent exchange -- and m goes to order[rank]; then one wave per table row finds its run of the sorted ids with a
 *   binary search and adds the run's gradient rows.  A row that one id fills is a serial chain of M adds on one wave.
 *   workspace   device memory of at least aspire_bert_embed_workspace_bytes(M, vocab) bytes (a multiple of 16, growing with M),
 *               16-byte aligned; read and written only when grad_word is wanted.
 *   The rank pass serves at most 65 536 token rows: grad_word wanted with M above that -> ASPIRE_ERR_UNSUPPORTED.
 * Errors, all before the device is touched, the offending value in aspire_last_error(): ASPIRE_ERR_INVALID_ARG for a NULL word / pos /
 * type / tok / out (forward), a NULL grad_emb_sum with a wanted table, a NULL tok with grad_word wanted, B < 0, L outside
 * (0, max_pos], vocab, max_pos or n_types <= 0, padding_idx outside [-1, vocab), a pointer that is not 16-byte aligned, a workspace
 * that is NULL or too small when grad_word is wanted.  B == 0, or all three outputs NULL -> ASPIRE_OK without a launch.
 * ------------------------------------------------------------------------------------------- */
int aspire_bert_embed_sum_f32(const float* word, const float* pos, const float* type, const int64_t* tok, const int64_t* typ, int64_t B,
                              int64_t L, int64_t vocab, int64_t max_pos, int64_t n_types, float* out, void* stream);
size_t aspire_bert_embed_workspace_bytes(int64_t M, int64_t vocab);
int aspire_bert_embed_backward_f32(const float* grad_emb_sum, const int64_t* tok, const int64_t* typ, int64_t B, int64_t L, int64_t vocab,
                                   int64_t max_pos, int64_t n_types, int64_t padding_idx, float* grad_word, float* grad_pos,
                                   float* grad_type, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The trainer's parameter update (src/learning/trainer.py:178-181: optim.Adam / optim.Adagrad at torch's defaults): one launch over
 * every tensor of a parameter set, torch's single-tensor formulas in fp32 (division and square root correctly rounded), in place.
 *   tensors[i]   param, grad, state1, state2: n fp32 elements each, on the device, 4-byte aligned (16-byte aligned tensors take
 *                16-byte accesses); step = this update's number for THIS tensor, >= 1 (torch's state['step'] after its increment: a
 *                parameter without a gradient at some steps lags behind the others); lr = the tensor's param group's learning rate
 *   Adam         state1 = exp_avg m, state2 = exp_avg_sq v:
 *                m += (g - m) (1 - beta1);  v = v beta2 + g g (1 - beta2);  p -= step_size (m / (sqrt(v) / bc2_sqrt + eps))
 *                step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step), formed in double per tensor, passed as floats
 *   Adagrad      state1 = sum s, state2 unused (may be NULL):
 *                s += g g;  p -= clr (g / (sqrt(s) + eps));  clr = lr / (1 + (step - 1) lr_decay)
 * No weight decay, amsgrad or maximize.  Non-finite gradients propagate as the formulas say.  Every element has one writer, no
 * atomics, the same bits on every run, and nothing outside [ptr, ptr + n) of a tensor is touched.
 *   workspace    device memory of at least aspire_optim_workspace_bytes(n_tensors) bytes (a multiple of 16, growing with
 *                n_tensors), 16-byte aligned: the library copies the table there on `stream` from pinned staging of its own, so
 *                `tensors` need not outlive the call and the call does not wait for the stream.  The workspace must stay untouched
 *                until the step has run; two steps in flight on different streams need two workspaces.  Not capturable into a graph.
 * Errors, all before the device is touched, the offending value in aspire_last_error(): ASPIRE_ERR_INVALID_ARG for n_tensors < 0;
 * a NULL table with n_tensors > 0; a tensor with n < 0, step < 1, lr negative or not finite, a NULL param / grad / state pointer with
 * n > 0 or a pointer that is not 4-byte aligned; eps / lr_decay negative or not finite; a beta outside [0, 1); a workspace that is
 * NULL, too small or not 16-byte aligned.  n_tensors == 0, or every n == 0 -> ASPIRE_OK without a launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float*       param;
    const float* grad;
    float*       state1;
    float*       state2;
    int64_t      n;
    int64_t      step;
    double       lr;
} aspire_optim_tensor;

size_t aspire_optim_workspace_bytes(int64_t n_tensors);
int aspire_adam_step_f32(const aspire_optim_tensor* tensors, int64_t n_tensors, double beta1, double beta2, double eps,
                         void* workspace, size_t workspace_bytes, void* stream);
int aspire_adagrad_step_f32(const aspire_optim_tensor* tensors, int64_t n_tensors, double lr_decay, double eps, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The two stabilisers of a BERT fine-tuning recipe inside the same one-launch step: a gradient scale read from the device (the clip
 * coefficient of aspire_grad_norm_f32 below) and AdamW's decoupled weight decay.  Everything the step above states holds; the two
 * entries above keep their kernels and their bits.
 *   grad_scale   one float on the device, 4-byte aligned, read once per workgroup: every rule is applied to g * (*grad_scale) -- ONE
 *                fp32 multiply, never contracted, in front of the formula: torch's grad.mul_(clip_coef) followed by the step.  The
 *                gradients in memory are not modified.  NULL: the unscaled kernel (for Adam / Adagrad: the entries above).
 *   AdamW        p = p * (float)(1 - lr * weight_decay) in front of Adam's update: ONE fp32 multiply, the factor formed in double
 *                per tensor (torch.optim.AdamW: _single_tensor_adam with decoupled_weight_decay=True).  lr and weight_decay are per
 *                tensor, so param groups that differ in them alone are one launch.  weight_decay == 0 gives Adam's bits.
 *                Coupled L2 decay (torch.optim.Adam(weight_decay=...)) and amsgrad are not built.
 * Errors: those of the step above; weight_decay negative or not finite; a grad_scale that is not 4-byte aligned.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float*       param;
    const float* grad;
    float*       state1;         /* exp_avg */
    float*       state2;         /* exp_avg_sq */
    int64_t      n;
    int64_t      step;
    double       lr;
    double       weight_decay;
} aspire_adamw_tensor;

int aspire_adam_step_scaled_f32(const aspire_optim_tensor* tensors, int64_t n_tensors, double beta1, double beta2, double eps,
                                const float* grad_scale, void* workspace, size_t workspace_bytes, void* stream);
int aspire_adagrad_step_scaled_f32(const aspire_optim_tensor* tensors, int64_t n_tensors, double lr_decay, double eps,
                                   const float* grad_scale, void* workspace, size_t workspace_bytes, void* stream);
int aspire_adamw_step_f32(const aspire_adamw_tensor* tensors, int64_t n_tensors, double beta1, double beta2, double eps,
                          const float* grad_scale, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The gradient bucket of data-parallel training (the reference trains through DistributedDataParallel, main_fsim.py ddp_train_model):
 * every gradient of a step packed and scaled into ONE flat fp32 buffer in one launch, so that one all-reduce sums it across the ranks
 * and the optimizer step above reads the reduced gradients where they lie.
 *   Layout       the library's, the same for every caller: tensor i takes [offsets[i], offsets[i] + n_i) with offsets[0] = 0 and
 *                offsets[i + 1] = offsets[i] + round_up(n_i, 4), so every offset is a multiple of 4 elements; behind the last region
 *                comes a tail of round_up(n_tensors, 4) floats.  aspire_grad_bucket_elems returns the total (the tail starts at
 *                total - round_up(n_tensors, 4)) and fills offsets[n_tensors] when it is not NULL; -1 for n_tensors < 0, a negative
 *                n, or n NULL with n_tensors > 0.  No device is touched.
 *   pack         flat[offsets[i] + j] = grad_i[j] * (float)scale -- ONE fp32 multiply, never contracted: torch's reducer arithmetic
 *                mul_out(bucket_view, grad, 1 / world) -- zeros where grad_i == NULL (no gradient on this rank), zeros in every pad
 *                element; flat[tail + i] = grad_i ? 1.0f : 0.0f, unscaled, zeros in the tail's pad: summed over the ranks, the
 *                tail holds the number of ranks that had a gradient for each tensor.  Every element of [flat, flat + flat_elems)
 *                has exactly one writer, nothing outside it is touched, no atomics, no zero fill in front, the same bits on every
 *                run and wherever a gradient's storage starts.  Non-finite gradients propagate as the multiply says.
 *   tensors[i]   grad: n fp32 elements on the device, 4-byte aligned (16-byte aligned ones are read with 16-byte loads), or NULL
 *   flat         flat_elems fp32 elements on the device, 16-byte aligned; flat_elems must equal aspire_grad_bucket_elems
 *   workspace    device memory of at least aspire_grad_bucket_workspace_bytes(n_tensors) bytes, 16-byte aligned; the rules of the
 *                optimizer step's workspace apply (the table is copied there on `stream` from pinned staging of the library; the
 *                call does not wait for the stream; not capturable into a graph)
 * Errors, all before the device is touched, the offending value in aspire_last_error(): ASPIRE_ERR_INVALID_ARG for n_tensors < 0; a
 * NULL table with n_tensors > 0; a scale that is not finite (as a float); flat NULL or not 16-byte aligned; a tensor with n < 0 or a
 * gradient pointer that is not 4-byte aligned; flat_elems other than aspire_grad_bucket_elems; a gradient that overlaps
 * [flat, flat + flat_elems) (a gradient that already lives in the bucket: the reduction ran twice on the same gradients); a
 * workspace that is NULL, too small or not 16-byte aligned.  ASPIRE_ERR_UNSUPPORTED beyond 2^30 chunks of 4096 elements.
 * n_tensors == 0 (flat_elems == 0) -> ASPIRE_OK without a launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const float* grad;   /* NULL: no gradient on this rank */
    int64_t      n;
} aspire_grad_tensor;

int64_t aspire_grad_bucket_elems(const int64_t* n, int64_t n_tensors, int64_t* offsets);
size_t aspire_grad_bucket_workspace_bytes(int64_t n_tensors);
int aspire_grad_bucket_pack_f32(const aspire_grad_tensor* tensors, int64_t n_tensors, double scale, float* flat, int64_t flat_elems,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Clipping the global gradient norm (torch.nn.utils.clip_grad_norm_, L2): the norm of all listed gradients viewed as one vector and
 * torch's clip coefficient, left on the device -- no host synchronisation anywhere -- for the scaled steps above to read.
 *   out[0]       the L2 norm.  Every element is squared in double (an fp32 square is exact there); each chunk of 4096 elements of
 *                a tensor gives one double partial (fixed lane ownership, fixed tree); a second launch of one workgroup adds the
 *                partials in a fixed order, takes the square root in double and rounds once to fp32.  The double sum of at most 2^27
 *                exact squares is off by at most 2^-26 relative: out[0] lies within 1 ulp of float(sqrt(exact sum of squares)).
 *                A deliberate departure from torch: because the sum is in double, gradients of 1e20 give a finite norm where
 *                torch's fp32 sum of squares overflows to inf.
 *   out[1]       the coefficient, in fp32 exactly as torch.nn.utils.clip_grads_with_norm_ forms it:
 *                clamp((1 / (out[0] + 1e-6f)) * (float)max_norm, max = 1) -- `max_norm / tensor` is tensor.reciprocal() * max_norm
 *                in torch -- every operation rounded once.  A NaN norm gives NaN, an infinite norm 0.
 *   tensors[i]   grad: n fp32 elements on the device, 4-byte aligned (16-byte aligned ones are read with 16-byte loads), or NULL:
 *                no gradient, the tensor stays out of the norm, as does one with n == 0
 *   One partial per chunk (not per workgroup), the same element-to-lane ownership on the 16-byte and the scalar path, no atomics,
 *   one writer per word: the bits depend neither on the grid, nor on where a gradient's storage starts, nor on the run.  With no
 *   element at all the norm is 0.  Nothing but out[0], out[1] and the workspace is written.
 *   workspace    device memory of at least aspire_grad_norm_workspace_bytes(n, n_tensors) bytes (the table + one double per chunk;
 *                0 for a negative count), 16-byte aligned; the rules of the optimizer step's workspace apply
 * aspire_grad_scale_f32: grad_i[j] *= *scale in place for every listed gradient, ONE fp32 multiply per element in one launch (the
 * second half of clip_grad_norm_; `scale` = out + 1).  Its workspace holds the table alone.
 * Errors, all before the device is touched, the offending value in aspire_last_error(): ASPIRE_ERR_INVALID_ARG for a max_norm that
 * is not a finite float above 0; out / scale NULL or not 4-byte aligned; n_tensors < 0; a NULL table with n_tensors > 0; a tensor
 * with n < 0 or a gradient pointer that is not 4-byte aligned; a workspace that is NULL, too small or not 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
size_t aspire_grad_norm_workspace_bytes(const int64_t* n, int64_t n_tensors);
int aspire_grad_norm_f32(const aspire_grad_tensor* tensors, int64_t n_tensors, double max_norm, float* out, void* workspace,
                         size_t workspace_bytes, void* stream);
size_t aspire_grad_scale_workspace_bytes(int64_t n_tensors);
int aspire_grad_scale_f32(const aspire_grad_tensor* tensors, int64_t n_tensors, const float* scale, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * caching_score's document-level term (src/learning/facetid_models/disent_models.py:305-307, taken when
 * abs_loss_prop > 0): functional.pairwise_distance(query_cls_reps, cand_cls_reps, p=2.0) = ||q - c + eps||_2 with torch's
 * eps = 1e-6 added to every coordinate of the difference.  (The caller negates and scales it.)
 *   q_cls [Q, 768], c_cls [C, 768]; dist [P] out: P = Q * C (CROSS, pair = q * C + c) or Q == C (PAIRED)
 * ------------------------------------------------------------------------------------------- */
int aspire_cls_l2_f32(const float* q_cls, int64_t Q, const float* c_cls, int64_t C, int64_t D, int pairing, double eps,
                      float* dist, void* stream);
/* Its gradient for ASPIRE_PAIR_PAIRED (the abstract term of the reference's rank loss, nn.TripletMarginLoss(p=2) over the CLS rows,
 * disent_models.py:582, :634): dist_p is formed again with the forward's arithmetic, then
 *   grad_q[p, :] = (q[p] - c[p] + eps) * (grad_dist[p] / dist_p)      grad_c[p, :] = -grad_q[p, :]      (zeros where dist_p == 0)
 * one wave per pair, every output row written once.  ASPIRE_PAIR_CROSS -> ASPIRE_ERR_UNSUPPORTED (a row would need an
 * accumulation across pairs); D != 768 -> ASPIRE_ERR_UNSUPPORTED; Q != C or a NULL pointer with pairs to do ->
 * ASPIRE_ERR_INVALID_ARG; no pairs -> ASPIRE_OK without a launch. */
int aspire_cls_l2_backward_f32(const float* q_cls, int64_t Q, const float* c_cls, int64_t C, int64_t D, int pairing, double eps,
                               const float* grad_dist, float* grad_q, float* grad_c, void* stream);

/* cdist formula selection, mirroring torch.cdist's default compute mode (used at
 * pair_distances.py:49 and :167): rows <= 25 on both sides -> direct sqrt(sum (x-y)^2),
 * otherwise the matmul expansion. */
#define ASPIRE_CDIST_AUTO 0
#define ASPIRE_CDIST_DIRECT 1
#define ASPIRE_CDIST_MM 2

/* How documents are paired.  CROSS: every query with every candidate, P = Q*C, pair p = q*C + c
 * (the ranking loops evaluate.py:72-74, pp_gen_nearest.py:182-202).  PAIRED: query p with candidate
 * p, P = Q = C (the reference's batched `compute_distance(query, cand)` signature). */
#define ASPIRE_PAIR_CROSS 0
#define ASPIRE_PAIR_PAIRED 1

/* ---------------------------------------------------------------------------------------------
 * fp16 planes of a rep store's row matrix: the many-query cost tiles (pair_distances.py:48-55 with >= ~8 query
 * documents: torch.cdist of every query sentence against every candidate sentence is a [sum S_c, sum S_q] x 768 GEMM)
 * run on v_mfma_f32_32x32x16_f16 at fp32 accuracy when both rep sets carry their rows a second time as two fp16
 * planes.  Row r is stored as h + l of s_r * (rows[r] - mu): mu = one vector per store (L2 distances do not change
 * under a common shift: the anisotropic common component of sentence embeddings comes off before anything is
 * rounded), s_r = the power of two that puts the row's largest entry into [2^14, 2^15) (any finite fp32 row fits:
 * nothing is rejected), h = fp16(.), l = fp16(. - h): 22+ significant bits per element, three exact matrix-pipe
 * products per term (h.h' + h.l' + l.h') accumulated in fp32 -- the encoder's scheme (aspire_bert_prepare_planes).
 * Layout: 48 k blocks of 16 coordinates; k block kb, row r: 64 bytes = pieces (plane pl, k half kh) at
 * ((kb * plane_rows + r) * 4 + 2 pl + kh) * 16, each the 8 fp16 of plane pl at coordinates 16 kb + 8 kh .. + 7;
 * rows [total_rows, plane_rows) are zero (what the tiles read for the rows a short document does not have).
 * The planes are prepared ONCE per resident store (4 B per element, like the fp32 rows: one more copy in HBM) and
 * per call for queries that are not part of the store, with the STORE's mu: two rep sets can meet in one call iff
 * their `mu` pointers are equal.  A rep set without planes (planes == NULL), or one whose mu differs, takes the
 * kernels that read the fp32 rows -- same results to rounding.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const void* planes;      /* [48][plane_rows][64 B] */
    const float* row_nrm;    /* [plane_rows]  |rows[r] - mu|^2 (0 for the zero rows) */
    const float* row_iscale; /* [plane_rows]  1 / s_r */
    const float* mu;         /* [D] */
    int64_t total_rows;      /* rows of the fp32 matrix the planes were made of */
    int64_t plane_rows;      /* > total_rows, a multiple of 16 */
} aspire_rep_planes;

/* bytes of the device blob aspire_rep_planes_prepare fills for a matrix of total_rows rows */
size_t aspire_rep_planes_bytes(int64_t total_rows);
/* rows [total_rows, D] -> blob; *out_host (a HOST struct) receives the pointers into it.
 *   mu   device [D] or NULL.  NULL: the mean of a sample of up to 4096 of the rows is formed (deterministic: rows
 *        k * stride) and kept in the blob.  Given: used as it is and out_host->mu == mu -- pass the store's mu when
 *        preparing query rows, and rank 0's mu on every shard of a sharded store: every shard then rounds its rows
 *        around the same point, and wherever the plane tiles run (a shard of >= 128 candidate tiles; a smaller or
 *        uneven last shard takes the kernels that read the fp32 rows, within 5e-5 of the tiles) sharded and
 *        un-sharded scores are the same bits. */
int aspire_rep_planes_prepare(const float* rows, int64_t total_rows, int64_t D, const float* mu, void* blob,
                              size_t blob_bytes, aspire_rep_planes* out_host, void* stream);

typedef struct {
    const float* rows;     /* [total_rows, D] */
    const int32_t* start;  /* [n] first row of each document */
    const int32_t* len;    /* [n] valid sentence rows (abs_lens) */
    int64_t n;             /* number of documents */
    /* Padded extent: if > 0 every document has `ext` readable rows (len[k] <= ext) and pair outputs
     * are laid out [.., ext, ..] with the reference's padding semantics; 0 = no padding (ext = len). */
    int32_t ext;
    /* Host-known upper bound of len[] (lens live on the device; the launcher needs the bound to size
     * the tile).  Ignored when ext > 0.  A document longer than the bound yields a NaN score.
     * Every document needs len >= 1: the reference raises on a document without sentences (torch.max over an
     * empty dimension, pair_distances.py:57) -- lens live on the device, so the HOST layer rejects it
     * (aspire_amd.ops.DeviceRepSet raises ValueError); the library does not look. */
    int32_t max_len;
    /* optional (NULL): fp16 planes of `rows` (aspire_rep_planes above; a HOST pointer, read during the call) */
    const aspire_rep_planes* planes;
    /* optional (NULL): the documents' per-coordinate bounding boxes, device [n][2][D] (min row, max row), as
     * aspire_repset_boxes_f32 forms them.  geomloss's epsilon schedule starts at the diameter of the two documents' joint box;
     * the many-query otAspire calls form every candidate's box per call (a pass over all its rows) unless a resident pool
     * brings them along. */
    const float* doc_box;
} aspire_repset;

/* boxes [n][2][D] of the documents of `set` (len[] >= 1): boxes[k][0] = per-coordinate minimum over document k's rows, [k][1] = maximum */
int aspire_repset_boxes_f32(const aspire_repset* set, int64_t D, float* boxes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A9  tsAspire max-sim.  Replaces allpair_masked_dist_l2max,
 * src/learning/facetid_models/pair_distances.py:138-186.
 *   scores    [P]  out: max over valid (i < q_len, j < c_len) of -||q_i - c_j||   (the "sims";
 *                  the reference's distance output is its negation)
 *   pair_sims [P, q.ext, c.ext] out, optional (NULL): -cdist + pad_mask, pad_mask = -10e8 outside
 *                  the valid block (pair_distances.py:156-170); requires q.ext > 0 and c.ext > 0.
 * ------------------------------------------------------------------------------------------- */
int aspire_l2max_scores_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                            int cdist_mode, float* scores, float* pair_sims, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sibling aggregations of the same masked -cdist block (score_agg_type 'l2top2' / 'l2attention',
 * src/learning/facetid_models/disent_models.py:238-245):
 *   ASPIRE_AGG_MAX        aspire_l2max_scores_f32 above.
 *   ASPIRE_AGG_TOP2       allpair_masked_dist_l2topk, pair_distances.py:295-345: sum of the two largest entries of
 *                         -cdist + pad_mask over the padded [q.ext, c.ext] block (torch.topk k = 2; with fewer than
 *                         two valid entries a masked one, ~ -1e9, is picked exactly as the reference does; without
 *                         padded extents the missing entry counts as -10e8).
 *   ASPIRE_AGG_ATTENTION  AllPairMaskedAttention.compute_distance, pair_distances.py:95-135 with
 *                         models_common/activations.py:35-61: sum_ij p_ij * (-d_ij), p = soft-max over the valid
 *                         block of -d_ij / temp (temp = cdatt_sm_temp).
 *   scores    [P]  out: the similarity (return_pair_sims=True value); the reference's distance is its negation
 *   pair_sims [P, q.ext, c.ext] out, optional: TOP2: -cdist + pad_mask; ATTENTION: -cdist, unmasked (:125)
 *   pair_softmax [P, q.ext, c.ext] out, optional, ATTENTION only: p_ij (zero outside the valid block)
 * ------------------------------------------------------------------------------------------- */
#define ASPIRE_AGG_MAX 0
#define ASPIRE_AGG_TOP2 1
#define ASPIRE_AGG_ATTENTION 2
int aspire_l2agg_scores_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                            int cdist_mode, int agg, double temp, float* scores, float* pair_sims,
                            float* pair_softmax, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward of the three aggregations: what the reference's autograd computes through the branches marked "Happens at
 * train time" of allpair_masked_dist_l2max (pair_distances.py:184-186), allpair_masked_dist_l2topk (:342-345) and
 * AllPairMaskedAttention.compute_distance (:130-135; the soft-max is models_common/activations.py:35-61) -- through
 * torch.max / torch.topk(k = 2) / the masked 2-D soft-max and torch.cdist (:167, :324, :120) down to the sentence rows.
 * With s_ij = -||q_i - c_j|| over the valid block (i < q_len, j < c_len) and W_ij = dscore / ds_ij:
 *   ASPIRE_AGG_MAX        W = 1 at the arg-max, 0 elsewhere.
 *   ASPIRE_AGG_TOP2       W = 1 at the two largest entries.  A block of one entry has one pick: the reference's second
 *                         pick is a masked pad entry there, its gradient belongs to a pad row and is dropped.
 *   ASPIRE_AGG_ATTENTION  p = soft-max of s / temp, score = sum p s:  W_ij = p_ij (1 + (s_ij - score) / temp).
 *   Ties: the first entry in row-major (i, j) order wins; the second pick is the next one.
 *   grad_q_i = -g sum_j A_ij (q_i - c_j),  grad_c_j = +g sum_i A_ij (q_i - c_j),  A_ij = W_ij / d_ij and 0 where d_ij == 0
 *   (torch.cdist's backward rule for coincident rows: no NaN).
 *   pairing      ASPIRE_PAIR_PAIRED only: every document then belongs to one pair, every gradient row has one writer and
 *                the result is the same bits on every run.  ASPIRE_PAIR_CROSS -> ASPIRE_ERR_UNSUPPORTED (a document's
 *                gradient would be a sum over many pairs: an accumulation across pairs that is not built).
 *   grad_scores  [P] in: g_p = dLoss / dscore_p, score_p the SIMILARITY aspire_l2agg_scores_f32 documents (a loss on the
 *                reference's distance passes minus its gradient)
 *   grad_q_rows, grad_c_rows  out, laid out like q->rows / c->rows (padded sets, ext > 0, and CSR sets alike).  Every row
 *                of every document is written: valid rows with the gradient, pad rows (len <= r < ext) with exact zeros;
 *                rows of the matrices that belong to no document are not touched.
 *                q->rows, c->rows and both gradient buffers must be 16-byte aligned (they are read and written 16 bytes at a
 *                time; a row is 3072 bytes, so an aligned base aligns every row).
 * The distances are recomputed here from direct differences; nothing is kept by the forward.  For documents of more than
 * 25 rows the forward may have used torch.cdist's matmul formula (ASPIRE_CDIST_AUTO): the pick of MAX / TOP2 can then
 * differ from the forward's only where two entries are within about 3e-5 of each other.
 * bad agg, temp <= 0 with ATTENTION, a NULL pointer, q->n != c->n -> ASPIRE_ERR_INVALID_ARG; D != 768, or documents of
 * more than aspire_max_sents() rows -> ASPIRE_ERR_UNSUPPORTED; no pairs -> ASPIRE_OK without a launch.  A document longer
 * than its set's max_len gets NaN rows (its score is NaN in the forward).  One launch on `stream`, no workspace.
 * ------------------------------------------------------------------------------------------- */
int aspire_l2agg_backward_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                              int agg, double temp, const float* grad_scores /* [P] */,
                              float* grad_q_rows, float* grad_c_rows /* laid out like q->rows / c->rows */,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * A5-A8  otAspire.  Replaces AllPairMaskedWasserstein.compute_distance,
 * src/learning/facetid_models/pair_distances.py:21-92 (copy at
 * examples/ex_aspire_consent_multimatch.py:118-189), including the geomloss==0.2.4
 * SamplesLoss("sinkhorn", p=1, blur, reach=None, scaling, debias=False) solver it calls.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    /* doubles: the reference holds these as Python floats and geomloss builds the epsilon schedule
     * from them in float64 (np.log / np.arange / np.exp) before any fp32 arithmetic. */
    double blur;         /* geoml_blur    (default 0.05) */
    double scaling;      /* geoml_scaling (default 0.9)  */
    double sent_sm_temp; /* sent_sm_temp  (default 1.0)  */
    int32_t cdist_mode;  /* ASPIRE_CDIST_*               */
    int32_t flags;       /* ASPIRE_OT_FLAG_* (0 = default) */
} aspire_ot_params;

/* ONE_FORM: score every pair with ONE kernel (the one-workgroup-per-pair long form, documents of 1 .. 128 rows) whatever the
 * size of the call.  By default the grid size selects among kernel families whose summation orders differ, so the same
 * (query, candidate) pair can come back a few 1e-5 apart from a per-query call and from a batched one and near-ties of a
 * ranking may swap; with this flag a pair's score depends on its two documents only -- aspire_ot_rank_f32 per query and
 * aspire_ot_rank_batch_f32 over all queries return the same bits and the same order.  Several times slower.  The max-sim
 * entry points take the same request as ASPIRE_CDIST_ONE_FORM or'ed into cdist_mode. */
#define ASPIRE_OT_FLAG_ONE_FORM 1
#define ASPIRE_CDIST_ONE_FORM 0x100
/* CENTER: the rows share a large common component (anisotropic embedding spaces: mean cosine of 0.5 .. 0.9 between unrelated
 * sentences is common).  The streaming kernels then subtract the mean of the query's rows from every row before forming
 * |x|^2 - 2 x.y + |y|^2 -- L2 distances do not change under a common shift, the expansion stops cancelling, and the
 * direct-formula fix-up that otherwise redoes nearly every entry (5 x slower at mean cosine 0.8) is back to the exception.
 * Same results to rounding (closer to the float64 value than the un-centred expansion).  Honoured by the streaming kernels
 * (fused / chunk forms, the 16-row tiles: centre = mean of the staged query rows) and by the matrix-pipe cost tiles of the
 * many-query calls and the small-pool cost kernels (centre = the tile's / the query's first row: 128 x 16 384 x 12 at mean cosine
 * 0.97 86 -> 8 ms; 1 x 1000 x 12 at 0.8 123 -> 49 us); the 33 .. 128-row kernel and padded reference tensors ignore it.
 * aspire_amd.ops sets it from a sample of the pool. */
#define ASPIRE_OT_FLAG_CENTER 2
#define ASPIRE_CDIST_CENTER 0x200

/* SHARED SENTENCES -- the one place where the product deliberately does NOT reproduce the reference's fp32 bits.  geomloss forms its
 * cost as sqrt(max(|x|^2 - 2 x.y + |y|^2, 1e-8)) (and torch.cdist beyond 25 rows forms -cdist the same way,
 * pair_distances.py:48-56).  Where a candidate sentence (nearly) EQUALS a query sentence the expansion cancels: in fp32 its value is
 * rounding noise of size ~1e-6 (|x|^2 + |y|^2), and the reference returns the square root of that noise -- 1.5e-2 .. 5.4e-2 from its
 * own float64 value on 768-d reps, different for every summation order (another BLAS, another batch size: other bits).  Every kernel
 * family here tests d^2 < 1e-4 (|x|^2 + |y|^2)^2 (the d below which the expansion's error exceeds ~5e-5 ABSOLUTE in the distance --
 * the bar is absolute, hence the squared norm on the right) and takes BOTH -cdist and geomloss's cost of such an entry from the exact
 * sum of squared differences: within 1.3e-5 of the float64 oracle (tests/test_gpu_coincident.py), and therefore up to 5e-2 away from
 * what the fp32 reference happens to return for that pair.  Rankings: a shared sentence gives the pair a cost entry of ~1e-4 instead
 * of ~2e-2, i.e. it scores (correctly) slightly better than the reference scores it.  The rule holds at ANY document length: also
 * where torch.cdist itself would pick its matmul formula (a side beyond 25 rows, ASPIRE_CDIST_MM) a cancelling entry's -cdist and cost
 * come from the exact sum (round 6; before, the kernels left those entries on the expansion, and geomloss's cost with them).  There is
 * no flag that reproduces the reference's noise. */
#define ASPIRE_OT_DISTANCE 0 /* return_pair_sims=False: OT_eps = <a,f> + <b,g>  (positive)          */
#define ASPIRE_OT_PLAN_SIM 1 /* return_pair_sims=True : sum_ij P_ij * neg_ij     (negative)         */
#define ASPIRE_OT_SIMILARITY 2 /* -OT_eps: what AspireModel.get_similarity returns (models.py:197), the ranking key */

/*   diameter   NULL: each pair uses the bounding-box diameter of its own valid rows (what the
 *              reference computes when called with B = 1, src/evaluation/utils/models.py:190-197).
 *              else: pair (q, c) uses diameter[q * ngroups + c / diam_group]
 *              with ngroups = ceil(C / diam_group) in CROSS mode, diameter[p / diam_group] in PAIRED
 *              mode -- geomloss derives ONE epsilon schedule per call from the whole batch
 *              (consecutive groups of 64 candidates in pp_gen_nearest.py:182-196); compute it with
 *              aspire_group_diameter_f32.
 *   scores     [P] out
 *   out_qdistr [P, q.ext], out_cdistr [P, c.ext], out_pairsims / out_plan [P, q.ext, c.ext]:
 *              optional (NULL) extra outputs of return_pair_sims=True (pair_distances.py:86):
 *              query_distr, cand_distr, pair_sims (masked neg L2, pads = 0), transport_plan.
 *              masked_sims = plan * pair_sims is left to the caller.  Require ext > 0.
 *   workspace  device scratch for the per-pair cost matrices handed from the cost kernel to the Sinkhorn
 *              kernel.  aspire_ot_workspace_bytes() gives the size that lets the whole job run in one
 *              pass (capped at 1 GiB); any size that holds one candidate's pairs is accepted and larger jobs
 *              are processed in candidate chunks.
 */
size_t aspire_ot_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int pairing);
int aspire_ot_sinkhorn_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                           const aspire_ot_params* prm, const float* diameter, int64_t diam_group,
                           int want, float* scores, float* out_qdistr, float* out_cdistr,
                           float* out_pairsims, float* out_plan, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward of the otAspire distance: the gradient of OT_eps = <a, f> + <b, g> with respect to the sentence rows, what the
 * reference's autograd computes through the train-time branch of AllPairMaskedWasserstein.compute_distance
 * (pair_distances.py:88-92: SamplesLoss("sinkhorn", p=1, debias=False, potentials=False)) and the marginals (:49-60).
 * A RESTATEMENT: geomloss 0.2.4 is not vendored and its solver is "parity unpinned" here, so this is the gradient of what its
 * sinkhorn_tensorized is read to do -- costs C_xy = cost(x, y.detach()), C_yx = cost(y, x.detach()); the epsilon-scaling
 * loop without grad; only the last extrapolation with grad, on detached (log-weight + potential / eps) arguments; the value
 * <a, b_x> + <b, a_y> with the marginals a, b NOT detached; the diameter a constant.  Per pair, gs = dLoss / dscore, la / lb
 * geomloss's log-weights, eps = blur, f0 / g0 the potentials after the last averaged step, tau = sent_sm_temp:
 *   f_i = -eps LSE_j(lb_j + (g0_j - C_ij) / eps),  g_j = -eps LSE_i(la_i + (f0_i - C_ij) / eps)   (the last extrapolation)
 *   C_ij = sqrt(max(d_ij^2, 1e-8)),  s_ij = -d_ij (the torch.cdist block of the marginals),  d_ij = ||x_i - y_j||
 *   W_ij = exp(lb_j + (g0_j - C_ij + f_i) / eps)   (every row i sums to 1)
 *   V_ij = exp(la_i + (f0_i - C_ij + g_j) / eps)   (every column j sums to 1)
 *   u_i = a_i (f_i - sum_k a_k f_k) / tau  at entry (i, j*(i)), j*(i) = the FIRST arg-max over j of s_ij in the valid block
 *   v_j = b_j (g_j - sum_l b_l g_l) / tau  at entry (i*(j), j), i*(j) = the first arg-max over i
 *   M_ij = u_i [j == j*(i)] + v_j [i == i*(j)]
 *   grad_x_i = gs sum_j ( a_i W_ij [d_ij^2 > 1e-8] / C_ij  -  M_ij [d_ij > 0] / d_ij ) (x_i - y_j)
 *   grad_y_j = gs sum_i ( M_ij [d_ij > 0] / d_ij  -  b_j V_ij [d_ij^2 > 1e-8] / C_ij ) (x_i - y_j)
 * x receives the transport term through f only, y through g only (the detach pattern); both receive the marginal term.
 *   pairing      ASPIRE_PAIR_PAIRED only (every gradient row has one writer: no atomics, the same bits on every run);
 *                ASPIRE_PAIR_CROSS -> ASPIRE_ERR_UNSUPPORTED.
 *   prm          blur, scaling, sent_sm_temp as in the forward; cdist_mode and flags are not read: d_ij comes from direct
 *                differences everywhere (C and s both), also where the forward used the matmul expansion -- the two
 *                differ by rounding, and the expansion cancels where training drives rows together.
 *   diameter, diam_group   as aspire_ot_sinkhorn_f32 reads them in PAIRED mode: diameter[p / diam_group], or the box of
 *                the pair's own valid rows when diameter is NULL.  Pass what the forward was given.
 *   want         ASPIRE_OT_DISTANCE, or ASPIRE_OT_SIMILARITY (the sign flips); ASPIRE_OT_PLAN_SIM has no backward
 *                (return_pair_sims is "only used at test time", pair_distances.py:62) -> ASPIRE_ERR_UNSUPPORTED.
 *   grad_scores  [P] in.   grad_q, grad_c  out, laid out like q->rows / c->rows (padded sets, ext > 0, and CSR sets alike):
 *                every row of every document is written, pad rows (len <= r < ext) with exact zeros; rows that belong to
 *                no document are not touched.  Rows and gradient buffers must be 16-byte aligned.
 * q->n != c->n, bad params, a NULL pointer -> ASPIRE_ERR_INVALID_ARG; D != 768 or documents of more than aspire_max_sents()
 * rows -> ASPIRE_ERR_UNSUPPORTED; no pairs -> ASPIRE_OK without a launch.  A document longer than its set's max_len gets
 * NaN rows.  One launch on `stream` (one workgroup per pair, the solve repeated in LDS), no workspace.
 * ------------------------------------------------------------------------------------------- */
int aspire_ot_backward_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                           const aspire_ot_params* prm, const float* diameter, int64_t diam_group, int want,
                           const float* grad_scores, float* grad_q, float* grad_c, void* stream);

/* geomloss max_diameter (sinkhorn_divergence.py of geomloss 0.2.4) for batched calls: the L2 norm of
 * the per-coordinate bounding box over ALL rows of the call's x and y tensors, zero pad rows included.
 *   CROSS : diameter[q * ngroups + g] covers query q's rows and the rows of candidates
 *           [g*group, min(C, (g+1)*group)); a zero row joins the box iff the group's candidates have
 *           unequal lengths (caching_score pads them to the group max, disent_models.py:269-281).
 *   PAIRED: diameter[g] covers queries and candidates [g*group, (g+1)*group); with ext > 0 all ext
 *           rows are read (the padded tensors as they are), else len rows.
 */
int aspire_group_diameter_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                              int64_t group, float* diameter, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A12  rank.  Per-query top-k of a [Q, C] score matrix, descending, ties by ascending candidate
 * index -- the order Python's stable sorted(..., reverse=True) gives (src/evaluation/evaluate.py:76,
 * src/pre_process/pp_gen_nearest.py:266,339).
 *   idx_base  added to every output index (the shard's first global candidate id)
 *   top_scores [Q, k], top_idx [Q, k] out; if C < k the tail is (-inf, -1).
 *   workspace  device scratch of at least aspire_topk_workspace_bytes(Q, C, k) bytes (0 when C <= 4096).
 *   Any C < 2^32 - 1 and any k: pools beyond one 4096-key chunk are ranked by chunk winners (k < 1024) or fully sorted
 *   (k >= 1024: sorted chunks + merge passes), e.g. k = C for the whole-pool sort of evaluate.py:76.
 */
size_t aspire_topk_workspace_bytes(int64_t Q, int64_t C, int64_t k);
int aspire_topk_desc_f32(const float* scores, int64_t Q, int64_t C, int64_t k, int64_t idx_base,
                         float* top_scores, int64_t* top_idx, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * A5-A8 + A12 in one call: the ranking step of evaluate.py:58-76 / pp_gen_nearest.py:131-204 for a pool --
 * scores [Q, C] exactly as aspire_ot_sinkhorn_f32 (pairing = ASPIRE_PAIR_CROSS, no pair outputs) followed by the
 * per-query rank exactly as aspire_topk_desc_f32 (top_scores, top_idx) or aspire_topk_keys_f32 (keys != NULL).
 * One host call, the kernels queued back to back on `stream`.  (A variant with the rank fused into the Sinkhorn
 * kernel's last workgroup was measured slower than the separate rank kernel -- NOTES.md -- and is not kept.)
 * Workspace: aspire_ot_rank_workspace_bytes(q, c, k).
 * ------------------------------------------------------------------------------------------- */
size_t aspire_ot_rank_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t k);
int aspire_ot_rank_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const aspire_ot_params* prm,
                       const float* diameter, int64_t diam_group, int want, float* scores, int64_t k,
                       int64_t idx_base, float* top_scores, int64_t* top_idx, uint64_t* keys, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The per-query loop of evaluate.py:58-76 batched over queries: J independent (query, pool) re-ranks in ONE call.
 * Job j scores the candidates [job_off[j], job_off[j+1]) of `c` -- query j's own pool (evaluate.py:60-62), all pools
 * laid back to back in one CSR rep set -- against query j of `q`, one epsilon schedule per pair
 * (AspireModel.get_similarity, src/evaluation/utils/models.py:190-197), and ranks each pool on its own (stable
 * descending, evaluate.py:76).  Launches on `stream`: ONE scoring launch over all pairs (costs and Sinkhorn solves fused
 * once the batch fills the chip; a pair whose sums leave fp32 range is re-solved in the max-shifted form by the wave that finds
 * it) and one rank launch with a workgroup per job; batches of more than 64 jobs, batches whose documents exceed 8 rows (a launch
 * that sorts the candidates into chunk items) and the small-batch kernel forms put a launch in front that builds the job tables
 * and the query boxes.  Documents of up to 128 rows are accepted (33 .. 128: one workgroup per pair).  Everything runs on the
 * caller's stream: independent calls on different streams (each with its own outputs and workspace) overlap.
 *   q          J query documents (q->n == J), CSR (ext == 0)
 *   c          every job's candidates (c->n == C == job_off[J]), CSR (ext == 0)
 *   job_off    DEVICE int32 [J + 1], non-decreasing, job_off[0] == 0, job_off[J] == C
 *   max_job    host-known upper bound of a job's candidate count (launch geometry only)
 *   scores     [C] out: candidate p against its job's query, as aspire_ot_sinkhorn_f32 would give it (`want`)
 *   k          0: scores only; else top_scores [J, k], top_idx [J, k] out: per job, index = job_base[j] + position in
 *              the job's pool, (-inf, -1) beyond the pool's size; or keys [J, k] (non-NULL: instead of top_scores /
 *              top_idx) in the sortable key form of aspire_topk_keys_f32, for the shard exchange of section 8(e)
 *   job_base   DEVICE int32 [J] or NULL (= 0): global index of the job's first candidate when this rank holds one
 *              contiguous block of every job's pool
 *   workspace  16-byte aligned, aspire_ot_rank_batch_workspace_bytes(q, c, max_job, k) bytes
 * Results equal J separate aspire_ot_rank_f32 calls up to the kernel form the grid size selects (bit for bit when the
 * forms are pinned to the same ones, see aspire_debug_set).
 * ------------------------------------------------------------------------------------------- */
size_t aspire_ot_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k);
int aspire_ot_rank_batch_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off,
                             int64_t max_job, const aspire_ot_params* prm, int want, float* scores, int64_t k,
                             const int32_t* job_base, float* top_scores, int64_t* top_idx, uint64_t* keys, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same per-query loop for tsAspire (allpair_masked_dist_l2max, pair_distances.py:138-186; caching_score's 'l2lse'
 * branch, disent_models.py:294-295): J independent (query, pool) re-ranks by max-sim in ONE call.  Arguments as
 * aspire_ot_rank_batch_f32 (no OT parameters; cdist_mode as aspire_l2max_scores_f32); scores [C] = -min L2 over the valid
 * sentence pairs of candidate p and its job's query.  Documents of up to 128 rows.  Launches: tables, then the streaming
 * max-sim kernels (documents of <= 16 rows, from 384 groups of four candidates) or one workgroup per candidate, then the
 * segmented rank.
 * ------------------------------------------------------------------------------------------- */
size_t aspire_l2max_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k);
int aspire_l2max_rank_batch_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off,
                                int64_t max_job, int cdist_mode, float* scores, int64_t k, const int32_t* job_base,
                                float* top_scores, int64_t* top_idx, uint64_t* keys, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same per-query loop for the sibling aggregations (score_agg_type 'l2top2' / 'l2attention', disent_models.py:238-245;
 * pp_gen_nearest.py rank_pool_sent*, :941-959): J independent (query, pool) re-ranks in ONE call.
 *   job_off, max_job, scores [C], k, job_base, top_scores, top_idx, keys, workspace: exactly the contract of
 *              aspire_jointsm_rank_batch_f32 (CSR rep sets, ties in pool order, (-inf, -1) beyond a pool's size, k == 0: scores only);
 *              the workspace, 16-byte aligned, is aspire_l2agg_rank_batch_workspace_bytes(q, c, max_job, k) bytes: the rank's
 *              scratch only, 0 for pools of <= 4096.
 *   agg        ASPIRE_AGG_TOP2 or ASPIRE_AGG_ATTENTION.  ASPIRE_AGG_MAX is ASPIRE_ERR_INVALID_ARG: aspire_l2max_rank_batch_f32 is the
 *              max-sim's batched entry.  temp (cdatt_sm_temp) must be positive with ATTENTION and is ignored with TOP2.
 *   scores [C] out: candidate p against its job's query, the similarity that aspire_l2agg_scores_f32 documents for CSR rep sets
 *              (TOP2: the two largest -d_ij of the valid block, a missing second entry counting -10e8; ATTENTION: sum_ij p_ij (-d_ij)).
 *              The value agrees with that entry point to rounding, NOT bit for bit: another kernel, another summation order.
 *   cdist_mode ASPIRE_CDIST_AUTO / DIRECT / MM are validated and all three are served by ONE formula,
 *                  d_ij = sqrt(max(|q_i|^2 + |c_j|^2 - 2 <q_i, c_j>, 0)),
 *              with exact fp32 products (v_mfma_f32_16x16x4_f32, sixteen accumulators per tile) and the row norms from the same
 *              operands.  Away from cancelling entries torch.cdist's two formulas differ by less than the 1e-4 parity bar, and a
 *              cancelling entry (d^2 < 1e-4 (|q|^2 + |c|^2)^2) follows the SHARED SENTENCES rule above in either mode: it is
 *              redone from the exact sum of squared differences.  ASPIRE_CDIST_ONE_FORM and ASPIRE_CDIST_CENTER may be or'ed in and
 *              change nothing: there is one kernel form (one wave per pair, 16 x 16 tiles) for every call size, so a pair's bits
 *              depend on its two documents only.
 *   Documents of 1 .. aspire_max_sents() rows (more: ASPIRE_ERR_UNSUPPORTED); a document longer than its set's max_len scores NaN;
 *   more than 2^33 - 4 pairs: ASPIRE_ERR_UNSUPPORTED.  Launches on `stream`: the scoring kernel, then the segmented rank.
 * ------------------------------------------------------------------------------------------- */
size_t aspire_l2agg_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k);
int aspire_l2agg_rank_batch_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off,
                                int64_t max_job, int cdist_mode, int agg, double temp, float* scores, int64_t k,
                                const int32_t* job_base, float* top_scores, int64_t* top_idx, uint64_t* keys,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A13  cosentbert / ictsentbert max-sim.  Replaces TrainedSentModel.get_similarity,
 * src/evaluation/utils/models.py:602-604 (float(np.max(sklearn.metrics.pairwise.cosine_similarity(x, y)))), and the
 * per-query scoring of pp_gen_nearest.py rank_pool_sent (:863-986; 'dotlse' takes np.matmul instead).
 *   scores [P] out: max over valid (i < q_len, j < c_len) of sim(q_i, c_j); P, pairing, CSR / padded rep sets and the
 *                   128-row limit as aspire_l2max_scores_f32.  The planes and doc_box fields are ignored.
 *   sim  ASPIRE_SIM_COSINE: sklearn's float32 path -- each row divided by n = sqrt(fp32 sum of squares), n < 10 * FLT_EPSILON
 *        replaced by 1 (a zero row scores 0, a row whose sum of squares underflows keeps its raw dot), a row whose sum of
 *        squares overflows to inf divides to zeros (scores 0 against everything, never NaN).  Non-finite rows are outside
 *        the contract (the host layer rejects them, as sklearn's check_array does).
 *        ASPIRE_SIM_DOT: the raw dot product.
 *   Exact fp32 matrix products (v_mfma_f32_16x16x4_f32), four independent accumulators over k; the similarity block is never
 *   written.  aspire_dotmax_rank_batch_f32 is the per-query loop over J (query, pool) jobs with the job_off / max_job /
 *   job_base / top-k / keys contract of aspire_l2max_rank_batch_f32 (CSR rep sets, ties in pool order); its workspace,
 *   16-byte aligned, is aspire_dotmax_rank_batch_workspace_bytes(q, c, max_job, k) bytes (0 for pools of <= 4096).
 * ------------------------------------------------------------------------------------------- */
#define ASPIRE_SIM_COSINE 0   /* sklearn cosine_similarity: rows / fp32 L2 norm, then dot (models.py:602-604) */
#define ASPIRE_SIM_DOT 1      /* np.matmul (pp_gen_nearest.py rank_pool_sent, 'dotlse') */
int aspire_dotmax_scores_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing, int sim,
                             float* scores, void* stream);
size_t aspire_dotmax_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k);
int aspire_dotmax_rank_batch_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off,
                                 int64_t max_job, int sim, float* scores, int64_t k, const int32_t* job_base,
                                 float* top_scores, int64_t* top_idx, uint64_t* keys, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A16  the alignment step of the co-citation data path.  Replaces the np.matmul(...).argmax() calls of
 * generate_examples_aligned_cocitabs_rand, src/pre_process/pre_proc_cocits.py:487-494 (three per training example), over
 * documents that are (start, len) views into resident row matrices.
 *   PAIRED only: P = q->n == c->n (else ASPIRE_ERR_INVALID_ARG).  For pair p with s_ij = <q_i, c_j>, i < q_len, j < c_len:
 *   arg  [P, 2] out: (i, j) = np.unravel_index(np.matmul(q, c.T).argmax(), (q_len, c_len)) -- numpy's rule in full: the first
 *                   maximum in row-major order of [q_len, c_len]; -0.0 and +0.0 tie; a NaN counts as the maximum and the first
 *                   NaN wins; a block of all -inf gives (0, 0).
 *   best [P] out, or NULL: s_ij at that entry -- the bits aspire_dotmax_scores_f32(..., ASPIRE_PAIR_PAIRED, ASPIRE_SIM_DOT) gives
 *                   the pair on NaN-free input (the same products on v_mfma_f32_16x16x4_f32, four accumulators over k; where the
 *                   maximum is a zero, the picked entry's sign).
 *   A document longer than its host bound (ext, or max_len): arg = (-1, -1), best = NaN.  A pair with a document of no rows:
 *   arg = (-1, -1), best = -inf.  D must be 768, rows 16-byte aligned, documents of up to aspire_max_sents() rows, as A13.  The
 *   planes and doc_box fields are ignored.  One launch on `stream`, one wave per pair; no atomics: every output has one writer,
 *   so every run gives the same bits.  P == 0: ASPIRE_OK, nothing is touched.
 * ------------------------------------------------------------------------------------------- */
int aspire_dot_argmax_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int32_t* arg, float* best, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A14  miswordpolyenc joint soft-max alignment ('jointsm').  Replaces pair_distances.allpair_joint_sm_negscore,
 * src/learning/facetid_models/pair_distances.py:348-402 with the mask of models_common/activations.py:35-61, as
 * WordSentAlignPolyEnc.score calls it (disent_models.py:877-925) under TrainedScoringModel.predict and its ranking callers
 * (src/pre_process/pp_gen_nearest.py:36-87, :366-466).
 *   scores [P] out: the SIMILARITY 2 * sum_ij p_ij d_ij with d_ij = <q_i, c_j> and p = the soft-max of d_ij / sqrtf(768) over
 *                   ALL valid (i < q_len, j < c_len) of the pair jointly -- what the reference forms as
 *                   sum_i <q_i, sum_j p_ij c_j> + sum_j <c_j, sum_i p_ij q_i> (allpair_joint_sm_negscore returns its negation,
 *                   score() negates back).  P, pairing, CSR / padded rep sets, the 128-row limit and NaN for a document
 *                   longer than its host bound (ext, or max_len) as aspire_dotmax_scores_f32; D must be 768.  The planes and
 *                   doc_box fields are ignored.  A pair's score depends on its two documents only: no schedule, no cdist mode.
 *   pair_softmax    NULL, or [P, q.ext, c.ext] out (padded rep sets only: ext > 0 on both): p_ij inside the valid block, exactly
 *                   0.0f outside it (the reference's pair_sm); NaN throughout for a document longer than its bound.
 *   Exact fp32 matrix products (v_mfma_f32_16x16x4_f32) as A13; the soft-max is shifted by the running maximum of the block and
 *   the similarity block is never written unless pair_softmax is asked for.  CROSS calls on documents of <= 16 rows take a
 *   kernel that keeps candidate rows in LDS; every other call one wave per pair.  The two sum the soft-max in different orders:
 *   a pair's score agrees between them to rounding, not bit for bit.
 *   aspire_jointsm_rank_batch_f32 is the per-query loop of pp_gen_nearest.py:412-456 over J (query, pool) jobs (scores [C], then
 *   each pool's stable descending rank, :450) with exactly the job_off / max_job / job_base / k / top_scores / top_idx / keys /
 *   workspace contract of aspire_dotmax_rank_batch_f32; its scores are the bits aspire_jointsm_scores_f32 gives the same pairs
 *   PAIRED.  Workspace: aspire_jointsm_rank_batch_workspace_bytes(q, c, max_job, k) bytes, 16-byte aligned (0 for pools of <= 4096).
 * ------------------------------------------------------------------------------------------- */
int aspire_jointsm_scores_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing, float* scores,
                              float* pair_softmax, void* stream);
size_t aspire_jointsm_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k);
int aspire_jointsm_rank_batch_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off,
                                  int64_t max_job, float* scores, int64_t k, const int32_t* job_base,
                                  float* top_scores, int64_t* top_idx, uint64_t* keys, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward of A14: what the reference's autograd computes for allpair_joint_sm_negscore (pair_distances.py:348-402) under
 * WordSentAlignPolyEnc's triplet loss (disent_models.py:868-875) -- through torch.bmm, masked_2d_softmax (activations.py:35-61)
 * and the two alignment loops down to the sentence rows.  Per PAIRED pair, over the valid block i < q_len, j < c_len:
 *   d_ij = <q_i, c_j>;  p = the soft-max of d_ij / sqrtf(768) over the whole block jointly;  S = 2 sum_ij p_ij d_ij (the similarity
 *   of aspire_jointsm_scores_f32);  g = dLoss / dS (a loss on the reference's distance -S passes minus its gradient).
 *     E        = sum_ij p_ij d_ij
 *     W_ij     = dS / dd_ij = 2 p_ij (1 + (d_ij - E) / sqrtf(768))
 *     grad_q_i = g sum_j W_ij c_j        grad_c_j = g sum_i W_ij q_i
 *   formed shifted by the block's maximum m (rows of norm 28 give d of about 1000: d - E must not cancel against a large E):
 *     e_ij = exp((d_ij - m) / sqrtf(768)),  Z = sum e,  T = sum e (d_ij - m),  E - m = T / Z
 *     W_ij = 2 (e_ij / Z) (1 + ((d_ij - m) - T / Z) / sqrtf(768))
 *   pairing      ASPIRE_PAIR_PAIRED only (ASPIRE_PAIR_CROSS -> ASPIRE_ERR_UNSUPPORTED: an accumulation across pairs that is not built).
 *   grad_scores  [P] in;  grad_q_rows, grad_c_rows  out, laid out like q->rows / c->rows (padded and CSR sets alike): every row of
 *                every document is written once -- valid rows with the gradient, pad rows (len <= r < ext) with exact zeros; rows
 *                of the matrices that belong to no document are not touched; pad rows of the inputs are never read; g == 0 gives
 *                exact zeros.  q->rows, c->rows and both gradient buffers must be 16-byte aligned.
 * The dot products are recomputed (direct fp32 FMA sums, one per entry); nothing is kept by the forward.  No atomics: the same bits
 * on every run.  A NULL pointer, a bad pairing, q->n != c->n -> ASPIRE_ERR_INVALID_ARG; D != 768, or documents of more than
 * aspire_max_sents() rows -> ASPIRE_ERR_UNSUPPORTED; no pairs -> ASPIRE_OK without a launch.  A document longer than its set's
 * host-known bound gets NaN rows up to the bound.  One launch on `stream`, no workspace.
 * ------------------------------------------------------------------------------------------- */
int aspire_jointsm_backward_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                                const float* grad_scores /* [P] */,
                                float* grad_q_rows, float* grad_c_rows /* laid out like q->rows / c->rows */,
                                void* stream);

/* ---------------------------------------------------------------------------------------------
 * The supervised-alignment distances, forward and backward.  Replaces allpair_masked_dist_l2sup and
 * allpair_masked_dist_l2sup_weighted (pair_distances.py:189-292), the criterion_sentsup of WordSentAbsSupAlignBiEnc
 * (disent_models.py:704-710, :818).  PAIRED only (pair p = query p with candidate p, q->n == c->n): there is no pairing argument.
 *   align        DEVICE int32 [P, 2]: (query row, candidate row) of the pre-aligned sentence pair.  An index above len - 1 is
 *                clipped to len - 1 (:214-215).  A negative index is the caller's error (the host layer raises ValueError): it reads
 *                nothing and gives NaN for that pair's score and for its valid gradient rows.
 *   weighted     0: similarity = -||q_i - c_j||;  non-zero: that divided by (float)(q_len * c_len)  (:264, :290)
 *   scores       [P] out: the SIMILARITY (the reference returns its negation), the distance from the direct difference.
 *   backward     torch.cdist's rule: grad_q_i = -g (q_i - c_j) / d, grad_c_j = +g (q_i - c_j) / d, both 0 where d == 0; every
 *                other row of the two documents gets exact zeros, pad rows (len <= r < ext) included; rows that belong to no
 *                document are not touched.  grad_scores, grad_q_rows, grad_c_rows and the alignment of the buffers as above.
 * A NULL pointer, q->n != c->n -> ASPIRE_ERR_INVALID_ARG; D != 768, or documents of more than aspire_max_sents() rows ->
 * ASPIRE_ERR_UNSUPPORTED; no pairs -> ASPIRE_OK without a launch; a document longer than its set's host-known bound: NaN score,
 * NaN rows up to the bound.  One launch on `stream` each, no workspace, no atomics.
 * ------------------------------------------------------------------------------------------- */
int aspire_l2sup_scores_f32(const aspire_repset* q, const aspire_repset* c, int64_t D,
                            const int32_t* align /* [P, 2] device: query row, candidate row */, int weighted,
                            float* scores /* [P] similarity */, void* stream);
int aspire_l2sup_backward_f32(const aspire_repset* q, const aspire_repset* c, int64_t D,
                              const int32_t* align, int weighted, const float* grad_scores,
                              float* grad_q_rows, float* grad_c_rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The cross-document distance matrix of the zero-padded sentence blocks, forward and backward: the
 *   pair_sims = -1 * torch.cdist(q_sent_reps.permute(0, 2, 1), p_sent_reps.permute(0, 2, 1))
 * of the two L1 regularisers, cd_l1_prop of WordSentAbsAlignBiEnc.forward_rank (disent_models.py:653-659) and cd_svalue_l1_prop of
 * WordSentAbsSupAlignBiEnc.forward_rank (:826-835), without the sign, and what autograd sends back through it.  PAIRED only (pair p =
 * query p with candidate p, q->n == c->n; no pairing argument) and padded sets only (ext > 0 on both, else ASPIRE_ERR_INVALID_ARG).
 *   dist         [P, q.ext, c.ext] out: d_ij = ||q_i - c_j|| from the direct difference for EVERY i < q.ext, j < c.ext.  A row at
 *                or beyond its document's length counts as the zero vector and is never read ("Pad values will be zeros", :654,
 *                :828): a real row against a pad row gives the real row's norm, pad against pad exactly 0.0f.
 *   grad_dist    [P, q.ext, c.ext] in: dLoss / dd.  torch.cdist's rule, A_ij = grad_dist_ij / d_ij and A_ij = 0 where d_ij == 0:
 *                  grad_q_i = sum_j A_ij (q_i - c_j)    j ascending over all c.ext columns, pad columns (c_j = 0) included
 *                  grad_c_j = sum_i A_ij (c_j - q_i)    i ascending over all q.ext rows
 *                for the valid rows; pad rows (len <= r < ext) get exact zeros.  The backward forms d_ij again from the rows by the
 *                forward's own loop (the same bits); it does not read the forward's output, so nothing has to be kept for it.
 *   grad_q_rows, grad_c_rows, the alignment of the buffers and the error codes as aspire_l2sup_backward_f32: every row of every
 *   document is written once with 16-byte stores, no atomics, no zero fill in front, the same bits on every run.  Documents of up
 *   to aspire_max_sents() rows (the backward keeps the pair's 128 x 128 weights in 64 KiB of LDS).  A document longer than its
 *   extent: NaN over the pair's whole dist block, NaN gradient rows, for that pair only.  One launch on `stream` each, one
 *   workgroup per pair, no workspace.
 * ------------------------------------------------------------------------------------------- */
int aspire_sent_cdist_f32(const aspire_repset* q, const aspire_repset* c, int64_t D,
                          float* dist /* [P, q.ext, c.ext] */, void* stream);
int aspire_sent_cdist_backward_f32(const aspire_repset* q, const aspire_repset* c, int64_t D,
                                   const float* grad_dist /* [P, q.ext, c.ext] */,
                                   float* grad_q_rows, float* grad_c_rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A15  precomputed-embedding rankers.  Replaces the per-query body of src/pre_process/pp_gen_nearest.py rank_pool (:683-717) and
 * rank_pool_faceted (:1166-1191): `all_doc_reps[pool_idxs, :]`, sklearn.neighbors.NearestNeighbors(algorithm='brute').fit on it and
 * kneighbors of the query row -- for J (query, pool) jobs in ONE call over ONE resident [N, 768] matrix of whole-document reps.
 * Nothing is gathered into a pool copy: a job is the matrix row of its query and a run of matrix rows, and a row that sits in many
 * pools is stored once.
 *   rows       [N, D] fp32, 16-byte aligned; D must be 768 (else ASPIRE_ERR_UNSUPPORTED); N < 2^31
 *   q_idx      DEVICE int32 [J]: matrix row of job j's query
 *   cand_idx   DEVICE int32 [C]: matrix rows of all jobs' candidates, back to back (C == job_off[J])
 *   J, C       the two counts (host values: job_off lives on the device)
 *   job_off, max_job, scores [C], k, job_base, top_scores, top_idx, keys, workspace: exactly the contract of
 *              aspire_dotmax_rank_batch_f32 (ties in pool order, (-inf, -1) beyond a pool's size, k == 0: scores only); the
 *              workspace, 16-byte aligned, is aspire_dense_rank_batch_workspace_bytes(J, C, max_job, k) bytes: the rank's scratch
 *              only, 0 for pools of <= 4096.
 *   metric     scores are SIMILARITIES, higher is better:
 *              ASPIRE_DENSE_L2      -sqrt(sum_k (q_k - c_k)^2) from direct differences in fp32 (what NearestNeighbors' default
 *                                   metric ranks by, negated): a candidate equal to its query scores exactly -0.0f; no expansion, no
 *                                   clamp rule, no cdist mode.  That is `scores`; top_scores and keys list it as +0.0f, since -0.0
 *                                   and +0.0 share one rank key (aspire_topk_desc_f32: a tie, decided by pool order).
 *              ASPIRE_DENSE_COSINE  the cosine as ASPIRE_SIM_COSINE documents it (sklearn's float32 normalisation rules).
 *              ASPIRE_DENSE_DOT     the raw dot product.
 *   One kernel form and one summation order for every call size: a pair's bits depend on its two rows only -- the same
 *   (query row, candidate row) scores the same bits in a call of one job and in a call of fifty.
 *   An index outside [0, N) in q_idx or cand_idx reads nothing and scores NaN for the pairs it touches (the host layer,
 *   aspire_amd.nearest, raises IndexError before it gets here); where such a pair lands in the ranked lists is not defined.
 *   Checked before any launch: a bad metric, negative counts, k < 0, k > 0 without (top_scores, top_idx) or keys, a null job_off,
 *   max_job outside [0, C], null scores / q_idx / cand_idx / rows with C > 0, misaligned rows or workspace, a workspace that is too
 *   small -> ASPIRE_ERR_INVALID_ARG; J >= 2^30 or C >= 2^31 - 8 -> ASPIRE_ERR_UNSUPPORTED; J == 0 -> ASPIRE_OK without a launch.
 *   Launches on `stream`: the scoring kernel (one wave per 8 consecutive candidates, the query row in registers), then the
 *   segmented rank.
 * ------------------------------------------------------------------------------------------- */
#define ASPIRE_DENSE_L2 0
#define ASPIRE_DENSE_COSINE 1
#define ASPIRE_DENSE_DOT 2
size_t aspire_dense_rank_batch_workspace_bytes(int64_t J, int64_t C, int64_t max_job, int64_t k);
int aspire_dense_rank_batch_f32(const float* rows, int64_t N, int64_t D, const int32_t* q_idx, int64_t J,
                                const int32_t* cand_idx, int64_t C, const int32_t* job_off, int64_t max_job, int metric,
                                float* scores, int64_t k, const int32_t* job_base, float* top_scores, int64_t* top_idx,
                                uint64_t* keys, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SURVEY.md 8(e)  shard merge.  The same rank in KEY form for the candidate-pool shards of a multi-GPU job:
 *   aspire_topk_keys_f32    per-query local top-k as sortable 64-bit keys [Q, k]:
 *                           (order-preserving score bits << 32) | (0xFFFFFFFF - global index), 0 = padding.
 *                           One unsigned descending sort of keys from ANY set of shards is the order of Python's
 *                           stable sorted(..., reverse=True) over the un-sharded pool (evaluate.py:76).
 *                           Needs idx_base + C < 2^32 - 1.  Workspace as aspire_topk_desc_f32.
 *   aspire_topk_merge_keys  keys [R, Q, k_in] as an all-gather of R ranks' [Q, k_in] blocks leaves them ->
 *                           top_scores [Q, k], top_idx [Q, k] (global indices; (-inf, -1) padding).
 *                           Limit: R * k_in <= 4096.
 * ------------------------------------------------------------------------------------------- */
int aspire_topk_keys_f32(const float* scores, int64_t Q, int64_t C, int64_t k, int64_t idx_base,
                         uint64_t* keys, void* workspace, size_t workspace_bytes, void* stream);
int aspire_topk_merge_keys(const uint64_t* keys, int64_t R, int64_t Q, int64_t k_in, int64_t k,
                           float* top_scores, int64_t* top_idx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Diagnostics (tests, bench.py, tuning) -- not part of the surface that replaces reference code.
 *   aspire_debug_set   pin a kernel form / grid: key = "SINKHORN" (wave | block | block-norepair | block16 | block-dense | block-wide), "COST_PATH"
 *                      (mfma | valu), "OT_FORM" (small | tile | fused), "COST1_BLOCKS" (n), "ATTN" (gemm), "GEMM" (f32 | bf16x3 | planes), "GEMM_TILE" (96 | 128 | 64), "GEMM_RING" (2 | 3), "GEMM_LN" (on | off: LayerNorm in / behind the N = 768 GEMMs),
 *                      "FUSED_VALU" (1),
 *                      "FUSED_NOSELF" (1), "FUSED_WAVES" (n: cap on the waves of a fused launch (max-sim launches too)), "FUSED_NOSOLVE" (1 | 2: timing only, invalid scores),
 *                      "TILE_WAVES" (n: cap on the waves of the 16-row streaming launches (tile16.hip, record items and max-sim too) and of the tiled cost
 *                      kernel for documents of <= 8 rows (OT_FORM tile); tests: several items per wave, the same bits),
 *                      "FUSED_SOLVE16" (0 | 1: the batched fused kernel's solve on sixteen / four lanes per pair; unset: four where
 *                      consecutive calls come on different streams; the same bits either way), "FUSED_NOREPAIR" (1: poisoned
 *                      pairs keep the fast solve's score -- invalid; tests); aspire_debug_get("FUSED_SOLVE16_LAUNCHES") counts the
 *                      launches of the four-lane form;
 *                      value NULL or "" restores the default.  The same switches are read
 *                      ONCE from the environment (ASPIRE_HIP_<key>) when the library is first used; nothing on the
 *                      launch path reads the environment.
 *   aspire_debug_ot_cost_stage_f32         the cost stage of aspire_ot_sinkhorn_f32 alone (no solve, scores untouched)
 *   aspire_debug_ot_rank_batch_stages_f32  chosen stages of aspire_ot_rank_batch_f32 alone: 1 tables + query boxes (nothing
 *                      for a batch whose scoring kernel derives them itself),
 *                      2 costs, 4 Sinkhorn solves (2 and 4 are ONE kernel in the fused form: either bit launches it),
 *                      8 rank (bench.py times the stages of a pass one by one this way, after a full call has filled
 *                      the workspace)
 *   aspire_debug_score_form  the kernel family a call would take, as short text in buf[0 .. len) -- e.g. "fused-self",
 *                      "tables+tiles cost=tile solve=block4x4+repair" -- without running it (no GPU needed).  kind: the entry family
 *                      (ASPIRE_FORM_*); the decision reads the sets' n / ext / max_len / planes / doc_box alone; asked: ASPIRE_ASKED_*
 *                      bits or'ed, for ASPIRE_FORM_OT_BATCH plus the debug entry's stage mask << 8 (0 = all stages); the otAspire
 *                      kinds read ONE_FORM and the scaling from prm; workspace_bytes 0 = what aspire_ot_workspace_bytes suggests.
 *                      Batched kinds take the jobs as equal shares of the candidates (max_job = ceil(c->n / q->n)).
 * ------------------------------------------------------------------------------------------- */
#define ASPIRE_FORM_L2AGG 0       /* aspire_l2agg_scores_f32 / aspire_l2max_scores_f32 */
#define ASPIRE_FORM_OT 1          /* aspire_ot_sinkhorn_f32 / aspire_ot_rank_f32 */
#define ASPIRE_FORM_OT_BATCH 2    /* aspire_ot_rank_batch_f32 */
#define ASPIRE_FORM_L2MAX_BATCH 3 /* aspire_l2max_rank_batch_f32 */
#define ASPIRE_ASKED_PAIR_OUTPUTS 1 /* pair_sims / plan / distribution outputs */
#define ASPIRE_ASKED_DIAMETERS 2    /* the caller's own diameters */
#define ASPIRE_ASKED_COST_ONLY 4    /* aspire_debug_ot_cost_stage_f32 */
#define ASPIRE_ASKED_PLAN_SIM 8     /* want == ASPIRE_OT_PLAN_SIM */
#define ASPIRE_ASKED_AGG_OTHER 16   /* an aggregation other than ASPIRE_AGG_MAX */
#define ASPIRE_ASKED_ONE_FORM 32    /* ASPIRE_CDIST_ONE_FORM (the max-sim kinds) */
int aspire_debug_score_form(int kind, const aspire_repset* q, const aspire_repset* c, int pairing, const aspire_ot_params* prm,
                            int asked, size_t workspace_bytes, char* buf, size_t len);
int aspire_debug_set(const char* key, const char* value);
/* the switch's current value as aspire_debug_set takes it ("" = default) into buf[0 .. len); for scoped pins that restore
 * what was set before them (an ASPIRE_HIP_* environment setting, an enclosing pin) */
int aspire_debug_get(const char* key, char* buf, size_t len);
int aspire_debug_ot_cost_stage_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                                   const aspire_ot_params* prm, float* scores, void* workspace, size_t workspace_bytes,
                                   void* stream);
int aspire_debug_ot_rank_batch_stages_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off,
                                          int64_t max_job, const aspire_ot_params* prm, int want, float* scores, int64_t k,
                                          float* top_scores, int64_t* top_idx, void* workspace, size_t workspace_bytes,
                                          void* stream, int stages);

/* Measurement aid: one wave spins for wall_us microseconds on `stream` and writes out[0] = shader-clock ticks, out[1] = 100 MHz
 * wall ticks: launched beside a kernel under study (another stream), out[0] / out[1] x 100 MHz is the clock the chip held under
 * it (the matrix-pipe kernels run power-limited well below the nominal 2.4 GHz; rooflines quote both). */
int aspire_debug_clock_probe(long long* out, long long wall_us, void* stream);

/* Cross-lane primitive self test (DPP / permlane forms vs ds_bpermute); out_mismatch_host[16] receives
 * the number of mismatching lanes per check (all 0 = ok; order: xor 1,2,4,8,16,32, row sum, col sum,
 * row max, col max, butterfly 64, butterfly 16).  Synchronous. */
int aspire_selftest_xlane(int* out_mismatch_host);

#ifdef __cplusplus
}
#endif
#endif /* ASPIRE_HIP_H */
