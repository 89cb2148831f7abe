"""ctypes binding of libaspire_hip.so (the C ABI declared in include/aspire_hip.h).

The library is the product: there is no CPU or PyTorch-eager fallback.  If it is missing the import
fails loudly; if it is present but no GPU is visible, every compute entry point raises.
"""
import ctypes
import os

# PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so).  It must be in the process BEFORE
# libaspire_hip.so is dlopen'ed so that both resolve the same runtime: device pointers and streams that
# torch hands out are only meaningful to the runtime that created them.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# ASPIRE_HIP_LIB: developer override (instrumented builds under build/); the product path is in-tree.
LIB_PATH = os.environ.get('ASPIRE_HIP_LIB') or os.path.join(_HERE, 'lib', 'libaspire_hip.so')

c_void_p, c_int, c_int32, c_int64, c_double, c_size_t = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int32,
                                                         ctypes.c_int64, ctypes.c_double, ctypes.c_size_t)

ASPIRE_OK, ASPIRE_ERR_INVALID_ARG, ASPIRE_ERR_UNSUPPORTED, ASPIRE_ERR_HIP = 0, 1, 2, 3
CDIST_AUTO, CDIST_DIRECT, CDIST_MM = 0, 1, 2
MATMUL_FP32, MATMUL_FP16 = 0, 4                 # ASPIRE_MATMUL_*: the inference forwards' _prec entries
ATTENTION_GEMM, ATTENTION_FLASH = 0, 1      # ASPIRE_ATTENTION_*: the _attn_ entry points of the training encoder
CDIST_ONE_FORM = 0x100       # or'ed into cdist_mode of the max-sim entry points: one kernel form whatever the call's size
OT_FLAG_ONE_FORM = 1         # aspire_ot_params.flags: the same for otAspire
CDIST_CENTER = 0x200         # rows with a large common component: subtract the query's mean row before the expansion (max-sim entries)
OT_FLAG_CENTER = 2           # the same for otAspire
PAIR_CROSS, PAIR_PAIRED = 0, 1
OT_DISTANCE, OT_PLAN_SIM, OT_SIMILARITY = 0, 1, 2
AGG_MAX, AGG_TOP2, AGG_ATTENTION = 0, 1, 2
SIM_COSINE, SIM_DOT = 0, 1
DENSE_L2, DENSE_COSINE, DENSE_DOT = 0, 1, 2
FORM_L2AGG, FORM_OT, FORM_OT_BATCH, FORM_L2MAX_BATCH = 0, 1, 2, 3      # aspire_debug_score_form: kind
ASKED_PAIR_OUTPUTS, ASKED_DIAMETERS, ASKED_COST_ONLY, ASKED_PLAN_SIM, ASKED_AGG_OTHER, ASKED_ONE_FORM = 1, 2, 4, 8, 16, 32


class RepPlanes(ctypes.Structure):
    """struct aspire_rep_planes"""
    _fields_ = [('planes', c_void_p), ('row_nrm', c_void_p), ('row_iscale', c_void_p), ('mu', c_void_p),
                ('total_rows', c_int64), ('plane_rows', c_int64)]


class RepSet(ctypes.Structure):
    """struct aspire_repset"""
    _fields_ = [('rows', c_void_p), ('start', c_void_p), ('len', c_void_p), ('n', c_int64),
                ('ext', c_int32), ('max_len', c_int32), ('planes', ctypes.POINTER(RepPlanes)), ('doc_box', c_void_p)]


class OtParams(ctypes.Structure):
    """struct aspire_ot_params"""
    _fields_ = [('blur', c_double), ('scaling', c_double), ('sent_sm_temp', c_double), ('cdist_mode', c_int32),
                ('flags', c_int32)]


class BertLayer(ctypes.Structure):
    """struct aspire_bert_layer"""
    _fields_ = [(n, c_void_p) for n in ('w_qkv', 'b_qkv', 'w_o', 'b_o', 'ln1_g', 'ln1_b', 'w_ffn1', 'b_ffn1',
                                        'w_ffn2', 'b_ffn2', 'ln2_g', 'ln2_b')]


class BertWeights(ctypes.Structure):
    """struct aspire_bert_weights"""
    _fields_ = [('word_emb', c_void_p), ('pos_emb', c_void_p), ('type_emb', c_void_p), ('emb_ln_g', c_void_p),
                ('emb_ln_b', c_void_p), ('layers', ctypes.POINTER(BertLayer)), ('n_layers', c_int32),
                ('n_heads', c_int32), ('hidden', c_int32), ('ffn_dim', c_int32), ('vocab', c_int32),
                ('max_pos', c_int32), ('n_types', c_int32), ('ln_eps', ctypes.c_float), ('planes', c_void_p)]


class BertLayerGrads(ctypes.Structure):
    """struct aspire_bert_layer_grads"""
    _fields_ = list(BertLayer._fields_)


class BertGrads(ctypes.Structure):
    """struct aspire_bert_grads"""
    _fields_ = [('emb_ln_g', c_void_p), ('emb_ln_b', c_void_p), ('layers', ctypes.POINTER(BertLayerGrads))]


class BertDropout(ctypes.Structure):
    """struct aspire_bert_dropout"""
    _fields_ = [('p_hidden', ctypes.c_float), ('p_attn', ctypes.c_float), ('seed', ctypes.c_uint64), ('step', ctypes.c_uint32)]


class BertPacking(ctypes.Structure):
    """struct aspire_bert_packing"""
    _fields_ = [('rows', c_int64), ('max_len', c_int32), ('prefix', c_int32), ('doc_start', c_void_p), ('row_src', c_void_p),
                ('row_dst', c_void_p)]


class BertExtras(ctypes.Structure):
    """struct aspire_bert_extras"""
    _fields_ = [('pos_ids', c_void_p), ('rel_bias', c_void_p), ('rel_span', c_int32)]


class OptimTensor(ctypes.Structure):
    """struct aspire_optim_tensor"""
    _fields_ = [('param', c_void_p), ('grad', c_void_p), ('state1', c_void_p), ('state2', c_void_p), ('n', c_int64),
                ('step', c_int64), ('lr', c_double)]


class AdamWTensor(ctypes.Structure):
    """struct aspire_adamw_tensor"""
    _fields_ = OptimTensor._fields_ + [('weight_decay', c_double)]


class GradTensor(ctypes.Structure):
    """struct aspire_grad_tensor"""
    _fields_ = [('grad', c_void_p), ('n', c_int64)]


class AspireHipError(RuntimeError):
    pass


# name -> (restype, argtypes); must list every function include/aspire_hip.h declares.
SIGNATURES = {
    'aspire_abi_version': (c_int, []),
    'aspire_last_error': (ctypes.c_char_p, []),
    'aspire_max_sents': (c_int, []),
    'aspire_span_mean_pool_f32': (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                          c_void_p, c_void_p, c_void_p]),
    'aspire_span_mean_pool_rows_f32': (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                               c_void_p, c_void_p, c_void_p, c_void_p]),
    'aspire_span_pool_ranges_f32': (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                            c_void_p, c_void_p, c_void_p, c_void_p]),
    'aspire_span_mean_pool_backward_f32': (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                                   c_void_p, c_void_p]),
    'aspire_cls_l2_f32': (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_double, c_void_p, c_void_p]),
    'aspire_cls_l2_backward_f32': (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_double, c_void_p, c_void_p,
                                           c_void_p, c_void_p]),
    'aspire_optim_workspace_bytes': (c_size_t, [c_int64]),
    'aspire_adam_step_f32': (c_int, [ctypes.POINTER(OptimTensor), c_int64, c_double, c_double, c_double, c_void_p, c_size_t, c_void_p]),
    'aspire_adagrad_step_f32': (c_int, [ctypes.POINTER(OptimTensor), c_int64, c_double, c_double, c_void_p, c_size_t, c_void_p]),
    'aspire_adam_step_scaled_f32': (c_int, [ctypes.POINTER(OptimTensor), c_int64, c_double, c_double, c_double, c_void_p, c_void_p, c_size_t,
                                            c_void_p]),
    'aspire_adagrad_step_scaled_f32': (c_int, [ctypes.POINTER(OptimTensor), c_int64, c_double, c_double, c_void_p, c_void_p, c_size_t,
                                               c_void_p]),
    'aspire_adamw_step_f32': (c_int, [ctypes.POINTER(AdamWTensor), c_int64, c_double, c_double, c_double, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    'aspire_grad_bucket_elems': (c_int64, [ctypes.POINTER(c_int64), c_int64, ctypes.POINTER(c_int64)]),
    'aspire_grad_bucket_workspace_bytes': (c_size_t, [c_int64]),
    'aspire_grad_bucket_pack_f32': (c_int, [ctypes.POINTER(GradTensor), c_int64, c_double, c_void_p, c_int64, c_void_p, c_size_t,
                                            c_void_p]),
    'aspire_grad_norm_workspace_bytes': (c_size_t, [ctypes.POINTER(c_int64), c_int64]),
    'aspire_grad_norm_f32': (c_int, [ctypes.POINTER(GradTensor), c_int64, c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_grad_scale_workspace_bytes': (c_size_t, [c_int64]),
    'aspire_grad_scale_f32': (c_int, [ctypes.POINTER(GradTensor), c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_bert_planes_bytes': (c_size_t, [ctypes.POINTER(BertWeights)]),
    'aspire_bert_prepare_planes': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_size_t, c_void_p]),
    'aspire_bert_workspace_bytes': (c_size_t, [ctypes.POINTER(BertWeights), c_int64, c_int64]),
    'aspire_bert_forward_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                        c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_bert_forward_var_f32': (c_int, [ctypes.POINTER(BertWeights), ctypes.POINTER(BertExtras), c_void_p, c_void_p, c_void_p,
                                            c_int64, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_bert_tape_bytes': (c_size_t, [ctypes.POINTER(BertWeights), c_int64, c_int64]),
    'aspire_bert_train_workspace_bytes': (c_size_t, [ctypes.POINTER(BertWeights), c_int64, c_int64]),
    'aspire_bert_layers_forward_train_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                                     c_size_t, c_void_p, c_size_t, c_void_p]),
    'aspire_bert_layers_backward_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_size_t,
                                                c_void_p, ctypes.POINTER(BertGrads), c_void_p, c_size_t, c_void_p]),
    'aspire_bert_layers_forward_train_dropout_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                                             c_void_p, c_size_t, c_void_p, c_size_t, ctypes.POINTER(BertDropout), c_void_p]),
    'aspire_bert_layers_backward_dropout_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                                        c_size_t, c_void_p, ctypes.POINTER(BertGrads), c_void_p, c_size_t,
                                                        ctypes.POINTER(BertDropout), c_void_p]),
    'aspire_bert_dropout_mask_u8': (c_int, [ctypes.c_uint64, ctypes.c_uint32, c_int32, ctypes.c_float, c_int64, c_int64, c_void_p,
                                            c_void_p]),
    'aspire_bert_cls_mix_train_f32': (c_int, [ctypes.POINTER(BertWeights), c_int64, c_int64, c_void_p, c_size_t, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p]),
    'aspire_bert_layers_backward_cls_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_void_p, c_size_t, c_void_p, ctypes.POINTER(BertGrads), c_void_p, c_void_p,
                                                    c_size_t, ctypes.POINTER(BertDropout), c_void_p]),
    'aspire_bert_layers_forward_train_prec_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                                          c_void_p, c_size_t, c_void_p, c_size_t, ctypes.POINTER(BertDropout), c_int, c_void_p]),
    'aspire_bert_layers_backward_prec_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                                     c_void_p, c_void_p, c_size_t, c_void_p, ctypes.POINTER(BertGrads), c_void_p, c_void_p,
                                                     c_size_t, ctypes.POINTER(BertDropout), c_int, c_void_p]),
    'aspire_bert_tape_bytes_attn': (c_size_t, [ctypes.POINTER(BertWeights), c_int64, c_int64, c_int]),
    'aspire_bert_train_workspace_bytes_attn': (c_size_t, [ctypes.POINTER(BertWeights), c_int64, c_int64, c_int]),
    'aspire_bert_layers_forward_train_attn_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                                          c_void_p, c_size_t, c_void_p, c_size_t, ctypes.POINTER(BertDropout), c_int, c_int,
                                                          c_void_p]),
    'aspire_bert_layers_backward_attn_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                                     c_void_p, c_void_p, c_size_t, c_void_p, ctypes.POINTER(BertGrads), c_void_p, c_void_p,
                                                     c_size_t, ctypes.POINTER(BertDropout), c_int, c_int, c_void_p]),
    'aspire_bert_cls_mix_train_attn_f32': (c_int, [ctypes.POINTER(BertWeights), c_int64, c_int64, c_void_p, c_size_t, c_void_p, c_void_p,
                                                   c_void_p, c_void_p, c_int, c_void_p]),
    'aspire_debug_flash_attn_train_f32': (c_int, [c_void_p, c_void_p, c_int64, c_int64, ctypes.POINTER(BertDropout), c_void_p, c_void_p,
                                                  c_void_p]),
    'aspire_debug_flash_attn_train_backward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                                           ctypes.POINTER(BertDropout), c_int, c_void_p, c_void_p, c_void_p]),
    'aspire_bert_tape_bytes_packed': (c_size_t, [ctypes.POINTER(BertWeights), c_int64, c_int64, c_int64]),
    'aspire_bert_train_workspace_bytes_packed': (c_size_t, [ctypes.POINTER(BertWeights), c_int64, c_int64, c_int64]),
    'aspire_bert_layers_forward_train_packed_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, ctypes.POINTER(BertPacking), c_int64, c_int64,
                                                            c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, ctypes.POINTER(BertDropout), c_int,
                                                            c_int, c_void_p]),
    'aspire_bert_layers_backward_packed_f32': (c_int, [ctypes.POINTER(BertWeights), ctypes.POINTER(BertPacking), c_int64, c_int64, c_void_p,
                                                       c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, ctypes.POINTER(BertGrads),
                                                       c_void_p, c_void_p, c_size_t, ctypes.POINTER(BertDropout), c_int, c_int, c_void_p]),
    'aspire_bert_cls_mix_train_packed_f32': (c_int, [ctypes.POINTER(BertWeights), ctypes.POINTER(BertPacking), c_int64, c_int64, c_void_p,
                                                     c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'aspire_debug_flash_attn_train_packed_f32': (c_int, [c_void_p, ctypes.POINTER(BertPacking), c_int64, c_int64, ctypes.POINTER(BertDropout),
                                                         c_void_p, c_void_p, c_void_p]),
    'aspire_debug_flash_attn_train_packed_backward_f32': (c_int, [c_void_p, ctypes.POINTER(BertPacking), c_void_p, c_void_p, c_void_p, c_int64,
                                                                  c_int64, ctypes.POINTER(BertDropout), c_int, c_void_p, c_void_p, c_void_p]),
    'aspire_debug_gemm_bf16_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int64,
                                           c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, ctypes.c_float, c_void_p, c_void_p,
                                           c_int64, c_int, c_void_p]),
    'aspire_debug_gemm_bf16x3_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int64,
                                             c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, ctypes.c_float, c_void_p, c_void_p,
                                             c_int64, c_int, c_void_p]),
    'aspire_bert_hplanes_bytes': (c_size_t, [ctypes.POINTER(BertWeights)]),
    'aspire_bert_prepare_hplanes': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_size_t, c_void_p]),
    'aspire_bert_workspace_bytes_prec': (c_size_t, [ctypes.POINTER(BertWeights), c_int64, c_int64, c_int]),
    'aspire_bert_cls_workspace_bytes_prec': (c_size_t, [ctypes.POINTER(BertWeights), c_int64, c_int64, c_int]),
    'aspire_bert_forward_prec_f32': (c_int, [ctypes.POINTER(BertWeights), ctypes.POINTER(BertExtras), c_void_p, c_int, c_void_p, c_void_p,
                                             c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_bert_forward_cls_prec_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                                 c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_debug_hplane_bytes': (c_size_t, [c_int64, c_int64]),
    'aspire_debug_split_hplane': (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int, c_void_p]),
    'aspire_debug_gemm_hplane': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int,
                                         c_void_p]),
    'aspire_inbatch_xent_f32': (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    'aspire_inbatch_xent_backward_f32': (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'aspire_bert_embed_sum_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64,
                                          c_void_p, c_void_p]),
    'aspire_bert_embed_workspace_bytes': (c_size_t, [c_int64, c_int64]),
    'aspire_bert_embed_backward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_token_mean_pool_f32': (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    'aspire_bert_status': (c_int, [ctypes.POINTER(ctypes.c_int32), c_void_p]),
    'aspire_bert_cls_workspace_bytes': (c_size_t, [ctypes.POINTER(BertWeights), c_int64, c_int64]),
    'aspire_bert_forward_cls_f32': (c_int, [ctypes.POINTER(BertWeights), c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_bert_pooler_f32': (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    'aspire_rep_planes_bytes': (c_size_t, [c_int64]),
    'aspire_rep_planes_prepare': (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_size_t, ctypes.POINTER(RepPlanes),
                                          c_void_p]),
    'aspire_repset_boxes_f32': (c_int, [ctypes.POINTER(RepSet), c_int64, c_void_p, c_void_p]),
    'aspire_l2max_scores_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p]),
    'aspire_l2agg_scores_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int, c_int, c_int,
                                        ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    'aspire_l2agg_backward_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int, c_int, ctypes.c_double,
                                          c_void_p, c_void_p, c_void_p, c_void_p]),
    'aspire_ot_sinkhorn_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int,
                                       ctypes.POINTER(OtParams), c_void_p, c_int64, c_int, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_ot_backward_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int, ctypes.POINTER(OtParams),
                                       c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'aspire_ot_workspace_bytes': (c_size_t, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int]),
    'aspire_group_diameter_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int, c_int64,
                                          c_void_p, c_void_p]),
    'aspire_topk_workspace_bytes': (c_size_t, [c_int64, c_int64, c_int64]),
    'aspire_topk_desc_f32': (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                     c_size_t, c_void_p]),
    'aspire_ot_rank_workspace_bytes': (c_size_t, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64]),
    'aspire_ot_rank_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, ctypes.POINTER(OtParams), c_void_p,
                                   c_int64, c_int, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                   c_void_p]),
    'aspire_topk_keys_f32': (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_topk_merge_keys': (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    'aspire_ot_rank_batch_workspace_bytes': (c_size_t, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int64]),
    'aspire_ot_rank_batch_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_void_p, c_int64,
                                         ctypes.POINTER(OtParams), c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_l2max_rank_batch_workspace_bytes': (c_size_t, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int64]),
    'aspire_l2max_rank_batch_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_void_p, c_int64, c_int,
                                            c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_l2agg_rank_batch_workspace_bytes': (c_size_t, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int64]),
    'aspire_l2agg_rank_batch_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_void_p, c_int64, c_int, c_int,
                                            ctypes.c_double, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_size_t, c_void_p]),
    'aspire_dotmax_scores_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int, c_int, c_void_p,
                                         c_void_p]),
    'aspire_dotmax_rank_batch_workspace_bytes': (c_size_t, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int64]),
    'aspire_dotmax_rank_batch_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_void_p, c_int64, c_int,
                                             c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_dot_argmax_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_void_p, c_void_p, c_void_p]),
    'aspire_jointsm_scores_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int, c_void_p, c_void_p,
                                          c_void_p]),
    'aspire_jointsm_rank_batch_workspace_bytes': (c_size_t, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int64]),
    'aspire_jointsm_rank_batch_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_void_p, c_int64,
                                              c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_jointsm_backward_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int, c_void_p, c_void_p,
                                            c_void_p, c_void_p]),
    'aspire_l2sup_scores_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    'aspire_l2sup_backward_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_void_p, c_int, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    'aspire_sent_cdist_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_void_p, c_void_p]),
    'aspire_sent_cdist_backward_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_void_p, c_void_p, c_void_p,
                                               c_void_p]),
    'aspire_dense_rank_batch_workspace_bytes': (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    'aspire_dense_rank_batch_f32': (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int,
                                            c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_debug_set': (c_int, [ctypes.c_char_p, ctypes.c_char_p]),
    'aspire_debug_get': (c_int, [ctypes.c_char_p, ctypes.c_char_p, c_size_t]),
    'aspire_debug_score_form': (c_int, [c_int, ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int, ctypes.POINTER(OtParams), c_int,
                                        c_size_t, ctypes.c_char_p, c_size_t]),
    'aspire_debug_ot_cost_stage_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_int,
                                               ctypes.POINTER(OtParams), c_void_p, c_void_p, c_size_t, c_void_p]),
    'aspire_debug_ot_rank_batch_stages_f32': (c_int, [ctypes.POINTER(RepSet), ctypes.POINTER(RepSet), c_int64, c_void_p, c_int64,
                                                      ctypes.POINTER(OtParams), c_int, c_void_p, c_int64, c_void_p, c_void_p,
                                                      c_void_p, c_size_t, c_void_p, c_int]),
    'aspire_debug_clock_probe': (c_int, [c_void_p, ctypes.c_longlong, c_void_p]),
    'aspire_selftest_xlane': (c_int, [ctypes.POINTER(c_int)]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f'{LIB_PATH} is missing: build it first with `python -c "import __graft_entry__ as g; g.build()"` '
            f'(hipcc --offload-arch=gfx950).  aspire_amd has no CPU fallback.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(status):
    if status != ASPIRE_OK:
        msg = lib.aspire_last_error().decode('utf-8', 'replace')
        if status == ASPIRE_ERR_INVALID_ARG:
            # the reference signals these with `assert`, keep the exception type
            raise AssertionError(msg)
        if status == ASPIRE_ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        raise AspireHipError(msg)


class pinned:
    """Context manager over aspire_debug_set: pin diagnostic switches (kernel forms, grids) for a block of calls, e.g.
    ``with pinned(SINKHORN='block', COST_PATH='valu'): ...``; on exit every switch goes back to what it was before the
    block (an enclosing pin, an ASPIRE_HIP_* environment setting, or the default)."""

    def __init__(self, **kv):
        self.kv = kv
        self.before = {}

    def __enter__(self):
        buf = ctypes.create_string_buffer(64)
        for k, v in self.kv.items():
            check(lib.aspire_debug_get(k.encode(), buf, len(buf)))
            self.before[k] = buf.value
            check(lib.aspire_debug_set(k.encode(), str(v).encode()))
        return self

    def __exit__(self, *exc):
        for k, v in self.before.items():
            lib.aspire_debug_set(k.encode(), v if v else None)
        self.before = {}
        return False
