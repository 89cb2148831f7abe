"""A1: BERT-base encoder on the GPU through libaspire_hip.so (aspire_bert_forward_f32).

``HipBertEncoder`` takes its weights from a HuggingFace ``BertModel`` (the object the reference builds with
``AutoModel.from_pretrained`` at examples/ex_aspire_consent.py:33) and exposes the one call the reference
makes on it: ``encoder(tokid_tt, token_type_ids=seg_tt, attention_mask=attnmask_tt).last_hidden_state``
(:72-73).  Weights are copied to HBM once, in nn.Linear layout; query/key/value are concatenated so the three
projections are one GEMM.  The bi-encoders' CLS read-out (aspire_bert_forward_cls_f32) runs on the same weights
(forward_cls), the pooler (aspire_bert_pooler_f32) behind it where the model has one (forward_pooled), and run_checked is the
one fall-back rule every model class applies to what it hands out.

The encoder also takes a ``RobertaModel`` or an ``MPNetModel`` (the SentenceTransformer baselines, aspire_amd/sbert.py): their
forward is aspire_bert_forward_var_f32 with the position ids those models number real tokens by (position_ids_from_input_ids)
and, for MPNet, the relative-position bias expanded per distance (relative_bias_table); forward_mean is the masked-mean read-out
(aspire_token_mean_pool_f32) behind it.  Nothing changes for a BertModel.
"""
import ctypes
import math
import warnings
from types import SimpleNamespace

import torch

from . import ops
from ._lib import MATMUL_FP16, MATMUL_FP32, BertExtras, BertLayer, BertWeights, check, lib, pinned

_LAYER_KEYS = ('attention.output.dense.weight', 'attention.output.dense.bias', 'attention.output.LayerNorm.weight',
               'attention.output.LayerNorm.bias', 'intermediate.dense.weight', 'intermediate.dense.bias', 'output.dense.weight',
               'output.dense.bias', 'output.LayerNorm.weight', 'output.LayerNorm.bias')


# MPNetLayer's parameter names in struct aspire_bert_layer's order behind w_qkv / b_qkv
_MPNET_LAYER_KEYS = ('attention.attn.o.weight', 'attention.attn.o.bias', 'attention.LayerNorm.weight', 'attention.LayerNorm.bias',
                     'intermediate.dense.weight', 'intermediate.dense.bias', 'output.dense.weight', 'output.dense.bias',
                     'output.LayerNorm.weight', 'output.LayerNorm.bias')
REL_SPAN = 512          # the bias table covers key - query in (-512, 512): every distance of the forward's L <= 512


def position_ids_from_input_ids(ids, padding_idx):
    """HF create_position_ids_from_input_ids (modeling_roberta.py, modeling_mpnet.py): real tokens count from padding_idx + 1,
    pad tokens get padding_idx.  int64 [B, L], on ids' device."""
    real = (ids != padding_idx).to(torch.int64)
    return torch.cumsum(real, dim=1) * real + padding_idx


def relative_bias_table(weight, span=REL_SPAN, num_buckets=32, max_distance=128):
    """MPNetEncoder.compute_position_bias per distance: float32 [n_heads, 2 span - 1], entry [h, (j - i) + span - 1] the bias of
    (query i, key j).  weight: relative_attention_bias.weight [num_buckets, n_heads].  The bucket arithmetic is HF's
    relative_position_bucket operation for operation (torch, the logarithm in float32), so bucket edges fall where HF puts them;
    the bias depends on j - i alone (compute_position_bias is called without position ids: the indices, not the RoBERTa-style ids)."""
    rel = torch.arange(-(span - 1), span, dtype=torch.long)        # memory_position - context_position
    n = -rel
    half = num_buckets // 2
    ret = (n < 0).to(torch.long) * half
    n = torch.abs(n)
    max_exact = half // 2
    is_small = n < max_exact
    val_if_large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (half - max_exact)).to(torch.long)
    val_if_large = torch.min(val_if_large, torch.full_like(val_if_large, half - 1))
    bucket = ret + torch.where(is_small, n, val_if_large)
    return weight.detach().to(device='cpu', dtype=torch.float32)[bucket].t().contiguous()


def fill_layers(struct_type, tensors):
    """A ctypes array of struct_type (BertLayer, BertLayerGrads: the same twelve pointer fields) over twelve tensors per layer, in the
    fields' order.  At least one element, so that the array is never empty; the caller keeps the tensors alive."""
    n_layers = len(tensors) // 12
    layers = (struct_type * max(n_layers, 1))()
    for i in range(n_layers):
        for (f, _), t in zip(struct_type._fields_, tensors[12 * i:12 * i + 12]):
            setattr(layers[i], f, ctypes.c_void_p(t.data_ptr()))
    return layers


def _pack(weights, n_tables, n_heads, ln_eps):
    """struct aspire_bert_weights over [the n_tables (3 or 0) embedding tables] + [emb_ln_g, emb_ln_b] + 12 per layer; tables that are
    not given stay NULL with 0 rows.  The geometry comes from the tensors' shapes."""
    w = [t.contiguous() for t in weights]
    assert all(t.is_cuda and t.dtype == torch.float32 for t in w)
    tables, stack = w[:n_tables], w[n_tables:]
    n_layers = (len(stack) - 2) // 12
    layers = fill_layers(BertLayer, stack[2:])
    hidden_size = stack[0].shape[0]
    ffn = stack[2 + 6].shape[0] if n_layers else 4 * hidden_size
    table_ptrs = [ctypes.c_void_p(t.data_ptr()) for t in tables] or [None] * 3
    table_rows = [t.shape[0] for t in tables] or [0] * 3
    bw = BertWeights(*table_ptrs, ctypes.c_void_p(stack[0].data_ptr()), ctypes.c_void_p(stack[1].data_ptr()), layers, n_layers, n_heads,
                     hidden_size, ffn, *table_rows, float(ln_eps), None)
    bw._keep = (layers, w)
    return bw


def pack_weights(weights, n_heads, ln_eps):
    """struct aspire_bert_weights over fp32 GPU tensors [word_emb, pos_emb, type_emb, emb_ln_g, emb_ln_b] + per layer [w_qkv, b_qkv,
    w_o, b_o, ln1_g, ln1_b, w_ffn1, b_ffn1, w_ffn2, b_ffn2, ln2_g, ln2_b] (struct aspire_bert_layer, nn.Linear layout); the geometry
    comes from the tensors' shapes.  The struct keeps the (contiguous) tensors and its layer array alive."""
    assert (len(weights) - 5) % 12 == 0 and len(weights) >= 5, 'weights: 5 embedding tensors + 12 per layer'
    return _pack(weights, 3, n_heads, ln_eps)


def pack_layer_stack(weights, n_heads, ln_eps):
    """struct aspire_bert_weights of the training entry points (aspire_bert_layers_forward_train_f32 / _backward_f32), which start behind
    the embedding lookup: fp32 GPU tensors [emb_ln_g, emb_ln_b] + the twelve per layer in pack_weights' order; the three tables stay
    NULL.  The struct keeps the (contiguous) tensors and its layer array alive."""
    assert (len(weights) - 2) % 12 == 0 and len(weights) >= 2, 'weights: emb_ln_g, emb_ln_b + 12 per layer'
    return _pack(weights, 0, n_heads, ln_eps)


def require_bert_base(cfg, ffn_multiple, who):
    """NotImplementedError unless cfg describes what the kernels are built for: BERT-base geometry with intermediate_size a multiple of
    ffn_multiple, erf-GELU, absolute position embeddings."""
    if cfg.hidden_size != 768 or cfg.num_attention_heads != 12 or cfg.intermediate_size % ffn_multiple:
        ffn = f', intermediate_size % {ffn_multiple} == 0' if ffn_multiple > 1 else ''
        raise NotImplementedError(f'{who}: only BERT-base geometry (hidden 768, 12 heads{ffn}) is built')
    if cfg.hidden_act != 'gelu':
        raise NotImplementedError(f'{who}: hidden_act {cfg.hidden_act!r}: only erf-GELU is built')
    if getattr(cfg, 'position_embedding_type', 'absolute') != 'absolute':
        raise NotImplementedError(f'{who}: only absolute position embeddings are built')


def run_checked(run, outputs_finite, who, status):
    """The encoder's fall-back rule around run() (a forward and whatever reads it out), each re-run at most once, in this order:
      * status() non-zero: a LayerNorm-epilogue GEMM gave up waiting for its row block (enc_gemm_p.hip: gemm_p_ln_kernel's bounded
        wait) and what run() made is invalid -- run again with the LayerNorm as its own pass, pinned(GEMM_LN='off');
      * outputs_finite(result) false: an activation left the fp16 planes' range (HipBertEncoder.forward_full_range) -- run again
        on the kernels that take any fp32 value, pinned(GEMM='bf16x3', ATTN='f32').
    status() and outputs_finite() are the host syncs of the rule: one of each per call.  Returns run()'s last result."""
    out = run()
    if status():
        warnings.warn(f'{who}: the fused GEMM + LayerNorm exchange timed out; encoding again with ASPIRE_HIP_GEMM_LN=off')
        with pinned(GEMM_LN='off'):
            out = run()
    if not outputs_finite(out):
        warnings.warn(f'{who}: non-finite reps on the fp16-plane encoder path (an activation beyond 65504); encoding again with '
                      'ASPIRE_HIP_GEMM=bf16x3, ASPIRE_HIP_ATTN=f32')
        with pinned(GEMM='bf16x3', ATTN='f32'):
            out = run()
    return out


class HipBertEncoder:
    """matmul: 'fp32' (default: every product fp32-accurate) or 'fp16' (opt-in: the four projections of a layer with every operand
    rounded to fp16 once, one matrix instruction per term -- include/aspire_hip.h, A1h; everything else as in 'fp32').  `matmul`
    reads the mode in force: 'fp32' when the weights leave the mode's range (a UserWarning says so)."""
    MATMUL_MODES = {'fp32': MATMUL_FP32, 'fp16': MATMUL_FP16}

    def __init__(self, bert_model, matmul='fp32'):
        if matmul not in self.MATMUL_MODES:
            raise ValueError(f"HipBertEncoder: matmul {matmul!r}: 'fp32' or 'fp16' (the training encoder has the bf16 modes)")
        dev = ops.require_gpu()
        cfg = bert_model.config
        require_bert_base(cfg, 1, 'HipBertEncoder')          # (any intermediate_size: the library checks it per call)
        sd = {k: v.detach() for k, v in bert_model.state_dict().items()}
        self.config = cfg
        self.device = dev
        # 'bert': BertModel.  'roberta' / 'mpnet': position ids from the token ids (padding_idx: RobertaEmbeddings takes the config's
        # pad_token_id, MPNetEmbeddings always 1), MPNet also the relative-position bias and no token types
        self.kind = kind = cfg.model_type if getattr(cfg, 'model_type', None) in ('roberta', 'mpnet') else 'bert'
        self.padding_idx = {'bert': None, 'roberta': cfg.pad_token_id, 'mpnet': 1}[kind]
        pre = next((p for p in ('bert.', 'roberta.', 'mpnet.') if any(k.startswith(p) for k in sd)), '')
        emb = pre + 'embeddings.'
        w = [sd[emb + k] for k in ('word_embeddings.weight', 'position_embeddings.weight')]
        # (MPNet: one zero row stands for the token-type table: (word + 0) + position is exact)
        w.append(torch.zeros(1, cfg.hidden_size) if kind == 'mpnet' else sd[emb + 'token_type_embeddings.weight'])
        w += [sd[emb + k] for k in ('LayerNorm.weight', 'LayerNorm.bias')]
        for i in range(cfg.num_hidden_layers):
            p = f'{pre}encoder.layer.{i}.'
            att = p + ('attention.attn.' if kind == 'mpnet' else 'attention.self.')
            q, k, v = ('q', 'k', 'v') if kind == 'mpnet' else ('query', 'key', 'value')
            w += [torch.cat([sd[att + q + '.weight'], sd[att + k + '.weight'], sd[att + v + '.weight']], 0),
                  torch.cat([sd[att + q + '.bias'], sd[att + k + '.bias'], sd[att + v + '.bias']], 0)]
            w += [sd[p + k] for k in (_MPNET_LAYER_KEYS if kind == 'mpnet' else _LAYER_KEYS)]
        self._rel_bias = None
        if kind == 'mpnet':
            self._rel_bias = relative_bias_table(sd[pre + 'encoder.relative_attention_bias.weight']).to(dev)
        self._w = pack_weights([t.to(device=dev, dtype=torch.float32) for t in w], cfg.num_attention_heads, cfg.layer_norm_eps)
        # HF BertPooler's dense layer, where the model has one (forward_pooled); it is no part of struct aspire_bert_weights
        self._pooler = None
        if pre + 'pooler.dense.weight' in sd:
            self._pooler = tuple(sd[pre + 'pooler.dense.' + k].to(device=dev, dtype=torch.float32).contiguous() for k in ('weight', 'bias'))
        self._ws = {}                       # one workspace per HIP stream: forwards on different streams overlap
        # the nn.Linear weights' fp16 planes, formed once (include/aspire_hip.h: aspire_bert_prepare_planes)
        nbytes = lib.aspire_bert_planes_bytes(ctypes.byref(self._w))
        if nbytes and cfg.intermediate_size % 128 == 0:
            self._planes = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            try:
                check(lib.aspire_bert_prepare_planes(ctypes.byref(self._w), ops._ptr(self._planes), nbytes, ops._stream()))
                self._w.planes = ctypes.c_void_p(self._planes.data_ptr())
            except NotImplementedError as e:        # a weight beyond the fp16 planes' range: the on-the-fly bf16x3 GEMMs take any fp32
                warnings.warn(f'HipBertEncoder: {e}; running without pre-split weights')
                self._planes = None
        # the fp16 matmul mode's single planes of the same weights (aspire_bert_prepare_hplanes): an argument of the _prec entries
        self.matmul = 'fp32'
        self.matmul_asked = matmul          # what a rebuilt encoder (load_state_dict) is asked for again
        self._hplanes = None
        if matmul == 'fp16':
            nbytes = lib.aspire_bert_hplanes_bytes(ctypes.byref(self._w))
            try:
                if not nbytes or cfg.intermediate_size % 128:
                    raise NotImplementedError('the fp16 matmul mode needs at least one layer and intermediate_size % 128 == 0')
                hp = torch.empty(nbytes, device=dev, dtype=torch.uint8)
                check(lib.aspire_bert_prepare_hplanes(ctypes.byref(self._w), ops._ptr(hp), nbytes, ops._stream()))
                self._hplanes, self.matmul = hp, 'fp16'
            except NotImplementedError as e:
                warnings.warn(f"HipBertEncoder: {e}; running with matmul='fp32'")

    @classmethod
    def from_state_dict(cls, config, sd, matmul='fp32'):
        """The encoder of a BertModel(config) holding state dict sd (with a pooler when sd has one: load_state_dict is strict)."""
        from transformers import BertModel
        bm = BertModel(config, add_pooling_layer=any(k.startswith('pooler.') for k in sd))
        bm.load_state_dict(sd)
        return cls(bm, matmul=matmul)

    def eval(self):
        return self

    def device_inputs(self, tokid_tt, token_type_ids=None, attention_mask=None, check_ids=True):
        """int64 [B, L] tensors (any device) -> (ids, type ids or None, mask) contiguous int64 on the GPU; no mask: all ones.
        check_ids: token ids outside the vocabulary raise IndexError (one host sync); False: the caller has validated them."""
        dev = self.device
        tok = tokid_tt.to(device=dev, dtype=torch.int64).contiguous()
        if check_ids and tok.numel() and (int(tok.max()) >= self.config.vocab_size or int(tok.min()) < 0):
            raise IndexError('token id out of range')   # nn.Embedding raises IndexError on the reference path
        typ = token_type_ids.to(device=dev, dtype=torch.int64).contiguous() if token_type_ids is not None else None
        msk = attention_mask.to(device=dev, dtype=torch.int64).contiguous() if attention_mask is not None \
            else torch.ones_like(tok)
        return tok, typ, msk

    def _workspace(self, need):
        """The current stream's workspace, grown to `need` bytes: a forward's scratch is reused by the next one on its stream."""
        sid = torch.cuda.current_stream().cuda_stream
        ws = self._ws.get(sid)
        if ws is None or ws.numel() < need:
            self._ws[sid] = ws = torch.empty(max(need, 16), device=self.device, dtype=torch.uint8)
        return ws

    def forward_full_range(self, tokid_tt, token_type_ids=None, attention_mask=None):
        """The forward on the kernels that take ANY fp32 activation: GEMM operands split into three bf16 planes on the fly, attention
        on the fp32-input MFMA.  The default path keeps activations as two fp16 planes (|x| <= 65504: far above what BERT-base
        checkpoints produce, but a fine-tuned model with an outlier feature beyond it turns into inf there); run_checked re-runs a
        forward with non-finite output on these kernels."""
        with pinned(GEMM='bf16x3', ATTN='f32'):
            return self.forward_hidden(tokid_tt, token_type_ids, attention_mask, check_ids=False)

    def _extras(self, tok):
        """struct aspire_bert_extras of a RoBERTa / MPNet forward over the device ids tok (None for a BertModel), and the tensors it
        points to.  The position ids are at most padding_idx + L by construction: checked against the table's rows without a sync."""
        if self.kind == 'bert':
            return None, None
        if self.padding_idx + tok.shape[1] >= self.config.max_position_embeddings:
            raise IndexError(f'{tok.shape[1]} tokens: position ids reach {self.padding_idx + tok.shape[1]}, beyond '
                             f'max_position_embeddings={self.config.max_position_embeddings}')
        pos = position_ids_from_input_ids(tok, self.padding_idx).contiguous()
        x = BertExtras(ctypes.c_void_p(pos.data_ptr()), ops._ptr(self._rel_bias), REL_SPAN if self._rel_bias is not None else 0)
        return x, pos

    def forward_hidden(self, tokid_tt, token_type_ids=None, attention_mask=None, check_ids=True):
        """int64 [B, L] tensors (any device) -> last_hidden_state [B, L, 768] on the GPU.  check_ids=False: the caller has
        validated the token ids already (encode_to_pool checks all its batches with one device round trip).  A RoBERTa / MPNet
        encoder runs aspire_bert_forward_var_f32 (MPNet takes no token types: they are ignored, as MPNetModel ignores them)."""
        tok, typ, msk = self.device_inputs(tokid_tt, token_type_ids, attention_mask, check_ids)
        b, l = tok.shape
        out = torch.empty(b, l, 768, device=self.device, dtype=torch.float32)
        if self.matmul != 'fp32':
            # the mode's entry (the extras NULL for a BertModel); a GEMM pin -- forward_full_range, run_checked -- overrides the mode inside
            mode = self.MATMUL_MODES[self.matmul]
            ws = self._workspace(lib.aspire_bert_workspace_bytes_prec(ctypes.byref(self._w), b, l, mode))
            x, _pos = self._extras(tok)
            check(lib.aspire_bert_forward_prec_f32(ctypes.byref(self._w), ctypes.byref(x) if x is not None else None, ops._ptr(self._hplanes),
                                                   mode, ops._ptr(tok), None if self.kind == 'mpnet' else ops._ptr(typ), ops._ptr(msk), b, l,
                                                   ops._ptr(out), ops._ptr(ws), ws.numel(), ops._stream()))
            return out
        ws = self._workspace(lib.aspire_bert_workspace_bytes(ctypes.byref(self._w), b, l))
        if self.kind == 'bert':
            check(lib.aspire_bert_forward_f32(ctypes.byref(self._w), ops._ptr(tok), ops._ptr(typ), ops._ptr(msk), b, l,
                                              ops._ptr(out), ops._ptr(ws), ws.numel(), ops._stream()))
            return out
        x, _pos = self._extras(tok)         # (_pos: alive until the launches are queued; the stream orders its reuse)
        check(lib.aspire_bert_forward_var_f32(ctypes.byref(self._w), ctypes.byref(x), ops._ptr(tok),
                                              None if self.kind == 'mpnet' else ops._ptr(typ), ops._ptr(msk), b, l, ops._ptr(out),
                                              ops._ptr(ws), ws.numel(), ops._stream()))
        return out

    def forward_mean(self, tokid_tt, token_type_ids=None, attention_mask=None, normalize=False, check_ids=True):
        """sentence-transformers' read-out: int64 [B, L] tensors (any device) -> the mean of last_hidden_state over the tokens with
        attention_mask != 0 [B, 768] on the GPU (Pooling in mean mode), with normalize divided by max(its L2 norm, 1e-12)
        (Normalize): forward_hidden, then aspire_token_mean_pool_f32.  check_ids as forward_hidden."""
        tok, typ, msk = self.device_inputs(tokid_tt, token_type_ids, attention_mask, check_ids)
        return ops.token_mean_pool(self.forward_hidden(tok, typ, msk, check_ids=False), msk, normalize)

    def forward_cls(self, tokid_tt, token_type_ids=None, attention_mask=None, layer_mix=None, want_layers=False, check_ids=True):
        """The bi-encoders' read-out (aspire_bert_forward_cls_f32): int64 [B, L] tensors (any device) -> (the CLS rows of the
        layer_mix-weighted sum of the n_layers + 1 hidden states [B, 768] -- of the last hidden state alone when layer_mix is None --,
        the CLS rows of every hidden state [n_layers + 1, B, 768] with want_layers, else None), on the GPU.  layer_mix: n_layers + 1
        float32 weights, already softmaxed.  check_ids as forward_hidden."""
        if self.kind != 'bert':
            raise NotImplementedError(f'forward_cls: the CLS-only forward is built for BertModel, not {self.kind}')
        tok, typ, msk = self.device_inputs(tokid_tt, token_type_ids, attention_mask, check_ids)
        b, l = tok.shape
        dev = self.device
        out = torch.empty(b, 768, device=dev, dtype=torch.float32)
        layers = torch.empty(self.config.num_hidden_layers + 1, b, 768, device=dev, dtype=torch.float32) if want_layers else None
        mix = ctypes.cast((ctypes.c_float * len(layer_mix))(*[float(x) for x in layer_mix]), ctypes.c_void_p) \
            if layer_mix is not None else None
        if self.matmul != 'fp32':
            mode = self.MATMUL_MODES[self.matmul]
            ws = self._workspace(lib.aspire_bert_cls_workspace_bytes_prec(ctypes.byref(self._w), b, l, mode))
            check(lib.aspire_bert_forward_cls_prec_f32(ctypes.byref(self._w), ops._ptr(self._hplanes), mode, ops._ptr(tok), ops._ptr(typ),
                                                       ops._ptr(msk), b, l, mix, ops._ptr(out), ops._ptr(layers), ops._ptr(ws), ws.numel(),
                                                       ops._stream()))
            return out, layers
        ws = self._workspace(lib.aspire_bert_cls_workspace_bytes(ctypes.byref(self._w), b, l))
        check(lib.aspire_bert_forward_cls_f32(ctypes.byref(self._w), ops._ptr(tok), ops._ptr(typ), ops._ptr(msk), b, l, mix,
                                              ops._ptr(out), ops._ptr(layers), ops._ptr(ws), ws.numel(), ops._stream()))
        return out, layers

    def forward_pooled(self, tokid_tt, token_type_ids=None, attention_mask=None, check_ids=True):
        """BertModel's two read-outs: int64 [B, L] tensors (any device) -> (last_hidden_state[:, 0] [B, 768], pooler_output [B, 768]
        = tanh(dense(that row))), on the GPU: forward_cls with no layer mix, then aspire_bert_pooler_f32.  ValueError for a model
        without a pooler.  Under run_checked, judge finiteness on the CLS rows: tanh turns an overflowed activation into +-1."""
        if self._pooler is None:
            raise ValueError('forward_pooled: the model has no pooler (pooler.dense.weight / pooler.dense.bias)')
        cls = self.forward_cls(tokid_tt, token_type_ids, attention_mask, check_ids=check_ids)[0]
        return cls, ops.bert_pooler(cls, *self._pooler)

    @staticmethod
    def status():
        """The encoder kernels' sticky status word (include/aspire_hip.h: aspire_bert_status), read and cleared; synchronises the current
        stream.  Non-zero: a LayerNorm-epilogue GEMM gave up waiting for its row block (ASPIRE_BERT_STATUS_LN_TIMEOUT) -- the forwards
        since the last check are invalid; run_checked runs them again under pinned(GEMM_LN='off')."""
        v = ctypes.c_int32(0)
        check(lib.aspire_bert_status(ctypes.byref(v), ops._stream()))
        return int(v.value)

    def checked(self, run, outputs_finite, who):
        """run_checked with this encoder's status word."""
        return run_checked(run, outputs_finite, who, self.status)

    def __call__(self, tokid_tt, token_type_ids=None, attention_mask=None):
        return SimpleNamespace(last_hidden_state=self.forward_hidden(tokid_tt, token_type_ids, attention_mask))
