"""A1t: the BERT encoder under training -- a HuggingFace ``BertModel`` whose layer stack runs forward AND backward on this library's
kernels (aspire_bert_layers_forward_train_f32 / aspire_bert_layers_backward_f32 behind torch.ops.aspire.bert_layers_train).

``HipBertTrainEncoder(bert_model)`` is an ``nn.Module`` around the model; the parameters stay the model's own, so
``torch.optim.Adam(enc.parameters())`` trains them, ``state_dict()`` / ``load_state_dict()`` speak HuggingFace's names, and what was
trained loads straight into ``HipBertEncoder.from_state_dict`` / ``AspireConSent``.  Per forward, torch does the plumbing only: the
embedding sum (word + token-type + position rows: the tables' scatter gradient stays torch's) and the ``torch.cat`` of the query / key /
value weights and biases (autograd splits their gradient back); everything from the embedding LayerNorm to ``last_hidden_state``, and its
gradient down to every parameter, is the library's.

``forward_cls(batch, mix=None)`` is the read-out of the models whose reps are CLS rows (aspire_amd/cls_train.py): the same plumbing, then
torch.ops.aspire.bert_layers_train_cls -- the CLS rows of last_hidden_state, or of a mix of all hidden states, whose backward starts
from the [B, 768] gradient (no [B, L, 768] gradient is built in torch).

Dropout is opt-in.  ``HipBertTrainEncoder(bert_model)`` trains as ``BertModel`` does with ``hidden_dropout_prob =
attention_probs_dropout_prob = 0`` (and says so once when the config asks for more).  ``HipBertTrainEncoder(bert_model, dropout=True)``
applies the config's two probabilities at HuggingFace's four sites per layer stack, inside the library
(torch.ops.aspire.bert_layers_train_dropout): the masks are Philox4x32-10 words keyed by ``(seed, step, site, element)``
(include/aspire_hip.h states the contract), never stored, formed again by the backward.  ``seed`` defaults to ``torch.initial_seed()``;
``step`` is a uint32 counter that advances once per training forward, so a run is reproduced by its seed alone and resumed through
``dropout_state()`` / ``set_dropout_state(seed, step)``.  ``eval()`` and ``torch.no_grad()`` run the inference forward: no dropout, and
the counter does not move.

The embedding lookup is opt-in too.  ``HipBertTrainEncoder(bert_model, hip_embeddings=True)`` forms the embedding sum with
torch.ops.aspire.bert_embed_sum (the same bits as torch's expression) and the three tables' gradients with its backward: every row
written once, every sum in a fixed order, no atomics -- with it a run's gradients are the same bits on every run with the tables
trained, which torch's scatter backward (atomics) does not promise.  ``padding_idx`` is the word table's (its row gets no gradient, as
in torch).  ``check_ids=True`` (the default) looks at the ids and type ids first and raises IndexError for one out of range, at one
host sync per forward; ``check_ids=False`` says the caller has validated them (an id out of range is then never read: its row of the
sum is NaN).  The default ``hip_embeddings=False`` is the graph described above.

The precision of the matrix products is opt-in as well.  ``HipBertTrainEncoder(bert_model, matmul='bf16')`` runs all 16 products of a
layer (the four projections, Q K^T and P V forward; the ten of the backward) with both operands rounded to bf16 once, fp32
accumulators and fp32 epilogues -- what ``torch.autocast(dtype=torch.bfloat16)`` asks of them (torch.ops.aspire.bert_layers_train_prec /
bert_layers_train_cls_prec; include/aspire_hip.h states the arithmetic).  LayerNorm, soft-max, GELU, the dropout passes, the tape, the
parameters and every gradient stay fp32, so optimizers, gradient buckets and clipping see what they always saw.
``HipBertTrainEncoder(bert_model, matmul='bf16x3')`` keeps fp32 accuracy and moves the products that ``'fp32'`` still runs on the
fp32-input matrix cores -- P V forward; the five dX-like and six dW-like products of the backward, whose operands are k-major -- onto
the bf16 matrix cores: each operand split into three bf16 values, six products per term, fp32 accumulators.  The other products are
``'fp32'``'s own launches, which are that arithmetic already; the mode's results sit inside the fp32 mode's error bound.  The default
``matmul='fp32'`` goes through the operators described above, untouched.  ``eval()`` and ``torch.no_grad()`` forwards stay on the
inference path in fp32 in every mode: the mode is a property of training steps.

The attention form is opt-in too, with ``matmul='bf16'`` alone.  ``HipBertTrainEncoder(bert_model, matmul='bf16', attention='flash')``
runs each layer's attention as one fused forward kernel and three backward kernels (torch.ops.aspire.bert_layers_train_attn /
bert_layers_train_cls_attn; aspire_amd/csrc/enc_attn_train.hip): the tape keeps two fp32 statistics per (document, head, query)
instead of the [L, L] probabilities, so it grows linearly in L, and the backward forms the probabilities and the dropout masks again.
Its operands (Q, K, V, the probabilities, dctx, dS) are rounded to bf16 once each, as the mode's other products are; the masks are the
ones ``attention='gemm'`` draws.  With ``matmul='fp32'`` or ``'bf16x3'`` it raises NotImplementedError (a fused attention at fp32
accuracy does not exist).  The default ``attention='gemm'`` is the launches and bits described above.

Padding-free batches are opt-in as well, with ``attention='flash'`` alone.  ``HipBertTrainEncoder(bert_model, matmul='bf16',
attention='flash', packed=True)`` runs the layer stack, its tape and its workspace over the ``R = attention_mask.sum()`` valid token rows
alone (torch.ops.aspire.bert_layers_train_packed / bert_layers_train_cls_packed over the row lists of ``aspire_amd.packed_rows``; the
gather and scatter: aspire_amd/csrc/enc_pack.hip): rows in document order and, inside a document, in position order, so a mask with
holes or left padding packs the same way as right padding.  What the mode returns:
  * ``forward`` returns [B, L, 768] as before.  Valid rows are the mode's result; masked rows are EXACT ZEROS -- a deliberate departure,
    HuggingFace computes something there (nothing downstream reads it: the rank loss, the span pool and the CLS read-out never touch a
    pad row).  A document whose mask is all zero has no rows and its output rows are zeros; ``R == 0`` returns zeros and launches
    nothing.
  * The gradient with respect to the embedding sum is [B, L, 768] with exact zeros on masked rows (``hip_embeddings=True`` sees those
    zeros); the incoming gradient of ``last_hidden_state`` is read on valid rows only.
  * ``forward_cls`` takes each document's CLS row at its first packed row: it requires ``attention_mask[:, 0] == 1`` for every
    document and raises ValueError on the host otherwise, before a launch.
  * Dropout is keyed by the PADDED logical index, the one the padded modes use (row ``b L + l`` for the hidden sites,
    ``((b H + h) L + i) L + j`` with ``i``, ``j`` the tokens' original positions for the probabilities): with the same ``(seed, step)`` a
    packed step draws, at valid positions, the masks a padded step draws.  A run switches modes only through a fresh encoder;
    RankTrainer's checkpoint records ``packed`` and refuses a mismatch (a checkpoint without the key means False).
  * No atomics anywhere: every element of every output has one writer and every sum a fixed order -- the same bits on every run.
With any other ``attention`` (so with ``matmul='fp32'`` or ``'bf16x3'`` too) it raises NotImplementedError before any launch.  The default
``packed=False`` is the launches, bits, tape size and operators described above; ``eval()`` and ``torch.no_grad()`` forwards stay padded.

Not supported: activation checkpointing around this module -- the recomputed forward would draw the next step's masks, not the first
forward's.
"""
import warnings

import torch

from . import ops
from .encoder import _LAYER_KEYS, require_bert_base
from .packing import packed_rows


class HipBertTrainEncoder(torch.nn.Module):
    MATMUL_MODES = {'fp32': 0, 'bf16': 1, 'bf16x3': 3}        # include/aspire_hip.h: ASPIRE_MATMUL_* (2 is not a mode)
    ATTENTION_MODES = {'gemm': 0, 'flash': 1}                 # include/aspire_hip.h: ASPIRE_ATTENTION_*

    def __init__(self, bert_model, dropout=False, seed=None, hip_embeddings=False, check_ids=True, matmul='fp32', attention='gemm',
                 packed=False):
        super().__init__()
        if matmul not in self.MATMUL_MODES:
            raise ValueError(f"HipBertTrainEncoder: matmul={matmul!r}: 'fp32', 'bf16' or 'bf16x3'")
        if attention not in self.ATTENTION_MODES:
            raise ValueError(f"HipBertTrainEncoder: attention={attention!r}: 'gemm' or 'flash'")
        if attention == 'flash' and matmul != 'bf16':
            raise NotImplementedError(f"HipBertTrainEncoder: attention='flash' is built for matmul='bf16' alone (got matmul={matmul!r}): "
                                      'a fused attention at fp32 accuracy does not exist')
        if packed and attention != 'flash':
            raise NotImplementedError(f"HipBertTrainEncoder: packed=True is built for attention='flash' alone (got matmul={matmul!r}, "
                                      f"attention={attention!r}): the three-kernel attention has per-document [L, L] matrices")
        self.matmul, self.attention, self.packed = matmul, attention, bool(packed)
        dev = ops.require_gpu()
        self.hip_embeddings, self.check_ids = bool(hip_embeddings), bool(check_ids)
        cfg = bert_model.config
        if getattr(cfg, 'model_type', 'bert') in ('roberta', 'mpnet') or not hasattr(bert_model.embeddings, 'token_type_embeddings'):
            raise NotImplementedError(f'{type(bert_model).__name__}: the training encoder is built for BertModel (the position ids and the '
                                      'relative-position bias of aspire_bert_extras have no backward)')
        require_bert_base(cfg, 64, 'HipBertTrainEncoder')
        self.p_hidden, self.p_attn = (float(cfg.hidden_dropout_prob), float(cfg.attention_probs_dropout_prob)) if dropout else (0.0, 0.0)
        for name, p in (('hidden_dropout_prob', self.p_hidden), ('attention_probs_dropout_prob', self.p_attn)):
            if not 0.0 <= p < 1.0:
                raise ValueError(f'HipBertTrainEncoder: {name} = {p} outside [0, 1)')
        self.dropout = bool(dropout)
        self._seed = (torch.initial_seed() if seed is None else int(seed)) % 2 ** 64
        self._step = 0
        if not dropout and (cfg.hidden_dropout_prob > 0 or cfg.attention_probs_dropout_prob > 0):
            # (the text is pinned by a test; "not built" here reads: not in this instance -- dropout=True applies it)
            warnings.warn(f'HipBertTrainEncoder: dropout is not built -- the model trains as with hidden_dropout_prob = '
                          f'attention_probs_dropout_prob = 0 (the config has {cfg.hidden_dropout_prob} / {cfg.attention_probs_dropout_prob})',
                          UserWarning)
        self.bert = bert_model.to(device=dev, dtype=torch.float32)      # (moved in place: the parameters stay the model's own)
        self.config = cfg

    # HuggingFace's names, not 'bert.'-prefixed ones: what is saved here is a BertModel's state dict
    def state_dict(self, *args, **kwargs):
        return self.bert.state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, *args, **kwargs):
        return self.bert.load_state_dict(state_dict, *args, **kwargs)

    def dropout_state(self):
        """(seed, step): the key of the NEXT training forward's masks"""
        return self._seed, self._step

    def set_dropout_state(self, seed, step):
        self._seed, self._step = int(seed) % 2 ** 64, int(step) % 2 ** 32

    def layer_weights(self):
        """[emb_ln_g, emb_ln_b] + per layer the twelve tensors of struct aspire_bert_layer (pack_weights' order), on the autograd graph of
        the model's parameters."""
        emb = self.bert.embeddings
        w = [emb.LayerNorm.weight, emb.LayerNorm.bias]
        for layer in self.bert.encoder.layer:
            att = layer.attention.self
            w.append(torch.cat([att.query.weight, att.key.weight, att.value.weight], 0))
            w.append(torch.cat([att.query.bias, att.key.bias, att.value.bias], 0))
            named = dict(layer.named_parameters())
            w += [named[k] for k in _LAYER_KEYS]
        return w

    def _emb_sum(self, tok, typ, seq_len):
        """BertEmbeddings' sum in its order, (word + token type) + position, [B, L, 768]: torch's lookups (the tables' gradients are then
        torch's scatter), or with hip_embeddings the library's operator, whose backward writes the three tables' gradients in a fixed
        order.  The two give the same bits forward."""
        emb = self.bert.embeddings
        if not self.hip_embeddings:
            return (emb.word_embeddings(tok) + emb.token_type_embeddings(typ)) + emb.position_embeddings.weight[:seq_len]
        word, types = emb.word_embeddings, emb.token_type_embeddings.weight
        if self.check_ids and tok.numel():
            # one host sync for the four extremes (nn.Embedding raises IndexError on the reference path)
            lo_t, hi_t, lo_y, hi_y = torch.stack([tok.min(), tok.max(), typ.min(), typ.max()]).tolist()
            if lo_t < 0 or hi_t >= word.weight.shape[0]:
                raise IndexError('token id out of range')
            if lo_y < 0 or hi_y >= types.shape[0]:
                raise IndexError('token type id out of range')
        return torch.ops.aspire.bert_embed_sum(tok, typ, word.weight, emb.position_embeddings.weight, types,
                                               -1 if word.padding_idx is None else int(word.padding_idx))

    def forward_cls(self, batch, mix=None):
        """The CLS read-out of the bi-encoders and the sentence encoders (MySPECTER.doc_reps_bert, SentBERTWrapper.sent_reps_bert):
        batch -- the reference's batch dict (tokid_tt, seg_tt, attnmask_tt) or an (ids, type ids, mask) tuple of int64 [B, L] tensors --
        -> [B, 768] fp32 on the GPU: the CLS rows of last_hidden_state, or with mix (post-soft-max weights [n_layers + 1], a device
        tensor that may carry a graph) of the mix-weighted sum of all n_layers + 1 hidden states.  In train() mode with grad enabled
        one operator (torch.ops.aspire.bert_layers_train_cls) runs the training forward, the read-out and, on backward, the layer stack's
        gradient from the [B, 768] gradient alone; the dropout counter advances once per call, as in forward.  In eval() or under
        torch.no_grad() it is the inference forward's read-out (no tape, no dropout, the counter stays)."""
        from . import torch_ops  # noqa: F401  (registers the operators)
        if isinstance(batch, dict):
            tokid_tt, token_type_ids, attention_mask = batch['tokid_tt'], batch.get('seg_tt'), batch.get('attnmask_tt')
        else:
            tokid_tt, token_type_ids, attention_mask = (tuple(batch) + (None, None))[:3] if isinstance(batch, (tuple, list)) else (batch, None, None)
        emb = self.bert.embeddings
        dev = emb.word_embeddings.weight.device
        tok = tokid_tt.to(device=dev, dtype=torch.int64)
        typ = token_type_ids.to(device=dev, dtype=torch.int64) if token_type_ids is not None else torch.zeros_like(tok)
        msk = attention_mask.to(device=dev, dtype=torch.int64) if attention_mask is not None else torch.ones_like(tok)
        cfg = self.config
        if mix is not None:
            mix = mix.to(device=dev, dtype=torch.float32).reshape(-1)
            if mix.numel() != cfg.num_hidden_layers + 1:
                raise ValueError(f'mix: expected {cfg.num_hidden_layers + 1} weights, got {mix.numel()}')
        if not (self.training and torch.is_grad_enabled()):
            with torch.no_grad():
                tables = [emb.word_embeddings.weight, emb.position_embeddings.weight, emb.token_type_embeddings.weight]
                return torch.ops.aspire.bert_cls_forward(tok, typ, msk, tables + self.layer_weights(), cfg.num_attention_heads,
                                                         cfg.layer_norm_eps, mix.cpu().tolist() if mix is not None else [])
        seq_len = tok.shape[1]
        if seq_len > cfg.max_position_embeddings:
            raise IndexError(f'{seq_len} tokens: beyond max_position_embeddings={cfg.max_position_embeddings}')
        if self.packed:
            # a document's CLS row is its first packed row: that is position 0 only where position 0 is a valid token
            if msk.numel() and not bool((msk[:, 0] != 0).all()):
                raise ValueError('HipBertTrainEncoder(packed=True).forward_cls: every document needs attention_mask[:, 0] == 1 -- the CLS '
                                 'row is read at the document\'s first packed row')
            rows = packed_rows(msk)
        emb_sum = self._emb_sum(tok, typ, seq_len)
        seed, step = self._seed, self._step
        if self.dropout:
            self._step = (step + 1) % 2 ** 32
        if self.packed:
            return torch.ops.aspire.bert_layers_train_cls_packed(emb_sum, rows.doc_start, rows.row_src, rows.row_dst, rows.max_len, rows.prefix,
                                                                 self.layer_weights(), mix, cfg.num_attention_heads, cfg.layer_norm_eps,
                                                                 self.p_hidden, self.p_attn, seed - 2 ** 64 if seed >= 2 ** 63 else seed, step)[0]
        args = (emb_sum, msk, self.layer_weights(), mix, cfg.num_attention_heads, cfg.layer_norm_eps, self.p_hidden, self.p_attn,
                seed - 2 ** 64 if seed >= 2 ** 63 else seed, step)
        if self.attention != 'gemm':
            return torch.ops.aspire.bert_layers_train_cls_attn(*args, self.MATMUL_MODES[self.matmul], self.ATTENTION_MODES[self.attention])[0]
        if self.matmul != 'fp32':
            return torch.ops.aspire.bert_layers_train_cls_prec(*args, self.MATMUL_MODES[self.matmul])[0]
        cls, _layer_cls, _tape = torch.ops.aspire.bert_layers_train_cls(*args)
        return cls

    def forward(self, tokid_tt, token_type_ids=None, attention_mask=None):
        """int64 [B, L] tensors (any device), or the reference's batch dict (tokid_tt, seg_tt, attnmask_tt) -> last_hidden_state
        [B, L, 768] fp32 on the GPU.  In train() mode with grad enabled the layer stack runs the training forward and keeps its tape for
        the backward; under torch.no_grad() or in eval() it is the plain inference forward (no tape, not differentiable)."""
        from . import torch_ops  # noqa: F401  (registers the operators)
        if isinstance(tokid_tt, dict):
            tokid_tt, token_type_ids, attention_mask = tokid_tt['tokid_tt'], tokid_tt.get('seg_tt'), tokid_tt.get('attnmask_tt')
        emb = self.bert.embeddings
        dev = emb.word_embeddings.weight.device
        tok = tokid_tt.to(device=dev, dtype=torch.int64)
        typ = token_type_ids.to(device=dev, dtype=torch.int64) if token_type_ids is not None else torch.zeros_like(tok)
        msk = attention_mask.to(device=dev, dtype=torch.int64) if attention_mask is not None else torch.ones_like(tok)
        cfg = self.config
        if not (self.training and torch.is_grad_enabled()):
            with torch.no_grad():
                tables = [emb.word_embeddings.weight, emb.position_embeddings.weight, emb.token_type_embeddings.weight]
                return torch.ops.aspire.bert_encoder_forward(tok, typ, msk, tables + self.layer_weights(), cfg.num_attention_heads,
                                                             cfg.layer_norm_eps)
        seq_len = tok.shape[1]
        if seq_len > cfg.max_position_embeddings:
            raise IndexError(f'{seq_len} tokens: beyond max_position_embeddings={cfg.max_position_embeddings}')
        emb_sum = self._emb_sum(tok, typ, seq_len)
        if self.matmul != 'fp32':
            # one operator pair for the mode, with and without dropout (probabilities of 0 launch no dropout pass)
            seed, step = self._seed, self._step
            if self.dropout:
                self._step = (step + 1) % 2 ** 32
            if self.packed:
                rows = packed_rows(msk)
                return torch.ops.aspire.bert_layers_train_packed(emb_sum, rows.doc_start, rows.row_src, rows.row_dst, rows.max_len, rows.prefix,
                                                                 self.layer_weights(), cfg.num_attention_heads, cfg.layer_norm_eps,
                                                                 self.p_hidden, self.p_attn, seed - 2 ** 64 if seed >= 2 ** 63 else seed, step)[0]
            args = (emb_sum, msk, self.layer_weights(), cfg.num_attention_heads, cfg.layer_norm_eps, self.p_hidden, self.p_attn,
                    seed - 2 ** 64 if seed >= 2 ** 63 else seed, step, self.MATMUL_MODES[self.matmul])
            if self.attention != 'gemm':
                return torch.ops.aspire.bert_layers_train_attn(*args, self.ATTENTION_MODES[self.attention])[0]
            hidden, _tape = torch.ops.aspire.bert_layers_train_prec(*args)
            return hidden
        if not self.dropout:
            hidden, _tape = torch.ops.aspire.bert_layers_train(emb_sum, msk, self.layer_weights(), cfg.num_attention_heads, cfg.layer_norm_eps)
            return hidden
        seed, step = self._seed, self._step
        self._step = (step + 1) % 2 ** 32
        # (an operator's int is a signed 64-bit one: the seed goes through as its two's complement)
        hidden, _tape = torch.ops.aspire.bert_layers_train_dropout(emb_sum, msk, self.layer_weights(), cfg.num_attention_heads, cfg.layer_norm_eps,
                                                                   self.p_hidden, self.p_attn, seed - 2 ** 64 if seed >= 2 ** 63 else seed, step)
        return hidden
