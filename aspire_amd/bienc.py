"""AspireBiEnc: the SPECTER-CoCite whole-abstract bi-encoder, drop-in for the class of the same name in
examples/ex_aspire_bienc.py:33-58 and for the test-time surface of MySPECTER
(src/learning/facetid_models/disent_models.py:53-205), the ``cospecter`` model of evaluate.py
(src/evaluation/utils/models.py:509-566).

    model = AspireBiEnc(bert_model=BertModel.from_pretrained(...))
    model.load_state_dict(torch.load('model_cur_best.pt'))         # bert_encoder.* + bert_layer_weights.weight [1, 13]
    doc_reps = model.forward(tokenizer(texts, padding=True, return_tensors='pt'))     # [B, 768]

A document's rep is the CLS row of a learned softmax mix of all n_layers + 1 hidden states (``*-full`` checkpoints), or of the last
hidden state alone when there are no mix weights (the README's plain AutoModel use).  Both come out of ONE encoder call,
HipBertEncoder.forward_cls: the encoder with the CLS rows tapped after every layer and a last layer that computes the CLS rows only.
The mix weights are softmaxed on the host, as SoftmaxMixLayers does, and passed in.
"""
import numpy as np
import torch

from . import ops
from .batch_prep import batch_tensors
from .model_front import EncoderFront, add_to_store, load_hf, refuse_keys, strip_prefix


def split_state_dict(sd):
    """The reference's state dict (AspireBiEnc / MySPECTER) -> (the BertModel's own state dict, layer weights [1, n + 1] or None).
    Keys: ``bert_encoder.<BertModel key>`` and ``bert_layer_weights.weight``; anything else is an error."""
    enc, other = strip_prefix(sd, 'bert_encoder.')
    refuse_keys([k for k in other if k != 'bert_layer_weights.weight'], 'bi-encoder')
    mix = sd.get('bert_layer_weights.weight')
    if mix is not None and (mix.dim() != 2 or mix.shape[0] != 1):
        raise ValueError(f'bert_layer_weights.weight: expected [1, n_layers + 1], got {tuple(mix.shape)}')
    return enc, mix


class AspireBiEnc(EncoderFront):
    def __init__(self, model_hparams=None, bert_model=None, layer_weights=None, matmul='fp32'):
        """
        :param model_hparams: dict with 'base-pt-layer' (the HF model the reference loads, ex_aspire_bienc.py:40).
        :param bert_model: an already constructed transformers BertModel (weights are copied to the GPU).
        :param layer_weights: the SoftmaxMixLayers weight [1, n_layers + 1] (before the softmax), or None: last_hidden_state[:, 0].
        :param matmul: the encoder's matmul mode, 'fp32' or the opt-in 'fp16' (HipBertEncoder).
        """
        self.bert_encoding_dim = 768
        name = model_hparams['base-pt-layer'] if bert_model is None else None
        self._build_encoder(load_hf(name, bert_model, want_tokenizer=False)[0], matmul)
        self.bert_layer_count = self.bert_encoder.config.num_hidden_layers + 1   # plus 1 for the bottom most layer
        self.layer_weights = None
        if layer_weights is not None:
            self.set_layer_weights(layer_weights)

    def set_layer_weights(self, w):
        w = torch.as_tensor(w).detach().to('cpu', torch.float32).reshape(1, -1)
        if w.shape[1] != self.bert_layer_count:
            raise ValueError(f'layer weights: expected {self.bert_layer_count}, got {w.shape[1]}')
        self.layer_weights = w

    def load_state_dict(self, sd):
        """AspireBiEnc / MySPECTER state dict: the encoder is rebuilt from bert_encoder.*, the mix from bert_layer_weights.weight."""
        enc, mix = split_state_dict(sd)
        if enc:
            self._rebuild_encoder(enc)
            self.bert_layer_count = self.bert_encoder.config.num_hidden_layers + 1
        self.layer_weights = None
        if mix is not None:
            self.set_layer_weights(mix)
        return self

    def layer_mix(self):
        """softmax(W, dim=1) as SoftmaxMixLayers.forward computes it (ex_aspire_bienc.py:24-29), [n_layers + 1] float32, or None."""
        if self.layer_weights is None:
            return None
        return torch.softmax(self.layer_weights, dim=1)[0].numpy().astype(np.float32)

    # ---- the forward ---------------------------------------------------------------------------------------------------
    def forward_device(self, tokid_tt, token_type_ids=None, attention_mask=None, want_layers=False):
        """int64 [B, L] tensors (any device) -> (cls reps [B, 768], the CLS rows of every hidden state [n_layers + 1, B, 768] or None),
        on the GPU, under the encoder's fall-back rule (encoder.run_checked)."""
        enc, mix = self.bert_encoder, self.layer_mix()
        return self._checked_read(lambda tok, typ, msk: enc.forward_cls(tok, typ, msk, mix, want_layers, check_ids=False),
                                  lambda r: r, tokid_tt, token_type_ids, attention_mask, 'AspireBiEnc')      # both outputs judged

    def forward(self, bert_batch):
        """AspireBiEnc.forward (ex_aspire_bienc.py:46-58): [B, 768] CLS reps, on the device of the input ids."""
        tok, typ, msk = batch_tensors(bert_batch)
        return self.forward_device(tok, typ, msk)[0].to(tok.device)

    def partial_forward(self, bert_batch):
        """MySPECTER.partial_forward (disent_models.py:164-176): [B, 768] on the GPU (a 1-document batch stays [1, 768])."""
        tok, typ, msk = batch_tensors(bert_batch)
        return self.forward_device(tok, typ, msk)[0]

    # ---- MySPECTER's test-time surface ----------------------------------------------------------------------------------
    def caching_encode(self, batch_dict):
        """MySPECTER.caching_encode (disent_models.py:96-114): -> list of {'doc_cls_reps': np [768]}."""
        reps = self.partial_forward(batch_dict['bert_batch']).cpu().numpy()
        return [{'doc_cls_reps': reps[i, :]} for i in range(reps.shape[0])]

    def encode(self, batch_dict):
        """MySPECTER.encode (disent_models.py:116-129): -> {'doc_reps': np [B, 768]}."""
        return {'doc_reps': self.partial_forward(batch_dict['bert_batch']).cpu().numpy()}

    @staticmethod
    def caching_score(query_encode_ret_dict, cand_encode_ret_dicts):
        """MySPECTER.caching_score (disent_models.py:56-94): -pairwise_distance(q, c, p=2, eps=1e-6) of the query against every
        candidate (aspire_cls_l2_f32, PAIRED) -> {'batch_scores', 'pair_scores'} (the same squeezed array twice)."""
        gpu = ops.require_gpu()
        c = torch.from_numpy(np.vstack([d['doc_cls_reps'] for d in cand_encode_ret_dicts]).astype(np.float32)).to(gpu)
        q = torch.from_numpy(np.asarray(query_encode_ret_dict['doc_cls_reps'], dtype=np.float32).reshape(1, -1)).to(gpu)
        scores = (-1 * ops.cls_l2(q.expand(c.shape[0], -1).contiguous(), c, eps=1e-6)).squeeze().cpu().numpy()
        return {'batch_scores': scores, 'pair_scores': scores}

    # ---- corpus encoding ------------------------------------------------------------------------------------------------
    def encode_to_store(self, batches, pids, store=None):
        """Every bert_batch of `batches` (prepare_abstract_seqs / prepare_eval_seqs / an HF tokenizer dict) encoded; document j
        overall gets pid pids[j] with a [1, 768] rep.  Returns the RepStore (new, or `store` with the reps added): evaluate.score(...,
        method='l2max') then ranks a pool by -cdist of the 1 x 1 pair = -euclidean, TrainedAbstractModel.get_similarity (models.py:565)."""
        def blocks():
            for bb in batches:
                reps = self.partial_forward(bb).cpu().numpy()
                for i in range(reps.shape[0]):
                    yield reps[i:i + 1]
        return add_to_store(store, pids, blocks(), 'documents')
