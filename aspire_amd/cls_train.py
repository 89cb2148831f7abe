"""The training side of the CLS-row models -- ``cospecter`` (MySPECTER, src/learning/facetid_models/disent_models.py:24-205),
``cosentbert`` (SentBERTWrapper, sentsim_models.py:10-78) and ``ictsentbert`` (ICTBERTWrapper, sentsim_models.py:81-126) -- over
``HipBertTrainEncoder.forward_cls`` and this project's loss kernels, in the shape ``RankTrainer`` takes:

    model = BiEncTrain(bert_model, {'fine_tune': True}, dropout=True)
    RankTrainer(model, {}, train_hparams, model_path, train_batches, loss_fn=ClsTripletLoss().forward_rank).train()
    AspireBiEnc(bert_model=...).load_state_dict(torch.load(model_path + '/model_final.pt'))

    model = IctEncTrain(sent_bert, context_bert, dropout=True)
    RankTrainer(model, {}, train_hparams, model_path, train_batches, loss_fn=IctLoss().forward_rank).train()
    AspireSentEnc(bert_model=...).load_state_dict(torch.load(...))          # the context tower is dropped there

``hip_embeddings`` / ``check_ids`` go to every tower's HipBertTrainEncoder (the embedding tables' gradients in HIP, in a fixed order),
and so does ``matmul`` ('fp32' | 'bf16' | 'bf16x3': the mode of the layer stack's matrix products; a module's ``matmul`` attribute is its towers')
and ``attention`` ('gemm' | 'flash': the fused training attention, with ``matmul='bf16'`` alone; the ``attention`` attribute likewise)
and ``packed`` (padding-free batches, with ``attention='flash'`` alone: every document's mask must start with a valid token).
A module's ``forward(bert_batch)`` gives the [B, 768] document (sentence) reps; ``state_dict()`` speaks the reference's key names, so
``model_final.pt`` / ``model_cur_best.pt`` load into ``AspireBiEnc`` / ``AspireSentEnc`` unchanged.  What runs where: the layer stack,
the read-out (with MySPECTER's soft-max layer mix) and their backward are torch.ops.aspire.bert_layers_train_cls; the soft-max over
the mix logits is torch's, on the device; the triplet loss is rank_loss._hinge over torch.ops.aspire.cls_l2_pair, the in-batch
cross-entropy torch.ops.aspire.inbatch_xent.
"""
import torch

from . import ops
from .model_front import refuse_keys, strip_prefix
from .rank_loss import CLS_EPS, _hinge
from .train_encoder import HipBertTrainEncoder


class _ClsTrainModule(torch.nn.Module):
    """What the three modules share: towers are HipBertTrainEncoder children named as the reference names its encoders, the state dict
    is ``<tower>.<HuggingFace key>`` (+ the module's own parameters), the dropout state the towers' (seed, step) pairs in order."""
    towers = ()
    own_keys = ()

    def load_state_dict(self, state_dict, strict=True):
        rest = dict(state_dict)
        for name in self.towers:
            sd, _ = strip_prefix(rest, name + '.')
            if sd or strict:
                getattr(self, name).load_state_dict(sd, strict=strict)
            rest = {k: v for k, v in rest.items() if not k.startswith(name + '.')}
        own = dict(self.named_parameters(recurse=True))
        for key in self.own_keys:
            if key in rest:
                with torch.no_grad():
                    own[key].copy_(rest.pop(key))
            elif strict:
                raise KeyError(f'missing key in the state dict: {key}')
        if strict:
            refuse_keys(sorted(rest), type(self).__name__)
        return self

    def dropout_state(self):
        """the towers' (seed, step) in order, flat: the key of the NEXT training forward's masks"""
        return tuple(x for name in self.towers for x in getattr(self, name).dropout_state())

    def set_dropout_state(self, *state):
        assert len(state) == 2 * len(self.towers), f'{2 * len(self.towers)} numbers: (seed, step) per tower'
        for i, name in enumerate(self.towers):
            getattr(self, name).set_dropout_state(*state[2 * i:2 * i + 2])


class BiEncTrain(_ClsTrainModule):
    """MySPECTER's training side: a document's rep is the CLS row of the soft-max mix of all n_layers + 1 hidden states.
    model_hparams: 'fine_tune' (default True; False freezes the encoder's parameters -- the mix logits still train)."""
    towers = ('bert_encoder',)
    own_keys = ('bert_layer_weights.weight',)

    def __init__(self, bert_model, model_hparams=None, dropout=False, seed=None, hip_embeddings=False, check_ids=True, matmul='fp32', attention='gemm',
                 packed=False):
        super().__init__()
        self.bert_encoding_dim = 768
        self.bert_encoder = HipBertTrainEncoder(bert_model, dropout=dropout, seed=seed, hip_embeddings=hip_embeddings, check_ids=check_ids,
                                                matmul=matmul, attention=attention, packed=packed)
        self.matmul, self.attention, self.packed = self.bert_encoder.matmul, self.bert_encoder.attention, self.bert_encoder.packed
        self.bert_layer_count = self.bert_encoder.config.num_hidden_layers + 1      # plus 1 for the bottom most layer
        if not (model_hparams or {}).get('fine_tune', True):
            for param in self.bert_encoder.parameters():
                param.requires_grad = False
        self.bert_layer_weights = torch.nn.Linear(self.bert_layer_count, 1, bias=False).to(ops.require_gpu())

    def forward(self, bert_batch):
        """MySPECTER.partial_forward: [B, 768] on the GPU (a 1-document batch stays [1, 768])"""
        mix = torch.softmax(self.bert_layer_weights.weight, dim=1)[0]
        return self.bert_encoder.forward_cls(bert_batch, mix=mix)


class SentEncTrain(_ClsTrainModule):
    """SentBERTWrapper's training side: a sentence's rep is the CLS row of last_hidden_state."""
    towers = ('sent_encoder',)

    def __init__(self, bert_model, dropout=False, seed=None, hip_embeddings=False, check_ids=True, matmul='fp32', attention='gemm', packed=False):
        super().__init__()
        self.bert_encoding_dim = 768
        self.sent_encoder = HipBertTrainEncoder(bert_model, dropout=dropout, seed=seed, hip_embeddings=hip_embeddings, check_ids=check_ids,
                                                matmul=matmul, attention=attention, packed=packed)
        self.matmul, self.attention, self.packed = self.sent_encoder.matmul, self.sent_encoder.attention, self.sent_encoder.packed

    def forward(self, bert_batch):
        """SentBERTWrapper.sent_reps_bert without its squeeze: [B, 768] on the GPU"""
        return self.sent_encoder.forward_cls(bert_batch)


class IctEncTrain(_ClsTrainModule):
    """ICTBERTWrapper's training side: a sentence tower and a context tower.  The context tower's dropout seed is seed + 1 mod 2^64:
    the two towers never share masks."""
    towers = ('sent_encoder', 'context_encoder')

    def __init__(self, sent_bert, context_bert, dropout=False, seed=None, hip_embeddings=False, check_ids=True, matmul='fp32', attention='gemm',
                 packed=False):
        super().__init__()
        self.bert_encoding_dim = 768
        seed = (torch.initial_seed() if seed is None else int(seed)) % 2 ** 64
        embed = dict(hip_embeddings=hip_embeddings, check_ids=check_ids, matmul=matmul, attention=attention, packed=packed)
        self.sent_encoder = HipBertTrainEncoder(sent_bert, dropout=dropout, seed=seed, **embed)
        self.context_encoder = HipBertTrainEncoder(context_bert, dropout=dropout, seed=(seed + 1) % 2 ** 64, **embed)
        self.matmul, self.attention, self.packed = self.sent_encoder.matmul, self.sent_encoder.attention, self.sent_encoder.packed

    def forward(self, bert_batch):
        """the sentence tower's reps [B, 768]: what the evaluation encodes with"""
        return self.sent_encoder.forward_cls(bert_batch)

    def forward_context(self, bert_batch):
        return self.context_encoder.forward_cls(bert_batch)


class ClsTripletLoss:
    """MySPECTER.forward_rank / SentBERTWrapper.forward_rank: nn.TripletMarginLoss(margin=1, p=2, reduction='sum') over the models'
    reps, as rank_loss._hinge over torch.ops.aspire.cls_l2_pair (F.pairwise_distance with eps 1e-6, HIP forward and backward)."""

    def forward_rank(self, batch_rank, model, random_idxs=None):
        """batch_rank: 'query_bert_batch', 'pos_bert_batch' and, for explicit negatives, 'neg_bert_batch'; model(bert_batch) -> [B, 768].
        Without negatives the positives permuted by random_idxs (default torch.randperm(B)) are the negatives.
        :return: loss_val; a scalar on the GPU."""
        from . import torch_ops  # noqa: F401  (registers the operators)
        q_reps = model(batch_rank['query_bert_batch'])
        p_reps = model(batch_rank['pos_bert_batch'])
        if 'neg_bert_batch' in batch_rank:
            n_reps = model(batch_rank['neg_bert_batch'])
        else:
            # Use a shuffled set of positives as the negatives. -- in-batch negatives.
            if random_idxs is None:
                random_idxs = torch.randperm(p_reps.size()[0])
            n_reps = p_reps[torch.as_tensor(random_idxs, dtype=torch.long).to(p_reps.device)]
        return _hinge(torch.ops.aspire.cls_l2_pair(q_reps, p_reps, CLS_EPS), torch.ops.aspire.cls_l2_pair(q_reps, n_reps, CLS_EPS))


class IctLoss:
    """ICTBERTWrapper.forward_rank: the soft-max cross-entropy of every query sentence against the batch's contexts, summed
    (torch.ops.aspire.inbatch_xent).  A batch of one row has a loss of exactly 0."""

    def forward_rank(self, batch_rank, model):
        """batch_rank: 'query_bert_batch', 'pos_bert_batch'; model: an IctEncTrain.  :return: loss_val; a scalar on the GPU."""
        from . import torch_ops  # noqa: F401  (registers the operators)
        q_reps = model(batch_rank['query_bert_batch'])
        c_reps = model.forward_context(batch_rank['pos_bert_batch'])
        loss, _row_lse = torch.ops.aspire.inbatch_xent(q_reps, c_reps)
        return loss.reshape(())
