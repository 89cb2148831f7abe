"""AspireSentEnc: the cosentbert / ictsentbert sentence encoder (``allenai/aspire-sentence-embedder``), drop-in for the test-time
surface of TrainedSentModel (src/evaluation/utils/models.py:568-604), SentBERTWrapper / ICTBERTWrapper
(src/learning/facetid_models/sentsim_models.py:13-110) and the SentenceTransformer they wrap.

    model = AspireSentEnc('allenai/scibert_scivocab_uncased')
    model.load_state_dict(torch.load('sent_encoder_cur_best.pt'))        # a plain BertModel state dict (models.py:579-580)
    reps = model.encode_papers(batch_papers)                               # per paper [n_sents, 768]
    sim = model.get_similarity(reps[0], reps[1])                           # max cosine over the sentence pairs

Every abstract sentence goes through SciBERT on its own; its rep is the CLS row of last_hidden_state (Pooling('cls')).  The
encoder is HipBertEncoder.forward_cls with no layer mix (AspireBiEnc's read-out), the score aspire_dotmax_scores_f32 /
aspire_dotmax_rank_batch_f32 (include/aspire_hip.h, A13).
"""
import numpy as np

from . import _lib, ops
from .batch_prep import batch_tensors, tokenize_sentences
from .model_front import EncoderFront, add_to_store, check_pid_count, encode_bucketed, load_hf, per_paper, refuse_keys, strip_prefix


def split_state_dict(sd):
    """A sentence-encoder state dict -> the BertModel's own state dict.  Two forms:
      * a plain BertModel state dict (what sent_encoder_cur_best.pt holds: models.py:579-580);
      * SentBERTWrapper / ICTBERTWrapper keys, ``sent_encoder.<BertModel key>``; ICTBERTWrapper's ``context_encoder.*`` (the
        context tower of its training loss) is dropped: the evaluation encodes with the sentence tower only.
    Any other key is a KeyError."""
    if any(k.startswith(('sent_encoder.', 'context_encoder.')) for k in sd):
        return strip_prefix(sd, 'sent_encoder.', drop=('context_encoder.',), who='sentence-encoder')[0]
    refuse_keys([k for k in sd if not k.startswith(('embeddings.', 'encoder.', 'pooler.'))], 'sentence-encoder')
    return dict(sd)


class AspireSentEnc(EncoderFront):
    def __init__(self, hf_model_name=None, bert_model=None, max_seq_length=512, tokenizer=None, matmul='fp32'):
        """
        :param hf_model_name: the HF model (and tokenizer) to load, e.g. 'allenai/aspire-sentence-embedder' or, as
            TrainedSentModel does before loading its checkpoint, 'allenai/scibert_scivocab_uncased'.
        :param bert_model: an already constructed transformers BertModel instead (weights are copied to the GPU).
        :param max_seq_length: models.Transformer(max_seq_length=512).
        :param tokenizer: the tokenizer encode() uses (default: AutoTokenizer.from_pretrained(hf_model_name)).
        :param matmul: the encoder's matmul mode, 'fp32' or the opt-in 'fp16' (HipBertEncoder).
        """
        self.bert_encoding_dim = 768
        self.max_seq_length = int(max_seq_length)
        bert_model, self.tokenizer = load_hf(hf_model_name, bert_model, tokenizer)
        self._build_encoder(bert_model, matmul)

    def load_state_dict(self, sd):
        """sent_encoder_cur_best.pt (a BertModel state dict) or a SentBERTWrapper / ICTBERTWrapper one (split_state_dict)."""
        self._rebuild_encoder(split_state_dict(sd))
        return self

    # ---- the forward ---------------------------------------------------------------------------------------------------
    def forward_device(self, tokid_tt, token_type_ids=None, attention_mask=None):
        """int64 [B, L] -> last_hidden_state[:, 0] [B, 768] on the GPU, under the encoder's fall-back rule (encoder.run_checked)."""
        enc = self.bert_encoder
        return self._checked_read(lambda tok, typ, msk: enc.forward_cls(tok, typ, msk, check_ids=False)[0], lambda out: out,
                                  tokid_tt, token_type_ids, attention_mask, 'AspireSentEnc')

    @staticmethod
    def sent_reps_bert(bert_batch, model=None):
        """SentBERTWrapper.sent_reps_bert (sentsim_models.py:62-78) on an HF or batcher dict: the CLS rows, ``.squeeze()``d
        ([B, 768]; [768] for one sentence).  The reference's bert_model argument is the encoder; here `model` (an AspireSentEnc)."""
        tok, typ, msk = batch_tensors(bert_batch)
        return model.forward_device(tok, typ, msk).squeeze()

    def encode(self, sentences, batch_size=32, show_progress_bar=False, convert_to_numpy=True, max_tokens=16384):
        """SentenceTransformer.encode with Transformer(max_seq_length) + Pooling('cls'): float32 [N, 768] in input order ([768]
        for one string).  What sentence-transformers does (recalled from its source; it is not a dependency here): every text
        .strip()ed, tokenizer(texts, padding=True, truncation='longest_first', max_length=max_seq_length), the CLS row of the
        last hidden state.  A sentence's rep does not depend on its batch mates (padding is masked), so instead of the reference's
        batches of `batch_size` sentences (accepted, not used) everything is tokenised once, sorted by token count and cut into
        encoder calls of at most `max_tokens` padded token rows (batch_prep.sentence_buckets): short sentences are padded to
        their neighbours' length only, and big calls reach the encoder's fused-LayerNorm GEMMs.  show_progress_bar is ignored.
        convert_to_numpy=False returns the [N, 768] GPU tensor."""
        single = isinstance(sentences, str)
        sents = [sentences] if single else list(sentences)
        dev = ops.require_gpu()
        ids, types, pad = [], [], None
        if sents:
            if self.tokenizer is None:
                raise ValueError('encode() needs a tokenizer: pass hf_model_name or tokenizer=')
            ids, types = tokenize_sentences(sents, self.tokenizer, self.max_seq_length)
            pad = self.tokenizer.pad_token_id
        out = encode_bucketed(self.forward_device, ids, types, pad, max_tokens, dev)
        if single:
            out = out[0]
        return out.cpu().numpy() if convert_to_numpy else out

    # ---- TrainedSentModel's surface -------------------------------------------------------------------------------------
    def encode_papers(self, batch_papers, **kw):
        """TrainedSentModel.encode (models.py:584-600): the ABSTRACT sentences of every paper, encoded, split back per paper with
        np.split semantics -> list of float32 [n_sents, 768]."""
        return per_paper(batch_papers, lambda batch: self.encode(batch, **kw))

    @staticmethod
    def get_similarity(x, y):
        """TrainedSentModel.get_similarity (models.py:602-604): float(np.max(cosine_similarity(x, y))) of one pair of
        [n, 768] / [m, 768] rep arrays (aspire_dotmax_scores_f32)."""
        x = np.atleast_2d(np.asarray(x, dtype=np.float32))
        y = np.atleast_2d(np.asarray(y, dtype=np.float32))
        q, c = ops.DeviceRepSet.from_list([x]), ops.DeviceRepSet.from_list([y])
        return float(ops.dotmax_scores(q, c, pairing=_lib.PAIR_PAIRED, sim=_lib.SIM_COSINE).item())

    # ---- corpus encoding ------------------------------------------------------------------------------------------------
    def encode_to_store(self, papers, pids, store=None, **kw):
        """Every paper's ABSTRACT sentences encoded (one encode call for the lot), one [n_sents, 768] row block per paper under
        pids[j] (pre_proc_buildreps.py:332-360 writes the same reps).  Returns the RepStore (new, or `store` with the reps added),
        ready for evaluate.score(..., method='cosine')."""
        papers, pids = list(papers), list(pids)
        check_pid_count(pids, len(papers))
        return add_to_store(store, pids, self.encode_papers(papers, **kw))
