"""The whole-abstract and sentence baselines of the reference's evaluate.py, drop-ins for the classes of the same names in
src/evaluation/utils/models.py:

    BertMLM   'specter'                    (:237-320)  last_hidden_state[:, 0] of TITLE + ' [SEP] ' + abstract, ranked by -euclidean
    BertNER   'specter_ner'                (:359-376)  the same model, the entity strings appended to the text
    SimCSE    'supsimcse' / 'unsupsimcse'  (:322-357)  every abstract sentence on its own, the rep is pooler_output

    model = BertMLM(name='specter')                       # or bert_model=BertModel(...), tokenizer=...: nothing is downloaded
    reps = model.encode(batch_papers)                     # [B, 768]
    sim = model.get_similarity(reps[0], reps[1])

All three are BERT-base models: the encoder is HipBertEncoder.forward_cls with no layer mix (the bi-encoders' read-out), SimCSE's
pooler aspire_bert_pooler_f32 behind it (HipBertEncoder.forward_pooled).  Ranking a pool: encode_to_store, then
evaluate.score(..., method='l2max') for BertMLM / BertNER and method='cosine' for SimCSE (see the classes).
"""
import numpy as np
import torch

from .batch_prep import MAX_NUM_TOKS, _with_special_tokens, _word_pieces, prepare_eval_ner_seqs, prepare_eval_seqs
from .model_front import EncoderFront, add_to_store, check_pid_count, encode_bucketed, load_hf, per_paper


def neg_euclidean(x, y):
    """-scipy.spatial.distance.euclidean(x, y) (models.py:319-320) of two [768] vectors, as a Python float; like scipy, anything
    that is not 1-D is a ValueError."""
    x, y = np.asarray(x), np.asarray(y)
    if x.ndim != 1 or y.ndim != 1:
        raise ValueError('Input vector should be 1-D.')
    return -float(np.linalg.norm(x - y))


class BertMLM(EncoderFront):
    """'specter' (models.py:237-320)."""
    MODEL_PATHS = {
        'specter': 'allenai/specter',
        'supsimcse': 'princeton-nlp/sup-simcse-bert-base-uncased',
        'unsupsimcse': 'princeton-nlp/unsup-simcse-bert-base-uncased',
    }
    encoding_type = 'abstract'

    def __init__(self, name='specter', hf_model_name=None, bert_model=None, tokenizer=None, matmul='fp32'):
        """
        :param name: a key of MODEL_PATHS: the HF model (and tokenizer) the reference loads for it.
        :param hf_model_name: another HF name or path to load instead of MODEL_PATHS[name].
        :param bert_model: an already constructed transformers BertModel instead (weights are copied to the GPU).
        :param tokenizer: default AutoTokenizer.from_pretrained(the model's name).
        :param matmul: the encoder's matmul mode, 'fp32' or the opt-in 'fp16' (HipBertEncoder).
        """
        self.name = name
        self.bert_max_seq_len = MAX_NUM_TOKS
        if hf_model_name is None and (bert_model is None or tokenizer is None):
            hf_model_name = self.MODEL_PATHS[name]
        bert_model, self.tokenizer = load_hf(hf_model_name, bert_model, tokenizer)
        self._build_encoder(bert_model, matmul)

    def _bert_batch(self, batch_papers):
        """_pre_process_input_batch + _prepare_batch (models.py:259-298)."""
        return prepare_eval_seqs(batch_papers, self.tokenizer)

    def encode(self, batch_papers):
        """BertMLM.encode (models.py:300-317): last_hidden_state[:, 0] of every paper's sequence, float32 [B, 768] on the CPU."""
        if not batch_papers:
            return torch.zeros(0, 768)
        bb = self._bert_batch(batch_papers)
        enc = self.bert_encoder
        return self._checked_read(lambda tok, typ, msk: enc.forward_cls(tok, typ, msk, check_ids=False)[0], lambda out: out,
                                  bb['tokid_tt'], bb['seg_tt'], bb['attnmask_tt']).cpu()

    @staticmethod
    def get_similarity(x, y):
        """BertMLM.get_similarity (models.py:319-320): -euclidean of two [768] reps."""
        return neg_euclidean(x, y)

    @staticmethod
    def get_faceted_encoding(unfaceted_encoding, facet=None, input_data=None):
        """SimilarityModel.get_faceted_encoding for encoding_type 'abstract' (models.py:141-143): one rep per abstract, no filter."""
        return unfaceted_encoding

    def encode_to_store(self, papers, pids, store=None, batch_size=8):
        """Every paper encoded (`batch_size` at a time: SimilarityModel's batch_size, models.py:34) into one [1, 768] block under
        pids[j].  Returns the RepStore (new, or `store` with the reps added): evaluate.score(..., method='l2max') then ranks a pool
        by -cdist of the 1 x 1 pair = -euclidean, this class's get_similarity (the route AspireBiEnc.encode_to_store documents)."""
        papers, pids = list(papers), list(pids)
        check_pid_count(pids, len(papers))

        def blocks():
            for lo in range(0, len(papers), batch_size):
                reps = self.encode(papers[lo:lo + batch_size]).numpy()
                for i in range(reps.shape[0]):
                    yield reps[i:i + 1]
        return add_to_store(store, pids, blocks())


class BertNER(BertMLM):
    """'specter_ner' (models.py:359-376): SPECTER on the text with the paper's entity strings appended."""

    def __init__(self, name='specter_ner', **kwargs):
        super().__init__(name=name.split('_ner')[0], **kwargs)
        self.name = name

    def _bert_batch(self, batch_papers):
        return prepare_eval_ner_seqs(batch_papers, self.tokenizer)


class SimCSE(BertMLM):
    """'supsimcse' / 'unsupsimcse' (models.py:322-357): per paper the pooler_output of every ABSTRACT sentence.

    The reference registers these models with encoding_type 'abstract' (models.py:749-750) and lets them inherit BertMLM's
    get_similarity, which cannot score two papers of more than one sentence; what it ranks them by is another route:
    pre_proc_buildreps.py:105-127, 390-398 (write_wholeabs_reps) writes the same reps as sentence reps and pp_gen_nearest.py's
    rank_pool_sent scores them with 'cosine', the max cosine over the sentence pairs.  Here: encode_to_store, then
    evaluate.score(..., method='cosine') / scorer.rank_pools(..., method='cosine')."""

    def __init__(self, name='supsimcse', **kwargs):
        super().__init__(name=name, **kwargs)

    def _pooled_checked(self, tokid_tt, token_type_ids, attention_mask):
        """int64 [B, L] -> pooler_output [B, 768] on the GPU, under the encoder's fall-back rule (encoder.run_checked) -- which
        judges the CLS rows: tanh maps an overflowed activation to +-1, the pooled rows of a broken forward can all be finite."""
        enc = self.bert_encoder
        return self._checked_read(lambda tok, typ, msk: enc.forward_pooled(tok, typ, msk, check_ids=False), lambda r: r[0],
                                  tokid_tt, token_type_ids, attention_mask, 'SimCSE')[1]

    def _encode_sentences(self, sents, max_tokens=16384):
        """pooler_output of every string, float32 [N, 768] (numpy) in input order.  _prepare_batch's tokenisation (models.py:259-293:
        the first 500 word pieces, [CLS] ids [SEP]); a sentence's rep does not depend on its batch mates (padding is masked: BERT
        vocabularies pad with id 0), so instead of one batch of all sentences padded to the longest, everything is tokenised once,
        sorted by length and cut into encoder calls of at most `max_tokens` padded token rows (batch_prep.sentence_buckets), as
        AspireSentEnc.encode does."""
        ids = [_with_special_tokens(self.tokenizer, piece_ids[:self.bert_max_seq_len])
               for _, piece_ids in _word_pieces(self.tokenizer, list(sents), want_text=False)]
        types = [[0] * len(x) for x in ids]
        return encode_bucketed(self._pooled_checked, ids, types, self.tokenizer.pad_token_id, max_tokens,
                               self.bert_encoder.device).cpu().numpy()

    def encode(self, batch_papers):
        """SimCSE.encode (models.py:326-357): the ABSTRACT sentences of all papers encoded, split back per paper with np.split
        semantics -> list of float32 [n_sents, 768] (a paper without sentences: [0, 768])."""
        return per_paper(batch_papers, self._encode_sentences)

    @staticmethod
    def get_similarity(x, y):
        """The reference's behaviour, which is BertMLM's -euclidean (models.py:319-320) on what encode returns: two one-row reps
        ([1, 768], which scipy 1.6 -- the reference's pin -- squeezes to vectors) give minus their distance; anything else raises
        ValueError, as scipy does on 2-D input.  Papers are ranked by the max-cosine route of the class docstring instead."""
        x, y = np.asarray(x), np.asarray(y)
        if x.ndim == 2 and y.ndim == 2 and x.shape[0] == 1 and y.shape[0] == 1:
            x, y = x[0], y[0]
        return neg_euclidean(x, y)

    def encode_to_store(self, papers, pids, store=None):
        """Every paper's ABSTRACT sentences encoded (one encode call for the lot), one [n_sents, 768] row block per paper under
        pids[j] (what write_wholeabs_reps stores).  Returns the RepStore (new, or `store` with the reps added), ready for
        evaluate.score(..., method='cosine')."""
        papers, pids = list(papers), list(pids)
        check_pid_count(pids, len(papers))
        return add_to_store(store, pids, self.encode(papers))
