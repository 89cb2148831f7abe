"""SentenceModel: the SentenceTransformer baselines of the reference's evaluate.py, drop-in for the class of the same name in
src/evaluation/utils/models.py:379-410 ('sbtinybertsota', 'sbrobertanli', 'sbmpnet1B').

    model = SentenceModel('sbmpnet1B')                                   # downloads what the reference downloads
    model = SentenceModel('sbrobertanli', model=RobertaModel(...), tokenizer=tok)     # nothing is downloaded
    reps = model.encode(batch_papers)                                     # per paper [n_sents, 768]
    sim = model.get_similarity(reps[0], reps[1])                          # max cosine over the sentence pairs

sentence-transformers is not a dependency: what ``SentenceTransformer(name).encode(sentences)`` does for these three models is
restated over the ``transformers`` model it wraps -- tokenise, run the transformer, mean of the token rows under the attention mask
(Pooling), for all-mpnet-base-v2 also an L2 normalisation (Normalize).  All three transformers have BERT-base geometry; the encoder
is HipBertEncoder (BertModel for TinyBERT, RobertaModel, MPNetModel: aspire_bert_forward_var_f32) and the read-out its forward_mean
(aspire_token_mean_pool_f32).  Ranking a pool: encode_to_store, then evaluate.score(..., method='cosine').
"""
import json
import os

import numpy as np

from .model_front import EncoderFront, add_to_store, check_pid_count, encode_bucketed, load_hf, per_paper, sentence_facet_rows


def _read_json(path):
    with open(path, 'r', encoding='utf-8') as fp:
        return json.load(fp)


class SentenceModel(EncoderFront):
    """'sbtinybertsota' / 'sbrobertanli' / 'sbmpnet1B' (models.py:379-410).

    max_seq_length and normalize default per name to DEFAULTS below.  Those values are RECALLED from the models' published
    sentence_bert_config.json (max_seq_length) and modules.json (a Normalize module behind the Pooling) and could not be checked
    against the files where this was written; when hf_model_name is a local directory that has those files, both are read from
    them instead.  An explicit argument wins over either."""
    MODEL_PATHS = {
        'sbtinybertsota': 'paraphrase-TinyBERT-L6-v2',
        'sbrobertanli': 'nli-roberta-base-v2',
        'sbmpnet1B': 'sentence-transformers/all-mpnet-base-v2',
    }
    DEFAULTS = {            # name -> (max_seq_length, normalize): recalled, see the class docstring
        'sbtinybertsota': (128, False),
        'sbrobertanli': (75, False),
        'sbmpnet1B': (384, True),
    }
    encoding_type = 'sentence'

    def __init__(self, name, hf_model_name=None, model=None, tokenizer=None, max_seq_length=None, normalize=None, matmul='fp32'):
        """
        :param name: a key of MODEL_PATHS: the model the reference hands to SentenceTransformer.
        :param hf_model_name: another HF name or a local directory to load instead.
        :param model: an already constructed transformers BertModel / RobertaModel / MPNetModel instead (weights are copied to
            the GPU).
        :param tokenizer: default AutoTokenizer.from_pretrained(the model's name).
        :param max_seq_length: tokens per sentence, special tokens included (models.Transformer(max_seq_length)).
        :param normalize: L2-normalise the reps (a Normalize module in the model's modules.json).
        :param matmul: the encoder's matmul mode, 'fp32' or the opt-in 'fp16' (HipBertEncoder).
        """
        self.name = name
        full_name = hf_model_name if hf_model_name is not None else self.hub_name(name)
        seq_default, norm_default = self.DEFAULTS.get(name, (None, None))
        if hf_model_name is not None and os.path.isdir(hf_model_name):
            seq_file, norm_file = self.read_local_settings(hf_model_name)
            seq_default = seq_file if seq_file is not None else seq_default
            norm_default = norm_file if norm_file is not None else norm_default
        model, self.tokenizer = load_hf(full_name, model, tokenizer)
        self.max_seq_length = int(max_seq_length if max_seq_length is not None else seq_default or 512)
        self.normalize = bool(normalize if normalize is not None else norm_default)
        self._build_encoder(model, matmul)

    @classmethod
    def hub_name(cls, name):
        """What AutoModel loads for MODEL_PATHS[name]: SentenceTransformer resolves a name without '/' under sentence-transformers/."""
        path = cls.MODEL_PATHS[name]
        return path if '/' in path else 'sentence-transformers/' + path

    @staticmethod
    def read_local_settings(directory):
        """(max_seq_length, normalize) of a sentence-transformers model directory: sentence_bert_config.json's max_seq_length and
        whether modules.json lists a Normalize module; None for whichever file is missing."""
        seq = norm = None
        p = os.path.join(directory, 'sentence_bert_config.json')
        if os.path.exists(p):
            seq = _read_json(p).get('max_seq_length')
        p = os.path.join(directory, 'modules.json')
        if os.path.exists(p):
            norm = any(str(m.get('type', '')).endswith('Normalize') for m in _read_json(p))
        return seq, norm

    def _mean_checked(self, tokid_tt, token_type_ids, attention_mask):
        """int64 [B, L] -> the sentence reps [B, 768] on the GPU, under the encoder's fall-back rule (encoder.run_checked)."""
        enc = self.bert_encoder
        return self._checked_read(lambda tok, typ, msk: enc.forward_mean(tok, typ, msk, normalize=self.normalize, check_ids=False),
                                  lambda out: out, tokid_tt, token_type_ids, attention_mask, 'SentenceModel')

    def _encode_sentences(self, sents, max_tokens=16384):
        """The rep of every string, float32 [N, 768] (numpy) in input order: SentenceTransformer.encode's text.strip() and
        tokenizer(text, truncation=True, max_length=max_seq_length), which puts in the tokenizer's own special tokens.  A sentence's
        rep does not depend on its batch mates (padding is masked out of the attention and of the mean), so instead of batches of 32
        in input order everything is tokenised once, sorted by length and cut into encoder calls of at most `max_tokens` padded
        token rows (batch_prep.sentence_buckets), padded with the tokenizer's pad id."""
        ids = [list(self.tokenizer(str(s).strip(), truncation=True, max_length=self.max_seq_length)['input_ids']) for s in sents]
        types = [[0] * len(x) for x in ids]
        return encode_bucketed(self._mean_checked, ids, types, self.tokenizer.pad_token_id, max_tokens,
                               self.bert_encoder.device).cpu().numpy()

    def encode(self, batch_papers):
        """SentenceModel.encode (models.py:392-406): the ABSTRACT sentences of all papers encoded, split back per paper with
        np.split semantics -> list of float32 [n_sents, 768] (a paper without sentences: [0, 768])."""
        return per_paper(batch_papers, self._encode_sentences)

    @staticmethod
    def get_similarity(x, y):
        """SentenceModel.get_similarity (models.py:408-410): float(np.max(sklearn's cosine_similarity(x, y))) of one pair of
        [n, 768] / [m, 768] rep arrays, computed as sklearn does (rows over their norm, a zero norm taken as 1, then the products).
        One pair on the host, as in the reference; pools are ranked by evaluate.score(..., method='cosine') on the GPU."""
        def unit(a):
            a = np.atleast_2d(np.asarray(a))
            nrm = np.sqrt(np.einsum('ij,ij->i', a, a))
            nrm[nrm == 0.0] = 1.0
            return a / nrm[:, None]
        return float(np.max(unit(x) @ unit(y).T))

    get_faceted_encoding = staticmethod(sentence_facet_rows)

    def encode_to_store(self, papers, pids, store=None):
        """Every paper's ABSTRACT sentences encoded (one encode call for the lot), one [n_sents, 768] row block per paper under
        pids[j].  Returns the RepStore (new, or `store` with the reps added), ready for evaluate.score(..., method='cosine')."""
        papers, pids = list(papers), list(pids)
        check_pid_count(pids, len(papers))
        return add_to_store(store, pids, self.encode(papers))
