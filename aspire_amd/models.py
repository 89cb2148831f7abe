"""get_model: the reference's model factory (src/evaluation/utils/models.py:738-768) over this project's classes.

    model = get_model('specter')                                        # downloads what the reference downloads
    model = get_model('supsimcse', bert_model=bm, tokenizer=tok)        # nothing is downloaded
    model = get_model('cospecter', trained_model_path='runs/cospecter')

MODEL_TABLE says which class stands for which of the reference's model names.
"""
import os

from .baselines import BertMLM, BertNER, SimCSE
from .bienc import AspireBiEnc
from .consent import AspireConSent
from .contextner import AspireContextNER, AspireNER
from .model_front import load_hf, ot_similarity, read_hparams, sentence_facet_rows
from .sentenc import AspireSentEnc

ASPIRE_MODEL_PATHS = {          # AspireModel.MODEL_PATHS, models.py:175-178
    'compsci': 'allenai/aspire-contextualsentence-multim-compsci',
    'biomed': 'allenai/aspire-contextualsentence-multim-biomed',
}


class AspireModel:
    """aspire_compsci / aspire_biomed (AspireModel, models.py:169-209): AspireConSent with its tokenizer, otAspire as the
    similarity, encoding_type 'sentence'."""
    encoding_type = 'sentence'

    def __init__(self, name='aspire_compsci', hf_model_name=None, bert_model=None, tokenizer=None, matmul='fp32'):
        self.name = name
        if hf_model_name is None and (bert_model is None or tokenizer is None):
            hf_model_name = ASPIRE_MODEL_PATHS[name.split('_')[-1]]
        bert_model, self.tokenizer = load_hf(hf_model_name, bert_model, tokenizer)
        self.model = AspireConSent(bert_model=bert_model, matmul=matmul)       # matmul: the encoder's mode, 'fp32' or the opt-in 'fp16'

    def encode(self, batch_papers):
        """:return: per paper [n_kept_sentences, 768]"""
        return self.model.encode(batch_papers, self.tokenizer)

    get_similarity = staticmethod(ot_similarity)
    get_faceted_encoding = staticmethod(sentence_facet_rows)


MODEL_TABLE = {
    'aspire_compsci': AspireModel, 'aspire_biomed': AspireModel,
    'specter': BertMLM,
    'supsimcse': SimCSE, 'unsupsimcse': SimCSE,
    'specter_ner': BertNER,
    'aspire_ner_compsci': AspireNER, 'aspire_ner_biomed': AspireNER,
    'aspire_context_ner_compsci': AspireContextNER, 'aspire_context_ner_biomed': AspireContextNER,
    'cospecter': AspireBiEnc,
    'cosentbert': AspireSentEnc, 'ictsentbert': AspireSentEnc,
}
SENTENCE_TRANSFORMER_NAMES = ('sbtinybertsota', 'sbrobertanli', 'sbmpnet1B')       # SentenceModel, models.py:379-410: aspire_amd/sbert.py


def _default_hf_name(kw, name):
    """hf_model_name for a class that loads nothing by itself, unless the caller brings the model (and, where used, the tokenizer)."""
    if 'hf_model_name' not in kw and kw.get('bert_model') is None:
        kw['hf_model_name'] = name
    return kw


def get_model(model_name, trained_model_path=None, **kw):
    """The reference's get_model (models.py:738-768).  **kw goes to the class's constructor (bert_model=, tokenizer=: nothing is
    downloaded when both are given; matmul='fp16': the encoder's opt-in fp16 matmul mode, HipBertEncoder).  trained_model_path: the run directory of 'cospecter' (run_info.json + model_cur_best.pt,
    models.py:522-555) or of 'cosentbert' / 'ictsentbert' (sent_encoder_cur_best.pt, models.py:573-582)."""
    if model_name in SENTENCE_TRANSFORMER_NAMES:
        raise NotImplementedError(f'{model_name}: the SentenceTransformer baselines (TinyBERT / RoBERTa / MPNet encoders) are not built '
                                  f'into get_model: construct aspire_amd.SentenceModel({model_name!r}, model=..., tokenizer=...)')
    if model_name not in MODEL_TABLE:
        raise NotImplementedError(f"No Implementation for model {model_name}")
    cls = MODEL_TABLE[model_name]
    if cls in (AspireModel, BertMLM, SimCSE, BertNER):
        return cls(name=model_name, **kw)
    if cls in (AspireNER, AspireContextNER):
        # (the reference's AspireContextNER loads the compsci model for both names, models.py:615)
        field = 'compsci' if cls is AspireContextNER else model_name.split('_')[-1]
        return cls(name=model_name, **_default_hf_name(kw, ASPIRE_MODEL_PATHS[field]))
    import torch
    if cls is AspireBiEnc:
        tokenizer = kw.pop('tokenizer', None)
        if trained_model_path is not None:
            kw.setdefault('model_hparams', read_hparams(trained_model_path))
        model = cls(**kw)
        if trained_model_path is not None:
            model.load_state_dict(torch.load(os.path.join(trained_model_path, 'model_cur_best.pt'), map_location='cpu'))
        if tokenizer is None and kw.get('model_hparams'):
            tokenizer = load_hf(kw['model_hparams']['base-pt-layer'], model=model)[1]       # (the model is built: the tokenizer only)
        model.tokenizer = tokenizer         # TrainedAbstractModel.tokenizer (models.py:555): prepare_eval_seqs' second argument
        return model
    model = cls(**_default_hf_name(kw, 'allenai/scibert_scivocab_uncased'))
    if trained_model_path is not None:
        model.load_state_dict(torch.load(os.path.join(trained_model_path, 'sent_encoder_cur_best.pt'), map_location='cpu'))
    return model
