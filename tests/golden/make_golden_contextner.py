"""Generate contextner.json / contextner.npz by RUNNING THE REFERENCE'S OWN CODE (the contextual-entity model).

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_contextner.py
The fixtures are data (inputs + expected outputs); no reference source is copied.

What executes from the reference (src/evaluation/utils/models.py):
  AspireContextNER._preprocess_input / _get_ner_token_idxs / find_sublist_range (:641-697), encode (:620-639),
  get_faceted_encoding (:708-734) and the base SimilarityModel.get_faceted_encoding (:127-163),
  AspireConSenContextual.forward / _get_sent_reps / _get_ner_reps (:413-508), AspireNER._append_entities (:224-233).

models.py imports h5py and sentence_transformers at module scope; neither is used by these classes and neither is in the build
container, so empty stand-in modules are registered for the import (geomloss: make_golden.py's stand-in).  The classes' __init__
(which download a checkpoint) are bypassed; the BERT forward is a module that returns a seeded hidden state.
The tokenizer is make_golden.py's: a BertTokenizer over a tiny local vocab.
"""
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference on sys.path, stubs geomloss)

for _name in ('h5py', 'sentence_transformers'):
    try:
        importlib.import_module(_name)
    except ImportError:
        sys.modules[_name] = types.ModuleType(_name)
if not hasattr(sys.modules['sentence_transformers'], 'SentenceTransformer'):
    sys.modules['sentence_transformers'].SentenceTransformer = None
    sys.modules['sentence_transformers'].models = types.ModuleType('sentence_transformers.models')
# the reference's src/pre_process/utils.py imports its neighbour data_utils by bare name
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(importlib.import_module('src').__path__[0])), 'src', 'pre_process'))
ref = importlib.import_module('src.evaluation.utils.models')

FACETS = ('background', 'method', 'result')


def make_docs():
    rng = np.random.RandomState(23)
    words = [w for w in mg.VOCAB[5:] if not w.startswith('##') and w not in ('x', 'y', 'z', 'science', 'bio')]

    def sent(n, early=None, late=None):
        w = list(rng.choice(words, size=n))
        if early:
            w[2:2] = early.split()
        if late:
            w[-2:-2] = late.split()
        return ' '.join(w) + ' .'

    return [
        # 0: two overlapping entities; an entity found twice (first match); a two-piece word; a VALID entity after an INVALID one
        {'TITLE': 'optimal transport',
         'ABSTRACT': ['we propose a graph neural network model .', 'the model is trained on the text data .',
                      'result show that the method is similar .'],
         'ENTITIES': [['graph neural network', 'neural network model'], ['the', 'trained'], ['optimal transport', 'method']],
         'FACETS': ['background_label', 'method_label', 'result_label']},
        # 1: no entities
        {'TITLE': 'graph learning', 'ABSTRACT': ['we learn a graph .', 'the result is a score .'], 'ENTITIES': [[], []],
         'FACETS': ['objective_label', 'method_label']},
        # 2: every entity invalid (its word pieces are not in its sentence)
        {'TITLE': 'text alignment', 'ABSTRACT': ['we align text with a model .', 'the score is similar .'],
         'ENTITIES': [['science'], ['bio', 'graph network']], 'FACETS': ['background_label', 'result_label']},
        # 3: every entity valid, an 'objective_label', a sentence without entities
        {'TITLE': 'document similarity', 'ABSTRACT': ['we rank a candidate document for a query .', 'the method is optimal transport .',
                                                      'we show that .', 'result on the data set show the alignment score .'],
         'ENTITIES': [['candidate document', 'query'], ['optimal transport'], [], ['data set', 'alignment score', 'result']],
         'FACETS': ['objective_label', 'method_label', 'method_label', 'result_label']},
        # 4: the 500-piece cap cuts sentence 4 in the middle: 'x y' sits in the kept part, 'z x' only in the cut part; sentence 5 is
        # dropped entirely (its entity gets no entry)
        {'TITLE': 'a model', 'ABSTRACT': [sent(100, early='x y'), sent(120), sent(130), sent(90), sent(120, early='y x', late='z x'),
                                          sent(50, early='x z')],
         'ENTITIES': [['x y'], [], [], [], ['y x', 'z x'], ['x z']],
         'FACETS': ['background_label', 'background_label', 'method_label', 'method_label', 'result_label', 'result_label']},
        # 5: the cap falls exactly between sentences: sentences 2, 3 are dropped with their entities, every kept entity is valid
        {'TITLE': 'x y', 'ABSTRACT': [sent(247, early='z z'), sent(248), sent(30, early='y y'), sent(5)],
         'ENTITIES': [['z z'], [], ['y y'], []],
         'FACETS': ['background_label', 'method_label', 'result_label', 'result_label']},
    ]


class _Out:
    pass


class _FakeBert(torch.nn.Module):
    def __init__(self, hidden):
        super().__init__()
        self.hidden = hidden

    def forward(self, tokid_tt, token_type_ids=None, attention_mask=None):
        out = _Out()
        out.last_hidden_state = self.hidden
        return out


def _models(tok, hidden=None):
    inner = ref.AspireConSenContextual.__new__(ref.AspireConSenContextual)
    torch.nn.Module.__init__(inner)
    inner.bert_encoding_dim = 768
    inner.bert_encoder = _FakeBert(hidden)
    model = ref.AspireContextNER.__new__(ref.AspireContextNER)
    model.name, model.encoding_type, model.cache = 'aspire_context_ner_compsci', 'sentence-entity', None
    model.model, model.tokenizer = inner, tok
    return model, inner


def _faceted(fn, n_rows, doc):
    out = {}
    for facet in FACETS:
        try:
            out[facet] = np.asarray(fn(np.arange(n_rows)[:, None], facet, doc))[:, 0].tolist()
        except IndexError:
            out[facet] = 'IndexError'
    return out


def main():
    docs = make_docs()
    small = [0, 1, 2, 3]
    with tempfile.TemporaryDirectory() as td:
        tok = mg.make_tokenizer(td)
        model, _ = _models(tok)
        cases = []
        for group in (small, [4], [5], [3, 4, 0]):
            batch = [docs[i] for i in group]
            bert_batch, abs_lens, sent_token_idxs, ner_token_idxs = model._preprocess_input(batch)
            cases.append({'doc_ids': group, 'tokid_tt': bert_batch['tokid_tt'].tolist(), 'seg_tt': bert_batch['seg_tt'].tolist(),
                          'attnmask_tt': bert_batch['attnmask_tt'].tolist(), 'seq_lens': bert_batch['seq_lens'],
                          'abs_lens': abs_lens, 'sent_token_idxs': sent_token_idxs, 'ner_token_idxs': ner_token_idxs})
            print('case', group, 'seq_lens', bert_batch['seq_lens'], 'abs_lens', abs_lens, 'ner', ner_token_idxs)
        # the facet filters: AspireContextNER's override (valid entities only) and the base one (AspireNER: every entity a row)
        ner_model = ref.AspireNER.__new__(ref.AspireNER)
        ner_model.name, ner_model.encoding_type, ner_model.cache = 'aspire_ner_compsci', 'sentence-entity', None
        facets, facets_ner = [], []
        for doc in docs:
            _, abs_lens, _, ner_idxs = model._preprocess_input([doc])
            n_rows = abs_lens[0] + sum(len(x) > 0 for x in ner_idxs[0])
            facets.append({'n_rows': n_rows, 'rows': _faceted(model.get_faceted_encoding, n_rows, doc)})
            n_rows = len(doc['ABSTRACT']) + sum(len(x) for x in doc['ENTITIES'])
            facets_ner.append({'n_rows': n_rows, 'rows': _faceted(ner_model.get_faceted_encoding, n_rows, doc)})
            print('facets', facets[-1], facets_ner[-1])
        appended = ref.AspireNER._append_entities(ner_model, docs)
        # a seeded hidden state through the reference's pooling and encode
        batch = [docs[i] for i in small]
        bert_batch, abs_lens, sent_token_idxs, ner_token_idxs = model._preprocess_input(batch)
        L = max(bert_batch['seq_lens'])
        assert L <= 40, L
        hidden = torch.randn(len(batch), L, 768, generator=torch.Generator().manual_seed(5))
        model, inner = _models(tok, hidden)
        with torch.no_grad():
            sent_reps = inner._get_sent_reps(hidden, sent_token_idxs, len(batch), max(abs_lens), L)
            ner_reps = inner._get_ner_reps(hidden, ner_token_idxs)
            cls_reps, sent_reps2, _ = inner.consent_reps_bert(bert_batch, sent_token_idxs, ner_token_idxs, abs_lens)
            encoded = model.encode(batch)
        assert torch.equal(sent_reps, sent_reps2)
        ner_rows = [r for paper in ner_reps for r in paper if len(r) > 0]
        np.savez(os.path.join(HERE, 'contextner.npz'), hidden=hidden.numpy(), cls_reps=cls_reps.numpy().astype(np.float32),
                 sent_reps=sent_reps.numpy().astype(np.float32),
                 ner_rows=torch.cat(ner_rows, 0).numpy().astype(np.float32),
                 ner_valid=np.array([len(r) > 0 for paper in ner_reps for r in paper]),
                 ner_per_paper=np.array([len(paper) for paper in ner_reps]),
                 encoded=torch.cat(encoded, 0).numpy().astype(np.float32), encoded_lens=np.array([len(e) for e in encoded]))
    with open(os.path.join(HERE, 'contextner.json'), 'w') as f:
        json.dump({'vocab': mg.VOCAB, 'docs': docs, 'cases': cases, 'facets': facets, 'facets_ner': facets_ner, 'appended': appended,
                   'hidden_doc_ids': small}, f)
    print('encoded lens', [len(e) for e in encoded], 'sent_reps', tuple(sent_reps.shape), sent_reps.dtype)


if __name__ == '__main__':
    main()
