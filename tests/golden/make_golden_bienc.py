"""Generate tests/golden/bienc_prep.json by RUNNING THE REFERENCE'S OWN CODE: the bi-encoder's batch preparation.

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_bienc.py
The fixture is data (inputs + expected outputs); no reference source is copied.

What executes from the reference:
  src/learning/batchers.py   SentTripleBatcher.prepare_bert_sentences (:209-254), AbsTripleBatcher.prepare_abstracts (:303-321)
and, restated here as the one line it is, the evaluate route of TrainedAbstractModel.encode (src/evaluation/utils/models.py:557-563):
TITLE + ' [SEP] ' + ' '.join(ABSTRACT) into prepare_bert_sentences.
The tokenizer is make_golden.py's: a BertTokenizer over a tiny local vocab, with its build_inputs_with_special_tokens adapter.
"""
import importlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference on sys.path, stubs geomloss)

batchers = importlib.import_module('src.learning.batchers')


def make_bienc_prep():
    rng = np.random.RandomState(11)
    words = [w for w in mg.VOCAB[5:] if not w.startswith('##')]

    def sent(n):
        return ' '.join(rng.choice(words, size=n)) + ' .'

    docs = [
        {'TITLE': 'optimal transport for document similarity', 'ABSTRACT': [sent(6), sent(9), sent(4)]},
        {'TITLE': 'graph neural networks', 'ABSTRACT': [sent(3)]},
        # over 500 word pieces in one sequence: cut at 500 before [CLS] / [SEP]
        {'TITLE': 'a model', 'ABSTRACT': [sent(150), sent(200), sent(180)]},
        # a literal [SEP] inside the title and a sentence: removed by prepare_abstracts, kept by the evaluate route
        {'TITLE': 'learning [SEP] to rank', 'ABSTRACT': [sent(5) + ' [SEP] ' + sent(3), sent(7)]},
        {'TITLE': 'x y', 'ABSTRACT': []},
    ]
    with tempfile.TemporaryDirectory() as td:
        tok = mg.make_tokenizer(td)
        cases = []
        for group in ([0, 1], [2], [3], [0, 1, 2, 3, 4]):
            batch = [docs[i] for i in group]
            abs_bb = batchers.AbsTripleBatcher.prepare_abstracts(batch_abs=batch, pt_lm_tokenizer=tok)
            eval_bb, _, _ = batchers.SentTripleBatcher.prepare_bert_sentences(
                sents=[p['TITLE'] + ' [SEP] ' + ' '.join(p['ABSTRACT']) for p in batch], tokenizer=tok)
            seqs = [sent(n) for n in (3, 520, 1)] if group == [2] else [docs[i]['TITLE'] for i in group]
            sent_bb, text, _ = batchers.SentTripleBatcher.prepare_bert_sentences(sents=seqs, tokenizer=tok)
            case = {'doc_ids': group, 'seqs': seqs, 'seqs_text': text}
            for name, bb in (('abs', abs_bb), ('eval', eval_bb), ('sents', sent_bb)):
                case[name] = {k: bb[k].tolist() for k in ('tokid_tt', 'seg_tt', 'attnmask_tt')}
                case[name]['seq_lens'] = bb['seq_lens']
            cases.append(case)
    with open(os.path.join(HERE, 'bienc_prep.json'), 'w') as f:
        json.dump({'vocab': mg.VOCAB, 'docs': docs, 'cases': cases}, f)
    for c in cases:
        print('bienc prep case', c['doc_ids'], 'abs', c['abs']['seq_lens'], 'eval', c['eval']['seq_lens'], 'sents', c['sents']['seq_lens'])


if __name__ == '__main__':
    make_bienc_prep()
