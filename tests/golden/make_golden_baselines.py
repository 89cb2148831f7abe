"""Generate tests/golden/baselines_prep.json by RUNNING THE REFERENCE'S OWN CODE: the inputs of the SPECTER / SimCSE baselines.

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_baselines.py
The fixture is data (inputs + expected outputs); no reference source is copied.

What executes from the reference (src/evaluation/utils/models.py):
  BertMLM._prepare_batch (:259-293), BertMLM._pre_process_input_batch (:295-298), BertNER._pre_process_input_batch (:368-376),
  and SimCSE.encode (:326-357) up to its model call: the model is a stand-in that records the tensors it is given and returns
  zeros, so the sentence list, its _prepare_batch output and the np.split sizes are the reference's.
The classes' __init__ (which download a checkpoint) are bypassed; models.py's module-scope imports of h5py and
sentence_transformers get make_golden_contextner.py's empty stand-ins.  The tokenizer is make_golden.py's: a BertTokenizer over a
tiny local vocab (the vocabulary of bienc_prep.json), with its build_inputs_with_special_tokens adapter.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference on sys.path, stubs geomloss)
import make_golden_contextner as mgc  # noqa: E402  (imports the reference's models.py behind its stand-in modules)

ref = mgc.ref


def make_papers():
    rng = np.random.RandomState(31)
    words = [w for w in mg.VOCAB[5:] if not w.startswith('##')]

    def sent(n):
        return ' '.join(rng.choice(words, size=n)) + ' .'

    return [
        # 0: entities in some sentences only
        {'TITLE': 'optimal transport for document similarity', 'ABSTRACT': [sent(6), sent(9), sent(4)],
         'ENTITIES': [['optimal transport', 'graph'], [], ['neural network model']]},
        # 1: over 500 word pieces: cut at 500 before [CLS] / [SEP] (the appended entities fall behind the cut)
        {'TITLE': 'a model', 'ABSTRACT': [sent(150), sent(200), sent(180)], 'ENTITIES': [['data set'], [], ['score']]},
        # 2: no entity list at all / 3: an empty list per sentence: both still get the trailing ' .'
        {'TITLE': 'graph neural networks', 'ABSTRACT': [sent(3)], 'ENTITIES': []},
        {'TITLE': 'text alignment', 'ABSTRACT': [sent(5), sent(2)], 'ENTITIES': [[], []]},
        # 4: no sentences
        {'TITLE': 'x y', 'ABSTRACT': [], 'ENTITIES': []},
    ]


def _stub(cls, tok):
    m = cls.__new__(cls)
    m.tokenizer = tok
    m.bert_max_seq_len = 500
    return m


def _batch(tokid_tt, seg_tt, attnmask_tt, seq_lens_tt):
    return {'tokid_tt': tokid_tt.tolist(), 'seg_tt': seg_tt.tolist(), 'attnmask_tt': attnmask_tt.tolist(),
            'seq_lens': [int(x) for x in seq_lens_tt.tolist()]}


def make_baselines_prep():
    papers = make_papers()
    cases = []
    with tempfile.TemporaryDirectory() as td:
        tok = mg.make_tokenizer(td)
        for group in ([0, 2], [1], [0, 1, 2, 3, 4]):
            batch = [papers[i] for i in group]
            case = {'doc_ids': group}
            for key, cls in (('specter', ref.BertMLM), ('specter_ner', ref.BertNER)):
                m = _stub(cls, tok)
                texts = m._pre_process_input_batch(batch)
                case[key] = dict(_batch(*m._prepare_batch(texts)), texts=texts)
            cases.append(case)
        # SimCSE: a 3-paper batch (sentence counts 3, 0, 2) through the reference's encode
        seen = {}

        def model(tokid_tt, token_type_ids=None, attention_mask=None):
            seen['bb'] = (tokid_tt, token_type_ids, attention_mask)
            return types.SimpleNamespace(pooler_output=np.zeros((tokid_tt.shape[0], 4), np.float32))

        m = _stub(ref.SimCSE, tok)
        m.model = model
        group = [0, 4, 3]
        reps = m.encode([papers[i] for i in group])
        tokid, seg, att = seen['bb']
        simcse = {'doc_ids': group, 'split_sizes': [int(r.shape[0]) for r in reps],
                  'tokid_tt': tokid.tolist(), 'seg_tt': seg.tolist(), 'attnmask_tt': att.tolist()}
    with open(os.path.join(HERE, 'baselines_prep.json'), 'w') as f:
        json.dump({'vocab': mg.VOCAB, 'papers': papers, 'cases': cases, 'simcse': simcse}, f)
    for c in cases:
        print('baselines prep case', c['doc_ids'], 'specter', c['specter']['seq_lens'], 'specter_ner', c['specter_ner']['seq_lens'])
    print('simcse', simcse['doc_ids'], simcse['split_sizes'], [sum(r) for r in simcse['attnmask_tt']])


if __name__ == '__main__':
    make_baselines_prep()
