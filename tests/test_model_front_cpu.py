"""CPU side of aspire_amd/model_front.py, the code the model classes share, around stub encoders and tokenizers (the style of
tests/test_sbert_cpu.py): the bucketed encode, the per-paper split, the store fill, checkpoint keys, the facet filter, the checked
read-out and the pool layout."""
import json

import numpy as np
import pytest
import torch


def _ids(n_tokens, first=10):
    """Sentence i: n_tokens[i] ids, all of them first + i."""
    return [[first + i] * n for i, n in enumerate(n_tokens)]


def _read_run(calls, pad_id):
    """A read-out that names each row: (the row's id, its token count), and records the padded call."""
    def read(tok, typ, msk):
        assert tok.dtype == typ.dtype == msk.dtype == torch.int64 and tok.shape == typ.shape == msk.shape
        assert bool((tok[msk == 0] == pad_id).all()) and bool((typ[msk == 0] == 0).all())
        assert bool((msk[:, 0] == 1).all()) and int(msk.sum(1).max()) == tok.shape[1]          # padded to its own longest member
        calls.append(tuple(tok.shape))
        out = torch.zeros(tok.shape[0], 768)
        out[:, 0] = tok[:, 0].float()
        out[:, 1] = msk.sum(1).float()
        return out
    return read


def test_encode_bucketed_order_padding_and_budget():
    from aspire_amd.model_front import encode_bucketed
    n_tokens = [5, 1, 9, 3, 2, 12, 4]
    ids = _ids(n_tokens)
    types = [[0] * n for n in n_tokens]
    calls = []
    out = encode_bucketed(_read_run(calls, pad_id=7), ids, types, 7, 16, torch.device('cpu'))
    assert out.shape == (7, 768) and out.dtype == torch.float32
    assert out[:, 0].tolist() == [10.0 + i for i in range(7)] and out[:, 1].tolist() == [float(n) for n in n_tokens]   # input order
    assert len(calls) > 1 and sum(b for b, _ in calls) == 7
    assert all(b * l <= 16 for b, l in calls)
    # one sentence longer than the budget is a call of its own
    calls = []
    out = encode_bucketed(_read_run(calls, pad_id=0), _ids([3, 40, 2]), [[0] * n for n in (3, 40, 2)], 0, 16, torch.device('cpu'))
    assert (1, 40) in calls and out[:, 1].tolist() == [3.0, 40.0, 2.0]
    # nothing to encode: no call
    calls = []
    assert encode_bucketed(_read_run(calls, 0), [], [], 0, 16, torch.device('cpu')).shape == (0, 768) and calls == []


def test_per_paper_splits_like_np_split():
    from aspire_amd.model_front import per_paper
    calls = []

    def encode(sents):
        calls.append(list(sents))
        return np.stack([np.full(768, float(s), np.float32) for s in sents])

    it = iter(range(100))
    papers = [{'ABSTRACT': [str(next(it)) for _ in range(n)]} for n in [2, 0, 1, 4]]
    reps = per_paper(papers, encode)
    assert calls == [[str(i) for i in range(7)]]
    assert [r.shape for r in reps] == [(2, 768), (0, 768), (1, 768), (4, 768)] and all(r.dtype == np.float32 for r in reps)
    assert [r[:, 0].tolist() for r in reps] == [[0.0, 1.0], [], [2.0], [3.0, 4.0, 5.0, 6.0]]
    empty = per_paper([{'ABSTRACT': []}, {'ABSTRACT': ()}], encode)
    assert [r.shape for r in empty] == [(0, 768), (0, 768)] and all(r.dtype == np.float32 for r in empty) and len(calls) == 1


def test_add_to_store():
    from aspire_amd.model_front import add_to_store, check_pid_count
    from aspire_amd.repstore import RepStore
    blocks = [np.full((n, 768), float(n), np.float32) for n in (2, 0, 3)]
    store = add_to_store(None, ['a', 'b', 'c'], blocks)
    assert isinstance(store, RepStore) and [store.get(p).shape for p in 'abc'] == [(2, 768), (0, 768), (3, 768)]
    assert add_to_store(store, ['d'], iter(blocks[:1])) is store and len(store) == 4 and np.array_equal(store.get('d'), blocks[0])
    with pytest.raises(ValueError, match='3 pids for 2 papers'):
        add_to_store(None, ['a', 'b', 'c'], blocks[:2])
    with pytest.raises(ValueError, match='2 pids for 1 documents'):
        add_to_store(None, ['a', 'b'], (b for b in blocks[:1]), 'documents')
    with pytest.raises(ValueError, match='pids'):
        check_pid_count(['a'], 3)
    check_pid_count(['a'], 1)
    # a block with its row layout
    store = add_to_store(None, ['e'], [(blocks[2], (2, [1, 0]))])
    assert np.array_equal(store.get('e'), blocks[2])


def test_strip_prefix_on_the_checkpoint_forms():
    from aspire_amd.model_front import strip_prefix
    good = {'bert_encoder.embeddings.w': 1, 'bert_encoder.encoder.layer.0.w': 2}
    assert strip_prefix(good, 'bert_encoder.', who='X') == ({'embeddings.w': 1, 'encoder.layer.0.w': 2}, [])
    stray = dict(good, **{'lin.weight': 3, 'bert_encoderx': 4})
    assert strip_prefix(stray, 'bert_encoder.') == ({'embeddings.w': 1, 'encoder.layer.0.w': 2}, ['lin.weight', 'bert_encoderx'])
    with pytest.raises(KeyError, match="unexpected keys in the X state dict: \\['lin.weight', 'bert_encoderx'\\]"):
        strip_prefix(stray, 'bert_encoder.', who='X')
    towers = {'sent_encoder.pooler.w': 5, 'context_encoder.pooler.w': 6}
    assert strip_prefix(towers, 'sent_encoder.', drop=('context_encoder.',), who='X') == ({'pooler.w': 5}, [])
    with pytest.raises(KeyError, match='context_encoder'):
        strip_prefix(towers, 'sent_encoder.', who='X')
    # the two split_state_dict functions are built on it: results and errors as before
    from aspire_amd import bienc, sentenc
    mix = torch.zeros(1, 3)
    assert bienc.split_state_dict({'bert_encoder.a': 1, 'bert_layer_weights.weight': mix}) == ({'a': 1}, mix)
    assert bienc.split_state_dict({'bert_encoder.a': 1}) == ({'a': 1}, None)
    with pytest.raises(KeyError, match='bi-encoder state dict'):
        bienc.split_state_dict({'bert_encoder.a': 1, 'bert_layer_weights.weightx': mix})
    assert sentenc.split_state_dict(towers) == {'pooler.w': 5} and sentenc.split_state_dict({'pooler.w': 5}) == {'pooler.w': 5}
    for bad in (dict(towers, other=1), {'pooler.w': 5, 'other': 1}):
        with pytest.raises(KeyError, match="sentence-encoder state dict: \\['other'\\]"):
            sentenc.split_state_dict(bad)


def test_read_hparams(tmp_path):
    from aspire_amd.model_front import read_hparams
    (tmp_path / 'run_info.json').write_text(json.dumps({'all_hparams': {'base-pt-layer': 'x', 'n': 3}, 'other': 1}), encoding='utf-8')
    assert read_hparams(str(tmp_path)) == {'base-pt-layer': 'x', 'n': 3}


def test_facet_sentence_ids():
    from aspire_amd.model_front import facet_sentence_ids, sentence_facet_rows
    from aspire_amd.contextner import facet_row_ids
    labels = ['background_label', 'objective_label', 'method_label', 'result_label', 'method_label']
    assert facet_sentence_ids(labels, 'background') == [0, 1]              # 'objective_label' counts as background
    assert facet_sentence_ids(labels, 'method') == [2, 4] and facet_sentence_ids(labels, 'objective') == []
    reps = np.arange(5, dtype=np.float32)[:, None] * np.ones((1, 768), np.float32)
    assert sentence_facet_rows(reps, 'method', {'FACETS': labels})[:, 0].tolist() == [2.0, 4.0]
    assert sentence_facet_rows(reps, 'other', {'FACETS': labels}).shape == (0, 768)
    # contextner.facet_row_ids: those sentences, then their entity rows, counted from len(labels)
    assert facet_row_ids(labels, [['a'], ['b', 'c'], [], ['d'], ['e']], 'background') == [0, 1, 5, 6, 7]


class _Encoder:
    """Only what the shared code may use of a HipBertEncoder: device_inputs, checked (run_checked's order of calls), device."""
    device = torch.device('cpu')

    def __init__(self):
        self.log = []

    def device_inputs(self, tok, typ, msk, check_ids=True):
        self.log.append('device_inputs')
        return tok + 0, typ, msk

    def checked(self, run, outputs_finite, who):
        out = run()
        self.log.append(('checked', who, outputs_finite(out)))
        return out


def test_checked_read_on_a_bare_instance():
    from aspire_amd.model_front import EncoderFront, all_finite

    class Reader(EncoderFront):
        pass

    model = Reader.__new__(Reader)
    model.bert_encoder = enc = _Encoder()
    assert model.eval() is model
    tok = torch.arange(6).reshape(2, 3)
    seen = []

    def read(t, y, m):
        seen.append((t, y, m))
        return t.float(), torch.full((2,), float('inf')), None

    out = model._checked_read(read, lambda r: (r[0], r[2]), tok, None, tok * 0 + 1)
    assert torch.equal(out[0], tok.float()) and out[2] is None
    assert len(seen) == 1 and seen[0][0] is not tok and torch.equal(seen[0][0], tok) and seen[0][1] is None    # device_inputs' tensors
    assert enc.log == ['device_inputs', ('checked', 'Reader', True)]          # who: the class name; the inf part is not judged
    model._checked_read(read, lambda r: r, tok, None, tok, who='Other.encode')
    assert enc.log[2:] == ['device_inputs', ('checked', 'Other.encode', False)]
    model._checked_read(lambda t, y, m: t.float(), lambda r: r, tok, None, tok)          # one tensor
    assert enc.log[-1] == ('checked', 'Reader', True)
    # __call__ is forward
    model.forward = lambda a, b=2: (a, b)
    assert model(1, b=3) == (1, 3)
    # an empty store is made without the rule, a filled one goes through it once
    assert model._checked_fill(lambda: 'made', 0, 'X') == 'made' and enc.log[-1] == ('checked', 'Reader', True)
    model._checked_fill(lambda: (torch.ones(2, 768), None), 2, 'X.encode_to_pool')
    assert enc.log[-1] == ('checked', 'X.encode_to_pool', True)
    assert all_finite() and all_finite(None) and all_finite(torch.ones(3), None, torch.zeros(0))
    assert not all_finite(torch.ones(3), torch.tensor([1.0, float('nan')]))


def test_pool_layout_and_token_id_check():
    from aspire_amd.model_front import check_token_ids, pool_layout
    lens_t, start_t, total = pool_layout([3, 0, 2, 4])
    assert lens_t.dtype == start_t.dtype == torch.int32 and lens_t.tolist() == [3, 0, 2, 4] and start_t.tolist() == [0, 3, 3, 5]
    assert total == 9 and isinstance(total, int)
    lens_t, start_t, total = pool_layout([])
    assert lens_t.shape == start_t.shape == (0,) and total == 0
    cpu = torch.device('cpu')
    toks = [torch.full((2, 3 + i % 4), i % 50) for i in range(130)]           # three groups of 64, 64 and 2 batches
    check_token_ids(toks, 50, cpu)
    check_token_ids(iter([]), 50, cpu)
    for bad, at in ((50, 0), (-1, 70), (50, 129)):
        broken = list(toks)
        broken[at] = torch.tensor([[1, bad, 2]])
        with pytest.raises(IndexError, match='token id out of range'):
            check_token_ids(broken, 50, cpu)


def test_load_hf_loads_nothing_that_is_given():
    """With a model and a tokenizer (or no name for one) load_hf does not touch transformers."""
    import sys
    from aspire_amd.model_front import load_hf
    m, t = object(), object()
    keep = sys.modules.get('transformers')
    sys.modules['transformers'] = None                 # any import of it raises ImportError
    try:
        assert load_hf('some/name', m, t) == (m, t)
        assert load_hf(None, m) == (m, None)
        assert load_hf('some/name', m, want_tokenizer=False) == (m, None)
        with pytest.raises(ImportError):
            load_hf('some/name', m)
    finally:
        if keep is None:
            del sys.modules['transformers']
        else:
            sys.modules['transformers'] = keep
