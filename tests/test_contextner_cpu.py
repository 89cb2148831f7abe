"""CPU: the host side of the contextual-entity model (aspire_amd/contextner.py, batch_prep's entity functions, RepStore's row
layout) against what the reference's own code returned (tests/golden/contextner.json, written by make_golden_contextner.py), the
new entry point's argument validation and the torch op's fake shapes.  No GPU is used."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def gold(golden_dir):
    return json.load(open(os.path.join(golden_dir, 'contextner.json')))


@pytest.fixture(scope='module')
def tokenizers(gold, tmp_path_factory):
    from transformers import BertTokenizer, BertTokenizerFast
    p = tmp_path_factory.mktemp('vocab') / 'vocab.txt'
    p.write_text('\n'.join(gold['vocab']) + '\n')
    return BertTokenizer(str(p), do_lower_case=True), BertTokenizerFast(str(p), do_lower_case=True)


def test_find_sublist_range():
    from aspire_amd.batch_prep import find_sublist_range
    assert find_sublist_range(list('abcabc'), list('bc')) == [1, 2]          # first match wins
    assert find_sublist_range(list('abc'), list('abc')) == [0, 1, 2]
    assert find_sublist_range(list('abc'), list('cd')) is None               # a match may not run off the end
    assert find_sublist_range(list('abc'), list('x')) is None
    assert find_sublist_range([], list('a')) is None
    assert find_sublist_range(list('abc'), []) == []
    assert find_sublist_range([], []) is None


def test_preparation_matches_reference(gold, tokenizers):
    """prepare_abstracts_entities / ner_token_idxs against AspireContextNER._preprocess_input: found entity, entity found twice,
    not found, overlapping entities, entity in the cut part of a capped sentence, entity of a sentence the cap dropped (no entry),
    papers without (valid) entities; slow and fast tokenizer."""
    from aspire_amd.batch_prep import ner_token_idxs, prepare_abstracts, prepare_abstracts_entities
    for tok in tokenizers:
        for case in gold['cases']:
            batch = [gold['docs'][i] for i in case['doc_ids']]
            bert_batch, abs_lens, sent_idxs, ner_idxs = prepare_abstracts_entities(batch, tok)
            assert bert_batch['tokid_tt'].tolist() == case['tokid_tt']
            assert bert_batch['seg_tt'].tolist() == case['seg_tt']
            assert bert_batch['attnmask_tt'].tolist() == case['attnmask_tt']
            assert bert_batch['seq_lens'] == case['seq_lens']
            assert abs_lens == case['abs_lens']
            assert sent_idxs == case['sent_token_idxs']
            assert ner_idxs == case['ner_token_idxs']
            assert ner_token_idxs(batch, prepare_abstracts(batch, tok)[2], tok) == case['ner_token_idxs']
    # the cases the fixture is meant to hold are in it
    by_doc = {tuple(c['doc_ids']): c['ner_token_idxs'] for c in gold['cases']}
    small = by_doc[(0, 1, 2, 3)]
    assert small[0][4] == [] and small[0][5] != []                 # a valid entity after an invalid one
    assert set(small[0][0]) & set(small[0][1])                      # overlapping entities
    assert small[1] == [] and small[2] == [[], [], []]              # no entities; all invalid
    cut = by_doc[(4,)][0]
    assert len(cut) == 3 and cut[2] == []                           # 4 entities given: the cut one is [], the dropped sentence's has no entry
    assert len(by_doc[(5,)][0]) == 1


def test_sentences_are_tokenised_once(gold, tokenizers):
    """with a fast tokenizer: one batched call for all sentences, one for all entities"""
    from aspire_amd.batch_prep import prepare_abstracts_entities
    fast = tokenizers[1]
    calls = []

    class Counting:
        is_fast = True

        def __getattr__(self, k):
            return getattr(fast, k)

        def __call__(self, texts, **kw):
            calls.append(list(texts))
            return fast(texts, **kw)

    batch = [gold['docs'][i] for i in (0, 3, 4)]
    prepare_abstracts_entities(batch, Counting())
    assert len(calls) == 2
    assert len(calls[0]) == sum(1 + len(d['ABSTRACT']) for d in batch)
    assert calls[1] == ['graph neural network', 'neural network model', 'the', 'trained', 'optimal transport', 'method',
                        'candidate document', 'query', 'optimal transport', 'data set', 'alignment score', 'result', 'x y', 'y x', 'z x']


def test_span_range_tables(gold):
    from aspire_amd.batch_prep import span_range_tables
    case = gold['cases'][0]
    sents, ners = case['sent_token_idxs'], case['ner_token_idxs']
    (doc, start, length, out_row), n_ent = span_range_tables(sents, ners)
    assert out_row is None and n_ent == [5, 0, 0, 6]
    assert all(a.dtype == np.int32 for a in (doc, start, length))
    want = []
    for d, (s, n) in enumerate(zip(sents, ners)):
        want += [(d, x[0], len(x)) for x in s] + [(d, x[0], len(x)) for x in n if x]
    assert list(zip(doc.tolist(), start.tolist(), length.tolist())) == want
    # into a store: a paper's rows are consecutive from its base
    (doc, _, _, out_row), _ = span_range_tables(sents, ners, row_base=[100, 0, 50, 10])
    assert out_row.dtype == np.int32
    for d, base in enumerate([100, 0, 50, 10]):
        assert out_row[doc == d].tolist() == list(range(base, base + len(sents[d]) + n_ent[d]))
    # the padded form: zero-length rows fill every paper's sentence block
    (doc, start, length, _), _ = span_range_tables(sents, ners, pad_sents=4)
    assert (doc == 1).sum() == 4 and length[doc == 1].tolist()[2:] == [0, 0]
    # an empty sentence span is a row of length 0; no entity lists at all
    (doc, start, length, _), n_ent = span_range_tables([[[1, 2], []]], None)
    assert length.tolist() == [2, 0] and n_ent == [0]
    with pytest.raises(ValueError, match='consecutive'):
        span_range_tables([[[1, 2, 4]]], [[]])
    with pytest.raises(ValueError, match='consecutive'):
        span_range_tables([[[1, 2]]], [[[5, 4]]])
    with pytest.raises(IndexError):
        span_range_tables([[[1, 2]]], [[[30, 31, 32]]], max_seq_len=32)
    with pytest.raises(IndexError):
        span_range_tables([[[-1, 0]]], [[]], max_seq_len=32)
    span_range_tables([[[1, 2]]], [[[30, 31]]], max_seq_len=32)


def test_append_entities(gold):
    from aspire_amd.batch_prep import append_entities
    assert append_entities(gold['docs']) == gold['appended']


def _rows(fn, n_rows, doc, facet):
    try:
        return np.asarray(fn(np.arange(n_rows)[:, None], facet, doc))[:, 0].tolist()
    except IndexError:
        return 'IndexError'


def test_facet_filters_match_reference(gold, tokenizers):
    """get_faceted_encoding on np.arange(n_rows)[:, None]: AspireContextNER's (valid entities only, with the reference's counter
    that stops at the first invalid entity, IndexError where the reference raises it) and the base one (AspireNER)."""
    from aspire_amd.contextner import AspireContextNER, AspireNER
    ctx = AspireContextNER.__new__(AspireContextNER)       # no encoder: the filter is host arithmetic
    ctx.tokenizer = tokenizers[0]
    ner = AspireNER.__new__(AspireNER)
    assert ctx.encoding_type == ner.encoding_type == 'sentence-entity'
    for doc, want, want_ner in zip(gold['docs'], gold['facets'], gold['facets_ner']):
        for facet in ('background', 'method', 'result'):
            assert _rows(ctx.get_faceted_encoding, want['n_rows'], doc, facet) == want['rows'][facet], (doc['TITLE'], facet)
            assert _rows(ner.get_faceted_encoding, want_ner['n_rows'], doc, facet) == want_ner['rows'][facet], (doc['TITLE'], facet)
    # the quirk is in the fixture: paper 0's last entity is valid (a row of the encoding) but follows an invalid one, so the filter
    # does not return it with its sentence's facet
    assert gold['facets'][0]['n_rows'] == 8 and gold['facets'][0]['rows']['result'] == [2]
    # torch tensors are filtered like arrays
    assert ctx.get_faceted_encoding(torch.arange(8)[:, None], 'method', gold['docs'][0])[:, 0].tolist() == gold['facets'][0]['rows']['method']


def test_repstore_faceted_with_layout(gold, tokenizers):
    from aspire_amd.batch_prep import prepare_abstracts_entities
    from aspire_amd.contextner import filter_valid_entities
    from aspire_amd.repstore import RepStore
    store = RepStore()
    for i, (doc, want) in enumerate(zip(gold['docs'], gold['facets'])):
        _, _, _, ner = prepare_abstracts_entities([doc], tokenizers[1])
        try:
            counts = [len(x) for x in filter_valid_entities(doc['ENTITIES'], [len(x) > 0 for x in ner[0]])]
        except IndexError:
            counts = None
        reps = np.tile(np.arange(want['n_rows'], dtype=np.float32)[:, None], (1, 768))
        store.add(f'p{i}', reps, layout=(len(doc['ABSTRACT']), counts))
        store.add(f'plain{i}', reps)
        for facet in ('background', 'method', 'result'):
            if want['rows'][facet] == 'IndexError':
                with pytest.raises(IndexError):
                    store.faceted(f'p{i}', facet, doc['FACETS'])
            else:
                assert store.faceted(f'p{i}', facet, doc['FACETS'])[:, 0].tolist() == want['rows'][facet]
            # without a layout: the sentence rows alone, as before
            labs = ['background' if lab == 'objective_label' else lab[:-6] for lab in doc['FACETS']]
            sent_only = [float(k) for k, lab in enumerate(labs) if lab == facet]
            if all(k < want['n_rows'] for k in sent_only):
                assert store.faceted(f'plain{i}', facet, doc['FACETS'])[:, 0].tolist() == sent_only
        assert store.faceted(f'p{i}', None, doc['FACETS']).shape[0] == want['n_rows']
    # adding a paper again without a layout forgets the old one
    store.add('p0', store.get('p0'))
    assert store.faceted('p0', 'method', gold['docs'][0]['FACETS'])[:, 0].tolist() == [1.0]


def test_span_pool_ranges_argument_validation_without_gpu():
    from aspire_amd import _lib
    f = _lib.lib.aspire_span_pool_ranges_f32
    p = 16          # any non-null address: nothing is dereferenced before the checks
    assert f(p, 1, 4, 512, p, p, p, 2, None, p, None, None) == _lib.ASPIRE_ERR_UNSUPPORTED
    assert b'768' in _lib.lib.aspire_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(_lib.ASPIRE_ERR_UNSUPPORTED)
    assert f(None, 1, 4, 768, p, p, p, 2, None, p, None, None) == _lib.ASPIRE_ERR_INVALID_ARG         # hidden
    assert f(p, 1, 4, 768, None, p, p, 2, None, p, None, None) == _lib.ASPIRE_ERR_INVALID_ARG         # row_doc
    assert f(p, 1, 4, 768, p, None, p, 2, None, p, None, None) == _lib.ASPIRE_ERR_INVALID_ARG         # row_start
    assert f(p, 1, 4, 768, p, p, None, 2, None, p, None, None) == _lib.ASPIRE_ERR_INVALID_ARG         # row_len
    assert f(p, 1, 4, 768, p, p, p, 2, None, None, None, None) == _lib.ASPIRE_ERR_INVALID_ARG         # rows
    assert f(p, 1, 0, 768, p, p, p, 2, None, p, None, None) == _lib.ASPIRE_ERR_INVALID_ARG            # L
    assert f(p, -1, 4, 768, p, p, p, 2, None, p, None, None) == _lib.ASPIRE_ERR_INVALID_ARG           # B
    assert f(p, 1, 4, 768, p, p, p, -1, None, p, None, None) == _lib.ASPIRE_ERR_INVALID_ARG           # R
    assert f(p, 0, 4, 768, p, p, p, 2, None, p, None, None) == _lib.ASPIRE_ERR_INVALID_ARG            # rows of no document
    with pytest.raises(AssertionError):
        _lib.check(_lib.ASPIRE_ERR_INVALID_ARG)
    # nothing to do: no launch, no GPU needed
    assert f(None, 0, 4, 768, None, None, None, 0, None, None, None, None) == _lib.ASPIRE_OK
    assert f(p, 3, 4, 768, None, None, None, 0, None, None, None, None) == _lib.ASPIRE_OK
    assert _lib.SIGNATURES['aspire_span_pool_ranges_f32'][1][-1] is ctypes.c_void_p


def test_span_pool_ranges_op_fake_shapes():
    import aspire_amd.torch_ops as to
    assert 'span_pool_ranges' in to.OPS
    m = lambda *s, dt=torch.float32: torch.empty(*s, device='meta', dtype=dt)
    i32 = torch.int32
    cls, rows = torch.ops.aspire.span_pool_ranges(m(3, 40, 768), m(17, dt=i32), m(17, dt=i32), m(17, dt=i32))
    assert cls.shape == (3, 768) and rows.shape == (17, 768) and rows.dtype == torch.float32
    cls, rows = torch.ops.aspire.span_pool_ranges(m(2, 9, 768), m(0, dt=i32), m(0, dt=i32), m(0, dt=i32))
    assert cls.shape == (2, 768) and rows.shape == (0, 768)
    z = torch.zeros(1, dtype=i32)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.span_pool_ranges(torch.zeros(1, 2, 768), z, z, z)


def test_models_are_exported():
    import aspire_amd
    from aspire_amd import contextner
    for name in ('AspireConSenContextual', 'AspireContextNER', 'AspireNER'):
        assert getattr(aspire_amd, name) is getattr(contextner, name)
