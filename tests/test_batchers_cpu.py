"""CPU: the jsonl batcher of the sentence-alignment models (aspire_amd/batchers.py) on a hand-written fixture
(tests/golden/cocit_examples.jsonl: 7 training lines, then 3 dev lines with 'neg_context'; every context carries 'cc_align' and
'abs_align').  JsonlRankBatches against batch_prep.make_batch on hand-sliced lines, the shuffled per-epoch copies, and the callables
the trainers take."""
import json
import os

import pytest
import torch

N_TRAIN, N_DEV = 7, 3


@pytest.fixture(scope='module')
def tok(tmp_path_factory):
    from transformers import BertTokenizer
    vocab = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'bienc_prep.json')))['vocab']
    p = tmp_path_factory.mktemp('vocab') / 'vocab.txt'
    p.write_text('\n'.join(vocab) + '\n')
    return BertTokenizer(str(p), do_lower_case=True)


@pytest.fixture(scope='module')
def lines():
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'cocit_examples.jsonl'), encoding='utf-8') as fp:
        out = fp.readlines()
    assert len(out) == N_TRAIN + N_DEV
    return out


@pytest.fixture()
def data(tmp_path, lines):
    """data_path with train-cocitabsalign.jsonl (7 lines) and dev-cocitabsalign.jsonl (3 lines)"""
    d = tmp_path / 'data'
    d.mkdir()
    (d / 'train-cocitabsalign.jsonl').write_text(''.join(lines[:N_TRAIN]), encoding='utf-8')
    (d / 'dev-cocitabsalign.jsonl').write_text(''.join(lines[N_TRAIN:]), encoding='utf-8')
    return str(d)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _feed(exs):
    feed = {'query_texts': [e['query'] for e in exs], 'pos_texts': [e['pos_context'] for e in exs]}
    if 'neg_context' in exs[0]:
        feed['neg_texts'] = [e['neg_context'] for e in exs]
    return feed


@pytest.mark.parametrize('num_examples,batch_size,sizes', [(7, 3, [3, 3, 1]), (7, 7, [7]), (3, 5, [3]), (6, 3, [3, 3])])
@pytest.mark.parametrize('align_type', ['cc_align', 'abs_align'])
def test_batches_equal_make_batch_on_hand_sliced_lines(data, lines, tok, num_examples, batch_size, sizes, align_type):
    from aspire_amd import JsonlRankBatches
    from aspire_amd.batch_prep import make_batch
    exs = [json.loads(x) for x in lines[:N_TRAIN]]
    batches = JsonlRankBatches(os.path.join(data, 'train-cocitabsalign.jsonl'), num_examples, batch_size, tok, align_type=align_type)
    assert batches.num_batches == len(sizes) == len(batches)
    got = list(batches)
    assert len(got) == len(sizes)
    lo = 0
    for b, n in zip(got, sizes):
        want = make_batch(_feed(exs[lo:lo + n]), tok, align_type=align_type)
        assert _same(b, want)
        assert b['pos_align_idxs'] == [e['pos_context'][align_type] for e in exs[lo:lo + n]] and len(b['query_abs_lens']) == n
        assert 'neg_bert_batch' not in b
        lo += n
    assert lo == num_examples          # 6 / 3 with 7 lines in the file: the 7th is not read
    assert _same(list(batches), got)   # iterating again opens the file anew


def test_alignment_keys_differ_in_the_fixture(lines):
    exs = [json.loads(x) for x in lines]
    assert any(e['pos_context']['cc_align'] != e['pos_context']['abs_align'] for e in exs[:N_TRAIN])
    for e in exs:
        for side in ('pos_context', 'neg_context'):
            if side in e:
                for key in ('cc_align', 'abs_align'):
                    i, j = e[side][key]
                    assert 0 <= i < len(e['query']['ABSTRACT']) and 0 <= j < len(e[side]['ABSTRACT'])
    assert all('neg_context' not in e for e in exs[:N_TRAIN]) and all('neg_context' in e for e in exs[N_TRAIN:])


def test_dev_lines_give_the_negatives_first(data, lines, tok):
    from aspire_amd import JsonlRankBatches
    from aspire_amd.batch_prep import make_batch
    exs = [json.loads(x) for x in lines[N_TRAIN:]]
    got = list(JsonlRankBatches(os.path.join(data, 'dev-cocitabsalign.jsonl'), 3, 2, tok))
    assert [len(b['query_abs_lens']) for b in got] == [2, 1]
    for b, part in zip(got, (exs[:2], exs[2:])):
        assert _same(b, make_batch(_feed(part), tok))
        assert b['neg_align_idxs'] == [e['neg_context']['cc_align'] for e in part]
        assert b['pos_align_idxs'] == [e['pos_context']['cc_align'] for e in part]


def test_a_short_file_raises_naming_both_counts(data, tok):
    from aspire_amd import JsonlRankBatches
    batches = JsonlRankBatches(os.path.join(data, 'train-cocitabsalign.jsonl'), 9, 4, tok)
    assert batches.num_batches == 3
    with pytest.raises(ValueError, match=r'has 7 examples.* 9'):
        list(batches)
    with pytest.raises(ValueError):
        JsonlRankBatches(os.path.join(data, 'train-cocitabsalign.jsonl'), 0, 4, tok)
    with pytest.raises(ValueError, match='align_type'):
        list(JsonlRankBatches(os.path.join(data, 'train-cocitabsalign.jsonl'), 2, 2, tok, align_type='no_align'))


def _hparams(**kw):
    return dict(dict(train_suffix='cocitabsalign', train_size=7, dev_size=3, batch_size=3, num_epochs=3), **kw)


def _read(fname):
    with open(fname, 'rb') as fp:
        return fp.read()


def test_shuffled_copies(data, lines, tmp_path):
    from aspire_amd import write_shuffled_copies
    hp = _hparams()
    run = str(tmp_path / 'run')
    names = write_shuffled_copies(data, run, hp, seed=11)
    assert names == [os.path.join(run, 'shuffled_data', f'train-cocitabsalign-{e}.jsonl') for e in range(3)]
    copies = [_read(n) for n in names]
    source = sorted(x.encode('utf-8') for x in lines[:N_TRAIN])
    for c in copies:
        assert sorted(c.splitlines(keepends=True)) == source          # a permutation of the source's lines
    assert len(set(copies)) == 3                                       # epochs differ
    again = write_shuffled_copies(data, str(tmp_path / 'run2'), hp, seed=11)
    assert [_read(n) for n in again] == copies                         # the same seed: the same bytes
    other = write_shuffled_copies(data, str(tmp_path / 'run3'), hp, seed=12)
    assert [_read(n) for n in other] != copies
    # world = 2 on 7 lines: two shards of 3 disjoint lines, the remainder line left out
    shards = write_shuffled_copies(data, str(tmp_path / 'ddp'), hp, seed=11, world=2)
    assert len(shards) == 3
    for e, per_rank in enumerate(shards):
        assert per_rank == [os.path.join(str(tmp_path / 'ddp'), 'shuffled_data', f'train-cocitabsalign-{r}-{e}.jsonl') for r in range(2)]
        parts = [_read(n).splitlines(keepends=True) for n in per_rank]
        assert [len(p) for p in parts] == [3, 3] and len(set(parts[0]) | set(parts[1])) == 6
        assert set(parts[0] + parts[1]) <= set(source)
        assert parts[0] + parts[1] == copies[e].splitlines(keepends=True)[:6]      # the un-sharded shuffle of this seed, cut
    # no suffix: train.jsonl; a source shorter than train_size raises
    os.rename(os.path.join(data, 'train-cocitabsalign.jsonl'), os.path.join(data, 'train.jsonl'))
    plain = write_shuffled_copies(data, str(tmp_path / 'plain'), _hparams(train_suffix='', train_size=5, num_epochs=1), seed=3)
    assert plain == [os.path.join(str(tmp_path / 'plain'), 'shuffled_data', 'train-0.jsonl')]
    assert sorted(_read(plain[0]).splitlines(keepends=True)) == sorted(x.encode('utf-8') for x in lines[:5])      # head -n train_size
    with pytest.raises(ValueError, match=r'has 7 examples.* 8'):
        write_shuffled_copies(data, str(tmp_path / 'short'), _hparams(train_suffix='', train_size=8), seed=3)


def test_rank_batch_sources_are_restartable_and_sharded(data, lines, tok, tmp_path):
    from aspire_amd import JsonlRankBatches, rank_batch_sources, write_shuffled_copies
    hp = _hparams(num_epochs=2)
    run = str(tmp_path / 'run')
    names = write_shuffled_copies(data, run, hp, seed=5)
    train_batches, dev_batches = rank_batch_sources(data, run, hp, tok)
    for epoch in range(2):
        first = list(train_batches(epoch))
        assert [len(b['query_abs_lens']) for b in first] == [3, 3, 1]
        assert _same(first, list(train_batches(epoch)))                                  # called again: the same batches, the same order
        assert _same(first, list(JsonlRankBatches(names[epoch], 7, 3, tok)))
    assert not _same(list(train_batches(0)), list(train_batches(1)))
    dev = list(dev_batches())
    assert len(dev) == 1 and 'neg_bert_batch' in dev[0] and len(dev[0]['neg_abs_lens']) == 3
    assert _same(dev, list(JsonlRankBatches(os.path.join(data, 'dev-cocitabsalign.jsonl'), 3, 3, tok)))
    # under DDP: this rank's shard, train_size // world examples
    ddp = str(tmp_path / 'ddp')
    shards = write_shuffled_copies(data, ddp, hp, seed=5, world=2)
    for rank in range(2):
        tb, _ = rank_batch_sources(data, ddp, hp, tok, rank=rank, world=2, align_type='abs_align')
        got = list(tb(1))
        assert [len(b['query_abs_lens']) for b in got] == [3]
        assert _same(got, list(JsonlRankBatches(shards[1][rank], 3, 3, tok, align_type='abs_align')))
    # one rank (a DDP rehearsal at world 1): the un-sharded copies write_shuffled_copies(world=1) wrote, whatever the rank
    solo, _ = rank_batch_sources(data, run, hp, tok, rank=0, world=1)
    assert _same(list(solo(1)), list(train_batches(1)))
