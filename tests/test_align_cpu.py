"""CPU: the alignment writer (aspire_amd/align.py) over a numpy stand-in for ops.dot_argmax, injected by argument -- the line schema
and the combination order of write_aligned_examples, which index of which product becomes cc_align / abs_align, the dev file's
negatives, and three arg-max calls in total whatever the number of examples."""
import itertools
import json
import types

import numpy as np
import pytest

D = 768


class Corpus:
    """8 papers of 2 .. 5 sentence rows stored out of order in one matrix, 3 co-cited sets with 2 .. 4 context rows"""

    def __init__(self, seed=0):
        rng = np.random.default_rng(seed)
        self.pids = [f'p{i}' for i in range(8)]
        lens = [3, 2, 5, 4, 2, 3, 5, 2]
        self.pid2abstract = {p: {'title': f'title of {p}', 'abstract': [f'{p} sentence {s} .' for s in range(n)]}
                             for p, n in zip(self.pids, lens)}
        order = [5, 2, 7, 0, 3, 6, 1, 4]                    # the store's row order is not the pid order
        rows, index, at = [], {}, 0
        for k in order:
            rows.append(rng.standard_normal((lens[k], D)).astype(np.float32))
            index[self.pids[k]] = (at, lens[k])
            at += lens[k]
        self.abs_store = types.SimpleNamespace(_dev_rows=np.concatenate(rows), _dev_index=index)
        self.cocited_sets = [('p0', 'p1', 'p2'), ('p3', 'p4'), ('p5', 'p1', 'p6', 'p7')]
        self.set_contexts = [[(f'c{s}{k}', f'context {k} of set {s}') for k in range(n)] for s, n in enumerate((3, 2, 4))]
        c_lens = np.array([3, 2, 4], dtype=np.int32)
        self.ctx_set = types.SimpleNamespace(rows=rng.standard_normal((int(c_lens.sum()), D)).astype(np.float32),
                                             start=np.array([0, 3, 5], dtype=np.int32), len=c_lens)

    def reps(self, pid):
        s, n = self.abs_store._dev_index[pid]
        return self.abs_store._dev_rows[s:s + n]

    def contexts(self, s):
        return self.ctx_set.rows[self.ctx_set.start[s]:self.ctx_set.start[s] + self.ctx_set.len[s]]


class NumpyArgmax:
    """the reference's np.matmul(...).argmax() per pair, counting its calls"""

    def __init__(self):
        self.calls = []

    def __call__(self, q, c):
        assert len(q.start) == len(q.len) == len(c.start) == len(c.len)
        self.calls.append(len(q.start))
        out = np.empty((len(q.start), 2), dtype=np.int32)
        for p, (qs, ql, cs, cl) in enumerate(zip(q.start, q.len, c.start, c.len)):
            sims = np.matmul(q.rows[qs:qs + ql], c.rows[cs:cs + cl].T)
            out[p] = np.unravel_index(sims.argmax(), sims.shape)
        return out


def _reference_loop(corpus, examples):
    """pre_proc_cocits.py:485-494, one example at a time"""
    cc, ab = [], []
    for s, anchor, pos in examples:
        q, p, ctx = corpus.reps(anchor), corpus.reps(pos), corpus.contexts(s)
        a2c = np.matmul(q, ctx.T)
        p2c = np.matmul(p, ctx.T)
        a2p = np.matmul(q, p.T)
        cc.append((int(np.unravel_index(a2c.argmax(), a2c.shape)[0]), int(np.unravel_index(p2c.argmax(), p2c.shape)[0])))
        ab.append(tuple(int(x) for x in np.unravel_index(a2p.argmax(), a2p.shape)))
    return cc, ab


def _examples(corpus):
    return [(s, pids[i], pids[j]) for s, pids in enumerate(corpus.cocited_sets) for i, j in itertools.combinations(range(len(pids)), 2)]


def test_align_cocited_takes_the_right_indices_in_three_calls():
    from aspire_amd import align_cocited
    corpus = Corpus()
    examples = _examples(corpus)
    assert len(examples) == 3 + 1 + 6
    argmax = NumpyArgmax()
    cc, ab = align_cocited(corpus.abs_store, corpus.ctx_set, examples, dot_argmax=argmax)
    assert argmax.calls == [len(examples)] * 3                         # three calls for the whole list
    want_cc, want_ab = _reference_loop(corpus, examples)
    assert cc == want_cc and ab == want_ab
    assert all(type(x) is int for pair in cc + ab for x in pair) and all(type(pair) is tuple for pair in cc + ab)
    # the second index of a context product (which context) is not what cc_align holds: some example must tell the two apart
    assert any(ab_ != cc_ for ab_, cc_ in zip(ab, cc))
    # whatever the number of examples: still three calls; none: none
    argmax = NumpyArgmax()
    align_cocited(corpus.abs_store, corpus.ctx_set, examples * 7, dot_argmax=argmax)
    assert argmax.calls == [7 * len(examples)] * 3
    argmax = NumpyArgmax()
    assert align_cocited(corpus.abs_store, corpus.ctx_set, [], dot_argmax=argmax) == ([], []) and argmax.calls == []
    with pytest.raises(KeyError):
        align_cocited(corpus.abs_store, corpus.ctx_set, [(0, 'p0', 'nobody')], dot_argmax=NumpyArgmax())


def test_written_lines_have_the_reference_schema_and_order(tmp_path):
    from aspire_amd import write_aligned_examples
    corpus = Corpus(seed=1)
    examples = _examples(corpus)
    want_cc, want_ab = _reference_loop(corpus, examples)
    argmax = NumpyArgmax()
    out = tmp_path / 'train-cocitabsalign.jsonl'
    n = write_aligned_examples(str(out), corpus.cocited_sets, corpus.set_contexts, corpus.pid2abstract, corpus.abs_store,
                               corpus.ctx_set, dot_argmax=argmax)
    assert n == len(examples) and argmax.calls == [n] * 3
    lines = out.read_text(encoding='utf-8').splitlines()
    assert len(lines) == n
    for line, (s, anchor, pos), cc, ab in zip(lines, examples, want_cc, want_ab):
        ex = json.loads(line)
        assert list(ex) == ['citing_pids', 'cited_pids', 'query', 'pos_context', 'citing_contexts']
        assert ex['citing_pids'] == [c[0] for c in corpus.set_contexts[s]]
        assert ex['citing_contexts'] == [c[1] for c in corpus.set_contexts[s]]
        assert ex['cited_pids'] == list(corpus.cocited_sets[s])
        assert ex['query'] == {'TITLE': corpus.pid2abstract[anchor]['title'], 'ABSTRACT': corpus.pid2abstract[anchor]['abstract']}
        assert ex['pos_context'] == {'TITLE': corpus.pid2abstract[pos]['title'], 'ABSTRACT': corpus.pid2abstract[pos]['abstract'],
                                     'cc_align': list(cc), 'abs_align': list(ab)}
    # itertools.combinations order inside a set, the sets in the order given
    assert [(json.loads(x)['query']['TITLE'], json.loads(x)['pos_context']['TITLE']) for x in lines[:3]] == \
        [('title of p0', 'title of p1'), ('title of p0', 'title of p2'), ('title of p1', 'title of p2')]


def test_dev_file_takes_its_negatives_from_the_sampler(tmp_path):
    import random
    from aspire_amd import random_neg_sampler, write_aligned_examples
    corpus = Corpus(seed=2)
    examples = _examples(corpus)
    asked = []

    def sampler(anchor_pid):
        asked.append(anchor_pid)
        k = len(asked)
        return f'p{k % 8}', (k, k + 1), (k + 2, k + 3)

    argmax = NumpyArgmax()
    out = tmp_path / 'dev-cocitabsalign.jsonl'
    write_aligned_examples(str(out), corpus.cocited_sets, corpus.set_contexts, corpus.pid2abstract, corpus.abs_store, corpus.ctx_set,
                           neg_sampler=sampler, dot_argmax=argmax)
    assert argmax.calls == [len(examples)] * 3                         # the negatives cost no arg-max
    assert asked == [anchor for _, anchor, _ in examples]
    for k, line in enumerate(out.read_text(encoding='utf-8').splitlines(), start=1):
        ex = json.loads(line)
        assert list(ex)[-1] == 'neg_context'
        neg = corpus.pid2abstract[f'p{k % 8}']
        assert ex['neg_context'] == {'TITLE': neg['title'], 'ABSTRACT': neg['abstract'], 'cc_align': [k, k + 1], 'abs_align': [k + 2, k + 3]}
    # the reference's draws (pre_proc_cocits.py:510-521) on a seeded generator: inside the two abstracts, repeatable
    draws = [random_neg_sampler(corpus.pid2abstract, random.Random(4))('p2') for _ in range(2)]
    assert draws[0] == draws[1]
    sample = random_neg_sampler(corpus.pid2abstract, random.Random(4))
    for _ in range(20):
        neg_pid, cc, ab = sample('p2')
        n_neg = len(corpus.pid2abstract[neg_pid]['abstract'])
        assert all(0 <= i < 5 and 0 <= j < n_neg for i, j in (cc, ab))


def test_alignment_encoder_names():
    from aspire_amd import alignment_encoder
    from aspire_amd.align import ALIGN_SUFFIX
    assert ALIGN_SUFFIX == {'cosentbert': 'cocitabsalign', 'sbmpnet1B': 'cocitabsalign-sb1b', 'specter': 'cocitabsalign-spec'}
    with pytest.raises(ValueError, match='Unknown alignment model'):
        alignment_encoder('word2vec')
