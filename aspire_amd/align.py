"""The alignment writer of the co-citation data path: ``generate_examples_aligned_cocitabs_rand`` from the encoded rows on
(src/pre_process/pre_proc_cocits.py:466-534), with its three ``np.matmul(...).argmax()`` per example as three
``ops.dot_argmax`` calls (include/aspire_hip.h: aspire_dot_argmax_f32) for the WHOLE list of examples.

    enc = alignment_encoder('cosentbert', trained_model_path)            # or 'sbmpnet1B' / 'specter'
    abs_store = enc.encode_to_store(papers, pids).to_device()            # every abstract's sentence rows, resident once
    ctx_set = context_set(enc, set_contexts)                             # one document per co-cited set: its context sentences' rows
    write_aligned_examples('train-cocitabsalign.jsonl', cocited_sets, set_contexts, pid2abstract, abs_store, ctx_set)
    write_aligned_examples('dev-cocitabsalign.jsonl', dev_sets, dev_contexts, pid2abstract, abs_store, dev_ctx_set,
                           neg_sampler=random_neg_sampler(pid2abstract, random.Random(seed)))

The reference's random choices -- the 80 / 20 split of the co-cited sets, the (at most 10) contexts sampled per set, the dev
negatives and their alignment picks -- stay arguments: this module forms and writes the examples of the sets it is given.  The files
are what aspire_amd.batchers.JsonlRankBatches reads.  An abstract or a set's contexts of more than aspire_max_sents() (128) rows is
refused by the kernel's host check (NotImplementedError).
"""
import codecs
import itertools
import json
import os
from collections import namedtuple

import numpy as np

# alignment_model -> the reference's output file suffix (pre_proc_cocits.py:401-416): {split}-{suffix}.jsonl
ALIGN_SUFFIX = {'cosentbert': 'cocitabsalign', 'sbmpnet1B': 'cocitabsalign-sb1b', 'specter': 'cocitabsalign-spec'}

# what a stand-in for ops.dot_argmax is handed in the place of DeviceRepSets: rows [R, 768], start / len int32 [P] (numpy)
HostView = namedtuple('HostView', 'rows start len')


def alignment_encoder(name, trained_model_path=None, **kw):
    """The reference's three sentence encoders for the alignments (pre_proc_cocits.py:401-416) over this project's classes; their
    ``encode_to_store`` encodes the abstracts (and, through ``context_set``, the contexts).
      'cosentbert'  AspireSentEnc (CLS rows) over allenai/scibert_scivocab_uncased with {trained_model_path}/sent_encoder_cur_best.pt
      'sbmpnet1B'   SentenceModel('sbmpnet1B'): sentence-transformers/all-mpnet-base-v2
      'specter'     SentenceModel over allenai/specter, 512 tokens, mean pooling, no normalisation
    kw goes to the class (bert_model= / model=, tokenizer=: an already constructed model instead of a download)."""
    if name == 'cosentbert':
        import torch
        from .sentenc import AspireSentEnc
        if kw.get('bert_model') is None:
            kw.setdefault('hf_model_name', 'allenai/scibert_scivocab_uncased')
        enc = AspireSentEnc(max_seq_length=512, **kw)
        if trained_model_path is not None:
            enc.load_state_dict(torch.load(os.path.join(trained_model_path, 'sent_encoder_cur_best.pt'), map_location='cpu'))
        return enc
    from .sbert import SentenceModel
    if name == 'sbmpnet1B':
        return SentenceModel('sbmpnet1B', **kw)
    if name == 'specter':
        # always named: SentenceModel looks a name without hf_model_name up in its own table, which has no 'specter'; with model=
        # and tokenizer= handed in nothing is loaded under the name
        kw.setdefault('hf_model_name', 'allenai/specter')
        return SentenceModel('specter', max_seq_length=512, normalize=False, **kw)
    raise ValueError(f'Unknown alignment model: {name}')


def context_set(encoder, set_contexts):
    """The context sentences of every co-cited set, encoded by `encoder.encode_to_store` and resident: a DeviceRepSet with one
    document per set, in the order given.  set_contexts[s] is the set's list of (citing pid, context sentence)."""
    papers = [{'TITLE': '', 'ABSTRACT': [cc[1] for cc in contexts]} for contexts in set_contexts]
    ids = list(range(len(papers)))
    return encoder.encode_to_store(papers, ids).to_device().pool(ids).repset


def _host_i64(x):
    return (x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)).astype(np.int64)


def device_view(rows, start, lens):
    """(start, len) numpy tables over a resident row matrix as a DeviceRepSet: the documents ops.dot_argmax is handed"""
    import torch
    from . import ops
    lens_host = lens.tolist()
    to = lambda a: torch.from_numpy(a.astype(np.int32)).to(rows.device)
    return ops.DeviceRepSet(rows, to(start), to(lens), ext=0, max_len=max(lens_host, default=0), lens_host=lens_host)


def align_cocited(abs_store, ctx_set, examples, dot_argmax=None):
    """pre_proc_cocits.py:485-494 for a list of examples at once.
    abs_store: a RepStore after to_device() that holds every abstract's sentence rows; ctx_set: the context sentences' rows, one
    document per co-cited set (``context_set``); examples: [(set index, anchor pid, positive pid)].
    Returns (cc_align, abs_align), one Python int pair per example:
      cc_align   (the row of argmax(anchor x contexts), the row of argmax(positive x contexts))
      abs_align  both indices of argmax(anchor x positive)
    Three dot_argmax calls whatever the number of examples; documents are (start, len) views into the two resident matrices, so a
    paper that sits in thousands of examples is stored once.  The index tables are numpy gathers: Python reads each example's
    tuple and numbers its ids through a dict, and looks a (start, len) up once per distinct paper.
    dot_argmax: a stand-in ``f(q: HostView, c: HostView) -> int [P, 2]`` for ops.dot_argmax."""
    examples = list(examples)
    if not examples:
        return [], []
    n = len(examples)
    set_idx = np.fromiter((e[0] for e in examples), dtype=np.int64, count=n)
    pids = [e[1] for e in examples] + [e[2] for e in examples]       # the anchors, then the positives
    index = abs_store._dev_index
    # every distinct paper gets a number; its (start, len) is looked up once, the examples' tables are numpy gathers.  Python still
    # passes over the example tuples: tools/align_time.py reports this host part (host_tables_ms, 23.6 of the call's 37.8 ms at
    # 100 000 examples)
    number = {p: k for k, p in enumerate(dict.fromkeys(pids))}
    uniq, which = list(number), np.fromiter(map(number.__getitem__, pids), dtype=np.int64, count=2 * n)
    where = np.array([index[p] for p in uniq], dtype=np.int64).reshape(len(uniq), 2)        # (start, len) per distinct paper
    start, lens = where[which, 0], where[which, 1]
    c_start, c_len = _host_i64(ctx_set.start)[set_idx], _host_i64(ctx_set.len)[set_idx]
    if dot_argmax is None:
        from . import ops
        view, run = device_view, lambda q, c: ops.dot_argmax(q, c, want_best=False)[0].cpu().numpy()
    else:
        view, run = HostView, dot_argmax
    anchor = view(abs_store._dev_rows, start[:n], lens[:n])
    positive = view(abs_store._dev_rows, start[n:], lens[n:])
    contexts = view(ctx_set.rows, c_start, c_len)
    a2c = np.asarray(run(anchor, contexts))
    p2c = np.asarray(run(positive, contexts))
    a2p = np.asarray(run(anchor, positive))
    cc_align = list(zip(a2c[:, 0].tolist(), p2c[:, 0].tolist()))
    abs_align = list(zip(a2p[:, 0].tolist(), a2p[:, 1].tolist()))
    return cc_align, abs_align


def random_neg_sampler(pid2abstract, rng):
    """The reference's dev negative (pre_proc_cocits.py:510-521) with `rng` (a random.Random) in the place of the global
    generator: a paper drawn from all of pid2abstract and two random (anchor sentence, negative sentence) pairs.  Returns the
    ``neg_sampler(anchor_pid) -> (neg_pid, cc_align, abs_align)`` that write_aligned_examples takes."""
    all_abs_pids = list(pid2abstract.keys())

    def sample(anchor_pid):
        neg_pid = rng.choice(all_abs_pids)
        n_anchor, n_neg = len(pid2abstract[anchor_pid]['abstract']), len(pid2abstract[neg_pid]['abstract'])
        cc_align = (rng.choice(range(n_anchor)), rng.choice(range(n_neg)))
        abs_align = (rng.choice(range(n_anchor)), rng.choice(range(n_neg)))
        return neg_pid, cc_align, abs_align
    return sample


def write_aligned_examples(out_fname, cocited_sets, set_contexts, pid2abstract, abs_store, ctx_set, neg_sampler=None,
                           dot_argmax=None):
    """pre_proc_cocits.py:466-534 for one split: one json line per 2-combination of every co-cited set, in
    itertools.combinations order, with the reference's keys --
      citing_pids, citing_contexts   the set's contexts: set_contexts[s] = [(citing pid, sentence)]
      cited_pids                     the set: cocited_sets[s]
      query                          TITLE, ABSTRACT of the anchor (pid2abstract[pid]['title'] / ['abstract'])
      pos_context                    TITLE, ABSTRACT of the positive + cc_align, abs_align (align_cocited)
      neg_context                    with a neg_sampler (the dev file): TITLE, ABSTRACT of the paper it names + the two pairs it gives
    Returns the number of lines written."""
    assert len(cocited_sets) == len(set_contexts)
    examples = [(s, pids[i], pids[j]) for s, pids in enumerate(cocited_sets)
                for i, j in itertools.combinations(range(len(pids)), 2)]
    cc_align, abs_align = align_cocited(abs_store, ctx_set, examples, dot_argmax=dot_argmax)
    with codecs.open(out_fname, 'w', 'utf-8') as out:
        for (s, anchor_pid, pos_pid), cc, ab in zip(examples, cc_align, abs_align):
            out_ex = {
                'citing_pids': [cc_[0] for cc_ in set_contexts[s]],
                'cited_pids': list(cocited_sets[s]),
                'query': {'TITLE': pid2abstract[anchor_pid]['title'], 'ABSTRACT': pid2abstract[anchor_pid]['abstract']},
                'pos_context': {'TITLE': pid2abstract[pos_pid]['title'], 'ABSTRACT': pid2abstract[pos_pid]['abstract'],
                                'cc_align': cc, 'abs_align': ab},
                'citing_contexts': [cc_[1] for cc_ in set_contexts[s]],
            }
            if neg_sampler is not None:
                neg_pid, neg_cc, neg_ab = neg_sampler(anchor_pid)
                out_ex['neg_context'] = {'TITLE': pid2abstract[neg_pid]['title'], 'ABSTRACT': pid2abstract[neg_pid]['abstract'],
                                         'cc_align': tuple(int(x) for x in neg_cc), 'abs_align': tuple(int(x) for x in neg_ab)}
            out.write(json.dumps(out_ex) + '\n')
    return len(examples)
