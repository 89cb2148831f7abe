"""Ragged span pooling (GPU box): aspire_span_pool_ranges_f32 beside aspire_span_mean_pool_rows_f32 fed the same spans in its
dense-slot form, and the contextual-entity model's encode stage beside AspireConSent's.

  python tools/spanbench.py --mode ranges|dense [--root TREE]     one kernel in a loop (run it under rocprofv3 --kernel-trace --stats
                                                                  for the kernel's own time; prints the device-event time per call)
  python tools/spanbench.py --mode check                          both kernels on the same spans: equal bits
  python tools/spanbench.py --mode encode                         papers/s of AspireContextNER.encode_to_pool / encode_to_store and of
                                                                  AspireConSent.encode_to_pool on the same papers without entities

The load: --papers documents of --tokens tokens, --sents sentence spans that tile a document, 0 .. --max-ents entity spans per
document of 1 - 6 tokens (mostly 1 - 3) inside a sentence.  --root: the tree whose aspire_amd is imported (default: this one); a
tree of the commit before the range kernel existed runs --mode dense."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ENT_LENS = (1, 1, 1, 2, 2, 2, 2, 3, 3, 4, 5, 6)


def make_spans(rng, papers, tokens, sents, max_ents):
    sent_idxs, ner_idxs = [], []
    for _ in range(papers):
        cuts = np.sort(rng.choice(np.arange(4, tokens - 1), size=sents - 1, replace=False))
        bounds = [1] + cuts.tolist() + [tokens - 1]
        sent_idxs.append([list(range(bounds[i], bounds[i + 1])) for i in range(sents)])
        ners = []
        for _ in range(int(rng.integers(0, max_ents + 1))):
            n = int(rng.choice(ENT_LENS))
            lo = int(rng.integers(1, tokens - 1 - n))
            ners.append(list(range(lo, lo + n)))
        ner_idxs.append(ners)
    return sent_idxs, ner_idxs


def time_loop(fn, iters):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def kernel_mode(args):
    import torch
    from aspire_amd import ops
    from aspire_amd.batch_prep import spans_to_csr
    rng = np.random.default_rng(args.seed)
    sent_idxs, ner_idxs = make_spans(rng, args.papers, args.tokens, args.sents, args.max_ents)
    docs = [s + n for s, n in zip(sent_idxs, ner_idxs)]
    lens = np.array([len(d) for d in docs])
    base = np.cumsum(lens) - lens
    total, slots = int(lens.sum()), int(lens.max())
    n_tok = sum(len(x) for d in docs for x in d)
    hidden = torch.randn(args.papers, args.tokens, 768, device='cuda', generator=torch.Generator('cuda').manual_seed(args.seed))
    print(f'{args.papers} papers x {args.tokens} tokens, {args.sents} sentences + 0..{args.max_ents} entities: {total} rows '
          f'({int(lens.min())}..{slots} per paper, dense grid {args.papers * slots} slots), {n_tok} token rows read', flush=True)
    out = {}
    if args.mode in ('dense', 'check'):
        tok_idx, span_off = (t.cuda() for t in spans_to_csr(docs, slots))
        slot = np.arange(slots)[None, :]
        out_row = torch.from_numpy(np.where(slot < lens[:, None], base[:, None] + slot, -1).astype(np.int32).reshape(-1)).cuda()
        rows = torch.zeros(total, 768, device='cuda')
        fn = lambda: ops.span_mean_pool_rows(hidden, tok_idx, span_off, slots, out_row, rows)
        print(f'dense  aspire_span_mean_pool_rows_f32: {time_loop(fn, args.iters):.2f} us/call (device events, launch included)', flush=True)
        out['dense'] = rows
    if args.mode in ('ranges', 'check'):
        from aspire_amd.batch_prep import span_range_tables
        (doc, start, length, orow), _ = span_range_tables(sent_idxs, ner_idxs, row_base=base, max_seq_len=args.tokens)
        doc, start, length, orow = (torch.from_numpy(t).cuda() for t in (doc, start, length, orow))
        rows = torch.zeros(total, 768, device='cuda')
        fn = lambda: ops.span_pool_ranges(hidden, doc, start, length, rows=rows, out_row=orow)
        print(f'ranges aspire_span_pool_ranges_f32:    {time_loop(fn, args.iters):.2f} us/call (device events, launch included)', flush=True)
        out['ranges'] = rows
    if args.mode == 'check':
        assert torch.equal(out['dense'], out['ranges'])
        print('equal bits')


def encode_mode(args):
    import torch
    from transformers import BertConfig, BertModel, BertTokenizerFast
    from aspire_amd.batch_prep import prepare_abstracts
    from aspire_amd.consent import AspireConSent
    from aspire_amd.contextner import AspireContextNER
    rng = np.random.default_rng(args.seed)
    words = [f'w{i}' for i in range(2900)]
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, 'vocab.txt')
        open(p, 'w').write('\n'.join(['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]', '.'] + words) + '\n')
        tok = BertTokenizerFast(p, do_lower_case=True)
    per_sent = max(2, (args.tokens - 6) // args.sents - 1)
    papers = []
    for _ in range(args.n_encode):
        abstract, entities = [], [[] for _ in range(args.sents)]
        sent_words = [list(rng.choice(words, size=per_sent)) for _ in range(args.sents)]
        for _ in range(int(rng.integers(0, args.max_ents + 1))):
            s, n = int(rng.integers(0, args.sents)), int(rng.choice(ENT_LENS))
            lo = int(rng.integers(0, per_sent - n + 1))
            entities[s].append(' '.join(sent_words[s][lo:lo + n]))
        papers.append({'TITLE': ' '.join(rng.choice(words, size=3)), 'ABSTRACT': [' '.join(w) + ' .' for w in sent_words],
                       'ENTITIES': entities})
    torch.manual_seed(0)
    bert = BertModel(BertConfig(vocab_size=3000, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                                max_position_embeddings=512), add_pooling_layer=False).eval()
    ctx = AspireContextNER(bert_model=bert, tokenizer=tok)
    plain = AspireConSent(bert_model=bert)
    pids = list(range(len(papers)))
    bs = 64

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t
    ctx_batches, t_prep_ctx = wall(lambda: [ctx.prepare(papers[i:i + bs]) for i in range(0, len(papers), bs)])
    plain_batches, t_prep_plain = wall(lambda: [prepare_abstracts(papers[i:i + bs], tok) for i in range(0, len(papers), bs)])
    n_rows = sum(n for b in ctx_batches for n in b[1]) + sum(len(x) > 0 for b in ctx_batches for paper in b[3] for x in paper)
    print(f'{len(papers)} papers, {ctx_batches[0][0]["tokid_tt"].shape[1]} tokens, {n_rows} rows '
          f'({sum(n for b in ctx_batches for n in b[1])} sentences); host prep {t_prep_ctx * 1e3:.0f} ms with entities, '
          f'{t_prep_plain * 1e3:.0f} ms without', flush=True)
    runs = {'context_ner encode_to_pool': lambda: ctx.encode_to_pool(ctx_batches, pids=pids),
            'consent     encode_to_pool (as given, 1 stream)': lambda: plain.encode_to_pool(plain_batches, pids=pids, sort_by_length=False),
            'context_ner encode_to_store (prep + encode + download)': lambda: ctx.encode_to_store(papers, pids, batch_size=bs)}
    for fn in runs.values():
        fn()                                     # warm-up of every shape
    for rep in range(args.reps):                 # alternating
        for name, fn in runs.items():
            _, t = wall(fn)
            print(f'rep {rep}  {name}: {t * 1e3:.1f} ms  {len(papers) / t:.0f} papers/s', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('ranges', 'dense', 'check', 'encode'), default='check')
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--papers', type=int, default=64)
    ap.add_argument('--tokens', type=int, default=256)
    ap.add_argument('--sents', type=int, default=8)
    ap.add_argument('--max-ents', type=int, default=40)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--n-encode', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    if args.mode == 'encode':
        encode_mode(args)
    else:
        kernel_mode(args)


if __name__ == '__main__':
    main()
