"""BASELINE config 5 end to end on ONE GPU's slice: token ids -> BERT forward -> span pooling straight into the resident rep store
-> 128 queries x otAspire + top-100 on it.  The reference's flow: pp_gen_nearest.py:141-202 (encode the papers in batches of 32 via
disent_models.py:344-371, then score every query against the pool and sort).

  python tools/e2ebench.py [N_DOCS L S N_QUERIES] [--matmul fp16]     (default 16384 256 12 128; synthetic tokens, random-init BERT-base;
                                                                       --matmul fp16: the encoder's opt-in fp16 matmul mode)

Prints docs/s of the encode stage, pairs/s of the score + rank stage, the time split (encoder kernels / pooling / host), and
spot-checks three pairs against HuggingFace BertModel (fp32, CPU) + the CPU oracle.  `run()` is what bench.py's `e2e` key calls."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

BATCH = 32          # pp_gen_nearest.py:141-160: papers are encoded 32 at a time


def synthetic_batches(n_docs, L, S, seed):
    """prepare_abstracts-shaped batches (ex_aspire_consent.py:185-212): CLS + S contiguous sentences + SEP = L tokens."""
    g = torch.Generator().manual_seed(seed)
    edges = np.linspace(1, L - 1, S + 1).astype(int)          # sentence s owns tokens [edges[s], edges[s + 1])
    spans = [list(range(int(edges[s]), int(edges[s + 1]))) for s in range(S)]
    batches = []
    for lo in range(0, n_docs, BATCH):
        b = min(BATCH, n_docs - lo)
        tok = torch.randint(1000, 30000, (b, L), generator=g)
        bert_batch = {'tokid_tt': tok, 'seg_tt': torch.zeros_like(tok), 'attnmask_tt': torch.ones_like(tok), 'seq_lens': [L] * b}
        batches.append((bert_batch, [S] * b, [spans] * b))
    return batches


def ragged_batches(n_docs, S, seed):
    """The same batches on documents of abstract-like, UNEVEN token length (log-normal around 220, clipped to [60, 500]), 32 at a
    time in corpus order, each batch padded to its longest document as prepare_abstracts pads."""
    rng = np.random.default_rng(seed)
    lens = np.clip(np.exp(rng.normal(np.log(220), 0.35, n_docs)).astype(int), 60, 500)
    batches = []
    for lo in range(0, n_docs, BATCH):
        ls = lens[lo:lo + BATCH]
        b, L = len(ls), int(ls.max())
        tok = torch.zeros(b, L, dtype=torch.long)
        mask = torch.zeros(b, L, dtype=torch.long)
        idxs = []
        for i, n in enumerate(ls):
            tok[i, :n] = torch.from_numpy(rng.integers(1000, 30000, n))
            mask[i, :n] = 1
            edges = np.linspace(1, n - 1, S + 1).astype(int)
            idxs.append([list(range(edges[s], edges[s + 1])) for s in range(S)])
        batches.append(({'tokid_tt': tok, 'seg_tt': torch.zeros_like(tok), 'attnmask_tt': mask, 'seq_lens': [int(n) for n in ls]}, [S] * b, idxs))
    return batches, lens


def run_ragged(model, n_docs=2048, S=8, seed=5):
    """encode_to_pool on documents of uneven length: the caller's corpus-order batches joined as given against the default
    (documents regrouped by token length, the store in corpus order)."""
    batches, lens = ragged_batches(n_docs, S, seed)
    for bb, _, _ in batches:
        for key in ('tokid_tt', 'seg_tt', 'attnmask_tt'):
            bb[key] = bb[key].cuda()
    rows_given = sum(len(a) * bb['tokid_tt'].shape[1] for bb, a, _ in batches)
    out = {'what': f'{n_docs} documents of 60 .. 500 tokens (log-normal around 220), {S} sentences, given {BATCH} at a time in corpus order '
                   f'(pp_gen_nearest.py:141-160); encode_to_pool with the batches joined as given / regrouped by token length (default)',
           'real_tokens': int(lens.sum()), 'token_rows_in_the_given_batches': int(rows_given)}
    stores = {}
    for name, sort in (('as_given', False), ('by_length', True)):
        model.encode_to_pool(batches[:4], sort_by_length=sort)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pool = model.encode_to_pool(batches, sort_by_length=sort)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        stores[name] = pool.repset.rows
        out[f'docs_per_s_{name}'] = n_docs / dt
    out['max_abs_diff_between_the_stores'] = float((stores['as_given'] - stores['by_length']).abs().max())
    return out


def run(n_docs=16384, L=256, S=12, n_queries=128, k=100, check=True, seed=2, planes=True, matmul='fp32'):
    from transformers import BertConfig, BertModel
    from aspire_amd import ops, scorer, _lib
    from aspire_amd.consent import AspireConSent
    dev = ops.require_gpu()
    torch.manual_seed(0)
    hf = BertModel(BertConfig(vocab_size=31090), add_pooling_layer=False).eval()
    model = AspireConSent(bert_model=hf) if matmul == 'fp32' else AspireConSent(bert_model=hf, matmul=matmul)
    batches = synthetic_batches(n_docs, L, S, seed)
    qbatches = synthetic_batches(n_queries, L, S, seed + 1)
    # move the token tensors to the GPU first: config 5 keeps everything resident, the PCIe-inclusive rate is not the metric
    for bb, _, _ in batches + qbatches:
        for key in ('tokid_tt', 'seg_tt', 'attnmask_tt'):
            bb[key] = bb[key].to(dev)
    model.encode_to_pool(batches[:2])             # warm-up (workspace allocation, clocks)
    torch.cuda.synchronize()
    stage_events = []
    t0 = time.perf_counter()
    extra = {'rows_per_forward': int(os.environ['E2E_ROWS_PER_FORWARD'])} if os.environ.get('E2E_ROWS_PER_FORWARD') else {}      # (A/B of the default)
    pool = model.encode_to_pool(batches, planes=planes, stage_events=stage_events, **extra)      # planes: + one pass over the finished store (inside the timed stage)
    torch.cuda.synchronize()
    t_encode = time.perf_counter() - t0
    # the stage's own split: HIP events recorded INSIDE the timed call, around every encoder forward and every pooling launch
    # (the GPU time between an event pair; what is left of the stage's wall time is host work with the GPU idle, launch gaps and the
    # planes pass at the end)
    enc_total_ms = sum(a.elapsed_time(b) for a, b, _ in stage_events)
    pool_total_ms = sum(b.elapsed_time(c) for _, b, c in stage_events)
    span_ms = stage_events[0][0].elapsed_time(stage_events[-1][2])
    n_batches = len(stage_events)
    calls = model._merge_batches(batches, 64)                 # what encode_to_pool runs: consecutive batches joined to 64 documents
    # queries: the same encoder, reps left on the GPU
    qreps = []
    for bb, abs_lens, idxs in qbatches:
        _, sent = model.forward_device(bb, abs_lens, idxs)
        qreps.extend(sent[i, :abs_lens[i]] for i in range(len(abs_lens)))
    q = ops.DeviceRepSet(torch.cat(qreps, 0).contiguous(), (torch.arange(n_queries, dtype=torch.int32) * S).to(dev),
                         torch.full((n_queries,), S, dtype=torch.int32, device=dev), ext=0, max_len=S, lens_host=[S] * n_queries)
    kk = min(k, n_docs)
    def timed(qq, cc):          # three warm-up calls (the clock governor settles over the first ~15 ms of a new load), median of three
        for _ in range(3):
            ops.ot_rank(qq, cc, kk, want=_lib.OT_SIMILARITY)
        torch.cuda.synchronize()
        ts, res = [], None
        for _ in range(3):
            t0 = time.perf_counter()
            res = ops.ot_rank(qq, cc, kk, want=_lib.OT_SIMILARITY)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[1], ts, res
    t_score, t_score_all, (scores, top_s, top_i) = timed(q, pool.repset)
    # the same score + rank stage on i.i.d. N(0, 1) reps of the same shapes: random-init BERT puts every sentence rep almost on
    # one line (cosine ~0.97), where |x|^2 - 2 x.y + |y|^2 cancels unless the rows are centred first (ASPIRE_OT_FLAG_CENTER, set by
    # aspire_amd.ops from a sample of the pool: NOTES.md, round-3 log)
    g = torch.Generator().manual_seed(seed + 7)
    iid_c = ops.DeviceRepSet(torch.randn(n_docs * S, 768, generator=g).to(dev), pool.repset.start, pool.repset.len, ext=0, max_len=S)
    if planes:
        iid_c.prepare_planes()
    iid_q = ops.DeviceRepSet(torch.randn(n_queries * S, 768, generator=g).to(dev), q.start, q.len, ext=0, max_len=S)
    t_score_iid, _, _ = timed(iid_q, iid_c)
    cosq = torch.nn.functional.normalize(pool.repset.rows[:2048], dim=1)
    mean_cos = float((cosq @ cosq.T).mean())
    out = {
        'what': f'config 5, one GPU slice: {n_docs} docs x {L} tokens ({S} sentences), prepared in batches of {BATCH}, encoded {len(calls[0][1])} per call straight into the resident '
                f'rep store, then {n_queries} queries x otAspire + top-{kk} on it (pp_gen_nearest.py:141-202); synthetic tokens, '
                f'random-init BERT-base',
        'docs': n_docs, 'tokens': L, 'sents': S, 'queries': n_queries, 'store_carries_fp16_planes': bool(planes),
        'encode_s': t_encode, 'docs_per_s': n_docs / t_encode,
        'score_rank_s': t_score, 'score_rank_s_calls': t_score_all, 'pairs_per_s': n_queries * n_docs / t_score,
        'score_rank_on_iid_reps_s': t_score_iid, 'pairs_per_s_on_iid_reps': n_queries * n_docs / t_score_iid,
        'mean_cosine_of_encoded_reps': mean_cos,
        'split_ms': {'encoder_kernels': enc_total_ms, 'pooling_kernels': pool_total_ms,
                     'gpu_gaps_between_calls': max(0.0, span_ms - enc_total_ms - pool_total_ms),
                     'encode_host_before_first_and_planes_after_last': max(0.0, t_encode * 1e3 - span_ms), 'ot_and_rank': t_score * 1e3,
                     'what': f'HIP events recorded inside the timed encode stage around each of its {n_batches} encoder calls and pooling launches; '
                             'the four encode entries add up to encode_s'},
        'encoder_share_of_total': enc_total_ms / (t_encode * 1e3 + t_score * 1e3),
        # 12 L (14 155 776 + 3072 L) flop per document; every product runs as three fp16 MFMAs (two planes per
        # operand), so the pipe's ceiling for this arithmetic is the dense fp16 peak / 3
        'encoder_roofline': {'bound': 'mfma', 'unit': 'TFLOP/s', 'peak': 2500.0 / 3,
                             'achieved': 12 * L * (14155776 + 3072 * L) * n_docs / t_encode / 1e12,
                             'frac': 12 * L * (14155776 + 3072 * L) * n_docs / t_encode / 1e12 / (2500.0 / 3),
                             'what': 'whole encode stage (GEMMs, attention, LayerNorms, pooling, host) against the fp16 MFMA peak / 3 products'},
    }
    try:
        out['ragged'] = run_ragged(model)
    except Exception as e:      # (a side measurement: never takes the block with it)
        out['ragged'] = {'error': repr(e)}
    if check:
        # three (query, candidate) pairs against HF BertModel (fp32, CPU) -> oracle pooling -> oracle OT
        from oracle import aspire_oracle as orc
        sc = scores.view(n_queries, n_docs)
        worst = 0.0
        with torch.no_grad():
            for qi, ci in ((0, 0), (n_queries // 2, n_docs // 3), (n_queries - 1, n_docs - 1)):
                reps = []
                for bset, i in ((qbatches, qi), (batches, ci)):
                    bb, abs_lens, idxs = bset[i // BATCH]
                    row = i % BATCH
                    h = hf(bb['tokid_tt'][row:row + 1].cpu(), token_type_ids=bb['seg_tt'][row:row + 1].cpu(),
                           attention_mask=bb['attnmask_tt'][row:row + 1].cpu()).last_hidden_state
                    _, sent = orc.span_mean_pool(h, [idxs[row]], [abs_lens[row]])
                    reps.append(sent[0, :abs_lens[row]])
                want = orc.get_similarity(reps[0], reps[1])
                worst = max(worst, abs(float(sc[qi, ci]) - want))
        out['spot_check'] = {'pairs': 3, 'max_abs_diff_vs_hf_plus_oracle': worst, 'tolerance': 2e-4, 'ok': worst < 2e-4}
    return out


def run_sharded(rank, world, group=None, n_docs=8192, L=256, S=12, n_queries=128, k=100, seed=2):
    """Config 5 as the 8-GPU job runs it, per rank (weak scaling: every rank n_docs documents of a corpus of world x n_docs): encode
    THIS rank's block straight into its HBM (with fp16 planes), wrap it as the rank's shard (ShardedPoolRanker.from_resident: one
    768-float broadcast fixes the planes' common centre), rank the replicated queries (otAspire) against it and merge the per-query
    top-k over ONE all-gather + one merge launch.  Returns this rank's numbers; bench.py gathers them from every rank."""
    from transformers import BertConfig, BertModel
    from aspire_amd import ops
    from aspire_amd.consent import AspireConSent
    from aspire_amd.parallel import ShardedPoolRanker
    import torch.distributed as dist
    dev = ops.require_gpu()
    torch.manual_seed(0)
    model = AspireConSent(bert_model=BertModel(BertConfig(vocab_size=31090), add_pooling_layer=False).eval())
    batches = synthetic_batches(n_docs, L, S, seed + 100 * (rank + 1))       # this rank's documents
    qbatches = synthetic_batches(n_queries, L, S, seed + 1)                  # the same queries on every rank
    for bb, _, _ in batches + qbatches:
        for key in ('tokid_tt', 'seg_tt', 'attnmask_tt'):
            bb[key] = bb[key].to(dev)
    model.encode_to_pool(batches[:2])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier(group)
    t0 = time.perf_counter()
    block = model.encode_to_pool(batches)
    ranker = ShardedPoolRanker.from_resident(block, rank * n_docs, world * n_docs, group=group, planes=True)      # (the planes pass and
    torch.cuda.synchronize()                                                          # the centre's broadcast belong to the stage, as in run())
    t_encode = time.perf_counter() - t0
    qreps = []
    for bb, abs_lens, idxs in qbatches:
        _, sent = model.forward_device(bb, abs_lens, idxs)
        qreps.extend(sent[i, :abs_lens[i]] for i in range(len(abs_lens)))
    kk = min(k, n_docs)
    ranker.rank_queries(qreps, kk, method='ot')
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier(group)
    t0 = time.perf_counter()
    top_s, top_i = ranker.rank_queries(qreps, kk, method='ot')
    torch.cuda.synchronize()
    t_rank = time.perf_counter() - t0
    return {'rank': rank, 'docs': n_docs, 'docs_per_s': n_docs / t_encode, 'encode_s': t_encode, 'score_rank_merge_s': t_rank,
            'pairs_per_s': n_queries * n_docs / t_rank, 'queries': n_queries, 'k': kk,
            'shards_in_top_k': int(len(torch.unique(top_i // n_docs))), 'top1_of_query0': int(top_i[0, 0])}


if __name__ == '__main__':
    argv = list(sys.argv[1:])
    mode = argv.pop(argv.index('--matmul') + 1) if '--matmul' in argv else 'fp32'
    argv = [v for v in argv if v != '--matmul']
    a = [int(v) for v in argv[:4]]
    r = run(*a, matmul=mode) if a else run(matmul=mode)
    r['matmul'] = mode          # (fp16: the spot check's 2e-4 is the fp32 path's tolerance and is expected to be missed)
    import json
    print(json.dumps(r, indent=1))
