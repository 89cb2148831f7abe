"""cosentbert throughput (GPU box): sentence encoding (AspireSentEnc's bucketed CLS forward) and the dot-product max-sim kernels.

    python tools/sentencbench.py [--part encode,score] [--out profiles/sentenc_bench.json]
    python tools/sentencbench.py --once encode|config4|config3      (one warmed run, for rocprofv3 --kernel-trace --stats)

Encoding: 65 536 synthetic sentences, BERT-base (12 layers, random init), token ids drawn at random.  ASSUMPTION (there is no
corpus here): token counts, [CLS] and [SEP] included, are log-normal with median 32 and sigma 0.5, clipped to 8 .. 128.  The sentences
are planned as AspireSentEnc.encode plans them (sorted by token count, calls of <= max_tokens padded rows) and the padded row count is
set against the reference's batching (SentenceTransformer.encode: length-sorted batches of 32, each padded to its longest).  FLOP/s
count REAL tokens only (14.16 M + 3072 n per token and layer, n the sentence's own length), quoted against the
fp16-plane encoder's roofline, 2 500 / 3 TFLOP/s (three fp16 products per term).

Scoring: config 4's shape (50 jobs x 125 candidates, documents of 1 .. 32 rows, aspire_dotmax_rank_batch_f32, k = 100) and config 3's
(32 queries x 50 000 candidates x 8 rows, aspire_dotmax_scores_f32 CROSS): kernel time by device events, and the matrix products'
FLOP over the time in % of the 155 TFLOP/s fp32 matrix rate (config 3: 157 GFLOP, floor 1.01 ms)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

F32_MATRIX_TF = 155.0
ENC_ROOF_TF = 2500.0 / 3


def _lengths(n, seed=0):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(np.exp(np.log(32) + 0.5 * rng.standard_normal(n))), 8, 128).astype(np.int64)


def _time(fn, iters, rounds=5):
    ev = lambda: torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(rounds):
        s, e = ev(), ev()
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters)
    return sorted(out)[len(out) // 2], out


def encode_part(once=False, n=65536, max_tokens=16384):
    from transformers import BertConfig, BertModel
    from aspire_amd.batch_prep import pad_sentences, sentence_buckets
    from aspire_amd.sentenc import AspireSentEnc
    torch.manual_seed(0)
    model = AspireSentEnc(bert_model=BertModel(BertConfig(vocab_size=31090), add_pooling_layer=False).eval())
    lens = _lengths(n)
    rng = np.random.default_rng(1)
    ids = [[2] + rng.integers(1000, 30000, int(k) - 2).tolist() + [3] for k in lens]
    types = [[0] * len(x) for x in ids]
    runs = sentence_buckets(lens, max_tokens)
    calls = [tuple(t.cuda() for t in pad_sentences(ids, types, r, 0)) for r in runs]
    out = torch.empty(n, 768, device='cuda')
    idx = [torch.from_numpy(r).cuda() for r in runs]

    def encode_all():
        for (tok, typ, msk), ix in zip(calls, idx):
            out[ix] = model.bert_encoder.forward_cls(tok, typ, msk, check_ids=False)[0]
    encode_all()
    torch.cuda.synchronize()
    assert model.bert_encoder.status() == 0 and bool(torch.isfinite(out).all())
    if once:
        encode_all()
        torch.cuda.synchronize()
        return None
    ms, rounds = _time(encode_all, 1, rounds=3)
    padded = int(sum(len(r) * lens[r].max() for r in runs))
    srt = np.sort(lens)[::-1]
    ref_padded = int(sum(len(srt[i:i + 32]) * srt[i:i + 32].max() for i in range(0, n, 32)))
    real = int(lens.sum())
    flops = float(np.sum(12 * lens * (14155776 + 3072 * lens)))
    tf = flops / ms / 1e9
    return {'sentences': n, 'length_assumption': 'log-normal token counts, median 32, sigma 0.5, clipped 8..128 (incl. [CLS]/[SEP])',
            'max_tokens': max_tokens, 'encoder_calls': len(runs), 'ms_total': round(ms, 2), 'rounds_ms': rounds,
            'sentences_per_s': round(n / ms * 1e3, 1), 'real_token_rows': real, 'padded_token_rows': padded,
            'padded_token_rows_ref_sort32': ref_padded, 'padding_overhead_pct': round(100 * (padded / real - 1), 2),
            'padding_overhead_ref_sort32_pct': round(100 * (ref_padded / real - 1), 2),
            'encoder_real_tflops': round(tf, 1), 'pct_of_fp16x3_roofline_833': round(100 * tf / ENC_ROOF_TF, 1)}


def _set(docs_lens, rng):
    from aspire_amd import ops
    rows = torch.from_numpy(rng.standard_normal((int(sum(docs_lens)), 768), dtype=np.float32))
    rows += torch.from_numpy(3.0 * rng.standard_normal(768, dtype=np.float32))         # anisotropic: mean cosine ~0.9
    lens = torch.tensor(docs_lens, dtype=torch.int32)
    start = (torch.cumsum(lens, 0) - lens).to(torch.int32)
    return ops.DeviceRepSet(rows.cuda(), start.cuda(), lens.cuda(), max_len=int(max(docs_lens)), lens_host=list(docs_lens))


def config4_part(once=False):
    from aspire_amd import ops
    rng = np.random.default_rng(4)
    J, C, k = 50, 125, 100
    q = _set(rng.integers(1, 33, J).tolist(), rng)
    c = _set(rng.integers(1, 33, J * C).tolist(), rng)
    job_off = torch.arange(0, J * C + 1, C, dtype=torch.int32).cuda()
    run = lambda: ops.dotmax_rank_batch(q, c, job_off, C, k)
    run()
    torch.cuda.synchronize()
    if once:
        run()
        torch.cuda.synchronize()
        return None
    ms, rounds = _time(run, 20)
    ql, cl = np.array(q.lens_host), np.array(c.lens_host).reshape(J, C)
    flops = float(2 * 768 * np.sum(ql[:, None] * cl))
    return {'shape': '50 jobs x 125 candidates, 1..32 rows each side, rank_batch k=100', 'ms': round(ms, 4), 'rounds_ms': rounds,
            'pairs_per_s': round(J * C / ms * 1e3, 1), 'gflop': round(flops / 1e9, 3),
            'pct_of_fp32_matrix_155': round(100 * flops / ms / 1e9 / F32_MATRIX_TF, 2)}


def config3_part(once=False):
    from aspire_amd import _lib, ops
    rng = np.random.default_rng(3)
    Q, C, S = 32, 50000, 8
    q = _set([S] * Q, rng)
    c = _set([S] * C, rng)
    run = lambda: ops.dotmax_scores(q, c, pairing=_lib.PAIR_CROSS)
    got = run()
    torch.cuda.synchronize()
    if once:
        run()
        torch.cuda.synchronize()
        return None
    # a sample against float64
    qr, cr = q.rows.cpu().numpy().astype(np.float64), c.rows.cpu().numpy()
    nq = qr / np.linalg.norm(qr, axis=1)[:, None]
    worst = 0.0
    g = got.view(Q, C).cpu().numpy()
    for ci in rng.integers(0, C, 64):
        y = cr[ci * S:(ci + 1) * S].astype(np.float64)
        y = y / np.linalg.norm(y, axis=1)[:, None]
        for qi in range(Q):
            worst = max(worst, abs(float((nq[qi * S:(qi + 1) * S] @ y.T).max()) - float(g[qi, ci])))
    ms, rounds = _time(run, 20)
    flops = 2.0 * Q * S * C * S * 768
    return {'shape': '32 queries x 50 000 candidates x 8 rows, CROSS cosine', 'ms': round(ms, 4), 'rounds_ms': rounds,
            'gflop': round(flops / 1e9, 1), 'floor_ms_at_155': round(flops / F32_MATRIX_TF / 1e9, 3),
            'pct_of_fp32_matrix_155': round(100 * flops / ms / 1e9 / F32_MATRIX_TF, 1), 'max_abs_err_vs_f64_sample': worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='encode,score')
    ap.add_argument('--once', choices=('encode', 'config4', 'config3'))
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.once:
        {'encode': encode_part, 'config4': config4_part, 'config3': config3_part}[a.once](once=True)
        print(f'one warmed {a.once} run')
        return
    res = {}
    parts = a.part.split(',')
    if 'score' in parts:
        res['config4_rank_batch'] = config4_part()
        print(json.dumps(res['config4_rank_batch']))
        res['config3_cross'] = config3_part()
        print(json.dumps(res['config3_cross']))
    if 'encode' in parts:
        res['encode'] = encode_part()
        print(json.dumps(res['encode']))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
