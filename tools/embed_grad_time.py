"""The embedding lookup under training -- torch.ops.aspire.bert_embed_sum forward + backward (the three tables' gradients in HIP, fixed
order, no atomics) next to torch's nn.Embedding sum under autograd on the same card, and the whole encoder step of
tools/encoder_backward_time.py with HipBertTrainEncoder(hip_embeddings=True) next to the default.

    ours   torch.ops.aspire.bert_embed_sum(tok, typ, word, pos, type, padding_idx) -> (emb_sum * G).sum().backward()
    torch  (F.embedding(tok, word, padding_idx) + F.embedding(typ, type)) + pos[:L]  -> the same loss and backward()
    step   HipBertTrainEncoder(model, hip_embeddings=True / False)(ids, type_ids, mask) -> (hidden * G).sum().backward()

BertConfig() tables (30 522 x 768, 512 positions, 2 types).  Ids: Zipf-distributed with a third of the positions pad (id 0, the
padding row), and once every id equal and not pad -- one table row takes every token row, a serial chain of B L adds on one wave.
Every side is warmed up, then timed with device events over windows of about 0.2 s, the sides alternating, five windows each; the
median and the spread of the per-call times are printed as one JSON line per measurement.  The integer-valued gradients of the two
lookup sides are compared first (exact in any order).  Needs a GPU; there is no CPU path.

    python tools/embed_grad_time.py [--shapes 3x512,10x256] [--layers 12] [--skip-step]
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls        # ms per call


def measure(sides, windows, window_s):
    """sides: [(name, fn)] -> {name_ms_median, name_ms_min_max, name_calls_per_window}; the sides alternate window by window"""
    times, calls = {n: [] for n, _ in sides}, {}
    for name, fn in sides:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(int(window_s * 1e3 / window(fn, 3)), 2)
    for _ in range(windows):
        for name, fn in sides:
            times[name].append(window(fn, calls[name]))
    res = {}
    for name, t in times.items():
        res[name + '_ms_median'] = round(float(np.median(t)), 4)
        res[name + '_ms_min_max'] = [round(min(t), 4), round(max(t), 4)]
        res[name + '_calls_per_window'] = calls[name]
    return res


def zipf_ids(b, l, vocab, gen):
    """Zipf-distributed ids (exponent 1 over ranks 1 .. vocab - 1); a third of the positions are pad (id 0), as the tails of documents
    whose lengths are uniform in [L / 3, L]"""
    w = 1.0 / torch.arange(1, vocab, dtype=torch.float64)
    tok = 1 + torch.multinomial(w, b * l, replacement=True, generator=gen).reshape(b, l)
    lens = (l * (1 + 2 * torch.rand(b, generator=gen)) / 3).round().long()
    tok[torch.arange(l)[None, :] >= lens[:, None]] = 0
    return tok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='3x512,10x256')
    ap.add_argument('--layers', type=int, default=12)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-s', type=float, default=0.2, help='seconds of calls per timed window (small under a profiler)')
    ap.add_argument('--skip-step', action='store_true', help='the lookup alone, not the encoder step')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from transformers import BertConfig, BertModel
    from aspire_amd import HipBertTrainEncoder
    import aspire_amd.torch_ops  # noqa: F401
    F = torch.nn.functional
    torch.manual_seed(0)
    cfg = BertConfig(num_hidden_layers=a.layers, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    pad = cfg.pad_token_id
    word, pos, typ_tab = (torch.nn.Parameter(torch.randn(n, 768, device='cuda')) for n in
                          (cfg.vocab_size, cfg.max_position_embeddings, cfg.type_vocab_size))
    tables = (word, pos, typ_tab)
    hf = None
    if not a.skip_step:
        hf = BertModel(cfg, add_pooling_layer=False).cuda().train()
        encs = {on: HipBertTrainEncoder(copy.deepcopy(hf), hip_embeddings=on, check_ids=False).train() for on in (True, False)}
    for shape in a.shapes.split(','):
        b, l = (int(x) for x in shape.split('x'))
        g = torch.Generator().manual_seed(b * 1000 + l)
        ids = {'zipf': zipf_ids(b, l, cfg.vocab_size, g).cuda(), 'equal': torch.full((b, l), 1037).cuda()}
        typ = (torch.arange(l)[None, :] >= l // 2).long().expand(b, l).contiguous().cuda()
        G = torch.randn(b, l, 768, generator=g).cuda()
        Gi = torch.randint(-3, 4, (b, l, 768), generator=g).float().cuda()
        for kind, tok in ids.items():
            def zero():
                for t in tables:
                    t.grad = None

            def ours(grad=G):
                zero()
                torch.ops.aspire.bert_embed_sum(tok, typ, word, pos, typ_tab, pad).backward(grad)

            def theirs(grad=G):
                zero()
                ((F.embedding(tok, word, padding_idx=pad) + F.embedding(typ, typ_tab)) + pos[:l]).backward(grad)

            ours(Gi)
            got = [t.grad.clone() for t in tables]
            theirs(Gi)
            assert all(torch.equal(x, t.grad) for x, t in zip(got, tables)), 'integer-valued gradients differ'
            res = dict(what='lookup forward + backward', ids=kind, B=b, L=l, distinct_ids=int(tok.unique().numel()),
                       largest_run=int(torch.bincount(tok[tok != pad].reshape(-1)).max()))
            res.update(measure([('ours', ours), ('torch', theirs)], a.windows, a.window_s))
            print(json.dumps(res), flush=True)
        if a.skip_step:
            continue
        tok = ids['zipf']
        mask = (tok != pad).long()

        def step(on):
            enc = encs[on]

            def run():
                enc.zero_grad(set_to_none=True)
                (enc(tok, token_type_ids=typ, attention_mask=mask) * G).sum().backward()
            return run

        res = dict(what='encoder step, hip_embeddings on / off', B=b, L=l, layers=a.layers)
        res.update(measure([('on', step(True)), ('off', step(False))], a.windows, a.window_s))
        res['gate_on_median_le_off_max'] = bool(res['on_ms_median'] <= res['off_ms_min_max'][1])
        res['peak_mem_gb'] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
