"""One training step of the encoder -- forward + backward of a 12-layer BERT-base (ffn 3072), fp32, dropout 0 or --dropout P -- on this library's
kernels next to HuggingFace BertModel under torch autograd on the same card: what a RankLoss caller runs with
aspire_amd.HipBertTrainEncoder, and what it ran before that class existed.

    ours   HipBertTrainEncoder(model)(ids, type_ids, mask) -> (hidden * G).sum().backward()
    torch  model(ids, token_type_ids, attention_mask).last_hidden_state -> the same loss and backward()

Both sides share one set of random-init weights, are warmed up, then timed with device events over windows of about 0.2 s, the two
sides alternating, five windows each; the median and the spread of the per-step times are printed as one JSON line per shape.  The
parameter gradients are compared first.  Needs a GPU; there is no CPU path.

    python tools/encoder_backward_time.py [--shapes 3x512,10x256] [--layers 12] [--dropout P]

--dropout P sets both of the config's probabilities on both sides: ours is HipBertTrainEncoder(model, dropout=True), torch's is
BertModel.train() with the same config.  The two sides then draw different masks, so the gradients are not compared.

The kernels' own times: the same command under rocprofv3 --kernel-trace --stats with --side ours --windows 1 --window-s 0.02
(tools/statsum.py sums the CSV by kernel).
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
    return start.elapsed_time(end) / calls        # ms per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='3x512,10x256')
    ap.add_argument('--layers', type=int, default=12)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-s', type=float, default=0.2, help='seconds of steps per timed window (small under a profiler)')
    ap.add_argument('--side', choices=['both', 'ours', 'torch'], default='both')
    ap.add_argument('--dropout', type=float, default=0.0, help='hidden_dropout_prob = attention_probs_dropout_prob, both sides')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from transformers import BertConfig, BertModel
    from aspire_amd import HipBertTrainEncoder
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=3000, hidden_size=768, num_hidden_layers=a.layers, num_attention_heads=12, intermediate_size=3072,
                     max_position_embeddings=512, hidden_dropout_prob=a.dropout, attention_probs_dropout_prob=a.dropout)
    hf = BertModel(cfg, add_pooling_layer=False).cuda().train()
    enc = HipBertTrainEncoder(copy.deepcopy(hf), dropout=a.dropout > 0).train()
    for shape in a.shapes.split(','):
        b, l = (int(x) for x in shape.split('x'))
        g = torch.Generator().manual_seed(b * 1000 + l)
        tok = torch.randint(5, 3000, (b, l), generator=g).cuda()
        typ = torch.zeros_like(tok)
        lens = torch.randint(l // 2, l + 1, (b,), generator=g)
        lens[0] = l
        mask = (torch.arange(l)[None, :] < lens[:, None]).long().cuda()
        G = torch.randn(b, l, 768, generator=g).cuda()

        def ours():
            enc.zero_grad(set_to_none=True)
            (enc(tok, token_type_ids=typ, attention_mask=mask) * G).sum().backward()

        def theirs():
            hf.zero_grad(set_to_none=True)
            (hf(tok, token_type_ids=typ, attention_mask=mask).last_hidden_state * G).sum().backward()

        sides = [s for s in (('ours', ours), ('torch', theirs)) if a.side in ('both', s[0])]
        res = dict(B=b, L=l, layers=a.layers, dropout=a.dropout)
        if a.side == 'both' and a.dropout == 0:
            ours()
            theirs()
            dev = 0.0
            for (n, p), (_, q) in zip(enc.bert.named_parameters(), hf.named_parameters()):
                if n.endswith('key.bias'):          # zero in exact arithmetic (the soft-max ignores a per-query constant): noise on both sides
                    continue
                dev = max(dev, float((p.grad - q.grad).abs().max()) / max(float(q.grad.abs().max()), 1e-30))
            res['max_rel_grad_diff'] = dev          # per tensor, relative to its largest entry
            assert dev < 1e-3, dev
        times, calls = {n: [] for n, _ in sides}, {}
        for name, fn in sides:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            calls[name] = max(int(a.window_s * 1e3 / window(fn, 3)), 2)
        for _ in range(a.windows):
            for name, fn in sides:
                times[name].append(window(fn, calls[name]))
        for name, t in times.items():
            res[name + '_ms_median'] = round(float(np.median(t)), 3)
            res[name + '_ms_min_max'] = [round(min(t), 3), round(max(t), 3)]
            res[name + '_steps_per_window'] = calls[name]
        res['peak_mem_gb'] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
