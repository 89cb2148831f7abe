"""One training step of the CLS-row models on this library's kernels, by tools/encoder_backward_time.py's method:
device events over windows of about 0.2 s, the sides alternating, five windows each; one JSON line per shape.

(a) the encoder step, forward + backward of a 12-layer BERT-base (ffn 3072, fp32, dropout 0) from a [B, 768] gradient:
    cls     HipBertTrainEncoder.forward_cls(batch)                   -> (cls * g).sum().backward()     torch.ops.aspire.bert_layers_train_cls
    slice   HipBertTrainEncoder(batch)[:, 0]                         -> the same loss                  the route before forward_cls existed:
                                                                                                       autograd fills a [B, L, 768] gradient
    mix     forward_cls(batch, mix=softmax(logits))                  -> the same loss, logits trained
    hf_mix  BertModel(output_hidden_states=True), the mix in torch   -> the same loss                  MySPECTER as the reference runs it
    GATED: the median of `cls` must not exceed the highest window of `slice` (the change removes a zero fill and adds B-row launches:
    the only allowance is the old route's own spread); the tool exits 1 otherwise.  mix against hf_mix is recorded, not gated (the
    backward GEMMs' known deficit dominates it: DESIGN.md section 8 item 0).
(b) the in-batch cross-entropy, forward + backward over [B, 768] rows: torch.ops.aspire.inbatch_xent against torch.matmul +
    F.cross_entropy(reduction='sum') under autograd.  Recorded, not gated: both sides sit near the launch floor.

    python tools/cls_train_time.py [--shapes 3x512,10x256] [--layers 12] [--xent 20,128]

Needs a GPU; there is no CPU path.
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.encoder_backward_time import window  # noqa: E402


def timed(sides, windows, window_s):
    """{name: fn} -> {name_ms_median, name_ms_min_max, name_steps_per_window}; the sides alternate window by window"""
    times, calls = {n: [] for n in sides}, {}
    for name, fn in sides.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(int(window_s * 1e3 / window(fn, 3)), 2)
    for _ in range(windows):
        for name, fn in sides.items():
            times[name].append(window(fn, calls[name]))
    res = {}
    for name, t in times.items():
        res[name + '_ms_median'] = round(float(np.median(t)), 4)
        res[name + '_ms_min_max'] = [round(min(t), 4), round(max(t), 4)]
        res[name + '_steps_per_window'] = calls[name]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='3x512,10x256')
    ap.add_argument('--layers', type=int, default=12)
    ap.add_argument('--xent', default='20,128')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-s', type=float, default=0.2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from transformers import BertConfig, BertModel
    from aspire_amd import HipBertTrainEncoder
    import aspire_amd.torch_ops  # noqa: F401
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=3000, hidden_size=768, num_hidden_layers=a.layers, num_attention_heads=12, intermediate_size=3072,
                     max_position_embeddings=512, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    hf = BertModel(cfg, add_pooling_layer=False).cuda().train()
    enc = HipBertTrainEncoder(copy.deepcopy(hf)).train()
    logits = torch.randn(1, a.layers + 1, device='cuda', requires_grad=True)
    ok = True
    for shape in [s for s in a.shapes.split(',') if s]:
        b, l = (int(x) for x in shape.split('x'))
        gen = torch.Generator().manual_seed(b * 1000 + l)
        tok = torch.randint(5, 3000, (b, l), generator=gen).cuda()
        typ = torch.zeros_like(tok)
        lens = torch.randint(l // 2, l + 1, (b,), generator=gen)
        lens[0] = l
        mask = (torch.arange(l)[None, :] < lens[:, None]).long().cuda()
        g = torch.randn(b, 768, generator=gen).cuda()

        def cls():
            enc.zero_grad(set_to_none=True)
            (enc.forward_cls((tok, typ, mask)) * g).sum().backward()

        def slice_():
            enc.zero_grad(set_to_none=True)
            (enc(tok, token_type_ids=typ, attention_mask=mask)[:, 0] * g).sum().backward()

        def mix():
            enc.zero_grad(set_to_none=True)
            logits.grad = None
            (enc.forward_cls((tok, typ, mask), mix=torch.softmax(logits, dim=1)[0]) * g).sum().backward()

        def hf_mix():
            hf.zero_grad(set_to_none=True)
            logits.grad = None
            hs = hf(tok, token_type_ids=typ, attention_mask=mask, output_hidden_states=True).hidden_states
            rows = torch.nn.functional.linear(torch.stack(hs, dim=3), torch.softmax(logits, dim=1)).squeeze(3)[:, 0, :]
            (rows * g).sum().backward()

        # the two routes give the same gradients (the new one the old one's bits but for the zero fill's -0 / +0)
        cls()
        new = {n: p.grad.clone() for n, p in enc.bert.named_parameters()}
        slice_()
        dev = max(float((p.grad - new[n]).abs().max()) / max(float(p.grad.abs().max()), 1e-30) for n, p in enc.bert.named_parameters()
                  if not n.endswith('key.bias'))
        assert dev < 1e-3, dev
        res = dict(B=b, L=l, layers=a.layers, max_rel_grad_diff_cls_vs_slice=dev)
        res.update(timed({'cls': cls, 'slice': slice_, 'mix': mix, 'hf_mix': hf_mix}, a.windows, a.window_s))
        res['gate_cls_median_le_slice_max'] = bool(res['cls_ms_median'] <= res['slice_ms_min_max'][1])
        ok = ok and res['gate_cls_median_le_slice_max']
        res['peak_mem_gb'] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
        print(json.dumps(res), flush=True)
    for b in [int(x) for x in a.xent.split(',') if x]:
        gen = torch.Generator().manual_seed(b)
        q = (torch.randn(b, 768, generator=gen) * 0.2).cuda().requires_grad_()
        c = (torch.randn(b, 768, generator=gen) * 0.2).cuda().requires_grad_()
        target = torch.arange(b, device='cuda')

        def ours():
            q.grad = c.grad = None
            torch.ops.aspire.inbatch_xent(q, c)[0].sum().backward()

        def theirs():
            q.grad = c.grad = None
            torch.nn.functional.cross_entropy(torch.matmul(q, c.T), target, reduction='sum').backward()

        res = dict(xent_B=b)
        res.update(timed({'ours': ours, 'torch': theirs}, a.windows, a.window_s))
        print(json.dumps(res), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
