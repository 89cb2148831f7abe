"""One training step of the encoder -- forward + backward of a 12-layer BERT-base (ffn 3072), dropout 0 -- in the three matmul modes of
aspire_amd.HipBertTrainEncoder and in its fused-attention mode, next to HuggingFace BertModel under torch autograd in fp32 and under
torch.autocast('cuda', dtype=torch.bfloat16), on the same card ("bf16 matrix products").

ONE side per process (a process's place on the card moves the step by more than the trees differ: DESIGN.md section 7), so a comparison
is several runs of this tool in one session on one card:

    python tools/bf16_step_time.py --side fp32          HipBertTrainEncoder(model)                 (also runs on a tree without the mode)
    python tools/bf16_step_time.py --side bf16          HipBertTrainEncoder(model, matmul='bf16')
    python tools/bf16_step_time.py --side bf16x3        HipBertTrainEncoder(model, matmul='bf16x3')
    python tools/bf16_step_time.py --side flash         HipBertTrainEncoder(model, matmul='bf16', attention='flash')
    python tools/bf16_step_time.py --side packed        HipBertTrainEncoder(model, matmul='bf16', attention='flash', packed=True)
    python tools/bf16_step_time.py --side hf            BertModel, fp32
    python tools/bf16_step_time.py --side hf-autocast   BertModel under torch.autocast('cuda', dtype=torch.bfloat16)

Every side: the same random-init weights and inputs, (hidden * G).sum().backward(), three warm-up steps, then device events over
windows of about 0.2 s, five windows; the median and the range of the per-step times, one JSON line per shape.  Needs a GPU.

--fill says how long the documents are: 'half' (the default, what this tool always drew: lengths uniform in [L/2, L], the first document
full), 'third' (lengths drawn once from a fixed seed uniformly in [L/3, L]: a mean fill of about 2/3, the project's "a third pad") and
'full' (every document full: what the padding-free mode's gather, scatter and row-map loads cost when nothing is saved).  The line
names the fill and the valid rows; the packed side adds the tape bytes of the packed and the padded size queries.

The kernels' own times: the bf16 or bf16x3 side under rocprofv3 --kernel-trace --stats --output-format csv with --windows 1 --window-s 0.02 (tools/statsum.py sums
the CSV by kernel).
"""
import argparse
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
    ap.add_argument('--side', choices=['fp32', 'bf16', 'bf16x3', 'flash', 'packed', 'hf', 'hf-autocast'], required=True)
    ap.add_argument('--shapes', default='3x512,10x256')
    ap.add_argument('--fill', choices=['half', 'third', 'full'], default='half')
    ap.add_argument('--layers', type=int, default=12)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-s', type=float, default=0.2, help='seconds of steps per timed window (small under a profiler)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from transformers import BertConfig, BertModel
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=3000, hidden_size=768, num_hidden_layers=a.layers, num_attention_heads=12, intermediate_size=3072,
                     max_position_embeddings=512, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = BertModel(cfg, add_pooling_layer=False).cuda().train()
    ours = a.side in ('fp32', 'bf16', 'bf16x3', 'flash', 'packed')
    if ours:
        from aspire_amd import HipBertTrainEncoder
        kw = {'fp32': {}, 'flash': dict(matmul='bf16', attention='flash'),
              'packed': dict(matmul='bf16', attention='flash', packed=True)}.get(a.side, dict(matmul=a.side))
        model = HipBertTrainEncoder(model, **kw).train()
    for shape in a.shapes.split(','):
        b, l = (int(x) for x in shape.split('x'))
        g = torch.Generator().manual_seed(b * 1000 + l)
        tok = torch.randint(5, 3000, (b, l), generator=g).cuda()
        typ = torch.zeros_like(tok)
        if a.fill == 'half':
            lens = torch.randint(l // 2, l + 1, (b,), generator=g)
            lens[0] = l
        elif a.fill == 'third':
            lens = torch.randint(l // 3, l + 1, (b,), generator=torch.Generator().manual_seed(7 * b + l))
        else:
            lens = torch.full((b,), l)
        mask = (torch.arange(l)[None, :] < lens[:, None]).long().cuda()
        G = torch.randn(b, l, 768, generator=g).cuda()

        def step():
            model.zero_grad(set_to_none=True)
            if ours:
                hidden = model(tok, token_type_ids=typ, attention_mask=mask)
            elif a.side == 'hf':
                hidden = model(tok, token_type_ids=typ, attention_mask=mask).last_hidden_state
            else:
                with torch.autocast('cuda', dtype=torch.bfloat16):
                    hidden = model(tok, token_type_ids=typ, attention_mask=mask).last_hidden_state
            (hidden.float() * G).sum().backward()

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        calls = max(int(a.window_s * 1e3 / window(step, 3)), 2)
        torch.cuda.reset_peak_memory_stats()      # the peak of this shape's steps alone
        t = [window(step, calls) for _ in range(a.windows)]
        line = dict(side=a.side, B=b, L=l, layers=a.layers, fill=a.fill, rows=int(lens.sum()), ms_median=round(float(np.median(t)), 3),
                    ms_min_max=[round(min(t), 3), round(max(t), 3)], steps_per_window=calls,
                    peak_mem_gb=round(torch.cuda.max_memory_allocated() / 1e9, 2))
        if a.side == 'packed':
            import ctypes
            from aspire_amd import _lib
            from aspire_amd.encoder import pack_layer_stack
            bw = pack_layer_stack([w.detach() for w in model.layer_weights()], 12, cfg.layer_norm_eps)
            line.update(tape_bytes_packed=_lib.lib.aspire_bert_tape_bytes_packed(ctypes.byref(bw), b, l, int(lens.sum())),
                        tape_bytes_padded=_lib.lib.aspire_bert_tape_bytes_attn(ctypes.byref(bw), b, l, 1))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
