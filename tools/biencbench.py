"""Bi-encoder read-out throughput (GPU box): aspire_bert_forward_cls_f32 with a 13-way layer mix (AspireBiEnc) against
aspire_bert_forward_f32 + a read of row 0 (the HF CLS the way the full forward gives it), BERT-base, 12 layers, all tokens real.

    python tools/biencbench.py [--shapes 64x256,64x512] [--iters 20] [--out profiles/bienc_bench.json]
    python tools/biencbench.py --once cls|full --shapes 64x256        (one warmed forward, for rocprofv3 --kernel-trace --stats)

The two forms run ALTERNATELY in one process (rounds of `iters` forwards each, device-event timing, after warm-up), on the same seeded
inputs; their outputs are checked against each other on those inputs (mix = one-hot on the last state: both are the last hidden
state's CLS row).  Prices: the encoder's flops (14.16 M + 3072 L per token and layer) of the FULL forward over the
measured time, in % of the 157.3 TFLOP/s fp32-MFMA figure the encoder is quoted against."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _model():
    from transformers import BertConfig, BertModel
    torch.manual_seed(0)
    return BertModel(BertConfig(vocab_size=31090), add_pooling_layer=False).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='64x256,64x512')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--once', choices=('cls', 'full'))
    ap.add_argument('--out')
    a = ap.parse_args()
    from aspire_amd.bienc import AspireBiEnc
    m = _model()
    W = torch.randn(1, 13, generator=torch.Generator().manual_seed(1))
    bi = AspireBiEnc(bert_model=m, layer_weights=W)
    enc = bi.bert_encoder
    results = []
    for shape in a.shapes.split(','):
        B, L = (int(x) for x in shape.split('x'))
        g = torch.Generator().manual_seed(B * 1000 + L)
        tok = torch.randint(1000, 30000, (B, L), generator=g).cuda()
        seg = torch.zeros_like(tok)
        mask = torch.ones_like(tok)
        cls = lambda: enc.forward_cls(tok, seg, mask, bi.layer_mix(), check_ids=False)[0]
        full = lambda: enc.forward_hidden(tok, seg, mask, check_ids=False)[:, 0]
        if a.once:            # one warm-up forward and one measured one of the chosen form: the stats count two forwards
            for _ in range(2):
                (cls if a.once == 'cls' else full)()
            torch.cuda.synchronize()
            print(f'two {a.once} forwards at {B} x {L}')
            continue
        for _ in range(3):
            cls(), full()
        torch.cuda.synchronize()
        ev = lambda: torch.cuda.Event(enable_timing=True)
        t = {'cls': [], 'full': []}
        for _ in range(a.rounds):
            for name, fn in (('cls', cls), ('full', full)):
                s, e = ev(), ev()
                s.record()
                for _ in range(a.iters):
                    fn()
                e.record()
                torch.cuda.synchronize()
                t[name].append(s.elapsed_time(e) / a.iters)
        # the same seeded inputs, mix one-hot on the last state: both forms give the last hidden state's CLS row
        keep = bi.layer_weights
        bi.set_layer_weights(torch.full((1, 13), -1e4).index_fill_(1, torch.tensor([12]), 0.))
        diff = (cls() - full()).abs().max().item()
        bi.layer_weights = keep
        assert enc.status() == 0
        ms = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        flops = B * 12 * L * (14155776 + 3072 * L)
        r = {'B': B, 'L': L, 'ms_cls_mix13': round(ms['cls'], 3), 'ms_full_row0': round(ms['full'], 3),
             'docs_per_s_cls_mix13': round(B / ms['cls'] * 1e3, 1), 'docs_per_s_full_row0': round(B / ms['full'] * 1e3, 1),
             'saving_ms': round(ms['full'] - ms['cls'], 3), 'saving_pct': round(100 * (1 - ms['cls'] / ms['full']), 2),
             'full_tflops': round(flops / ms['full'] / 1e9, 1), 'full_pct_of_157': round(flops / ms['full'] / 1e9 / 157.3 * 100, 1),
             'rounds_ms': t, 'max_abs_diff_cls_vs_full_row0': diff}
        print(json.dumps(r))
        results.append(r)
    if a.out and results:
        with open(a.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
