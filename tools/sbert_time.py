"""The relative-position bias's cost (NOTES.md, "SentenceTransformer baselines"): the 12-layer forward + masked mean at 64 x 128 on
random-init BertModel weights (no bias, positions by index) or MPNetModel weights (bias table in LDS, position ids from a table)
in the same build.  Prints the mean time of a forward over event-timed repetitions; run each model in a process of its own under

    rocprofv3 --kernel-trace --stats -d prof_mpnet -o mpnet --output-format csv -- python tools/sbert_time.py --model mpnet

and read the flash_attn_p_kernel row of prof_mpnet/**/mpnet_kernel_stats.csv for the attention kernel's share."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from aspire_amd.encoder import HipBertEncoder  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--model', choices=('bert', 'mpnet'), required=True)
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--len', type=int, default=128)
ap.add_argument('--reps', type=int, default=20)
args = ap.parse_args()

torch.manual_seed(0)
kw = dict(vocab_size=3000, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
if args.model == 'bert':
    from transformers import BertConfig, BertModel
    model = BertModel(BertConfig(max_position_embeddings=512, **kw), add_pooling_layer=False)
else:
    from transformers import MPNetConfig, MPNetModel
    model = MPNetModel(MPNetConfig(max_position_embeddings=514, **kw), add_pooling_layer=False)
enc = HipBertEncoder(model.eval())
B, L = args.batch, args.len
tok = torch.randint(5, 3000, (B, L), generator=torch.Generator().manual_seed(B)).cuda()
msk = torch.ones_like(tok)
for _ in range(3):
    out = enc.forward_mean(tok, None, msk, normalize=True, check_ids=False)
torch.cuda.synchronize()
start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
start.record()
for _ in range(args.reps):
    out = enc.forward_mean(tok, None, msk, normalize=True, check_ids=False)
stop.record()
torch.cuda.synchronize()
assert enc.status() == 0 and bool(torch.isfinite(out).all())
print(f'{args.model} {B} x {L}: {start.elapsed_time(stop) / args.reps:.3f} ms per forward + mean pool ({args.reps} repetitions)')
