"""The pooler kernel next to the CLS forward: a 12-layer random BertModel with its pooler through
HipBertEncoder.forward_pooled, one warm-up and three calls each at B = 32 (L = 32) and B = 16384 (L = 8).  Run under

    rocprofv3 --kernel-trace --stats -d prof -o pooler --output-format csv -- python tools/pooler_time.py

and read prof/**/pooler_kernel_trace.csv: the bert_pooler_kernel rows are the kernel's time, the kernels between two of them the
CLS forward's at the same B."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from transformers import BertConfig, BertModel  # noqa: E402

from aspire_amd.encoder import HipBertEncoder  # noqa: E402

torch.manual_seed(0)
cfg = BertConfig(vocab_size=3000, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                 max_position_embeddings=512)
enc = HipBertEncoder(BertModel(cfg, add_pooling_layer=True).eval())
for B, L in ((32, 32), (16384, 8)):
    tok = torch.randint(5, 3000, (B, L), generator=torch.Generator().manual_seed(B)).cuda()
    seg, msk = torch.zeros_like(tok), torch.ones_like(tok)
    for _ in range(4):
        cls, pooled = enc.forward_pooled(tok, seg, msk, check_ids=False)
        torch.cuda.synchronize()
    assert enc.status() == 0 and bool(torch.isfinite(cls).all()) and bool(torch.isfinite(pooled).all())
    print('done', B, L)
