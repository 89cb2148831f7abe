"""The fused training attention's own arithmetic (aspire_amd/csrc/enc_attn_train.hip), emulated on the CPU in fp32: what
tests/test_gpu_flash_attn_train.py holds dQ and dK to.

tests/bf16_matmul_ref.py emulates the bf16 mode's THREE-KERNEL attention: a soft-max backward dS = P (dP - rowsum(dP P)) whose two terms
come from the same rounded product, so that with one key (L = 1, P = 1) dS, dQ and dK are exact zeros and the bound made of that
emulation's error is 0.  The fused backward forms the row term as D = rowsum(bf16(dctx) . ctx) from the forward's ctx -- equal to rowsum(dP P) in exact
arithmetic, different from it by the rounding of the probabilities into the forward's product and by the order of the fp32 sums -- so
its dS carries a residue that the three-kernel form does not have.  This module restates the fused arithmetic: Q, K, V and
dctx rounded to bf16 once, fp32 scores in log2 units, the UNNORMALISED probability rounded into the product with V and the division
by the row sum behind it, D from the rounded dctx and the fp32 ctx, P and dS rounded as they enter dV, dK and dQ.  (The online rescaling by the running
maximum is not restated: it moves the rounding of a probability by one bf16 ulp at most.)"""
import torch

H, DH, D = 12, 64, 768
SCALE_LOG2 = 0.125 * 1.4426950408889634
FLT_MAX = float(torch.finfo(torch.float32).max)


def r(x):
    return x.to(torch.bfloat16).to(x.dtype)


def attention(qkv, mask, G, dtype=torch.float32):
    """qkv [B, L, 2304], mask int64 [B, L], G [B, L, 768] = dctx -> ctx [B, L, 768], m, l [B, H, L], dqkv [B, L, 2304] in dtype"""
    b, l = mask.shape
    x = qkv.to(dtype)
    q, k, v = (x[..., i * D:(i + 1) * D].reshape(b, l, H, DH).transpose(1, 2) for i in range(3))
    g = G.to(dtype).reshape(b, l, H, DH).transpose(1, 2)
    rq, rk, rv, rg = r(q), r(k), r(v), r(g)
    bias = torch.where(mask != 0, 0.0, -FLT_MAX).to(dtype)[:, None, None, :]
    s = torch.matmul(rq, rk.transpose(-1, -2)) * SCALE_LOG2 + bias
    m = s.max(-1).values
    pt = torch.exp2(s - m[..., None])
    lsum = pt.sum(-1)
    ctx = torch.matmul(r(pt), rv) / lsum[..., None]
    dsum = (rg * ctx).sum(-1)
    p = pt * (1.0 / lsum)[..., None]
    dv = torch.matmul(r(p).transpose(-1, -2), rg)
    ds = r(p * (torch.matmul(rg, rv.transpose(-1, -2)) - dsum[..., None]))
    dq = torch.matmul(ds, rk) * 0.125
    dk = torch.matmul(ds.transpose(-1, -2), rq) * 0.125
    flat = [t.transpose(1, 2).reshape(b, l, D) for t in (ctx, dq, dk, dv)]
    return flat[0], m, lsum, torch.cat(flat[1:], -1)
