"""The arithmetic of the bf16x3 matmul mode (HipBertTrainEncoder(matmul='bf16x3'), include/aspire_hip.h: ASPIRE_MATMUL_BF16X3) emulated
on the CPU with torch.bfloat16's rounding: the three-plane split of an fp32 operand and the six-term product.

    split3(x)            x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2), each round to nearest even, as fp32 tensors; both
                         subtractions are exact in fp32 (split3_bf16 of aspire_amd/csrc/common.h)
    six_terms(a, b)      a3 b1 + a1 b3 + a2 b2 + a2 b1 + a1 b2 + a1 b1 in float64 (every term is exact there): what the kernels would
                         accumulate if their fp32 sums were exact
    product(A, B)        A [M, K] . B [N, K]^T of six_terms, float64
"""
import torch

TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))       # (plane of a, plane of b), the kernels' order: smallest first


def split3(x):
    assert x.dtype == torch.float32
    x1 = x.to(torch.bfloat16).float()
    r1 = x - x1
    x2 = r1.to(torch.bfloat16).float()
    r2 = r1 - x2
    x3 = r2.to(torch.bfloat16).float()
    return x1, x2, x3


def six_terms(a, b):
    pa, pb = [p.double() for p in split3(a)], [p.double() for p in split3(b)]
    out = torch.zeros_like(pa[0])
    for i, j in TERMS:
        out = out + pa[i] * pb[j]
    return out


def product(A, B):
    pa, pb = [p.double() for p in split3(A)], [p.double() for p in split3(B)]
    return sum(pa[i] @ pb[j].t() for i, j in TERMS)


def abs_product(A, B):
    """sum over k of (|a1| + |a2| + |a3|) (|b1| + |b2| + |b3|): no partial sum of the six-term product, in any order, is larger"""
    sa, sb = sum(p.double().abs() for p in split3(A)), sum(p.double().abs() for p in split3(B))
    return sa @ sb.t()
