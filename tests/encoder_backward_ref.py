"""A torch restatement, in the tensors' dtype, of the formulas the encoder backward's row kernels implement (enc_bwd.hip): written out
term by term as the kernels compute them, so that holding them against torch autograd in float64 (tests/test_encoder_backward_cpu.py)
checks the formulas where no GPU is.  Not the product path, and nothing here is differentiated by autograd."""
import math

import torch

FLT_MAX = 3.4028234663852886e38


def layernorm_forward(x, gamma, beta, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def layernorm_backward(x, gamma, eps, dy, dy_res=None):
    """layernorm_backward_kernel: the moments again from the saved pre-norm rows x [rows, D]; dy (+ dy_res, the residual branch's
    gradient, in the same pass) -> dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)), dgamma = sum_rows dy xhat, dbeta = sum_rows dy."""
    if dy_res is not None:
        dy = dy + dy_res
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (x - mean) * rstd
    gdy = gamma * dy
    m1 = gdy.mean(-1, keepdim=True)
    m2 = (gdy * xhat).mean(-1, keepdim=True)
    dx = rstd * ((gdy - m1) - xhat * m2)
    return dx, colsum(dy * xhat), colsum(dy)


def gelu_forward(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu_backward(dy, u):
    """gelu_backward_kernel: dy (Phi(u) + u phi(u))."""
    cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return dy * (cdf + u * pdf)


def softmax_mask_forward(s, mask, scale):
    """softmax_mask_kernel: s [B, H, L, L] raw scores, mask [B, L] 0/1 -> P; a masked key gets -FLT_MAX (finite: an all-zero mask row
    comes out uniform), as HF's (1 - mask) * finfo.min in float32."""
    bias = torch.where(mask[:, None, None, :] != 0, torch.zeros((), dtype=s.dtype), torch.full((), -FLT_MAX, dtype=s.dtype))
    v = s * scale + bias                        # (a score of order 1 plus -FLT_MAX rounds to -FLT_MAX itself, in float32 and in float64)
    e = torch.exp(v - v.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_backward(dp, p, scale):
    """softmax_backward_kernel: dS = scale P (dP - sum_j dP_j P_j), the gradient of the RAW scores (the scale is the soft-max kernel's)."""
    return scale * (p * (dp - (dp * p).sum(-1, keepdim=True)))


def colsum(x):
    """colsum_partial_kernel + colsum_final_kernel: the sum over every leading row, per column."""
    return x.reshape(-1, x.shape[-1]).sum(0)
