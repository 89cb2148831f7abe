"""What the CLS-row training tests measure against, written from the formulas in torch (any dtype; the tests use float64) without the
library: the soft-max layer mix's CLS read-out, the summed triplet margin loss and the in-batch soft-max cross-entropy."""
import torch


def layer_mix_cls(hidden_states, weight):
    """hidden_states: n_layers + 1 tensors [B, L, D]; weight [1, n_layers + 1] (the logits of a bias-free Linear(n_layers + 1, 1)) ->
    the CLS rows [B, D] of sum_l softmax(weight, 1)[0, l] * hidden_states[l]"""
    mix = torch.softmax(weight, dim=1)[0]
    stacked = torch.stack(list(hidden_states), dim=3)                   # [B, L, D, n_layers + 1]
    return (stacked * mix).sum(dim=3)[:, 0, :]


def layer_cls_rows(hidden_states):
    """[n_layers + 1, B, D]: every state's CLS rows"""
    return torch.stack([h[:, 0, :] for h in hidden_states], dim=0)


def triplet_sum(anchor, pos, neg, margin=1.0, eps=1e-6):
    """sum_b max(margin + ||a_b - p_b + eps||_2 - ||a_b - n_b + eps||_2, 0): the triplet margin loss with p = 2, summed"""
    d_pos = ((anchor - pos + eps) ** 2).sum(dim=1).sqrt()
    d_neg = ((anchor - neg + eps) ** 2).sum(dim=1).sqrt()
    return torch.clamp_min(margin + d_pos - d_neg, 0).sum()


def inbatch_xent(q, c):
    """s = q c^T; -> (sum_i (logsumexp_j s_ij - s_ii), the rows' logsumexp [B])"""
    s = q @ c.t()
    lse = torch.logsumexp(s, dim=1)
    return (lse - torch.diagonal(s)).sum(), lse
