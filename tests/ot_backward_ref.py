"""The yardstick of the otAspire backward (tests/test_ot_backward_cpu.py, tests/test_gpu_ot_backward.py): torch on the CPU.

`restated_distance` is the reference's AllPairMaskedWasserstein.compute_distance (pair_distances.py:21-60, 88-92) with geomloss
0.2.4's sinkhorn_tensorized for SamplesLoss("sinkhorn", p=1, debias=False, potentials=False) RESTATED with the detach pattern that
package's source is read to have -- geomloss is not available here, the Sinkhorn oracle is "parity unpinned" (oracle/aspire_oracle.py),
and so is this gradient:
    C_xy = cost(x, y.detach()), C_yx = cost(y, x.detach()); the whole eps-scaling loop under no_grad; the last extrapolation with grad
    on (a_log + b_x / eps).detach() and (b_log + a_y / eps).detach(); the value <a, b_x> + <b, a_y> with the soft-max marginals a, b
    attached; max_diameter an .item().
It reuses the oracle's _softmin, _log_weights, epsilon_schedule and max_diameter.  Two cost formulas: geomloss's matmul expansion
(the float64 yardstick) and direct differences (the fp32 run that gives the scale of fp32 rounding: in fp32 the expansion is noise
where two rows nearly coincide).

`closed_form_grads` is the formula sheet of include/aspire_hip.h (aspire_ot_backward_f32) evaluated with torch, no autograd."""
import torch

from oracle import aspire_oracle as orc


def _pad_mask(qlens, clens, sq, sc, dtype):
    mask = torch.full((len(qlens), sq, sc), -10e8, dtype=dtype)
    for i, (ql, cl) in enumerate(zip(qlens, clens)):
        mask[i, :ql, :cl] = 0.0
    return mask


def _cost(x, y, direct):
    if not direct:
        return orc._distances(x, y)             # sqrt(clamp_min(|x|^2 - 2 x.y + |y|^2, 1e-8))
    diff = x.unsqueeze(2) - y.unsqueeze(1)
    return torch.sqrt(torch.clamp_min((diff * diff).sum(-1), 1e-8))


def _neg_cdist(x, y, direct):
    return -1 * torch.cdist(x, y, compute_mode='donot_use_mm_for_euclid_dist' if direct else 'use_mm_for_euclid_dist_if_necessary')


def _solve(c_xy, c_yx, a_log, b_log, eps_s):
    """geomloss sinkhorn_loop up to the last averaged step: (f0, g0) -- call under no_grad"""
    eps = eps_s[0]
    g = orc._softmin(eps, c_yx, a_log)
    f = orc._softmin(eps, c_xy, b_log)
    for eps in eps_s:
        gt = orc._softmin(eps, c_yx, a_log + f / eps)
        ft = orc._softmin(eps, c_xy, b_log + g / eps)
        g, f = 0.5 * (g + gt), 0.5 * (f + ft)
    return f, g


def restated_distance(x, y, qlens, clens, blur=0.05, scaling=0.9, temp=1.0, diameter=None, direct=False, parts=False):
    """x [B, Sq, 768], y [B, Sc, 768] (the reference's embeds after its permute), in x's dtype -> OT_eps [B], attached to x and y.
    diameter None: geomloss's max_diameter over the whole batch, pad rows included.  parts: also everything the closed formulas
    read (a dict)."""
    b, sq, _ = x.shape
    sc = y.shape[1]
    neg = _neg_cdist(x, y, direct) + _pad_mask(qlens, clens, sq, sc, x.dtype)
    a_w, b_w = orc.marginals(neg, temp)
    c_xy, c_yx = _cost(x, y.detach(), direct), _cost(y, x.detach(), direct)
    if diameter is None:
        diameter = orc.max_diameter(x.detach(), y.detach())
    eps_s = orc.epsilon_schedule(1, diameter, blur, scaling)
    eps = eps_s[-1]
    with torch.no_grad():
        a_log, b_log = orc._log_weights(a_w.detach().clone()), orc._log_weights(b_w.detach().clone())
        f0, g0 = _solve(c_xy, c_yx, a_log, b_log, eps_s)
    g = orc._softmin(eps, c_yx, (a_log + f0 / eps).detach())
    f = orc._softmin(eps, c_xy, (b_log + g0 / eps).detach())
    value = (a_w * f).sum(1) + (b_w * g).sum(1)
    if parts:
        return value, dict(neg=neg.detach(), a=a_w.detach(), b=b_w.detach(), la=a_log, lb=b_log, f0=f0, g0=g0, f=f.detach(), g=g.detach(),
                           c=c_xy.detach(), eps=eps)
    return value


def autograd_grads(x, y, qlens, clens, gs, dtype, direct, **kw):
    """(grad_x, grad_y) of sum(gs * restated_distance) in `dtype`"""
    x = x.to(dtype).clone().requires_grad_()
    y = y.to(dtype).clone().requires_grad_()
    (restated_distance(x, y, qlens, clens, direct=direct, **kw) * gs.to(dtype)).sum().backward()
    return x.grad, y.grad


def closed_form_grads(x, y, qlens, clens, gs, **kw):
    """The formulas of include/aspire_hip.h, pair by pair, from the restatement's own C, s, marginals and potentials (no autograd)."""
    with torch.no_grad():
        _, p = restated_distance(x, y, qlens, clens, parts=True, **kw)
        temp, eps = kw.get('temp', 1.0), p['eps']
        gx, gy = torch.zeros_like(x), torch.zeros_like(y)
        for n, (ql, cl) in enumerate(zip(qlens, clens)):
            s, c = p['neg'][n, :ql, :cl], p['c'][n, :ql, :cl]
            d = -s
            a, b, f, g = p['a'][n, :ql], p['b'][n, :cl], p['f'][n, :ql], p['g'][n, :cl]
            w = torch.exp(p['lb'][n, None, :cl] + (p['g0'][n, None, :cl] - c + f[:, None]) / eps)
            v = torch.exp(p['la'][n, :ql, None] + (p['f0'][n, :ql, None] - c + g[None, :]) / eps)
            u_i = a * (f - (a * f).sum()) / temp
            v_j = b * (g - (b * g).sum()) / temp
            m = torch.zeros_like(s)
            m[torch.arange(ql), first_argmax(s, 1)] += u_i
            m[first_argmax(s, 0), torch.arange(cl)] += v_j
            on_c = (d * d > 1e-8).to(x.dtype) / c
            on_d = torch.where(d > 0, m / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(d))
            diff = x[n, :ql, None, :] - y[n, None, :cl, :]
            gx[n, :ql] = gs[n] * ((a[:, None] * w * on_c - on_d)[:, :, None] * diff).sum(1)
            gy[n, :cl] = gs[n] * ((on_d - b[None, :] * v * on_c)[:, :, None] * diff).sum(0)
    return gx, gy


def first_argmax(s, dim):
    """index of the FIRST largest entry along `dim` of a 2-D block"""
    best = s.max(dim=dim, keepdim=True)[0]
    n = s.shape[dim]
    idx = torch.arange(n).view(-1, 1) if dim == 0 else torch.arange(n).view(1, -1)
    return torch.where(s == best, idx, torch.full_like(idx, n)).min(dim=dim)[0]


def pick_margins(x, y, qlens, clens):
    """float64: the smallest gap between the best and the second-best entry of s = -cdist over every valid row and column that has
    two entries (inf when none has) -- how far the arg-max picks j*(i), i*(j) are from flipping."""
    gap = float('inf')
    d = torch.cdist(x.double(), y.double(), compute_mode='donot_use_mm_for_euclid_dist')
    for n, (ql, cl) in enumerate(zip(qlens, clens)):
        blk = d[n, :ql, :cl]
        for lines in (blk, blk.t()):
            if lines.shape[1] >= 2:
                two = torch.topk(lines, 2, dim=1, largest=False)[0]
                gap = min(gap, (two[:, 1] - two[:, 0]).min().item())
    return gap


def valid_dev(got_x, got_y, want_x, want_y, qlens, clens):
    """largest |got - want| over the valid rows"""
    dev = 0.0
    for n, (ql, cl) in enumerate(zip(qlens, clens)):
        dev = max(dev, (got_x[n, :ql].double() - want_x[n, :ql].double()).abs().max().item(),
                  (got_y[n, :cl].double() - want_y[n, :cl].double()).abs().max().item())
    return dev
