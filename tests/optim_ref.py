"""The yardstick of the optimizer tests: torch's single-tensor Adam / Adagrad formulas restated in numpy with PER-TENSOR step counts
(float64 as the reference, float32 to show what the formulas' own rounding costs), and the one parameter set all of them run on.

The case is chosen for where a multi-tensor kernel can go wrong, not for size (CHUNK = the kernel's chunk, tuning.h's kOptimChunk):
element counts 1, 3, 7, 768, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 5 and a (5, 768) matrix whose every second gradient row is exactly
zero; a contiguous view at storage offset 1 (4-byte aligned pointers only); a parameter whose grad is None on even steps; a frozen one;
two tensors whose gradient magnitudes spread over 1e-20 .. 1e2 per element; two param groups with different lr, an ExponentialLR
between the steps.
"""
import math

import numpy as np
import torch

CHUNK = 4096
GAMMA = 0.9
LRS = (1e-2, 3e-3)
STEPS = 6
ADAM = dict(betas=(0.9, 0.999), eps=1e-8)
ADAGRAD = dict(lr_decay=0.0, eps=1e-10)


def case_specs(chunk=CHUNK):
    """name, shape, flags; the group is the index's parity"""
    specs = [dict(name=f'n{n}', shape=(n,)) for n in (1, 3, 7, 768, chunk - 1, chunk, chunk + 1, 2 * chunk + 5)]
    specs.append(dict(name='rows', shape=(5, 768), zero_rows=True))
    specs.append(dict(name='offset1', shape=(chunk + 7,), offset1=True))
    specs.append(dict(name='lagging', shape=(770,), none_on_even=True))
    specs.append(dict(name='frozen', shape=(33,), frozen=True))
    specs.append(dict(name='spread_a', shape=(1501,), spread=True))
    specs.append(dict(name='spread_b', shape=(chunk + 3,), spread=True))
    for i, s in enumerate(specs):
        s['index'], s['group'] = i, i % 2
    return specs


def init_value(spec):
    rng = np.random.default_rng(1000 + spec['index'])
    return rng.standard_normal(spec['shape']).astype(np.float32)


def grad_value(spec, step):
    """the gradient of 1-based global step `step` (float32), or None where the parameter has none at that step"""
    if spec.get('frozen') or (spec.get('none_on_even') and step % 2 == 0):
        return None
    rng = np.random.default_rng(7919 * step + spec['index'])
    g = rng.standard_normal(spec['shape'])
    if spec.get('spread'):
        g = g * 10.0 ** rng.uniform(-20.0, 2.0, spec['shape'])
    g = g.astype(np.float32)
    if spec.get('zero_rows'):
        g[1::2] = 0.0
    return g


# ---- the formulas (torch/optim/adam.py _single_tensor_adam, torch/optim/adagrad.py _single_tensor_adagrad) -----------------------------
def adam_update(p, m, v, g, t, lr, betas=(0.9, 0.999), eps=1e-8):
    """arrays of one dtype (float64: the reference; float32: the formulas' own rounding); t: this tensor's step, from 1; returns new p, m, v"""
    ft = p.dtype.type
    b1, b2 = betas
    m = m + (g - m) * ft(1 - b1)
    v = v * ft(b2) + g * g * ft(1 - b2)
    step_size = ft(lr / (1 - b1 ** t))
    bc2_sqrt = ft(math.sqrt(1 - b2 ** t))
    p = p - step_size * (m / (np.sqrt(v) / bc2_sqrt + ft(eps)))
    return p, m, v


def adagrad_update(p, s, g, t, lr, lr_decay=0.0, eps=1e-10):
    ft = p.dtype.type
    s = s + g * g
    clr = ft(lr / (1 + (t - 1) * lr_decay))
    p = p - clr * (g / (np.sqrt(s) + ft(eps)))
    return p, s


def run_reference(rule, dtype=np.float64, steps=STEPS, specs=None, grads=None, lrs=LRS, gamma=GAMMA, hyper=None):
    """-> {name: dict(p, step, exp_avg, exp_avg_sq | sum)} after `steps` steps; the lr of global step k (from 1) is lr0 gamma^(k - 1).
    grads(spec, step) replaces grad_value."""
    specs = specs or case_specs()
    grads = grads or grad_value
    hyper = hyper or (ADAM if rule == 'adam' else ADAGRAD)
    out = {}
    for spec in specs:
        p = init_value(spec).astype(dtype)
        s1, s2, t = np.zeros_like(p), np.zeros_like(p), 0
        with np.errstate(all='ignore'):
            for k in range(1, steps + 1):
                g = grads(spec, k)
                if g is None:
                    continue
                t += 1
                lr = lrs[spec['group']] * gamma ** (k - 1)
                if rule == 'adam':
                    p, s1, s2 = adam_update(p, s1, s2, g.astype(dtype), t, lr, **hyper)
                else:
                    p, s1 = adagrad_update(p, s1, g.astype(dtype), t, lr, **hyper)
        out[spec['name']] = dict(p=p, step=t, **({'exp_avg': s1, 'exp_avg_sq': s2} if rule == 'adam' else {'sum': s1}))
    return out


STATE_KEYS = {'adam': ('exp_avg', 'exp_avg_sq'), 'adagrad': ('sum',)}


# ---- the same case through a torch.optim.Optimizer ----------------------------------------------------------------------------------------
class Run:
    """The case's parameters as torch leaves on `device`, and the loop that feeds an optimizer the case's gradients."""

    def __init__(self, device, specs=None, grads=None):
        self.specs = specs or case_specs()
        self.grads = grads or grad_value
        self.device = torch.device(device)
        self.params = []
        for spec in self.specs:
            v = torch.from_numpy(init_value(spec))
            if spec.get('offset1'):
                base = torch.zeros(v.numel() + 1, device=self.device)
                p = base[1:].view(v.shape).detach()
                p.copy_(v)
                assert p.storage_offset() == 1 and p.is_contiguous()
            else:
                p = v.to(self.device).clone()
            p.requires_grad_(not spec.get('frozen', False))
            self.params.append(p)
        self.done = 0       # global steps taken

    def groups(self, lrs=LRS):
        return [{'params': [p for p, s in zip(self.params, self.specs) if s['group'] == g], 'lr': lrs[g]} for g in (0, 1)]

    def steps(self, opt, n, gamma=GAMMA):
        """n more global steps on `opt`, an ExponentialLR(gamma) stepping between them (continuing a loaded optimizer's lr)"""
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=gamma)
        for _ in range(n):
            self.done += 1
            for p, spec in zip(self.params, self.specs):
                g = self.grads(spec, self.done)
                p.grad = None if g is None else torch.from_numpy(g).to(self.device)
            opt.step()
            sched.step()
        return self

    def result(self, opt, rule):
        out = {}
        for p, spec in zip(self.params, self.specs):
            st = opt.state.get(p, {})
            d = dict(p=p.detach().cpu().numpy(), step=int(st['step']) if 'step' in st else 0)
            for key in STATE_KEYS[rule]:
                d[key] = st[key].detach().cpu().numpy() if key in st else np.zeros(spec['shape'], np.float32)
            out[spec['name']] = d
        return out


def bound(ref_err, max_ref):
    """the project's parity rule (tests/golden/trainside_inputs.bound): four times the reference arithmetic's own fp32 error, and never
    less than four fp32 roundings of the largest entry"""
    return max(4.0 * float(ref_err), 4.0 * 2.0 ** -23 * float(max_ref))


def compare(got, ref64, torch32, rule, tag, report=print):
    """every tensor of `got` inside bound(|torch32 - ref64|, max|ref64|) of ref64; prints each figure before it asserts.
    -> the largest error / bound"""
    worst, bad = 0.0, []
    for name in ref64:
        for key in ('p',) + STATE_KEYS[rule]:
            r = ref64[name][key]
            err = float(np.abs(got[name][key].astype(np.float64) - r).max())
            tol = bound(np.abs(torch32[name][key].astype(np.float64) - r).max(), np.abs(r).max())
            report(f'[{tag}] {name:9s} {key:10s} |got - float64| {err:.3e}  bound {tol:.3e}')
            worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else math.inf))
            if not err <= tol:
                bad.append((name, key, err, tol))
    assert not bad, bad
    return worst
