"""The yardstick of the clipping / AdamW tests: the global gradient norm, torch's clip coefficient and torch's single-tensor AdamW
restated in numpy (float64 as the reference), step-major -- the clip couples every tensor of a step -- over the parameter set of
tests/optim_ref.py: element counts 1 .. 2 CHUNK + 5, a view at storage offset 1, a lagging and a frozen parameter, gradients spread over
1e-20 .. 1e2; two param groups with different lr AND different weight decay.
"""
import math

import numpy as np
import torch

import optim_ref as orf

WEIGHT_DECAYS = (0.01, 0.1)         # per group
MAX_NORM = 1.0                      # bites at every step: the spread tensors alone carry a norm in the thousands
ADAMW = dict(betas=(0.9, 0.999), eps=1e-8)
STATE_KEYS = dict(orf.STATE_KEYS, adamw=('exp_avg', 'exp_avg_sq'))


def total_norm(grads):
    """float64: sqrt of the sum of every element's square (None entries stay out)"""
    return math.sqrt(sum(float(np.sum(np.square(g.astype(np.float64)))) for g in grads if g is not None))


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grads_with_norm_: min(max_norm / (norm + 1e-6), 1), here in float64"""
    return min(max_norm / (norm + 1e-6), 1.0)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def adamw_update(p, m, v, g, t, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8):
    """torch/optim/adam.py _single_tensor_adam with decoupled_weight_decay=True: param.mul_(1 - lr * weight_decay), then Adam"""
    p = p * p.dtype.type(1 - lr * weight_decay)
    return orf.adam_update(p, m, v, g, t, lr, betas, eps)


def run_reference(rule, max_norm=None, steps=orf.STEPS, dtype=np.float64, weight_decays=WEIGHT_DECAYS):
    """-> {name: dict(p, step, state...)} after `steps` global steps; with max_norm every step's gradients are multiplied by the step's
    clip coefficient first.  The lr of global step k (from 1) is lr0 gamma^(k - 1), as in optim_ref.run_reference."""
    specs = orf.case_specs()
    st = {s['name']: dict(p=orf.init_value(s).astype(dtype), s1=np.zeros(s['shape'], dtype), s2=np.zeros(s['shape'], dtype), t=0) for s in specs}
    with np.errstate(all='ignore'):
        for k in range(1, steps + 1):
            grads = {s['name']: orf.grad_value(s, k) for s in specs}
            coef = 1.0 if max_norm is None else clip_coef(total_norm(list(grads.values())), max_norm)
            for s in specs:
                g = grads[s['name']]
                if g is None:
                    continue
                e = st[s['name']]
                e['t'] += 1
                g = g.astype(dtype) * dtype(coef)
                lr = orf.LRS[s['group']] * orf.GAMMA ** (k - 1)
                if rule == 'adamw':
                    e['p'], e['s1'], e['s2'] = adamw_update(e['p'], e['s1'], e['s2'], g, e['t'], lr, weight_decays[s['group']], **ADAMW)
                elif rule == 'adam':
                    e['p'], e['s1'], e['s2'] = orf.adam_update(e['p'], e['s1'], e['s2'], g, e['t'], lr, **orf.ADAM)
                else:
                    e['p'], e['s1'] = orf.adagrad_update(e['p'], e['s1'], g, e['t'], lr, **orf.ADAGRAD)
    keys = STATE_KEYS[rule]
    return {n: dict(p=e['p'], step=e['t'], **dict(zip(keys, (e['s1'], e['s2'])))) for n, e in st.items()}


def groups(run, weight_decays=WEIGHT_DECAYS):
    """optim_ref.Run's two groups, each with its own weight decay"""
    return [dict(g, weight_decay=wd) for g, wd in zip(run.groups(), weight_decays)]


def drive(run, opt, n, update, gamma=orf.GAMMA):
    """n more global steps: the case's gradients into .grad, then update(opt, run.params) -- the clip and the step, however the
    caller pairs them -- then an ExponentialLR(gamma) step, as optim_ref.Run.steps does"""
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=gamma)
    for _ in range(n):
        run.done += 1
        for p, spec in zip(run.params, run.specs):
            g = run.grads(spec, run.done)
            p.grad = None if g is None else torch.from_numpy(g).to(run.device)
        update(opt, run.params)
        sched.step()
    return run


def result(run, opt, rule):
    out = {}
    for p, spec in zip(run.params, run.specs):
        st = opt.state.get(p, {})
        d = dict(p=p.detach().cpu().numpy(), step=int(st['step']) if 'step' in st else 0)
        for key in STATE_KEYS[rule]:
            d[key] = st[key].detach().cpu().numpy() if key in st else np.zeros(spec['shape'], np.float32)
        out[spec['name']] = d
    return out


def compare(got, ref64, torch32, rule, tag, report=print):
    """optim_ref.compare with this module's state keys: every tensor inside bound(|torch32 - ref64|, max|ref64|) of ref64"""
    worst, bad = 0.0, []
    for name in ref64:
        for key in ('p',) + STATE_KEYS[rule]:
            r = ref64[name][key]
            err = float(np.abs(got[name][key].astype(np.float64) - r).max())
            tol = orf.bound(np.abs(torch32[name][key].astype(np.float64) - r).max(), np.abs(r).max())
            report(f'[{tag}] {name:9s} {key:10s} |got - float64| {err:.3e}  bound {tol:.3e}')
            worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else math.inf))
            if not err <= tol:
                bad.append((name, key, err, tol))
    assert not bad, bad
    return worst


def torch_cpu(rule, max_norm=None, steps=orf.STEPS):
    """torch's side of the bound: torch.optim (foreach=False) and torch.nn.utils.clip_grad_norm_ in fp32 on the CPU"""
    run = orf.Run('cpu')
    if rule == 'adamw':
        opt = torch.optim.AdamW(groups(run), foreach=False, **ADAMW)
    elif rule == 'adam':
        opt = torch.optim.Adam(run.groups(), foreach=False, **orf.ADAM)
    else:
        opt = torch.optim.Adagrad(run.groups(), foreach=False, **orf.ADAGRAD)

    def update(opt, params):
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
        opt.step()

    return result(drive(run, opt, steps, update), opt, rule)
