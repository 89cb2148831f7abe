"""The reference trainer's two update rules (src/learning/trainer.py:178-181: ``optim.Adam`` / ``optim.Adagrad`` at torch's defaults) on
this library's multi-tensor kernel (optim.hip): ONE launch per ``step()`` over every tensor, of every param group, that has a gradient.
Beyond the reference: AdamW and clipping of the global gradient norm, inside the same launch.

``HipAdam`` / ``HipAdagrad`` are ``torch.optim.Optimizer`` subclasses: torch's and transformers' schedulers drive
``param_groups[...]['lr']`` as they drive torch's optimizers, and the state keeps torch's keys and layouts -- ``'step'`` a CPU float32
scalar tensor, ``'exp_avg'`` / ``'exp_avg_sq'`` (Adam), ``'sum'`` (Adagrad) -- and the param groups carry every key of the installed
torch's optimizer, so ``state_dict()`` / ``load_state_dict()`` go to and from ``torch.optim.Adam`` / ``Adagrad`` in both directions.

As in torch, the step count is per parameter: one with ``grad is None`` (or ``requires_grad=False``) is skipped, its step does not
advance, and its state is created when it first has a gradient.  The arithmetic is torch's single-tensor formulas in fp32
(include/aspire_hip.h states them).

``HipAdamW`` is ``torch.optim.AdamW`` on the same launch: decoupled decay, ``p *= 1 - lr * weight_decay`` in front of Adam's update, with
``lr`` and ``weight_decay`` per tensor in the table, so param groups that differ in them alone (``decay_groups``) stay ONE launch.
``step(closure=None, grad_scale=None)`` on all three: ``grad_scale`` is a one-element fp32 GPU tensor by which every gradient is
multiplied as the kernel loads it (``.grad`` is left as it is) -- the clip coefficient of ``grad_norm(parameters, max_norm)``, which
leaves the global L2 norm and torch's coefficient on the GPU without a host synchronisation (grad_norm.hip).  ``clip_grad_norm_`` is
torch's in-place form: the norm, then one launch that multiplies every gradient.

Failing loudly: a sparse gradient or a parameter / gradient that is not on the GPU raises RuntimeError, not fp32 TypeError, not contiguous
ValueError; ``weight_decay != 0`` (coupled L2 decay: ``HipAdam`` / ``HipAdagrad``), ``amsgrad``, ``maximize``, ``capturable``, ``differentiable``, a tensor ``lr`` and (Adagrad)
``initial_accumulator_value != 0`` raise NotImplementedError -- at construction, and again at ``step()`` for values that arrived through
``load_state_dict`` or a param group edited by hand.  ``foreach`` / ``fused`` in a loaded group are torch's choice among ITS
implementations and are ignored.  ``step(closure)`` evaluates the closure once, with grad enabled, before the update (torch's pattern).

Host cost.  With 199 tensors the Python around the launch decides the step's time, not the kernel, so ``step()``
keeps a plan per set of parameters that have a gradient -- the checks, the state tensors and the table's static columns once; every
address is read again each step -- and every ``state['step']`` is a 0-dim view into one CPU float32 tensor, advanced by one operation.
"""
import operator

import numpy as np
import torch

from . import ops

_UNBUILT = ('amsgrad', 'maximize', 'capturable', 'differentiable')


class _HipOptimizer(torch.optim.Optimizer):
    _torch_class = None
    _state_keys = ()
    _decoupled_decay = False        # HipAdamW: weight_decay is built, as a per-tensor column of the table

    def __init__(self, params, **hyper):
        params = list(params)
        # the installed torch's own defaults dict: every key its step() reads is then in every group of a state dict saved here
        template = self._torch_class([torch.zeros(1)], **{k: v for k, v in hyper.items() if k != 'lr'}, lr=1.0)
        defaults = dict(template.defaults)
        defaults['lr'] = hyper['lr']
        self._refuse(defaults)
        if hyper['lr'] < 0.0:
            raise ValueError(f'Invalid learning rate: {hyper["lr"]}')
        self._plans, self._step_base, self._slot = {}, None, {}
        super().__init__(params, defaults)

    def _refuse(self, group):
        name = type(self).__name__
        if isinstance(group['lr'], torch.Tensor):
            raise NotImplementedError(f'{name}: a tensor lr is not built (the kernel takes its scalars from the host)')
        if isinstance(group.get('weight_decay', 0), torch.Tensor):
            raise NotImplementedError(f'{name}: a tensor weight_decay is not built')
        if group.get('weight_decay', 0) != 0 and not self._decoupled_decay:
            raise NotImplementedError(f'{name}: coupled (L2) weight_decay is not built; HipAdamW has the decoupled one')
        for key in _UNBUILT:
            if group.get(key, False):
                raise NotImplementedError(f'{name}: {key} is not built')
        if group.get('initial_accumulator_value', 0) != 0:
            raise NotImplementedError(f'{name}: initial_accumulator_value is not built')

    # ---- the step.  What does not change from step to step -- which tensors take part, their checks, the table's static columns -- is
    # a plan, kept per set of parameters that have a gradient (the pooler never has one under RankLoss; a lagging parameter alternates
    # between two sets) and dropped whenever the groups or the state may have changed under it.  Every address is read again each step.
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._refuse(self.param_groups[-1])
        self._plans = {}
        self._step_base = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():      # torch's layout for the steps of a non-fused, non-capturable optimizer
            if 'step' in st:
                st['step'] = torch.as_tensor(st['step']).detach().to(device='cpu', dtype=torch.float32).reshape(())
        self._plans = {}
        self._home_steps()

    def _home_steps(self):
        """Every state['step'] is a CPU float32 scalar tensor, torch's layout -- here a 0-dim view into ONE tensor with a slot per
        parameter, so that a step advances all its counts with one host operation instead of one per tensor."""
        params = [p for group in self.param_groups for p in group['params']]
        base = torch.zeros(max(len(params), 1), dtype=torch.float32)
        for i, p in enumerate(params):
            st = self.state[p] if p in self.state else None
            if st and 'step' in st:
                base[i] = float(st['step'])
                st['step'] = base[i]
        self._step_base, self._slot = base, {p: i for i, p in enumerate(params)}

    def _plan(self, sig, entries):
        """entries: (parameter, group index) of every parameter with a gradient -> the launches, one per (device, call-wide scalars)"""
        name = type(self).__name__
        launches = {}
        for p, gi in entries:
            ops.optim_tensor_check(p, f'{name}: a parameter')
            state = self.state[p]
            if self._step_base is None or p not in self._slot:
                self._home_steps()
            slot = self._step_base[self._slot[p]]
            if len(state) == 0:
                state['step'] = slot
                for key in self._state_keys:
                    state[key] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            for key in self._state_keys:
                ops.optim_tensor_check(state[key], f'{name}: state {key!r}')
                if state[key].shape != p.shape or state[key].device != p.device:
                    raise ValueError(f'{name}: state {key!r} of shape {tuple(state[key].shape)} on {state[key].device} for a parameter '
                                     f'of shape {tuple(p.shape)} on {p.device}')
            if state['step'].data_ptr() != slot.data_ptr():         # replaced by hand
                slot.fill_(float(state['step']))
                state['step'] = slot
            key = (p.device, self._call_scalars(self.param_groups[gi]))
            launches.setdefault(key, []).append((p, gi, state))
        plan = []
        for (dev, scalars), items in launches.items():
            table = np.zeros(len(items), dtype=ops.ADAMW_TABLE if self._decoupled_decay else ops.OPTIM_TABLE)
            table['n'] = [p.numel() for p, _, _ in items]
            plan.append(dict(dev=dev, scalars=scalars, table=table, params=[p for p, _, _ in items],
                             slots=np.array([self._slot[p] for p, _, _ in items]),
                             group=np.array([gi for _, gi, _ in items]), group_ids=sorted({gi for _, gi, _ in items}),
                             state_dicts=[st for _, _, st in items], steps=[st['step'] for _, _, st in items],
                             states=[[st[key] for _, _, st in items] for key in self._state_keys]))
        return plan

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        """grad_scale: a one-element fp32 GPU tensor (grad_norm()'s clip_coef): the update runs on every gradient times it, in the same
        one launch; .grad is left as it is."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = type(self).__name__
        groups = self.param_groups
        for group in groups:
            self._refuse(group)
        entries = [(p, gi) for gi, group in enumerate(groups) for p in group['params'] if p.grad is not None]
        if not entries:
            return loss
        sig = tuple([id(p) for p, _ in entries])
        plan = self._plans.get(sig)
        if plan is not None:
            for launch in plan:     # a group's betas / eps edited by hand, a state entry replaced by hand: plan again
                sds = launch['state_dicts']
                if any(self._call_scalars(groups[gi]) != launch['scalars'] for gi in launch['group_ids']) or not all(
                        all(map(operator.is_, [st.get(key) for st in sds], cached))
                        for key, cached in zip(('step',) + self._state_keys, [launch['steps']] + launch['states'])):
                    plan = None
                    break
        if plan is None:
            if len(self._plans) >= 16:
                self._plans = {}
            plan = self._plans[sig] = self._plan(sig, entries)
        lr_of_group = np.array([float(group['lr']) for group in groups])
        if self._decoupled_decay:
            decay_of_group = np.array([float(group['weight_decay']) for group in groups])
        for launch in plan:
            params = launch['params']
            grads = [p.grad for p in params]
            for g in grads:
                if g.layout is not torch.strided or g.dtype is not torch.float32 or not g.is_cuda or not g.is_contiguous():
                    ops.optim_tensor_check(g, f'{name}: a gradient')
            table = launch['table']
            table['param'] = [p.data_ptr() for p in params]
            table['grad'] = [g.data_ptr() for g in grads]
            for col, tensors in zip(('state1', 'state2'), launch['states']):
                table[col] = [t.data_ptr() for t in tensors]
            counts = self._step_base.numpy()       # (shares the tensor's memory: every state['step'] is a view of it)
            table['step'] = counts[launch['slots']] + 1.0
            table['lr'] = lr_of_group[launch['group']]
            if self._decoupled_decay:
                table['weight_decay'] = decay_of_group[launch['group']]
            if grad_scale is None:
                ops.optim_launch(self._rule, table, launch['scalars'], launch['dev'])
            else:
                ops.optim_launch(self._rule, table, launch['scalars'], launch['dev'], grad_scale)
            counts[launch['slots']] += 1.0          # (behind the call: an argument error leaves the counts alone)
        return loss


class HipAdam(_HipOptimizer):
    """torch.optim.Adam(params, lr, betas, eps) without weight decay / amsgrad, one HIP launch per step()."""
    _torch_class = torch.optim.Adam
    _state_keys = ('exp_avg', 'exp_avg_sq')
    _rule = 'adam'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)

    @staticmethod
    def _call_scalars(group):
        return float(group['betas'][0]), float(group['betas'][1]), float(group['eps'])


class HipAdamW(_HipOptimizer):
    """torch.optim.AdamW(params, lr, betas, eps, weight_decay) without amsgrad, one HIP launch per step(): decoupled decay
    p *= 1 - lr * weight_decay in front of Adam's update, lr and weight_decay per tensor in the table -- param groups that differ in
    them alone (decay_groups) share the launch.  torch's state keys; with weight_decay=0 the bits are HipAdam's."""
    _torch_class = torch.optim.AdamW
    _state_keys = ('exp_avg', 'exp_avg_sq')
    _rule = 'adamw'
    _decoupled_decay = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)

    _call_scalars = staticmethod(HipAdam._call_scalars)


class HipAdagrad(_HipOptimizer):
    """torch.optim.Adagrad(params, lr, lr_decay, eps) without weight decay / initial accumulator value, one HIP launch per step()."""
    _torch_class = torch.optim.Adagrad
    _state_keys = ('sum',)
    _rule = 'adagrad'

    def __init__(self, params, lr=1e-2, lr_decay=0, eps=1e-10, weight_decay=0, initial_accumulator_value=0, **kw):
        super().__init__(params, lr=lr, lr_decay=lr_decay, eps=eps, weight_decay=weight_decay,
                         initial_accumulator_value=initial_accumulator_value, **kw)

    @staticmethod
    def _call_scalars(group):
        return float(group['lr_decay']), float(group['eps'])


# ---- the global gradient norm and its clip (grad_norm.hip) ----------------------------------------------------------------------------------
def _grads_of(parameters):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    return [p.grad for p in parameters if p.grad is not None]


def grad_norm(parameters, max_norm):
    """-> (total_norm, clip_coef): 0-dim views of ONE two-element fp32 GPU tensor -- the L2 norm of every ``p.grad`` viewed as one vector
    and torch's coefficient clamp(max_norm / (total_norm + 1e-6), max=1), in two launches with no host synchronisation.  For the fused
    route: ``optimizer.step(grad_scale=clip_coef)`` applies the clip as the step loads each gradient.  The sum of squares is formed in
    double, so the norm stays finite where torch's fp32 sum overflows (include/aspire_hip.h)."""
    out = ops.grad_norm(_grads_of(parameters), max_norm)
    return out[0], out[1]


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ on this library's kernels: the norm (two launches) and ONE multi-tensor launch that multiplies
    every gradient in place by the coefficient -- by 1.0 too, as torch does.  Returns the total norm as a GPU tensor.  Only the L2 norm
    is built; the gradients must be what optim_tensor_check takes.  `foreach` is torch's choice among ITS implementations: ignored."""
    if float(norm_type) != 2.0:
        raise NotImplementedError(f'clip_grad_norm_: norm_type = {norm_type} is not built (only the L2 norm is)')
    grads = _grads_of(parameters)
    out = ops.grad_norm(grads, max_norm)
    if error_if_nonfinite and not bool(torch.isfinite(out[0])):
        raise RuntimeError('The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be clipped.')
    ops.grad_scale_(grads, out[1:])
    return out[0]


def decay_groups(module, weight_decay):
    """The usual two param groups of a BERT fine-tuning recipe: [{'params': ..., 'weight_decay': weight_decay}, {'params': ...,
    'weight_decay': 0.0}] -- no decay for parameters whose name ends in 'bias' and for the weights of LayerNorm modules (a
    torch.nn.LayerNorm, or HuggingFace's naming, '...LayerNorm.weight').  An empty group is left out."""
    norm_weights = {id(p) for m in module.modules() if isinstance(m, torch.nn.LayerNorm) for p in m.parameters(recurse=False)}
    decay, no_decay = [], []
    for name, p in module.named_parameters():
        plain = name.endswith('bias') or id(p) in norm_weights or 'LayerNorm' in name
        (no_decay if plain else decay).append(p)
    groups = [{'params': decay, 'weight_decay': float(weight_decay)}, {'params': no_decay, 'weight_decay': 0.0}]
    return [g for g in groups if g['params']]
