"""GPU: the multi-tensor optimizer step (optim.hip: aspire_adam_step_f32 / aspire_adagrad_step_f32) behind aspire_amd.HipAdam /
HipAdagrad and ops.adam_step / ops.adagrad_step.

Yardstick: tests/optim_ref.py -- torch's single-tensor formulas in float64 numpy with per-tensor steps -- and the project's parity rule:
per tensor, max |kernel - float64| <= max(4 |torch fp32 (CPU, foreach=False) - float64|, 4 * 2^-23 max |float64|).  tests/test_optim_cpu.py
shows that a plain fp32 restatement reaches at most 0.29 of that bound on this case.  Every comparison prints its figures before it
asserts (pytest -s shows them).  On an MI355X the largest |kernel - float64| / bound over the 14 tensors is 0.288 for Adam and 0.241 for
Adagrad: the figures of the fp32 numpy restatement.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as orf  # noqa: E402

pytestmark = pytest.mark.gpu
RULES = ['adam', 'adagrad']


def _hip(rule, groups):
    from aspire_amd import HipAdam, HipAdagrad
    return HipAdam(groups, **orf.ADAM) if rule == 'adam' else HipAdagrad(groups, **orf.ADAGRAD)


def _torch(rule, groups, **kw):
    return torch.optim.Adam(groups, **orf.ADAM, **kw) if rule == 'adam' else torch.optim.Adagrad(groups, **orf.ADAGRAD, **kw)


@functools.lru_cache(maxsize=None)
def _ref64(rule):
    return orf.run_reference(rule)


@functools.lru_cache(maxsize=None)
def _torch32(rule):
    run = orf.Run('cpu')
    opt = _torch(rule, run.groups(), foreach=False)
    return run.steps(opt, orf.STEPS).result(opt, rule)


def _hip_run(rule, steps=orf.STEPS):
    run = orf.Run('cuda')
    opt = _hip(rule, run.groups())
    run.steps(opt, steps)
    return run, opt


@pytest.mark.parametrize('rule', RULES)
def test_six_steps_match_float64(rule, monkeypatch):
    from aspire_amd import ops
    calls = []
    inner = ops.optim_launch
    monkeypatch.setattr(ops, 'optim_launch', lambda r, table, *a: (calls.append((r, len(table))), inner(r, table, *a))[1])
    run, opt = _hip_run(rule)
    got = run.result(opt, rule)
    worst = orf.compare(got, _ref64(rule), _torch32(rule), rule, f'Hip{rule}')
    print(f'largest error / bound: {worst:.3f}')
    # one launch per step() over both groups' tensors that have a gradient: 13 on odd steps, 12 on even ones (the lagging parameter)
    assert calls == [(rule, 13), (rule, 12)] * 3
    for p, spec in zip(run.params, run.specs):
        want = _torch32(rule)[spec['name']]['step']
        if spec.get('frozen'):
            assert p not in opt.state and want == 0
            assert np.array_equal(p.detach().cpu().numpy(), orf.init_value(spec))
            continue
        st = opt.state[p]
        assert st['step'].device.type == 'cpu' and st['step'].dtype == torch.float32 and st['step'].dim() == 0     # torch's layout
        assert int(st['step']) == want, spec['name']
        for key in orf.STATE_KEYS[rule]:
            assert st[key].shape == p.shape and st[key].is_cuda and st[key].dtype == torch.float32
    # rows whose gradient has always been zero: m = v = 0 (s = 0), and the parameter moved by exactly 0
    rows = got['rows']
    init = orf.init_value(next(s for s in run.specs if s['name'] == 'rows'))
    assert np.array_equal(rows['p'][1::2], init[1::2]) and not np.array_equal(rows['p'][0::2], init[0::2])
    for key in orf.STATE_KEYS[rule]:
        assert not rows[key][1::2].any() and rows[key][0::2].all()


@pytest.mark.parametrize('rule', RULES)
def test_first_step_leaves_frozen_and_zero_gradient_rows(rule):
    run, opt = _hip_run(rule, steps=1)
    got = run.result(opt, rule)
    for spec in run.specs:
        init, p = orf.init_value(spec), got[spec['name']]['p']
        if spec.get('frozen'):
            assert np.array_equal(p, init)
        elif spec.get('zero_rows'):
            assert np.array_equal(p[1::2], init[1::2]) and (p[0::2] != init[0::2]).all()
        else:
            # every tensor with a gradient moved, tails and all (a gradient below ~1e-13 is too small to move a parameter of size 1)
            assert (p != init).mean() > (0.5 if spec.get('spread') else 0.99), spec['name']
            assert p.flat[-1] != init.flat[-1] or spec.get('spread'), spec['name']


@pytest.mark.parametrize('rule', RULES)
def test_same_bits_twice(rule):
    a = _hip_run(rule)
    b = _hip_run(rule)
    ra, rb = a[0].result(a[1], rule), b[0].result(b[1], rule)
    for name in ra:
        for key in ('p',) + orf.STATE_KEYS[rule]:
            assert np.array_equal(ra[name][key].view(np.int32), rb[name][key].view(np.int32)), (name, key)


@pytest.mark.parametrize('rule', RULES)
def test_arena_bytes_outside_the_tensors_are_untouched(rule):
    """ops level: param, grad and state of every tensor are carved from ONE arena filled with a bit pattern, at starts that are 16-byte
    aligned for some tensors and 4-byte aligned only for others; after six steps every arena word outside the tensors, and every
    gradient word, holds what it held"""
    from aspire_amd import ops
    c = orf.CHUNK
    sizes = [1, 3, 7, 768, c - 1, c, c + 1, 2 * c + 5, 5 * 768, c + 7, 6, c + 2]
    shifts = [0] * 9 + [1, 2, 3]              # the last three: pointers off the 16-byte grid (all four, or the state alone below)
    n_arr = 4 if rule == 'adam' else 3
    PATTERN = 0x5A5AA5A5
    cursor, slots = 8, []
    for i, (n, shift) in enumerate(zip(sizes, shifts)):
        arrs = []
        for a in range(n_arr):
            start = (cursor + 3) // 4 * 4 + (shift if (i != len(sizes) - 1 or a == 2) else 0)
            arrs.append((start, n))
            cursor = start + n + 1 + (i + a) % 7
        slots.append(arrs)
    total = cursor + 8
    arena = torch.full((total,), PATTERN, dtype=torch.int32, device='cuda')
    fl = arena.view(torch.float32)
    inside = np.zeros(total, dtype=bool)
    gen = torch.Generator(device='cuda').manual_seed(4)
    views = []
    for arrs in slots:
        v = [fl[s:s + n] for s, n in arrs]
        for s, n in arrs:
            assert not inside[s:s + n].any()
            inside[s:s + n] = True
        v[0].copy_(torch.randn(v[0].shape, device='cuda', generator=gen))
        for state in v[2:]:
            state.zero_()
        views.append(v)
    assert (~inside).sum() > 8 * len(sizes)
    p0 = [v[0].clone() for v in views]
    for step in range(1, 7):
        for v in views:
            v[1].copy_(torch.randn(v[1].shape, device='cuda', generator=gen))
        grads_before = arena.clone()
        args = ([v[0] for v in views], [v[1] for v in views], [v[2] for v in views])
        steps, lrs = [step] * len(views), [1e-2 if i % 2 else 3e-3 for i in range(len(views))]
        if rule == 'adam':
            ops.adam_step(*args, [v[3] for v in views], steps, lrs)
        else:
            ops.adagrad_step(*args, steps, lrs)
        after = arena.cpu().numpy()
        assert (after[~inside] == PATTERN).all(), step
        before = grads_before.cpu().numpy()
        for arrs in slots:
            s, n = arrs[1]
            assert np.array_equal(after[s:s + n], before[s:s + n])
    for v, before in zip(views, p0):
        assert torch.isfinite(v[0]).all() and (v[0] != before).all()
        assert (v[2] != 0).all() and torch.isfinite(v[2]).all()


def test_alignment_does_not_change_the_bits():
    """the scalar path (pointers off the 16-byte grid) and the 16-byte path give the same bits for the same values"""
    from aspire_amd import ops
    n = 2 * orf.CHUNK + 7
    gen = torch.Generator(device='cuda').manual_seed(9)
    vals = [torch.randn(n, device='cuda', generator=gen) for _ in range(2)]
    outs = []
    for shift in (0, 1):
        t = [torch.zeros(n + 4, device='cuda')[shift:shift + n] for _ in range(4)]
        t[0].copy_(vals[0])
        t[1].copy_(vals[1])
        assert t[0].data_ptr() % 16 == 4 * shift
        for step in (1, 2):
            ops.adam_step([t[0]], [t[1]], [t[2]], [t[3]], [step], [1e-2])
        outs.append([x.clone() for x in t])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _bad_grad(spec, step):
    g = orf.grad_value(spec, step)
    if step == 2:
        for pos, val in spec['bad']:
            g[pos] = val
    return g


def test_non_finite_gradients_propagate_as_in_torch():
    c = orf.CHUNK
    nan, inf = float('nan'), float('inf')
    specs = [dict(name='big', shape=(c + 5,), index=0, group=0, bad=[(0, nan), (3, inf), (5, nan), (c, inf), (c + 1, nan), (c + 4, -inf)]),
             dict(name='small', shape=(7,), index=1, group=1, bad=[(6, inf)]),
             dict(name='clean', shape=(9,), index=2, group=0, bad=[])]
    results = []
    for make in (lambda groups: _hip('adam', groups), lambda groups: _torch('adam', groups)):
        run = orf.Run('cuda', specs=specs, grads=_bad_grad)
        opt = make(run.groups())
        run.steps(opt, 3)
        results.append(run.result(opt, 'adam'))
    hip, ref = results
    for spec in specs:
        want = sorted(pos for pos, _ in spec['bad'])
        for key in ('p', 'exp_avg', 'exp_avg_sq'):
            got_bad = np.flatnonzero(~np.isfinite(hip[spec['name']][key])).tolist()
            ref_bad = np.flatnonzero(~np.isfinite(ref[spec['name']][key])).tolist()
            print(f'{spec["name"]} {key}: non-finite at {got_bad} (torch: {ref_bad})')
            assert got_bad == ref_bad == want, (spec['name'], key)


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('direction', ['torch_to_hip', 'hip_to_torch'])
def test_state_dicts_are_interchangeable(rule, direction):
    """three steps on one implementation, load_state_dict into the other, three more: inside the bound against six float64 steps"""
    run = orf.Run('cuda')
    first, second = (_torch, _hip) if direction == 'torch_to_hip' else (_hip, _torch)
    a = first(rule, run.groups())
    run.steps(a, 3)
    b = second(rule, run.groups())
    b.load_state_dict(a.state_dict())
    assert [g['lr'] for g in b.param_groups] == [g['lr'] for g in a.param_groups] != list(orf.LRS)
    run.steps(b, 3)
    got = run.result(b, rule)
    orf.compare(got, _ref64(rule), _torch32(rule), rule, f'{direction} {rule}')
    for spec in run.specs:
        assert got[spec['name']]['step'] == _torch32(rule)[spec['name']]['step']


def test_unsupported_tensor_kinds_raise():
    from aspire_amd import HipAdam, HipAdagrad
    for cls in (HipAdam, HipAdagrad):
        half = torch.zeros(8, device='cuda', dtype=torch.float16, requires_grad=True)
        half.grad = torch.zeros_like(half)
        with pytest.raises(TypeError, match='fp32'):
            cls([half]).step()
        strided = torch.zeros(4, 6, device='cuda').t().detach().requires_grad_()
        assert not strided.is_contiguous()
        strided.grad = torch.zeros(6, 4, device='cuda')
        with pytest.raises(ValueError, match='contiguous'):
            cls([strided]).step()
        dense = torch.zeros(4, 3, device='cuda', requires_grad=True)
        dense.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3)).cuda()
        with pytest.raises(RuntimeError, match='sparse'):
            cls([dense]).step()
        host = torch.zeros(3, requires_grad=True)
        host.grad = torch.zeros(3)
        with pytest.raises(RuntimeError, match='GPU'):
            cls([host]).step()
        ok = torch.ones(5, device='cuda', requires_grad=True)
        ok.grad = torch.ones(5, device='cuda')
        opt = cls([ok])
        opt.param_groups[0]['maximize'] = True
        with pytest.raises(NotImplementedError, match='maximize'):
            opt.step()
        assert torch.equal(ok.detach(), torch.ones(5, device='cuda')) and len(opt.state) == 0       # nothing ran
        # torch's plain closure pattern: evaluated once, with grad enabled, its loss returned
        opt.param_groups[0]['maximize'] = False
        seen = []
        assert opt.step(lambda: (seen.append(torch.is_grad_enabled()), 2.5)[1]) == 2.5 and seen == [True]
        assert (ok.detach() < 1).all()
