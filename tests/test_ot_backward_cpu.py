"""CPU: the backward of the otAspire distance without a GPU -- the C-ABI entry (declared, exported, signed), the argument checks of
aspire_ot_backward_f32 and ops.ot_backward that are decided on the host, the fake kernels of the two new operators, and the
yardstick of the GPU test: the float64 restatement with geomloss's detach pattern (tests/ot_backward_ref.py) against the closed
formulas of include/aspire_hip.h -- on its own inputs and on every edge case of tests/ot_backward_cases.py, with the conditions on
those cases that the reference alone decides."""
import ctypes
import os
import re

import pytest
import torch

import ot_backward_cases as cases
import ot_backward_ref as ref

FAKE = 16            # a non-null, 16-byte aligned "device pointer" that no call of this file reaches
NAME = 'aspire_ot_backward_f32'


def test_entry_is_declared_exported_and_signed():
    from aspire_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'aspire_hip.h')).read(), flags=re.S)
    decl = [a.strip() for a in re.search(NAME + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')]
    assert decl == ['const aspire_repset* q', 'const aspire_repset* c', 'int64_t D', 'int pairing', 'const aspire_ot_params* prm',
                    'const float* diameter', 'int64_t diam_group', 'int want', 'const float* grad_scores', 'float* grad_q',
                    'float* grad_c', 'void* stream']
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), f'{NAME} is not exported'
    rs, vp = ctypes.POINTER(_lib.RepSet), ctypes.c_void_p
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, [rs, rs, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(_lib.OtParams), vp,
                                                    ctypes.c_int64, ctypes.c_int, vp, vp, vp, vp])
    assert callable(ops.ot_backward)
    assert _lib.lib.aspire_abi_version() == 6          # an entry added, none changed


def _set(n, ext=8, max_len=8):
    from aspire_amd import _lib
    return _lib.RepSet(FAKE, FAKE, FAKE, n, ext, max_len)


def test_backward_entry_validation_without_gpu():
    from aspire_amd import _lib
    INVALID, UNSUPPORTED, OK = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED, _lib.ASPIRE_OK
    err = _lib.lib.aspire_last_error
    q, c = _set(3), _set(3)
    base = dict(D=768, pairing=_lib.PAIR_PAIRED, prm=(0.05, 0.9, 1.0), diam=None, group=0, want=_lib.OT_DISTANCE, gs=FAKE, gq=FAKE, gc=None)

    def status(q=q, c=c, **kw):
        a = dict(base, **kw)
        prm = _lib.OtParams(*a['prm'], 0, 0) if a['prm'] is not None else None
        return _lib.lib.aspire_ot_backward_f32(ctypes.byref(q), ctypes.byref(c), a['D'], a['pairing'], ctypes.byref(prm) if prm else None,
                                               a['diam'], a['group'], a['want'], a['gs'], a['gq'], a['gc'], None)

    # (grad_c is null in every call: a call that passed every other check ends in "is null", never in a launch)
    assert status() == INVALID and b'is null' in err()
    assert status(want=_lib.OT_SIMILARITY) == INVALID and b'is null' in err()
    assert status(diam=FAKE, group=3) == INVALID and b'is null' in err()
    assert status(gs=None, gc=FAKE) == INVALID and b'is null' in err()
    assert status(gq=None, gc=FAKE) == INVALID and b'is null' in err()
    # CROSS would need an accumulation across pairs; the plan-weighted similarity is a test-time output: neither has a backward
    assert status(pairing=_lib.PAIR_CROSS, gc=FAKE) == UNSUPPORTED and b'accumulation across pairs' in err()
    assert status(pairing=_lib.PAIR_CROSS, c=_set(5), gc=FAKE) == UNSUPPORTED
    with pytest.raises(NotImplementedError, match='ASPIRE_PAIR_PAIRED'):
        _lib.check(status(pairing=_lib.PAIR_CROSS, gc=FAKE))
    assert status(want=_lib.OT_PLAN_SIM, gc=FAKE) == UNSUPPORTED and b'PLAN_SIM' in err()
    with pytest.raises(NotImplementedError, match='PLAN_SIM'):
        _lib.check(status(want=_lib.OT_PLAN_SIM, gc=FAKE))
    assert status(pairing=2) == INVALID and b'bad pairing' in err()
    assert status(want=3) == INVALID and b'bad want' in err()
    assert status(prm=None) == INVALID and b'null params' in err()
    for prm in ((0.0, 0.9, 1.0), (0.05, 1.0, 1.0), (0.05, 0.0, 1.0), (0.05, 0.9, 0.0)):
        assert status(prm=prm) == INVALID and b'need blur > 0' in err()
    assert status(diam=FAKE, group=0) == INVALID and b'diam_group' in err()
    assert status(c=_set(4)) == INVALID and b'equal batch sizes' in err()
    assert status(D=512) == UNSUPPORTED and b'768' in err()
    prm = _lib.OtParams(0.05, 0.9, 1.0, 0, 0)
    null = _lib.lib.aspire_ot_backward_f32(None, ctypes.byref(c), 768, _lib.PAIR_PAIRED, ctypes.byref(prm), None, 0, 0, FAKE, FAKE, FAKE, None)
    assert null == INVALID and b'null repset' in err()
    # the forward's row limit, padded and CSR, either side (every pointer given: the check sits in front of the launch)
    for kw in (dict(q=_set(3, ext=129)), dict(c=_set(3, ext=129)), dict(q=_set(3, ext=0, max_len=129)), dict(c=_set(3, ext=0, max_len=129))):
        assert status(gc=FAKE, **kw) == UNSUPPORTED
        assert b'more than 128 sentence rows' in err()
    assert status(q=_set(3, ext=128), c=_set(3, ext=0, max_len=128)) == INVALID and b'is null' in err()
    # no pairs: nothing to do, no buffers needed
    assert status(q=_set(0), c=_set(0), gs=None, gq=None) == OK


def _m(*s, dt=torch.float32):
    return torch.empty(*s, device='meta', dtype=dt)


def test_fake_kernels_of_the_two_operators():
    import aspire_amd.torch_ops as to
    i32 = torch.int32
    for name in ('ot_pair_scores', 'ot_pair_backward'):
        assert name in to.OPS and hasattr(torch.ops.aspire, name)
    prm = (0.05, 0.9, 1.0, 4)
    for want in (0, 2):
        s = torch.ops.aspire.ot_pair_scores(_m(4, 8, 768), _m(4, dt=i32), _m(4, 6, 768), _m(4, dt=i32), *prm, want)
        assert s.shape == (4,) and s.dtype == torch.float32 and s.device.type == 'meta'
        gq, gc = torch.ops.aspire.ot_pair_backward(_m(4), _m(4, 8, 768), _m(4, dt=i32), _m(4, 6, 768), _m(4, dt=i32), *prm, want)
        assert gq.shape == (4, 8, 768) and gc.shape == (4, 6, 768) and gq.dtype == gc.dtype == torch.float32
    with pytest.raises(AssertionError):      # pair_distances.py:46
        torch.ops.aspire.ot_pair_scores(_m(3, 8, 768), _m(3, dt=i32), _m(5, 6, 768), _m(5, dt=i32), *prm, 0)
    # the first operator carries an autograd formula: a fake forward of inputs that require grad is attached to the graph
    q = torch.empty(2, 8, 768, device='meta', requires_grad=True)
    c = torch.empty(2, 5, 768, device='meta', requires_grad=True)
    s = torch.ops.aspire.ot_pair_scores(q, _m(2, dt=i32), c, _m(2, dt=i32), 0.05, 0.9, 1.0, 2, 0)
    assert s.requires_grad and s.grad_fn is not None
    s.sum().backward()
    assert q.grad.shape == (2, 8, 768) and c.grad.shape == (2, 5, 768)


def test_no_cpu_kernel_behind_the_new_operators():
    import aspire_amd.torch_ops  # noqa: F401
    z, n = torch.zeros(1, 2, 768), torch.ones(1, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.ot_pair_scores(z, n, z, n, 0.05, 0.9, 1.0, 1, 0)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.ot_pair_backward(torch.zeros(1), z, n, z, n, 0.05, 0.9, 1.0, 1, 0)


def test_float64_restatement_equals_the_closed_formulas():
    """Three pairs of 6 x 5 rows, lengths (6, 5), (3, 5), (1, 2), one nearly coincident and one coincident row, mixed-sign upstream
    gradients: float64 autograd through the detach-pattern restatement against the formula sheet, to 1e-12; pad rows exactly 0."""
    gen = torch.Generator().manual_seed(31)
    qlens, clens = [6, 3, 1], [5, 5, 2]
    x, y = torch.zeros(3, 6, 768, dtype=torch.float64), torch.zeros(3, 5, 768, dtype=torch.float64)
    for b, (ql, cl) in enumerate(zip(qlens, clens)):
        x[b, :ql] = 0.3 * torch.randn(ql, 768, generator=gen, dtype=torch.float64)
        y[b, :cl] = 0.3 * torch.randn(cl, 768, generator=gen, dtype=torch.float64)
    y[0, 3] = x[0, 1] * (1.0 + 3e-4 * torch.randn(768, generator=gen, dtype=torch.float64))
    y[1, 0] = x[1, 2]
    gs = torch.tensor([0.8, -1.1, 0.5], dtype=torch.float64)
    for kw in ({}, dict(temp=0.2, blur=0.1)):
        ax, ay = ref.autograd_grads(x, y, qlens, clens, gs, torch.float64, direct=False, **kw)
        cx, cy = ref.closed_form_grads(x, y, qlens, clens, gs, **kw)
        dev = max((ax - cx).abs().max().item(), (ay - cy).abs().max().item())
        print(f'OTBWD closed formulas vs float64 autograd {kw}: {dev:.3e}, largest |gradient| {ax.abs().max().item():.3e}')
        assert dev < 1e-12
        assert torch.isfinite(ax).all() and torch.isfinite(ay).all() and ax.abs().max() > 1e-3
        for b, (ql, cl) in enumerate(zip(qlens, clens)):
            assert torch.count_nonzero(ax[b, ql:]) == 0 and torch.count_nonzero(ay[b, cl:]) == 0
            assert torch.count_nonzero(cx[b, ql:]) == 0 and torch.count_nonzero(cy[b, cl:]) == 0
    # every row of W and every column of V sums to 1 (they are the soft-max weights of the last extrapolation)
    with torch.no_grad():
        _, p = ref.restated_distance(x, y, qlens, clens, parts=True)
        w = torch.exp(p['lb'][0, None, :5] + (p['g0'][0, None, :5] - p['c'][0] + p['f'][0, :, None]) / p['eps'])
        v = torch.exp(p['la'][0, :, None] + (p['f0'][0, :, None] - p['c'][0] + p['g'][0, None, :5]) / p['eps'])
        assert (w.sum(1) - 1).abs().max() < 1e-12 and (v.sum(0) - 1).abs().max() < 1e-12


# ---- the edge cases of the GPU test (tests/ot_backward_cases.py): everything that the reference alone decides, before any GPU time
@pytest.mark.parametrize('name', list(cases.CASES))
def test_edge_case_yardstick_and_closed_formulas(name):
    """Every edge case: the pick gaps exceed 1e-4 * (noise scale / 0.3) and the fp32 restatement stays within 1e-4 of float64 (both
    asserted by cases.yardstick), the batch's diameter is more than 1e-5 (relative) from a jump of the schedule length, float64
    autograd equals the formula sheet to 1e-12 under the case's settings and diameters, pad rows are exact zeros."""
    inp, yard = cases.inputs(name), cases.yardstick(name)
    assert yard.gap > 1.0 and yard.dev32 < 1e-4 and yard.tol == max(4.0 * yard.dev32, 1e-6)
    if inp.group is None:       # the GPU side forms the batch's diameter itself: a few fp32 ulps must not change the schedule
        assert cases.schedule_clearance(name) > 1e-5, cases.schedule_clearance(name)
    cx, cy = cases.closed_form(inp)
    dev = max((yard.gx - cx).abs().max().item(), (yard.gy - cy).abs().max().item())
    print(f'OTBWD closed formulas vs float64 autograd ({name}): {dev:.3e}')
    assert dev < 1e-12
    assert torch.isfinite(yard.gx).all() and torch.isfinite(yard.gy).all() and max(yard.gx.abs().max(), yard.gy.abs().max()) > 1e-3
    for b, (ql, cl) in enumerate(zip(inp.ql, inp.cl)):
        assert torch.count_nonzero(yard.gx[b, ql:]) == 0 and torch.count_nonzero(yard.gy[b, cl:]) == 0
        assert torch.count_nonzero(inp.x[b, ql:]) == 0 and torch.count_nonzero(inp.y[b, cl:]) == 0


def test_edge_case_schedules_and_marginals():
    """What the solver-setting cases are there for, from the reference alone: the schedule lengths (12, 655, 426 steps; 2 where the
    diameter is below the blur, so that the kernel's n_mid has to clamp at 0), uniform marginals at temp 5000, and marginals that are
    exactly 0.0 in fp32 on both sides at temp 0.02 over 3.0-scale rows (the -100000 rule of the log-weights) -- with none of them
    denormal, so that whether a device's expf flushes denormals does not enter."""
    assert cases.schedule_lengths('scaling0.5') == [12]
    assert cases.schedule_lengths('scaling0.99') == [655]
    assert cases.schedule_lengths('blur0.5scaling0.99') == [426]
    inp = cases.inputs('blur_above_diam')
    assert cases.schedule_lengths('blur_above_diam') == [2] and cases.orc.max_diameter(inp.x, inp.y) < inp.kw['blur']
    a, b = cases.fp32_marginals('temp5000')
    uniform_a = torch.cat([torch.full((n,), 1.0 / n) for n in cases.inputs('temp5000').ql])
    uniform_b = torch.cat([torch.full((n,), 1.0 / n) for n in cases.inputs('temp5000').cl])
    assert ((a - uniform_a).abs() < 1e-3 * uniform_a).all() and ((b - uniform_b).abs() < 1e-3 * uniform_b).all()
    a, b = cases.fp32_marginals('zero_marginal')
    tiny = torch.finfo(torch.float32).tiny
    print(f'OTBWD zero marginals: {int((a == 0).sum())} of {a.numel()} in a, {int((b == 0).sum())} of {b.numel()} in b')
    assert (a == 0).sum() >= 1 and (b == 0).sum() >= 1
    assert not ((a > 0) & (a < tiny)).any() and not ((b > 0) & (b < tiny)).any()


@pytest.mark.parametrize('name', ['groups2', 'groups1'])
def test_edge_case_diameter_groups_are_told_apart(name):
    """The diameters of 'groups2' differ by at least 20 % from one another; with one diameter read for every pair the float64
    gradient leaves the yardstick by more than 10 x the bound, whichever diameter that is -- and in 'groups2' so does every single
    group under either other group's diameter."""
    inp, yard = cases.inputs(name), cases.yardstick(name)
    assert len(inp.diams) == (3 if name == 'groups2' else 5)
    if name == 'groups2':
        d = sorted(float(v) for v in inp.diams)
        assert all(hi >= 1.2 * lo for lo, hi in zip(d, d[1:])), d
    whole, per_group = cases.wrong_group_margin(name)
    print(f'OTBWD wrong diameter group ({name}): float64 gradient moves {whole:.3e} (a single group at least {per_group:.3e}), bound {yard.tol:.3e}')
    assert whole > 10.0 * yard.tol
    if name == 'groups2':
        assert per_group > 10.0 * yard.tol


def test_edge_case_schedule_steps_are_told_apart():
    """The 33 diameters straddle at least 6 schedule lengths; across a discontinuity (diameters 2e-7 apart, one step more) the
    float64 gradient moves by more than 10 x the bound, and the float64 distance by more than twice the 1e-4 that the forward's
    own tests allow it (tests/test_gpu_edges.py): a forward or a backward one step off cannot pass."""
    yard = cases.yardstick('schedule')
    lens = cases.schedule_lengths('schedule')
    assert len(lens) == 33 and len(set(lens)) >= 6, sorted(set(lens))
    grad_step, value_step = cases.schedule_step_margin()
    print(f'OTBWD one schedule step: float64 gradient moves {grad_step:.3e}, bound {yard.tol:.3e}; float64 distance moves {value_step:.3e}')
    assert grad_step > 10.0 * yard.tol
    assert value_step > 2.0 * cases.FORWARD_ATOL


def test_edge_case_route_settings_are_told_apart():
    """'route' (blur 0.1, scaling 0.5, temp 0.2): the float64 gradient with all three settings, or any one of them, at its default
    leaves the yardstick by more than 10 x the bound -- a backward that lost a setting on its way from the forward cannot pass."""
    yard = cases.yardstick('route')
    assert set(cases.inputs('route').kw) == set(cases.DEFAULTS)
    margin = cases.default_settings_margin()
    print(f'OTBWD a setting at its default (route): float64 gradient moves at least {margin:.3e}, bound {yard.tol:.3e}')
    assert margin > 10.0 * yard.tol
