"""Inputs and float64 yardsticks of the otAspire backward's edge cases (tests/test_ot_backward_cpu.py checks every condition that
the reference alone decides, tests/test_gpu_ot_backward_edges.py holds the kernel to the yardsticks): solver settings, row scales, a
marginal that is exactly zero in fp32, extreme aspect ratios, several diameter groups in one call, the schedule length at its
discontinuities and the Python route with non-default settings.

The recipe is tests/test_gpu_ot_backward.py's, unchanged: the yardstick is ot_backward_ref.autograd_grads(float64, direct=False);
dev32 is the deviation of autograd_grads(float32, direct=True) from it and is asserted below 1e-4; the kernel gets
max(4 * dev32, 1e-6).  The arg-max picks are kept from flipping by a gap that scales with the rows: every pair's pick_margins exceeds
1e-4 * (noise scale / 0.3), the noise scale being the standard deviation of the random part of that pair's rows.  Pad rows are zero.

A case with `group` holds one diameter per `group` consecutive pairs (fp32, formed here on the CPU: geomloss's max_diameter over the
group's rows, pad rows included, or given outright); the kernel is handed that tensor and the restatement the same numbers group by
group as diameter=float(d).  A case without takes the box of the whole batch on both sides."""
import collections
import functools

import numpy as np
import torch

import ot_backward_ref as ref
from oracle import aspire_oracle as orc

D = 768
DEFAULTS = dict(blur=0.05, scaling=0.9, temp=1.0)
LENS8 = [(8, 8), (3, 8), (1, 2), (5, 1)]
GS4 = [0.9, -1.3, 0.7, 0.6]
LENS5 = [(8, 8), (1, 2), (3, 8), (5, 1), (6, 7)]            # (in groups of two, every group holds a pair with two rows a side)
GS5 = [0.9, 0.7, -1.3, 0.6, -0.8]
SCALES5 = [0.1, 0.1, 0.2, 0.2, 0.4]
FORWARD_ATOL = 1e-4            # what the forward's own tests allow a distance (tests/test_gpu_edges.py)
SCHEDULE_KS = (56, 62, 66)
SCHEDULE_RELS = (0.0, 1e-7, -1e-7, 3e-7, -3e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-3, -1e-3)


def _case(lens=LENS8, exts=(8, 8), seed=4100, scale=0.3, offset=False, gs=None, group=None, **kw):
    assert set(kw) <= set(DEFAULTS)
    gs = (GS4 if len(lens) == 4 else GS5) if gs is None else gs
    return dict(lens=lens, exts=exts, seed=seed, scale=scale, offset=offset, gs=gs, group=group, kw=kw)


# name -> padded extents, [(q_len, c_len)], seed, the rows' noise scale (one number, or one per pair), solver keywords, ...
CASES = {
    # 1  scaling and blur: schedules of 12, 655 and 426 steps; a diameter (0.12) below the blur: 2 steps, n_mid clamps to 0
    'scaling0.5':         _case(scaling=0.5),
    'scaling0.99':        _case(scaling=0.99),
    'blur0.5scaling0.99': _case(blur=0.5, scaling=0.99),
    'blur_above_diam':    _case(blur=0.5, scale=1e-3),
    # 2  temperature: sharp marginals, and marginals that 5000 makes uniform
    'temp10':             _case(temp=10.0),
    'temp5000':           _case(temp=5000.0),
    # 3  row scale: BERT-sized rows, tiny rows, and rows of norm 28 that are 2 apart (0.05 N(0, 1) + one shared N(0, 1) offset)
    'rows1':              _case(scale=1.0),
    'rows3':              _case(scale=3.0),
    'rows1e-2':           _case(scale=1e-2),
    'rows1e-3':           _case(scale=1e-3),
    'offset':             _case(scale=0.05, offset=True),
    # 4  a marginal that is exactly 0.0 in fp32: the -100000 rule of the log-weights
    'zero_marginal':      _case(scale=3.0, temp=0.02),
    # 5  extreme aspect: distance-block strides (cl | 1) of 1 and 129, row counts 1, 2, 3 mod 4 for the four-wave row loops
    'aspect':             _case(lens=[(128, 1), (1, 128), (127, 3), (2, 128)], exts=(128, 128), seed=4110),
    # 6  several diameter groups in one call: {0, 1}, {2, 3}, {4} and one group per pair; the row scale differs between the groups
    'groups2':            _case(lens=LENS5, seed=4144, scale=SCALES5, group=2),
    'groups1':            _case(lens=LENS5, seed=4144, scale=SCALES5, group=1),
    # 7  the schedule length at its discontinuities: one 6 x 7 pair under 33 given diameters
    'schedule':           _case(lens=[(6, 7)] * (len(SCHEDULE_KS) * len(SCHEDULE_RELS)), exts=(6, 7), seed=4120, scale=0.5, group=1,
                                gs=[1.1] * (len(SCHEDULE_KS) * len(SCHEDULE_RELS))),
    # 8  the Python route: every setting off its default, one schedule for the batch (compute_distance's reading)
    'route':              _case(lens=LENS5, blur=0.1, scaling=0.5, temp=0.2),
}
STRUCTURAL = ('scaling0.5', 'scaling0.99', 'blur0.5scaling0.99', 'blur_above_diam', 'temp10', 'temp5000', 'rows1', 'rows3',
              'rows1e-2', 'rows1e-3', 'offset', 'zero_marginal', 'aspect')          # the cases of 1 to 5
CSR = ('scaling0.5', 'offset', 'aspect')                                            # one of 1, one of 3, and 5

Inputs = collections.namedtuple('Inputs', 'x y ql cl gs kw scales diams group')
Yardstick = collections.namedtuple('Yardstick', 'gx gy dev32 tol gap')


def settings(kw):
    """the solver keywords of a case with the defaults filled in: blur, scaling, temp"""
    return dict(DEFAULTS, **kw)


def schedule_diameters(blur=0.05, scaling=0.9):
    """fp32 diameters on, and a few ulps to a part in a thousand either side of, blur * scaling**-k: where the number of annealed
    steps ceil((log blur - log diameter) / log scaling) jumps"""
    return np.array([np.float32(blur * scaling ** (-k) * (1.0 + rel)) for k in SCHEDULE_KS for rel in SCHEDULE_RELS], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> Inputs: x [B, Sq, 768], y [B, Sc, 768] fp32 (valid rows scale * N(0, 1) (+ one shared N(0, 1) vector), pad rows zero), the
    lengths, gs [B] = dLoss / dscore, the solver keywords, the noise scale of every pair, and the fp32 diameters [ceil(B / group)]
    with `group` (None, None: the box of the whole batch)."""
    spec = CASES[name]
    lens, exts = spec['lens'], spec['exts']
    gen = torch.Generator().manual_seed(spec['seed'])
    scales = spec['scale'] if isinstance(spec['scale'], list) else [spec['scale']] * len(lens)
    off = torch.randn(D, generator=gen) if spec['offset'] else torch.zeros(D)
    x, y = torch.zeros(len(lens), exts[0], D), torch.zeros(len(lens), exts[1], D)
    for b, (ql, cl) in enumerate(lens):
        if name == 'schedule' and b > 0:         # one pair, repeated
            x[b], y[b] = x[0], y[0]
            continue
        x[b, :ql] = scales[b] * torch.randn(ql, D, generator=gen) + off
        y[b, :cl] = scales[b] * torch.randn(cl, D, generator=gen) + off
    group, diams = spec['group'], None
    if name == 'schedule':
        diams = torch.from_numpy(schedule_diameters())
    elif group is not None:
        diams = torch.tensor([orc.max_diameter(x[s:s + group], y[s:s + group]) for s in range(0, len(lens), group)], dtype=torch.float32)
    return Inputs(x, y, [l[0] for l in lens], [l[1] for l in lens], torch.tensor(spec['gs']), spec['kw'], scales, diams, group)


def grads(inp, dtype, direct, kw=None, diams=None):
    """(grad_x, grad_y) of sum(gs * restated distance) in `dtype`, group by group under the case's diameters (diams: others to
    use in their place, one per group), under the solver keywords `kw` (default: the case's)"""
    kw = inp.kw if kw is None else kw
    diams = inp.diams if diams is None else diams
    if inp.group is None:
        return ref.autograd_grads(inp.x, inp.y, inp.ql, inp.cl, inp.gs, dtype, direct, **kw)
    gx, gy = [], []
    for n, s in enumerate(range(0, len(inp.ql), inp.group)):
        e = s + inp.group
        g = ref.autograd_grads(inp.x[s:e], inp.y[s:e], inp.ql[s:e], inp.cl[s:e], inp.gs[s:e], dtype, direct, diameter=float(diams[n]), **kw)
        gx.append(g[0])
        gy.append(g[1])
    return torch.cat(gx), torch.cat(gy)


def closed_form(inp):
    """ot_backward_ref.closed_form_grads in float64 under the case's diameters and keywords"""
    x, y = inp.x.double(), inp.y.double()
    gs = inp.gs.double()
    if inp.group is None:
        return ref.closed_form_grads(x, y, inp.ql, inp.cl, gs, **inp.kw)
    gx, gy = [], []
    for n, s in enumerate(range(0, len(inp.ql), inp.group)):
        e = s + inp.group
        g = ref.closed_form_grads(x[s:e], y[s:e], inp.ql[s:e], inp.cl[s:e], gs[s:e], diameter=float(inp.diams[n]), **inp.kw)
        gx.append(g[0])
        gy.append(g[1])
    return torch.cat(gx), torch.cat(gy)


def dev(inp, got, want):
    """largest |got - want| over the valid rows of the case"""
    return ref.valid_dev(*got, *want, inp.ql, inp.cl)


def pick_gap(inp):
    """the smallest pick_margins of a pair over 1e-4 * (its noise scale / 0.3): above 1 the arg-max picks are far from flipping"""
    return min(ref.pick_margins(inp.x[b:b + 1], inp.y[b:b + 1], inp.ql[b:b + 1], inp.cl[b:b + 1]) / (1e-4 * inp.scales[b] / 0.3)
               for b in range(len(inp.ql)))


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """-> Yardstick: the float64 gradients, the fp32 restatement's deviation from them, the kernel's bound and the pick gap (as a
    multiple of what it has to exceed) -- computed once per case and never changed; the two conditions that the reference alone
    decides are asserted here"""
    inp = inputs(name)
    gap = pick_gap(inp)
    assert gap > 1.0, (name, gap)
    g64 = grads(inp, torch.float64, False)
    dev32 = dev(inp, grads(inp, torch.float32, True), g64)
    # fp32 rounding of these gradients is far below this; beyond it the fp32 restatement itself would have gone another way (a
    # pick, a schedule length), and the bound must not grow from that unnoticed
    assert dev32 < 1e-4, (name, dev32)
    tol = max(4.0 * dev32, 1e-6)
    print(f'OTBWD yardstick ({name}) pick gap {gap:.3e} x its condition, CPU fp32 restatement deviation {dev32:.3e} -> bound {tol:.3e}, '
          f'largest |gradient| {max(g64[0].abs().max().item(), g64[1].abs().max().item()):.3e}')
    return Yardstick(g64[0], g64[1], dev32, tol, gap)


def schedule_lengths(name):
    """the length of geomloss's epsilon schedule of every group of the case (or of the whole batch)"""
    inp = inputs(name)
    s = settings(inp.kw)
    diams = [orc.max_diameter(inp.x, inp.y)] if inp.diams is None else [float(d) for d in inp.diams]
    return [len(orc.epsilon_schedule(1, d, s['blur'], s['scaling'])) for d in diams]


def schedule_clearance(name):
    """how far, relatively, the batch's diameter is from the nearest diameter at which the schedule gains a step: the kernel's side
    forms this diameter itself, in fp32 and in another summation order, and must not land on the other side by a few ulps"""
    inp = inputs(name)
    s = settings(inp.kw)
    q = (np.log(s['blur']) - np.log(orc.max_diameter(inp.x, inp.y))) / np.log(s['scaling'])
    return abs(q - round(q)) * abs(np.log(s['scaling']))


def fp32_marginals(name):
    """(a, b): the valid entries of the fp32 restatement's marginals, one tensor per side"""
    inp = inputs(name)
    with torch.no_grad():
        _, p = ref.restated_distance(inp.x, inp.y, inp.ql, inp.cl, direct=True, parts=True, **inp.kw)
    return (torch.cat([p['a'][n, :ql] for n, ql in enumerate(inp.ql)]), torch.cat([p['b'][n, :cl] for n, cl in enumerate(inp.cl)]))


# ---- the sensitivity conditions: how far the float64 gradient moves under the mistake a case is there to catch, from the reference
# alone; each has to exceed 10 x the case's bound.  (A condition on the inputs, not a measurement.)
def wrong_group_margin(name):
    """'groups2' / 'groups1': the float64 gradient with ONE of the case's diameters read for every pair, against the yardstick ->
    (the smallest deviation over those diameters, the smallest deviation of a GROUP under another group's diameter).  The first is
    the reading "diam_group ignored"; the second covers every mix-up of two groups, and needs a pair with two rows a side in every
    group (a pair with one row on a side is solved in its first step, whatever the schedule)."""
    inp, yard = inputs(name), yardstick(name)
    whole, per_group = float('inf'), float('inf')
    for k, d in enumerate(inp.diams):
        g = grads(inp, torch.float64, False, diams=[d] * len(inp.diams))
        whole = min(whole, dev(inp, g, yard[:2]))
        for n, s in enumerate(range(0, len(inp.ql), inp.group)):
            if n != k:
                e = s + inp.group
                per_group = min(per_group, ref.valid_dev(g[0][s:e], g[1][s:e], yard.gx[s:e], yard.gy[s:e], inp.ql[s:e], inp.cl[s:e]))
    return whole, per_group


def schedule_step_margin():
    """'schedule': the smallest distance between the float64 gradients either side of a discontinuity (rel = -1e-7 and +1e-7: the
    diameters agree to 2e-7, the schedules differ by one step), and the same for the float64 distance itself"""
    yard = yardstick('schedule')
    lens = schedule_lengths('schedule')
    n = len(SCHEDULE_RELS)
    lo, hi = SCHEDULE_RELS.index(-1e-7), SCHEDULE_RELS.index(1e-7)
    value = schedule_values()
    grad_step, value_step = float('inf'), float('inf')
    for k in range(len(SCHEDULE_KS)):
        a, b = k * n + lo, k * n + hi
        assert lens[b] == lens[a] + 1, (lens[a], lens[b])
        grad_step = min(grad_step, (yard.gx[a] - yard.gx[b]).abs().max().item(), (yard.gy[a] - yard.gy[b]).abs().max().item())
        value_step = min(value_step, abs(value[a] - value[b]))
    return grad_step, value_step


@functools.lru_cache(maxsize=None)
def schedule_values():
    """'schedule': the float64 restatement's distance under every diameter"""
    inp = inputs('schedule')
    with torch.no_grad():
        return [ref.restated_distance(inp.x[:1].double(), inp.y[:1].double(), inp.ql[:1], inp.cl[:1], diameter=float(d), **inp.kw).item()
                for d in inp.diams]


def default_settings_margin(name='route'):
    """'route': the smallest deviation from the yardstick of the float64 gradient with ALL, or any ONE, of blur / scaling / temp at
    its default -- a backward that dropped a setting on its way cannot pass"""
    inp, yard = inputs(name), yardstick(name)
    wrong = [{}] + [{k: v for k, v in inp.kw.items() if k != drop} for drop in inp.kw]
    return min(dev(inp, grads(inp, torch.float64, False, kw=kw), yard[:2]) for kw in wrong)
