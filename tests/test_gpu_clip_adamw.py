"""GPU: the global gradient norm (grad_norm.hip: aspire_grad_norm_f32 / aspire_grad_scale_f32), the scaled and decayed optimizer steps
(optim.hip: aspire_adam_step_scaled_f32 / aspire_adagrad_step_scaled_f32 / aspire_adamw_step_f32) behind aspire_amd.grad_norm /
clip_grad_norm_ / HipAdamW / step(grad_scale=...), and the trainers with update_rule='adamw' and max_grad_norm.

Yardsticks.  The norm: float32(sqrt(float64 sum of squares)), within 1 ulp -- derived: the squares are exact in double and a double sum
of at most 2^27 terms is off by at most 2^-26 relative, under half an fp32 ulp.  The coefficient: torch's own fp32 operations on the
norm, bit for bit.  The step: tests/clip_ref.py -- torch's AdamW and clip in float64 numpy -- under the project's parity rule, per tensor
max |kernel - float64| <= max(4 |torch fp32 (CPU) - float64|, 4 * 2^-23 max |float64|).  Every comparison prints its figures before it
asserts (pytest -s shows them).  On an MI355X the largest |kernel - float64| / bound over the 14 tensors is 0.288 for HipAdamW without
a clip and 0.509 with max_norm = 1.0, and every norm measured sits at |diff| / ulp 0.00.
"""
import datetime
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import clip_ref as crf  # noqa: E402
import optim_ref as orf  # noqa: E402
import readout_inputs as ri  # noqa: E402

pytestmark = pytest.mark.gpu
CHUNK = orf.CHUNK
MAX_GRID = 256 * 8          # tuning.h: kOptimMaxGrid
SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8197)
SEED = 0x9E3779B97F4A7C15


# ---- the norm ---------------------------------------------------------------------------------------------------------------------------
def _at_offset(values, shift):
    """the values in a contiguous view that starts `shift` elements into its storage"""
    base = torch.zeros(values.numel() + 4, device='cuda')
    view = base[shift:shift + values.numel()]
    view.copy_(values)
    assert view.data_ptr() % 16 == (4 * shift) % 16 and view.is_contiguous()
    return view


def _case(seed=0, scale=None):
    """gradients of SIZES elements (the 4097 one as a view at storage offset 1) as numpy float32"""
    rng = np.random.default_rng(seed)
    out = []
    for n in SIZES:
        g = rng.standard_normal(n)
        if scale is not None:
            g = g * scale(rng, n)
        out.append(g.astype(np.float32))
    return out


def _params(values, offset_of=(4097,), absent=1):
    """leaf parameters carrying `values` as .grad; one more parameter in the middle has no gradient"""
    ps = []
    for v in values:
        p = torch.nn.Parameter(torch.zeros(v.size, device='cuda'))
        g = torch.from_numpy(v).cuda()
        p.grad = _at_offset(g, 1) if v.size in offset_of else g
        ps.append(p)
    for _ in range(absent):
        ps.insert(3, torch.nn.Parameter(torch.zeros(77, device='cuda')))
    return ps


def _within_one_ulp(got, values, tag):
    want = np.float32(crf.total_norm(values))
    err, ulp = abs(float(got) - float(want)), crf.ulp32(want)
    print(f'[{tag}] norm {float(got):.9g}  float32(float64 norm) {float(want):.9g}  |diff| / ulp {err / ulp:.2f}')
    assert err <= ulp, tag


def _torch_coef(norm, max_norm):
    """torch.nn.utils.clip_grads_with_norm_'s two fp32 operations (and its clamp) on a float32 norm, on the CPU"""
    return torch.clamp(max_norm / (norm.detach().cpu() + 1e-6), max=1.0)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_norm_of_the_sizes_case_is_within_one_ulp():
    from aspire_amd import grad_norm
    values = _case()
    ps = _params(values)
    assert ps[3].grad is None and any(p.grad is not None and p.grad.storage_offset() == 1 for p in ps)
    for max_norm in (1.0, 1e4, 0.37):
        norm, coef = grad_norm(ps, max_norm)
        assert norm.is_cuda and coef.is_cuda and norm.dim() == 0 and norm.untyped_storage().data_ptr() == coef.untyped_storage().data_ptr()
        _within_one_ulp(norm, values, f'sizes max_norm={max_norm}')
        assert torch.equal(_bits(coef), _bits(_torch_coef(norm, max_norm))), max_norm
    assert float(grad_norm(ps, 1e4)[1]) == 1.0 and float(grad_norm(ps, 1.0)[1]) < 0.01
    for p, v in zip([p for p in ps if p.grad is not None], values):         # the norm reads, nothing else
        assert np.array_equal(p.grad.cpu().numpy(), v)
    # every tensor alone, at every alignment: the scalar path, the 16-byte path and their tails
    for v in values:
        for shift in (0, 1, 2, 3):
            p = torch.nn.Parameter(torch.zeros(v.size, device='cuda'))
            p.grad = _at_offset(torch.from_numpy(v).cuda(), shift)
            _within_one_ulp(grad_norm([p], 1.0)[0], [v], f'n={v.size} shift={shift}')


def test_norm_bits_depend_neither_on_alignment_nor_on_the_run():
    from aspire_amd import grad_norm
    values = _case(seed=1)
    outs = []
    for offset_of in ((), SIZES, (4097,), (4097,)):          # all aligned, all at offset 1, the mixed case twice
        ps = _params(values, offset_of=offset_of)
        norm, coef = grad_norm(ps, 2.5)
        outs.append((_bits(norm), _bits(coef)))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


def test_norm_with_more_chunks_than_the_grid():
    """the grid is capped at MAX_GRID workgroups, which stride over the chunk list: one partial per CHUNK elements all the same, and
    the final launch adds more partials than it has lanes"""
    from aspire_amd import ops
    n = (MAX_GRID + 301) * CHUNK + 5
    gen = torch.Generator(device='cuda').manual_seed(3)
    big = torch.randn(n, device='cuda', generator=gen)
    small = torch.randn(CHUNK + 1, device='cuda', generator=gen)
    values = [small.cpu().numpy(), big.cpu().numpy()]
    norm, coef = ops.grad_norm([small, big], 1.0)
    _within_one_ulp(norm, values, f'{n + CHUNK + 1} elements')
    assert torch.equal(_bits(coef), _bits(_torch_coef(norm, 1.0)))
    again = ops.grad_norm([big, small], 1.0)[0]            # another chunk order: another summation order, the same bound
    _within_one_ulp(again, values, 'reordered')
    assert torch.equal(_bits(ops.grad_norm([small, _at_offset(big, 1)], 1.0)[0]), _bits(norm))


def test_norm_of_spread_and_of_huge_gradients():
    from aspire_amd import grad_norm
    values = _case(seed=2, scale=lambda rng, n: 10.0 ** rng.uniform(-20.0, 2.0, n))
    _within_one_ulp(grad_norm(_params(values), 1.0)[0], values, 'spread over 1e-20 .. 1e2')
    tiny = [np.full(5, 1e-30, np.float32), np.full(3, 3e-38, np.float32)]      # squares far below fp32's range
    _within_one_ulp(grad_norm(_params(tiny, absent=0), 1.0)[0], tiny, 'tiny')
    # the deliberate departure from torch: the squares are summed in double, so 1e20 does not overflow
    huge = [np.full(4099, 1e20, np.float32), np.full(7, -3e19, np.float32)]
    ps = _params(huge, absent=0)
    norm, coef = grad_norm(ps, 1.0)
    assert torch.isfinite(norm) and float(norm) > 6e21
    _within_one_ulp(norm, huge, 'huge')
    assert torch.equal(_bits(coef), _bits(_torch_coef(norm, 1.0))) and 0 < float(coef) < 1e-21
    theirs = torch.nn.utils.get_total_norm([p.grad for p in ps])
    print(f'huge gradients: norm {float(norm):.6e}, torch {float(theirs)}')
    assert torch.isinf(theirs)


def test_non_finite_norms_give_torchs_coefficients_and_touch_nothing_else():
    from aspire_amd import ops
    PATTERN = 0x5A5AA5A5
    nan, inf = float('nan'), float('inf')
    for bad, want_norm, want_coef in (([(0, 0, nan)], nan, nan), ([(6, 4096, inf)], inf, 0.0), ([(7, 100, -inf)], inf, 0.0),
                                      ([(4, 1, inf), (6, 4000, nan)], nan, nan)):
        values = _case(seed=4)
        for t, i, v in bad:
            values[t][i] = v
        grads = [p.grad for p in _params(values)]
        arena = torch.full((16,), PATTERN, dtype=torch.int32, device='cuda')
        out = arena.view(torch.float32)[5:7]
        assert ops.grad_norm(grads, 1.0, out=out) is out
        got = out.cpu().numpy()
        print(f'{bad}: norm {got[0]} coef {got[1]}')
        assert (np.isnan(got[0]) if np.isnan(want_norm) else got[0] == want_norm)
        assert (np.isnan(got[1]) if np.isnan(want_coef) else got[1] == want_coef)
        theirs = _torch_coef(out[0], 1.0)
        assert bool(torch.isnan(theirs)) if np.isnan(want_coef) else float(theirs) == want_coef
        rest = arena.cpu().numpy()
        assert (rest[:5] == PATTERN).all() and (rest[7:] == PATTERN).all()
    # no gradient anywhere: the norm of nothing is 0 (torch's value)
    p = torch.nn.Parameter(torch.zeros(3, device='cuda'))
    out = ops.grad_norm([p.grad], 0.5)
    assert out.tolist() == [0.0, 1.0]


# ---- the step ---------------------------------------------------------------------------------------------------------------------------
RULES = ['adam', 'adagrad', 'adamw']


def _hip(rule, run):
    from aspire_amd import HipAdam, HipAdagrad, HipAdamW
    if rule == 'adamw':
        return HipAdamW(crf.groups(run), **crf.ADAMW)
    return HipAdam(run.groups(), **orf.ADAM) if rule == 'adam' else HipAdagrad(run.groups(), **orf.ADAGRAD)


def _fused(max_norm):
    from aspire_amd import grad_norm

    def update(opt, params):
        if max_norm is None:
            opt.step()
        else:
            opt.step(grad_scale=grad_norm(params, max_norm)[1])
    return update


def _clip_then_step(max_norm):
    from aspire_amd import clip_grad_norm_

    def update(opt, params):
        norm = clip_grad_norm_(params, max_norm)
        assert norm.is_cuda and norm.dim() == 0
        opt.step()
    return update


@pytest.mark.parametrize('rule', RULES)
def test_fused_clip_equals_clip_then_step(rule):
    """clip_grad_norm_ (the norm + one in-place multi-tensor multiply) followed by a plain step, against the step that multiplies as it
    loads: the same bits in every parameter and state tensor over three steps -- and the fused route leaves .grad as it was"""
    results = []
    for update in (_clip_then_step(crf.MAX_NORM), _fused(crf.MAX_NORM)):
        run = orf.Run('cuda')
        opt = _hip(rule, run)
        crf.drive(run, opt, 3, update)
        results.append((crf.result(run, opt, rule), [None if p.grad is None else p.grad.clone() for p in run.params]))
    (a, clipped), (b, kept) = results
    for name in a:
        for key in ('p',) + crf.STATE_KEYS[rule]:
            assert np.array_equal(a[name][key].view(np.int32), b[name][key].view(np.int32)), (name, key)
        assert a[name]['step'] == b[name]['step']
    # the last step's gradients: untouched on the fused route, every one multiplied (by far less than 1) on the other
    for spec, g_clipped, g_kept in zip(orf.case_specs(), clipped, kept):
        want = orf.grad_value(spec, 3)
        if want is None:
            assert g_kept is None and g_clipped is None
            continue
        assert np.array_equal(g_kept.cpu().numpy(), want), spec['name']
        assert not np.array_equal(g_clipped.cpu().numpy(), want) or not want.any(), spec['name']
    # clip_grad_norm_ multiplies by exactly 1.0 when the norm is inside max_norm, and returns torch's norm within an ulp
    from aspire_amd import clip_grad_norm_
    ps = _params(_case(seed=5))
    before = [None if p.grad is None else p.grad.clone() for p in ps]
    versions = [None if p.grad is None else p.grad._version for p in ps]
    norm = clip_grad_norm_(ps, 1e6)
    _within_one_ulp(norm, _case(seed=5), 'clip_grad_norm_')
    for p, g, v in zip(ps, before, versions):
        assert (p.grad is None and g is None) or (torch.equal(p.grad, g) and p.grad._version > v)
    clip_grad_norm_(ps, 0.5)
    coef = _torch_coef(norm, 0.5).cuda()
    for p, g in zip(ps, before):
        assert p.grad is None or torch.equal(p.grad, g * coef)


def test_adamw_without_decay_is_adam_bit_for_bit():
    from aspire_amd import HipAdam, HipAdamW
    results = []
    for cls in (HipAdam, HipAdamW):
        for update in (_fused(None), _fused(crf.MAX_NORM)):
            run = orf.Run('cuda')
            opt = cls(run.groups(), weight_decay=0, **orf.ADAM)
            crf.drive(run, opt, 3, update)
            results.append(crf.result(run, opt, 'adam'))
    for a, b in ((results[0], results[2]), (results[1], results[3])):
        for name in a:
            for key in ('p', 'exp_avg', 'exp_avg_sq'):
                assert np.array_equal(a[name][key].view(np.int32), b[name][key].view(np.int32)), (name, key)
    assert any(not np.array_equal(results[0][n]['p'], results[1][n]['p']) for n in results[0])      # the clip changed something


@functools.lru_cache(maxsize=None)
def _ref64(max_norm):
    return crf.run_reference('adamw', max_norm)


@functools.lru_cache(maxsize=None)
def _torch32(max_norm):
    return crf.torch_cpu('adamw', max_norm)


@pytest.mark.parametrize('max_norm', [None, crf.MAX_NORM])
def test_six_adamw_steps_match_float64(max_norm, monkeypatch):
    from aspire_amd import ops
    calls = []
    inner = ops.optim_launch
    monkeypatch.setattr(ops, 'optim_launch', lambda r, table, *a: (calls.append((r, len(table), sorted(set(table['weight_decay'])))),
                                                                   inner(r, table, *a))[1])
    run = orf.Run('cuda')
    opt = _hip('adamw', run)
    crf.drive(run, opt, orf.STEPS, _fused(max_norm))
    got = crf.result(run, opt, 'adamw')
    worst = crf.compare(got, _ref64(max_norm), _torch32(max_norm), 'adamw', f'HipAdamW clip={max_norm}')
    print(f'largest error / bound: {worst:.3f}')
    # ONE launch (one table) per step() over both groups -- they differ in lr and weight_decay alone: 13 tensors on odd steps, 12 on
    # even ones (the lagging parameter), both decays in every table
    assert calls == [('adamw', 13, sorted(crf.WEIGHT_DECAYS)), ('adamw', 12, sorted(crf.WEIGHT_DECAYS))] * 3
    for p, spec in zip(run.params, run.specs):
        want = _torch32(max_norm)[spec['name']]['step']
        if spec.get('frozen'):
            assert p not in opt.state and want == 0 and np.array_equal(p.detach().cpu().numpy(), orf.init_value(spec))
        else:
            assert int(opt.state[p]['step']) == want, spec['name']
    # the decay is at work: the rows whose gradient is always zero shrink by exactly the product of the six factors, in fp32
    spec = next(s for s in run.specs if s['name'] == 'rows')
    want = orf.init_value(spec)[1::2].copy()
    for k in range(1, orf.STEPS + 1):
        want = want * np.float32(1 - orf.LRS[spec['group']] * orf.GAMMA ** (k - 1) * crf.WEIGHT_DECAYS[spec['group']])
    assert np.array_equal(got['rows']['p'][1::2], want) and not np.array_equal(want, orf.init_value(spec)[1::2])


def test_grad_scale_must_be_a_one_element_gpu_float():
    from aspire_amd import HipAdamW
    p = torch.nn.Parameter(torch.ones(5, device='cuda'))
    p.grad = torch.ones(5, device='cuda')
    opt = HipAdamW([p])
    for bad, exc in ((torch.ones(2, device='cuda'), ValueError), (torch.ones(1), RuntimeError), (0.5, ValueError),
                     (torch.ones(1, device='cuda', dtype=torch.float64), TypeError)):
        with pytest.raises(exc):
            opt.step(grad_scale=bad)
    assert torch.equal(p.detach(), torch.ones(5, device='cuda')) and float(opt.state[p]['step']) == 0.0      # nothing ran
    opt.step(grad_scale=torch.zeros(1, device='cuda'))          # a zero gradient: the decay alone moves the parameter
    assert torch.equal(p.detach(), torch.full((5,), np.float32(1 - 1e-3 * 1e-2), device='cuda'))


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
def _bert(seed, dropout=0.1):
    from transformers import BertConfig, BertModel
    torch.manual_seed(seed)
    cfg = BertConfig(vocab_size=300, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=256,
                     max_position_embeddings=64, layer_norm_eps=1e-12, hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout,
                     attn_implementation='eager')
    return BertModel(cfg, add_pooling_layer=True)


def _train_hparams(**over):
    hp = dict(es_check_every=1000, train_size=12, dev_size=3, batch_size=3, num_epochs=2, update_rule='adamw', weight_decay=0.05,
              max_grad_norm=1e-3, learning_rate=1e-3, lr_decay_method='exponential', decay_lr_by=0.7, decay_lr_every=1)
    hp.update(over)
    return hp


def _state(enc, opt):
    out = {}
    for n, p in enc.bert.named_parameters():
        out[n] = p.detach().cpu().clone()
        for k, v in opt.state.get(p, {}).items():
            out[f'{n}/{k}'] = torch.as_tensor(v).detach().cpu().clone()
    return out


def _same(a, b, what):
    assert set(a) == set(b), what
    for key in a:
        assert torch.equal(a[key], b[key]), (what, key)


def test_adamw_trainer_clips_every_step_repeats_and_resumes(tmp_path):
    import test_gpu_ddp as tg
    from aspire_amd import HipAdamW, HipBertTrainEncoder, RankTrainer
    batches = tg._batches(str(tmp_path), 'clip')
    hparams = ri.hparams('l2max', 0.5)

    def make(seed, tag, **over):
        enc = HipBertTrainEncoder(_bert(seed), dropout=True, seed=SEED, hip_embeddings=True)
        return RankTrainer(enc, hparams, _train_hparams(**over), str(tmp_path / tag), lambda epoch: batches)

    straight = make(5, 'straight')
    assert isinstance(straight.optimizer, HipAdamW) and [g['weight_decay'] for g in straight.optimizer.param_groups] == [0.05, 0.0]
    names = {id(p): n for n, p in straight.encoder.bert.named_parameters()}
    assert all(names[id(p)].endswith('bias') or 'LayerNorm' in names[id(p)] for p in straight.optimizer.param_groups[1]['params'])
    norms = []
    step = straight.optimizer.step

    def spy(closure=None, grad_scale=None):
        assert grad_scale is not None and grad_scale.is_cuda
        norms.append((float(straight.last_grad_norm), float(grad_scale)))
        return step(closure, grad_scale=grad_scale)

    straight.optimizer.step = spy
    straight.train(max_iterations=6)
    print('(norm, coefficient) per step:', norms)
    assert len(norms) == 6 and all(np.isfinite(n) and n > 1e-3 and 0 < c < 1 for n, c in norms)         # every step clips
    assert straight.loss_checked_iters == [0, 5] and straight.loss_history['grad_norm'] == [norms[0][0], norms[5][0]]
    again = make(5, 'again')
    again.train(max_iterations=6)
    _same(_state(again.encoder, again.optimizer), _state(straight.encoder, straight.optimizer), 'the run repeated')
    assert again.loss_history == straight.loss_history
    first = make(5, 'first')
    first.train(max_iterations=3)
    first.save_checkpoint(tmp_path / 'ck.pt')
    second = make(99, 'second')
    second.encoder.set_dropout_state(1, 0)
    second.load_checkpoint(tmp_path / 'ck.pt')
    second.train(max_iterations=3)
    _same(_state(second.encoder, second.optimizer), _state(straight.encoder, straight.optimizer), 'resumed against straight')
    assert second.loss_history == straight.loss_history and second.encoder.dropout_state() == straight.encoder.dropout_state()
    # the clip and the decay both matter: without either the parameters end elsewhere
    w = 'encoder.layer.1.output.dense.weight'
    for over in (dict(max_grad_norm=None), dict(weight_decay=0.0)):
        other = make(5, 'other', **over)
        other.train(max_iterations=6)
        assert not torch.equal(_state(other.encoder, other.optimizer)[w], _state(straight.encoder, straight.optimizer)[w]), over
        assert ('grad_norm' in other.loss_history) == (over.get('max_grad_norm', 1) is not None)


def _ddp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    for p in (ROOT, HERE, os.path.join(HERE, 'golden')):
        sys.path.insert(0, p)
    import test_gpu_ddp as tg
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from aspire_amd import HipAdamW, HipBertTrainEncoder, RankTrainerDDP
    batches = tg._batches(out_dir, f'r{rank}')
    enc = HipBertTrainEncoder(_bert(3 + rank), dropout=True, seed=SEED, hip_embeddings=True)
    tr = RankTrainerDDP(enc, ri.hparams('l2max', 0.5), _train_hparams(train_size=12), os.path.join(out_dir, f'ddp{rank}'),
                        lambda epoch: [batches[(2 * (2 * epoch + i) + rank) % 4] for i in range(2)])
    calls = []
    inner = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    done = tr.train()
    res = dict(done=done, iteration=tr.iteration, state=_state(enc, tr.optimizer), is_adamw=isinstance(tr.optimizer, HipAdamW),
               history=dict(tr.loss_history), all_reduces=len(calls), last_norm=float(tr.last_grad_norm))
    torch.save(res, os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_alike_and_equal_one_process_on_the_mean_gradient(tmp_path):
    import torch.multiprocessing as mp
    import test_gpu_ddp as tg
    from aspire_amd import HipAdamW, HipBertTrainEncoder, RankLoss, grad_norm
    from aspire_amd.optim import decay_groups
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    mp.spawn(_ddp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    outs = [torch.load(os.path.join(str(tmp_path), f'r{r}.pt'), weights_only=False) for r in (0, 1)]
    for o in outs:
        assert o['done'] is True and o['iteration'] == 4 and o['is_adamw']
        # per iteration: the "I have a batch" flag and the bucket, plus the flag that ends each of the two epochs -- nothing for the clip
        assert o['all_reduces'] == 2 * 4 + 2
    assert outs[0]['last_norm'] == outs[1]['last_norm'] and len(outs[0]['history']['grad_norm']) == 1 and outs[1]['history'] == {}
    _same(outs[0]['state'], outs[1]['state'], 'rank 0 against rank 1')
    # one process: every iteration's gradient formed as 0.5 g_a + 0.5 g_b, the norm of that, the fused step
    batches = tg._batches(str(tmp_path), 'parent')
    enc = HipBertTrainEncoder(_bert(3), dropout=True, seed=SEED, hip_embeddings=True).train()
    hp = _train_hparams()
    opt = HipAdamW(decay_groups(enc, hp['weight_decay']), lr=hp['learning_rate'])
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=hp['decay_lr_by'])
    loss = RankLoss(ri.hparams('l2max', 0.5)).forward_rank
    params = [p for g in opt.param_groups for p in g['params']]
    for it in range(4):
        per_rank = []
        for r in (0, 1):
            opt.zero_grad()
            enc.set_dropout_state(SEED + r, 3 * it)
            loss(batches[(2 * it + r) % 4], enc).backward()
            per_rank.append([None if p.grad is None else p.grad.clone() for p in params])
        for p, ga, gb in zip(params, *per_rank):
            if ga is None and gb is None:
                p.grad = None
            else:
                za = ga if ga is not None else torch.zeros_like(p)
                zb = gb if gb is not None else torch.zeros_like(p)
                p.grad = 0.5 * za + 0.5 * zb
        norm, coef = grad_norm(params, hp['max_grad_norm'])
        assert 0 < float(coef) < 1
        opt.step(grad_scale=coef)
        if it > 0:
            sched.step()
    assert float(norm) == outs[0]['last_norm']
    _same(outs[0]['state'], _state(enc, opt), 'the ranks against one process on the mean gradient')
