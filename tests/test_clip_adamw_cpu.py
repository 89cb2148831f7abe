"""CPU: what of AdamW and gradient clipping needs no GPU -- HipAdamW's construction, refusals and state-dict interchange with
torch.optim.AdamW, decay_groups, the argument checks of the new C entries (no device is touched), the yardstick of tests/clip_ref.py
against torch on the CPU, and the trainers' host logic with the norm, the optimizer and the loss injected (under gloo for
RankTrainerDDP, as tests/test_ddp_cpu.py runs it)."""
import copy
import ctypes
import datetime
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as crf  # noqa: E402
import optim_ref as orf  # noqa: E402

TIMEOUT = datetime.timedelta(seconds=120)


# ---- HipAdamW without a device ------------------------------------------------------------------------------------------------------------
def test_adamw_constructs_and_refuses_what_is_not_built():
    from aspire_amd import HipAdam, HipAdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    opt = HipAdamW(p, lr=0.5, weight_decay=0.02)
    assert set(opt.param_groups[0]) == set(torch.optim.AdamW(p).param_groups[0])
    assert opt.param_groups[0]['weight_decay'] == 0.02 and opt.param_groups[0]['lr'] == 0.5
    assert HipAdamW(p).param_groups[0]['weight_decay'] == torch.optim.AdamW(p).param_groups[0]['weight_decay'] == 1e-2
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(NotImplementedError):
            HipAdamW(p, **kw)
    with pytest.raises(ValueError):
        HipAdamW(p, weight_decay=-0.1)
    with pytest.raises(NotImplementedError):         # coupled L2 decay stays unbuilt
        HipAdam(p, weight_decay=0.01)
    assert opt.step() is None and len(opt.state) == 0          # no gradient anywhere: nothing to launch, no state
    p[0].grad = torch.zeros(3)
    for key in ('amsgrad', 'maximize', 'capturable', 'differentiable'):      # edited by hand (or loaded): refused again at step()
        opt.param_groups[0][key] = True
        with pytest.raises(NotImplementedError, match=key):
            opt.step()
        opt.param_groups[0][key] = False
    opt.param_groups[0]['lr'] = torch.tensor(0.5)
    with pytest.raises(NotImplementedError, match='lr'):
        opt.step()
    opt.param_groups[0]['lr'] = 0.5
    with pytest.raises(RuntimeError, match='GPU'):              # the parameter is on the host: no CPU fallback
        opt.step()
    with pytest.raises(RuntimeError, match='GPU'):
        opt.step(grad_scale=torch.ones(1))


def test_adamw_state_dict_goes_through_torch_and_back():
    from aspire_amd import HipAdamW
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (3, 5, 2)]
    a = torch.optim.AdamW([{'params': ps[:2], 'lr': 0.1, 'weight_decay': 0.3}, {'params': ps[2:], 'lr': 0.2, 'weight_decay': 0.0}])
    for k in range(3):
        for i, p in enumerate(ps):
            p.grad = None if (i == 1 and k != 1) else torch.randn_like(p)
        a.step()
    b = HipAdamW([{'params': ps[:2]}, {'params': ps[2:]}])
    b.load_state_dict(a.state_dict())
    assert [(g['lr'], g['weight_decay']) for g in b.param_groups] == [(0.1, 0.3), (0.2, 0.0)]
    steps = [b.state[p]['step'] for p in ps]
    assert [float(s) for s in steps] == [3.0, 1.0, 3.0]
    assert all(s.dtype == torch.float32 and s.device.type == 'cpu' and s.dim() == 0 for s in steps)
    for key in ('exp_avg', 'exp_avg_sq'):
        assert all(torch.equal(b.state[p][key], a.state[p][key]) for p in ps)
    sd = copy.deepcopy(b.state_dict())
    assert set(sd['param_groups'][0]) == set(a.state_dict()['param_groups'][0])
    c = torch.optim.AdamW([{'params': ps[:2]}, {'params': ps[2:]}])
    c.load_state_dict(sd)
    before = [p.detach().clone() for p in ps]
    c.step()
    assert [float(c.state[p]['step']) for p in ps] == [4.0, 1.0, 4.0]
    assert not torch.equal(ps[0].detach(), before[0]) and torch.equal(ps[1].detach(), before[1])


def test_decay_groups_split_a_bert():
    from transformers import BertConfig, BertModel
    from aspire_amd.optim import decay_groups
    bert = BertModel(BertConfig(vocab_size=50, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                                max_position_embeddings=16), add_pooling_layer=True)
    groups = decay_groups(bert, 0.01)
    assert [g['weight_decay'] for g in groups] == [0.01, 0.0]
    names = {id(p): n for n, p in bert.named_parameters()}
    plain = {names[id(p)] for p in groups[1]['params']}
    decayed = {names[id(p)] for p in groups[0]['params']}
    assert plain == {n for n in names.values() if n.endswith('bias') or n.endswith('LayerNorm.weight')}
    assert decayed == set(names.values()) - plain and decayed and all(n.endswith('weight') for n in decayed)
    assert 'embeddings.LayerNorm.weight' in plain and 'encoder.layer.0.output.LayerNorm.weight' in plain
    assert 'embeddings.word_embeddings.weight' in decayed and 'pooler.dense.weight' in decayed
    assert len(plain) + len(decayed) == len(list(bert.parameters()))
    # a LayerNorm under another name is found by its type; a module with nothing to decay gives one group
    seq = torch.nn.Sequential(torch.nn.Linear(3, 3), torch.nn.LayerNorm(3))
    groups = decay_groups(seq, 0.1)
    assert [len(g['params']) for g in groups] == [1, 3] and groups[0]['params'][0] is seq[0].weight
    assert [g['weight_decay'] for g in decay_groups(torch.nn.LayerNorm(3), 0.1)] == [0.0]


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------------
def _grad_table(*entries):
    from aspire_amd import _lib
    return (_lib.GradTensor * max(len(entries), 1))(*[_lib.GradTensor(g, n) for g, n in entries])


def test_norm_and_scale_argument_errors_need_no_device():
    from aspire_amd import _lib
    lib, bad, err = _lib.lib, _lib.ASPIRE_ERR_INVALID_ARG, lambda: _lib.lib.aspire_last_error().decode()
    nan, inf = float('nan'), float('inf')

    def norm(table=None, n=1, max_norm=1.0, out=256, ws=4096, ws_bytes=1 << 20):
        return lib.aspire_grad_norm_f32(table if table is not None else _grad_table((128, 8)), n, max_norm, out, ws, ws_bytes, None)

    def scale(table=None, n=1, s=256, ws=4096, ws_bytes=1 << 20):
        return lib.aspire_grad_scale_f32(table if table is not None else _grad_table((128, 8)), n, s, ws, ws_bytes, None)

    for m in (0.0, -1.0, nan, inf, 1e39):
        assert norm(max_norm=m) == bad and 'max_norm' in err()
    assert norm(out=None) == bad and 'out' in err()
    assert norm(out=258) == bad and 'aligned' in err()
    assert scale(s=None) == bad and 'scale' in err()
    assert scale(s=258) == bad and 'aligned' in err()
    for call in (norm, scale):
        assert call(n=-2) == bad and '-2' in err()
        assert call(_grad_table((128, -5))) == bad and '-5' in err()
        assert call(_grad_table((130, 8))) == bad and 'aligned' in err()
        assert call(ws=None) == bad and 'workspace' in err()
        assert call(ws=4100) == bad and '16-byte' in err()
    sizes = (ctypes.c_int64 * 3)(8, 4097, 0)
    need = lib.aspire_grad_norm_workspace_bytes(sizes, 3)
    assert need % 16 == 0 and need >= 3 * 32 + 4 * 4 + 3 * 8          # three records, four prefix sums, three chunks' partials
    table = _grad_table((128, 8), (4096, 4097), (0, 0))
    assert norm(table, n=3, ws_bytes=need - 16) == bad and str(need) in err()
    assert lib.aspire_grad_norm_workspace_bytes(sizes, -1) == 0 and lib.aspire_grad_norm_workspace_bytes(None, 2) == 0
    assert lib.aspire_grad_norm_workspace_bytes((ctypes.c_int64 * 1)(-3), 1) == 0
    assert lib.aspire_grad_norm_workspace_bytes(None, 0) == 16
    assert scale(ws_bytes=lib.aspire_grad_scale_workspace_bytes(1) - 1) == bad and 'small' in err()
    # nothing to scale: no launch, no device
    assert scale(_grad_table((0, 0))) == _lib.ASPIRE_OK and scale(None, n=0) == _lib.ASPIRE_OK
    assert scale(_grad_table((0, 9))) == _lib.ASPIRE_OK               # a NULL gradient is an absent one


def _optim_table(cls, **over):
    base = dict(param=64, grad=128, state1=192, state2=256, n=8, step=1, lr=1e-3)
    base.update(over)
    return (cls * 1)(cls(**base))


def test_scaled_and_decayed_step_argument_errors_need_no_device():
    from aspire_amd import _lib
    lib, bad, err = _lib.lib, _lib.ASPIRE_ERR_INVALID_ARG, lambda: _lib.lib.aspire_last_error().decode()
    nan, inf = float('nan'), float('inf')
    assert ctypes.sizeof(_lib.AdamWTensor) == 64 and ctypes.sizeof(_lib.OptimTensor) == 56      # the old record keeps its layout

    def adamw(table=None, n=1, gs=512, ws=4096, ws_bytes=1 << 20, **over):
        table = table if table is not None else _optim_table(_lib.AdamWTensor, weight_decay=0.01, **over)
        return lib.aspire_adamw_step_f32(table, n, 0.9, 0.999, 1e-8, gs, ws, ws_bytes, None)

    def adam(gs=512, ws=4096, **over):
        return lib.aspire_adam_step_scaled_f32(_optim_table(_lib.OptimTensor, **over), 1, 0.9, 0.999, 1e-8, gs, ws, 1 << 20, None)

    def adagrad(gs=512, ws=4096, **over):
        return lib.aspire_adagrad_step_scaled_f32(_optim_table(_lib.OptimTensor, **over), 1, 0.0, 1e-10, gs, ws, 1 << 20, None)

    for call in (adamw, adam, adagrad):
        assert call(gs=514) == bad and 'grad_scale' in err()
        assert call(step=0) == bad and 'step = 0' in err()
        assert call(param=66) == bad and 'aligned' in err()
        assert call(lr=-1.0) == bad and 'lr' in err()
        assert call(ws=None) == bad and 'workspace' in err()
        assert call(n=0, param=0, grad=0, state1=0, state2=0) == _lib.ASPIRE_OK         # nothing to do: no launch
        assert call(gs=None, n=0, param=0, grad=0, state1=0, state2=0) == _lib.ASPIRE_OK
    for wd in (-0.01, nan, inf):
        assert adamw(_optim_table(_lib.AdamWTensor, weight_decay=wd)) == bad and 'weight_decay' in err()
    assert adamw(None, n=-2) == bad and '-2' in err()
    assert adamw(state2=0) == bad and 'null' in err()


# ---- the yardstick against torch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_norm', [None, crf.MAX_NORM])
def test_float64_restatement_is_what_torch_computes(max_norm):
    """tests/clip_ref.py's AdamW (+ clip) in float32 numpy stays inside bound(|torch fp32 - float64|, max|float64|) of its float64
    form on every tensor: the bound the GPU test uses is one the formulas' own fp32 arithmetic meets, and the clip bites"""
    ref64 = crf.run_reference('adamw', max_norm)
    t32 = crf.torch_cpu('adamw', max_norm)
    np32 = crf.run_reference('adamw', max_norm, dtype=np.float32)
    worst = crf.compare(np32, ref64, t32, 'adamw', f'numpy fp32 adamw clip={max_norm}')
    print(f'largest error / bound: {worst:.3f}')
    for spec in orf.case_specs():
        assert ref64[spec['name']]['step'] == t32[spec['name']]['step'] == (0 if spec.get('frozen') else 3 if spec.get('none_on_even') else 6)
    plain = orf.run_reference('adam')
    assert any(np.abs(ref64[n]['p'] - plain[n]['p']).max() > 1e-4 for n in ref64)          # the decay is not a no-op
    if max_norm is not None:
        for k in range(1, orf.STEPS + 1):
            norm = crf.total_norm([orf.grad_value(s, k) for s in orf.case_specs()])
            assert crf.clip_coef(norm, max_norm) < 1e-2                                      # every step is clipped, hard


# ---- RankTrainer's host logic ----------------------------------------------------------------------------------------------------------
class _ScaledSGD(torch.optim.SGD):
    """an optimizer with the project's step(closure, grad_scale) on the host"""

    def __init__(self, params, lr, events):
        super().__init__(params, lr=lr)
        self.events = events

    def step(self, closure=None, grad_scale=None):
        self.events.append(('step', None if grad_scale is None else float(grad_scale)))
        if grad_scale is not None:
            for group in self.param_groups:
                for p in group['params']:
                    if p.grad is not None:
                        p.grad = p.grad * grad_scale
        return super().step(closure)

    def zero_grad(self, set_to_none=True):
        self.events.append(('zero', None))
        return super().zero_grad(set_to_none)


def _host_grad_norm(events):
    def grad_norm(parameters, max_norm):
        grads = [p.grad for p in parameters if p.grad is not None]
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
        events.append(('norm', float(norm)))
        return norm, torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return grad_norm


def _hparams(**over):
    hp = dict(es_check_every=1000, train_size=8, dev_size=2, batch_size=2, num_epochs=2, update_rule='adam', learning_rate=0.1,
              lr_decay_method='exponential', decay_lr_by=0.5, decay_lr_every=1000, num_warmup_steps=3)
    hp.update(over)
    return hp


def _toy(tmp_path, hp, monkeypatch, events):
    from aspire_amd import RankTrainer, optim
    monkeypatch.setattr(optim, 'grad_norm', _host_grad_norm(events))
    torch.manual_seed(0)
    enc = torch.nn.Linear(3, 1)
    opt = _ScaledSGD(enc.parameters(), 0.1, events)
    batches = [torch.randn(2, 3) for _ in range(4)]
    tr = RankTrainer(enc, None, hp, str(tmp_path), lambda epoch: list(batches), optimizer=opt, loss_fn=lambda b, e: e(b).pow(2).sum())
    return tr, enc, batches


def test_trainer_takes_the_norm_then_steps_with_its_coefficient(tmp_path, monkeypatch):
    events = []
    tr, enc, batches = _toy(tmp_path, _hparams(max_grad_norm=0.05), monkeypatch, events)
    probe = copy.deepcopy(enc)
    tr.train()
    assert [e[0] for e in events] == ['zero', 'norm', 'step'] * 8
    for (_, norm), (_, coef) in zip(events[1::3], events[2::3]):
        assert coef == pytest.approx(0.05 / (norm + 1e-6)) and coef < 1             # every step is clipped
    # the first update: one SGD step on the clipped gradient
    probe(batches[0]).pow(2).sum().backward()
    norm = torch.sqrt(sum(p.grad.pow(2).sum() for p in probe.parameters()))
    assert float(norm) == pytest.approx(events[1][1], rel=1e-6)
    # the norm is logged where the loss is, and the checkpoint needs nothing else to carry it on
    assert tr.loss_checked_iters == [0, 5] and len(tr.loss_history['loss']) == len(tr.loss_history['grad_norm']) == 2
    assert tr.loss_history['grad_norm'] == [pytest.approx(events[1][1]), pytest.approx(events[3 * 5 + 1][1])]
    tr.save_checkpoint(tmp_path / 'ck.pt')
    events2 = []
    tr2, *_ = _toy(tmp_path / 'b', _hparams(max_grad_norm=0.05), monkeypatch, events2)
    tr2.load_checkpoint(tmp_path / 'ck.pt')
    assert tr2.loss_history['grad_norm'] == tr.loss_history['grad_norm'] and tr2.last_grad_norm == pytest.approx(events[-2][1])


@pytest.mark.parametrize('off', [dict(), dict(max_grad_norm=None), dict(max_grad_norm=0), dict(max_grad_norm=0.0)])
def test_trainer_without_max_grad_norm_steps_as_before(off, tmp_path, monkeypatch):
    events = []
    tr, *_ = _toy(tmp_path, _hparams(**off), monkeypatch, events)
    tr.train()
    assert events == [('zero', None), ('step', None)] * 8 and 'grad_norm' not in tr.loss_history and tr.last_grad_norm is None


def test_trainer_clips_once_per_accumulated_group(tmp_path, monkeypatch):
    events = []
    tr, enc, batches = _toy(tmp_path, _hparams(max_grad_norm=0.05, accumulated_batch_size=6), monkeypatch, events)
    probe = copy.deepcopy(enc)
    tr.train()
    assert tr.iteration == 8 and [e[0] for e in events] == ['norm', 'step', 'zero'] * 2       # after iterations 2 and 5
    sum(probe(b).pow(2).sum() for b in batches[:3]).backward()                                   # the norm of the accumulated SUM
    want = torch.sqrt(sum(p.grad.pow(2).sum() for p in probe.parameters()))
    assert events[0][1] == pytest.approx(float(want), rel=1e-6)
    for bad in (-1.0, float('inf')):
        with pytest.raises(ValueError, match='max_grad_norm'):
            _toy(tmp_path, _hparams(max_grad_norm=bad), monkeypatch, [])


def test_adamw_is_an_update_rule(tmp_path):
    from aspire_amd import HipAdamW, RankTrainer
    enc = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.LayerNorm(4))
    tr = RankTrainer(enc, None, _hparams(update_rule='adamw'), str(tmp_path), lambda e: [], loss_fn=lambda b, e: None)
    assert isinstance(tr.optimizer, HipAdamW)
    assert [(len(g['params']), g['weight_decay'], g['lr']) for g in tr.optimizer.param_groups] == [(1, 0.01, 0.1), (3, 0.0, 0.1)]
    tr = RankTrainer(enc, None, _hparams(update_rule='adamw', weight_decay=0.3), str(tmp_path), lambda e: [], loss_fn=lambda b, e: None)
    assert [g['weight_decay'] for g in tr.optimizer.param_groups] == [0.3, 0.0]
    with pytest.raises(ValueError, match='upate rule'):
        RankTrainer(enc, None, _hparams(update_rule='sgd'), str(tmp_path), lambda e: [], loss_fn=lambda b, e: None)


def test_only_the_l2_norm_is_built():
    from aspire_amd import clip_grad_norm_
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    for norm_type in (1.0, float('inf'), 3):
        with pytest.raises(NotImplementedError, match='norm_type'):
            clip_grad_norm_([p], 1.0, norm_type=norm_type)
    with pytest.raises(RuntimeError, match='GPU'):              # what optim_tensor_check refuses
        clip_grad_norm_([p], 1.0)
    with pytest.raises(ValueError, match='max_norm'):
        clip_grad_norm_([p], 0.0)


# ---- two ranks over gloo --------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _entry(rank, world, port, fn, ret, *args):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world, timeout=TIMEOUT)
    try:
        ret[rank] = fn(rank, world, *args)
    finally:
        dist.destroy_process_group()


def _spawn(fn, world, *args):
    ret = mp.Manager().dict()
    mp.spawn(_entry, args=(world, _free_port(), fn, ret) + args, nprocs=world, join=True)
    return dict(ret)


def _encoder(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3), torch.nn.Linear(3, 2))


def _batch(rank, it):
    return torch.randn(4, 5, generator=torch.Generator().manual_seed(100 + 10 * it + rank))


def _loss(batch, encoder):
    return encoder[:3](batch).pow(2).sum()          # the last Linear never has a gradient, on any rank


COLLECTIVES = ('all_reduce', 'broadcast', 'barrier', 'all_gather_into_tensor', 'all_gather', 'reduce', 'gather', 'scatter',
               'reduce_scatter_tensor', 'all_to_all_single', 'send', 'recv')


def _clip_worker(rank, world, path, max_grad_norm):
    from aspire_amd import RankTrainerDDP, optim
    events, calls = [], []
    optim.grad_norm = _host_grad_norm(events)
    enc = _encoder(7 + rank)
    opt = _ScaledSGD(enc.parameters(), 0.05, events)
    hp = _hparams(es_check_every=4, train_size=24, batch_size=4, num_epochs=1, learning_rate=0.05, max_grad_norm=max_grad_norm)
    tr = RankTrainerDDP(enc, None, hp, os.path.join(path, f'rank{rank}'), lambda epoch: [_batch(rank, it) for it in range(3)],
                        (lambda: [_batch(9, 9)]) if rank == 0 else None, optimizer=opt, loss_fn=_loss)
    for name in COLLECTIVES:        # counted from here on: construction is the same with and without clipping
        inner = getattr(dist, name)
        setattr(dist, name, lambda *a, _inner=inner, _name=name, **k: (calls.append(_name), _inner(*a, **k))[1])
    seen = []
    step = tr._step

    def spy():
        step()
        seen.append([None if p.grad is None else p.grad.clone() for p in enc.parameters()])

    tr._step = spy
    tr.train()
    return dict(calls=calls, events=events, params=[p.detach().clone() for p in enc.parameters()], grads=seen,
                history=dict(tr.loss_history))


def test_clipping_under_ddp_issues_no_collective_of_its_own(tmp_path):
    plain = _spawn(_clip_worker, 2, str(tmp_path / 'plain'), None)
    clipped = _spawn(_clip_worker, 2, str(tmp_path / 'clipped'), 0.01)
    for r in (0, 1):
        assert clipped[r]['calls'] == plain[r]['calls'] and clipped[r]['calls'].count('all_reduce') >= 3
        assert [e[0] for e in plain[r]['events']] == ['zero', 'step'] * 3
        assert [e[0] for e in clipped[r]['events']] == ['zero', 'norm', 'step'] * 3          # the norm behind the reduction
    # both ranks formed the same norm and coefficient from the same reduced bits, and end on the same parameters
    assert clipped[0]['events'] == clipped[1]['events'] and all(e[1] < 1 for e in clipped[0]['events'] if e[0] == 'step')
    for a, b in zip(clipped[0]['params'], clipped[1]['params']):
        assert torch.equal(a, b)
    assert len(clipped[0]['history']['grad_norm']) == len(clipped[0]['history']['loss']) == 2 and clipped[1]['history'] == {}
    # one process, rank 0's start, the gradient 0.5 g_a + 0.5 g_b, the same clip: the unused Linear stays out of the norm
    enc = _encoder(7)
    for it in range(3):
        grads = []
        for r in (0, 1):
            enc.zero_grad()
            _loss(_batch(r, it), enc).backward()
            grads.append([None if p.grad is None else p.grad.clone() for p in enc.parameters()])
        mean = [None if ga is None else 0.5 * ga + 0.5 * gb for ga, gb in zip(*grads)]
        assert [g is None for g in mean] == [False] * 4 + [True] * 2
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in mean if g is not None]))
        assert float(norm) == clipped[0]['events'][3 * it + 1][1]
        coef = torch.clamp(0.01 / (norm + 1e-6), max=1.0)
        with torch.no_grad():
            for p, g in zip(enc.parameters(), mean):
                if g is not None:
                    p -= 0.05 * (g * coef)
    for p, got in zip(enc.parameters(), clipped[0]['params']):
        assert torch.equal(p.detach(), got)
