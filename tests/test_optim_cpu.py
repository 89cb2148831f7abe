"""CPU: the optimizer entries' argument checks (no device is touched), the yardstick of tests/optim_ref.py against torch.optim on the
CPU, and RankTrainer's host logic on a toy (a Linear encoder, a loss function and a CPU torch.optim optimizer injected)."""
import copy
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as orf  # noqa: E402


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------------
def _table(**over):
    from aspire_amd import _lib
    base = dict(param=64, grad=128, state1=192, state2=256, n=8, step=1, lr=1e-3)
    base.update(over)
    return (_lib.OptimTensor * 1)(_lib.OptimTensor(**base))


def _adam(table, n=1, b1=0.9, b2=0.999, eps=1e-8, ws=4096, ws_bytes=1 << 20):
    from aspire_amd import _lib
    return _lib.lib.aspire_adam_step_f32(table, n, b1, b2, eps, ws, ws_bytes, None)


def _adagrad(table, n=1, lr_decay=0.0, eps=1e-10, ws=4096, ws_bytes=1 << 20):
    from aspire_amd import _lib
    return _lib.lib.aspire_adagrad_step_f32(table, n, lr_decay, eps, ws, ws_bytes, None)


def test_argument_errors_need_no_device():
    from aspire_amd import _lib
    bad, err = _lib.ASPIRE_ERR_INVALID_ARG, lambda: _lib.lib.aspire_last_error().decode()
    nan, inf = float('nan'), float('inf')
    for call in (_adam, _adagrad):
        assert call(None, n=3) == bad and '3' in err()                                     # NULL table with tensors to do
        assert call(_table(), n=-2) == bad and '-2' in err()
        assert call(_table(n=-5)) == bad and '-5' in err()
        assert call(_table(step=0)) == bad and 'step = 0' in err()
        for field in ('param', 'grad', 'state1'):
            assert call(_table(**{field: 0})) == bad and 'null' in err()
        assert call(_table(param=66)) == bad and 'aligned' in err()
        for lr in (-1e-3, nan, inf):
            assert call(_table(lr=lr)) == bad and 'lr' in err()
        for eps in (-1e-8, nan, inf):
            assert call(_table(), eps=eps) == bad and 'eps' in err()
        assert call(_table(), ws=None) == bad and 'workspace' in err()
        need = _lib.lib.aspire_optim_workspace_bytes(1)
        assert call(_table(), ws_bytes=need - 1) == bad and str(need) in err()
        # nothing to do: no launch, no device
        assert call(None, n=0) == _lib.ASPIRE_OK
        assert call(_table(n=0, param=0, grad=0, state1=0, state2=0)) == _lib.ASPIRE_OK
    assert _adam(_table(state2=0)) == bad and 'null' in err()
    assert _adagrad(_table(state2=0, n=0)) == _lib.ASPIRE_OK                               # Adagrad has no second state
    for b in (-0.1, 1.0, nan):
        assert _adam(_table(), b1=b) == bad and 'beta1' in err()
        assert _adam(_table(), b2=b) == bad and 'beta2' in err()
    for d in (-1.0, nan, inf):
        assert _adagrad(_table(), lr_decay=d) == bad and 'lr_decay' in err()
    with pytest.raises(AssertionError):
        _lib.check(_adam(_table(step=-1)))


def test_workspace_bytes():
    from aspire_amd import _lib
    sizes = [_lib.lib.aspire_optim_workspace_bytes(n) for n in range(0, 400)]
    assert all(s % 16 == 0 and s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[399] > sizes[1]
    assert ctypes.sizeof(_lib.OptimTensor) == 56


def test_chunk_matches_the_kernels():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'aspire_amd', 'csrc', 'tuning.h')).read()
    assert f'constexpr int kOptimChunk = {orf.CHUNK};' in text


# ---- the yardstick against torch -------------------------------------------------------------------------------------------------------
def _torch_cpu(rule):
    run = orf.Run('cpu')
    if rule == 'adam':
        opt = torch.optim.Adam(run.groups(), foreach=False, **orf.ADAM)
    else:
        opt = torch.optim.Adagrad(run.groups(), foreach=False, **orf.ADAGRAD)
    return run.steps(opt, orf.STEPS).result(opt, rule)


@pytest.mark.parametrize('rule', ['adam', 'adagrad'])
def test_fp32_restatement_is_inside_the_bound(rule):
    """the bound the GPU tests use is one the formulas' own fp32 arithmetic meets: a plain float32 numpy restatement stays inside
    bound(|torch fp32 - float64|, max|float64|) on every tensor of the shared case, with the per-tensor step counts equal to torch's"""
    ref64 = orf.run_reference(rule)
    t32 = _torch_cpu(rule)
    np32 = orf.run_reference(rule, dtype=np.float32)
    worst = orf.compare(np32, ref64, t32, rule, f'numpy fp32 {rule}')
    print(f'largest error / bound: {worst:.3f}')
    for spec in orf.case_specs():
        assert ref64[spec['name']]['step'] == t32[spec['name']]['step'] == (0 if spec.get('frozen') else 3 if spec.get('none_on_even') else 6)
    # torch's own fp32 against float64 is not zero (the bound is not vacuous) and the frozen tensor did not move
    assert any(np.abs(t32[n]['p'] - ref64[n]['p']).max() > 0 for n in ref64)
    frozen = next(s for s in orf.case_specs() if s.get('frozen'))
    assert np.array_equal(t32['frozen']['p'], orf.init_value(frozen))


# ---- RankTrainer's host logic ------------------------------------------------------------------------------------------------------------
class _Spy(torch.optim.SGD):
    def __init__(self, params, lr):
        super().__init__(params, lr=lr)
        self.events = []

    def step(self, closure=None):
        self.events.append('step')
        return super().step(closure)

    def zero_grad(self, set_to_none=True):
        self.events.append('zero')
        return super().zero_grad(set_to_none)


def _hparams(**over):
    hp = dict(es_check_every=1000, train_size=8, dev_size=2, batch_size=2, num_epochs=2, update_rule='adam', learning_rate=0.1,
              lr_decay_method='exponential', decay_lr_by=0.5, decay_lr_every=2, num_warmup_steps=3)
    hp.update(over)
    return hp


def _toy(tmp_path, hp, dev=None, n_batches=4, **kw):
    from aspire_amd import RankTrainer
    torch.manual_seed(0)
    enc = torch.nn.Linear(3, 1)
    opt = _Spy(enc.parameters(), lr=hp.get('learning_rate', 0.1))
    batches = [torch.randn(2, 3) for _ in range(n_batches)]
    seen = []

    def loss_fn(batch, encoder):
        seen.append(batch)
        return encoder(batch).pow(2).sum()

    tr = RankTrainer(enc, None, hp, str(tmp_path), lambda epoch: list(batches), dev, optimizer=opt, loss_fn=loss_fn, **kw)
    return tr, enc, opt, seen


@pytest.mark.parametrize('method', ['exponential', 'warmuplin', 'warmupcosine'])
def test_schedule_follows_the_reference_rule(method, tmp_path):
    """(iteration -> lr, step taken, zero_grad taken) equals what torch's / transformers' schedulers give when driven by the reference's
    rule written out here: scheduler.step() when iteration > 0 and iteration % decay_lr_every == 0 (trainer.py:287), zero_grad + step every
    iteration (trainer.py:261-268), num_training_steps = num_epochs * num_batches (trainer.py:200)"""
    import transformers
    hp = _hparams(lr_decay_method=method)
    tr, enc, opt, _ = _toy(tmp_path, hp)
    lrs = []
    orig = tr._iterate

    def spy(batch):
        orig(batch)
        lrs.append(opt.param_groups[0]['lr'])

    tr._iterate = spy
    assert tr.num_batches == 4 and tr.total_iters == 8
    assert tr.train() is True
    want_opt = torch.optim.SGD(torch.nn.Linear(3, 1).parameters(), lr=0.1)
    if method == 'exponential':
        sch = torch.optim.lr_scheduler.ExponentialLR(want_opt, gamma=0.5)
    elif method == 'warmuplin':
        sch = transformers.get_linear_schedule_with_warmup(want_opt, num_warmup_steps=3, num_training_steps=8)
    else:
        sch = transformers.get_cosine_schedule_with_warmup(want_opt, num_warmup_steps=3, num_training_steps=8)
    want = []
    for it in range(8):
        want_opt.step()
        if it > 0 and it % 2 == 0:
            sch.step()
        want.append(want_opt.param_groups[0]['lr'])
    assert lrs == want and len(set(want)) > 1
    assert opt.events == ['zero', 'step'] * 8
    assert tr.iteration == 8 and tr.loss_checked_iters == [0, 5] and len(tr.loss_history['loss']) == 2
    assert os.path.exists(tmp_path / 'model_final.pt') and not os.path.exists(tmp_path / 'model_cur_best.pt')


def test_accumulation_applies_whole_groups_only(tmp_path):
    """update_params_every = 3 over 8 iterations: two updates, after iterations 2 and 5 (trainer.py:256); the trailing two batches are
    never applied; gradients are summed, not averaged"""
    hp = _hparams(accumulated_batch_size=6, num_epochs=2, decay_lr_every=1000)
    tr, enc, opt, seen = _toy(tmp_path, hp)
    probe = torch.nn.Linear(3, 1)
    probe.load_state_dict(enc.state_dict())
    tr.train(max_iterations=3)
    assert opt.events == ['step', 'zero']
    # one SGD step on the SUM of the three batches' gradients
    sum(probe(b).pow(2).sum() for b in seen[:3]).backward()
    assert torch.allclose(enc.weight.detach(), probe.weight.detach() - 0.1 * probe.weight.grad, rtol=1e-6, atol=1e-7)
    tr.train()
    assert tr.iteration == 8 and opt.events == ['step', 'zero'] * 2
    assert tr.update_params_every == 3
    with pytest.raises(AssertionError):
        _toy(tmp_path, _hparams(accumulated_batch_size=5))
    assert _toy(tmp_path, _hparams(accumulated_batch_size=-1))[0].accumulate_gradients is False


def test_early_stop_keeps_the_best(tmp_path):
    script = iter([5.0, 3.0, 4.0, 2.0, 6.0])
    hp = _hparams(es_check_every=1, num_epochs=1, train_size=12, decay_lr_every=1000)
    tr, enc, opt, _ = _toy(tmp_path, hp, dev=lambda: [None], n_batches=6)
    inner = tr.loss_fn
    saved = []

    def loss_fn(batch, encoder):
        if batch is None:
            assert not encoder.training and not torch.is_grad_enabled()
            return torch.tensor(next(script))
        return inner(batch, encoder)

    tr.loss_fn = loss_fn
    save = tr._save_model
    tr._save_model = lambda suffix: (saved.append((suffix, tr.iteration)), save(suffix))
    tr.train()
    # iteration 0 is never checked (trainer.py:294); the scripted losses arrive at iterations 1..5
    assert tr.dev_checked_iters == [1, 2, 3, 4, 5] and tr.dev_score_history == [-5.0, -3.0, -4.0, -2.0, -6.0]
    assert tr.best_dev_score == -2.0 and tr.best_iter == 4
    assert saved == [('cur_best', 1), ('cur_best', 2), ('cur_best', 4), ('final', 6)]
    best = torch.load(tmp_path / 'model_cur_best.pt', weights_only=True)
    final = torch.load(tmp_path / 'model_final.pt', weights_only=True)
    assert set(best) == set(final) == {'weight', 'bias'} and not torch.equal(best['weight'], final['weight'])
    assert torch.equal(final['weight'], enc.weight.detach())
    # early_stop=False: no dev pass at all
    tr2, *_ = _toy(tmp_path / 'b', hp, dev=lambda: pytest.fail('dev pass without early_stop'), n_batches=6, early_stop=False)
    tr2.train()
    assert tr2.dev_checked_iters == []


def test_unknown_rules_raise(tmp_path):
    from aspire_amd import RankTrainer
    enc = torch.nn.Linear(3, 1)
    with pytest.raises(ValueError, match='upate rule'):
        RankTrainer(enc, None, _hparams(update_rule='sgd'), str(tmp_path), lambda e: [], loss_fn=lambda b, e: None)
    with pytest.raises(ValueError, match='lr_decay_method'):
        _toy(tmp_path, _hparams(lr_decay_method='plateau'))


class _DropEnc(torch.nn.Linear):
    seed, step = 11, 0

    def dropout_state(self):
        return self.seed, self.step

    def set_dropout_state(self, seed, step):
        self.seed, self.step = seed, step


def test_checkpoint_round_trips_every_field(tmp_path):
    from aspire_amd import RankTrainer
    hp = _hparams(lr_decay_method='warmupcosine', decay_lr_every=1, es_check_every=2, num_epochs=3)
    torch.manual_seed(3)
    batches = [torch.randn(2, 3) for _ in range(4)]
    dev = [torch.randn(2, 3)]
    consumed = []

    def make(tag):
        torch.manual_seed(5)
        enc = _DropEnc(3, 1)
        opt = torch.optim.Adam(enc.parameters(), lr=0.1)

        def loss_fn(batch, encoder):
            if encoder.training:
                encoder.step += 1
                consumed.append((tag, int(batch[0, 0] * 1e6)))
            return encoder(batch).pow(2).sum()

        return RankTrainer(enc, None, hp, str(tmp_path / tag), lambda epoch: list(batches), lambda: dev, optimizer=opt, loss_fn=loss_fn)

    straight = make('straight')
    straight.train(max_iterations=10)
    first = make('first')
    first.train(max_iterations=6)          # stops inside the second epoch, two batches in
    assert (first.iteration, first.epoch, first.batch_in_epoch) == (6, 1, 2)
    first.save_checkpoint(tmp_path / 'ck.pt')
    second = make('second')
    second.encoder.set_dropout_state(0, 0)
    second.load_checkpoint(tmp_path / 'ck.pt')
    for field in ('iteration', 'epoch', 'batch_in_epoch', 'best_dev_score', 'best_iter', 'loss_checked_iters', 'dev_score_history',
                  'dev_checked_iters'):
        assert getattr(second, field) == getattr(first, field), field
    assert dict(second.loss_history) == dict(first.loss_history) and first.dev_checked_iters == [2, 4]
    assert second.encoder.dropout_state() == first.encoder.dropout_state() == (11, 6)
    assert second.scheduler.state_dict() == first.scheduler.state_dict()
    assert second.optimizer.param_groups[0]['lr'] == first.optimizer.param_groups[0]['lr'] != 0.1
    for a, b in zip(second.encoder.parameters(), first.encoder.parameters()):
        assert torch.equal(a, b)
        sa, sb = second.optimizer.state[a], first.optimizer.state[b]
        assert all(torch.equal(sa[k], sb[k]) for k in ('step', 'exp_avg', 'exp_avg_sq'))
    second.train(max_iterations=4)
    # the resumed run consumed the batches the straight run did after iteration 6, and ends where it ends, bit for bit
    assert [b for t, b in consumed if t == 'second'] == [b for t, b in consumed if t == 'straight'][6:]
    assert second.iteration == straight.iteration == 10
    for a, b in zip(second.encoder.parameters(), straight.encoder.parameters()):
        assert torch.equal(a, b)
    assert second.optimizer.param_groups[0]['lr'] == straight.optimizer.param_groups[0]['lr']
    assert second.dev_score_history == straight.dev_score_history and second.loss_history == straight.loss_history
    # inside a group of accumulated batches there is nothing consistent to save
    acc, *_ = _toy(tmp_path / 'acc', _hparams(accumulated_batch_size=4))
    acc.train(max_iterations=1)
    with pytest.raises(ValueError, match='accumulated'):
        acc.save_checkpoint(tmp_path / 'no.pt')


@pytest.mark.parametrize('rule', ['adam', 'adagrad'])
def test_state_dict_layout_goes_through_torch_and_back(rule):
    """host side of the interchange, no GPU: a torch optimizer's state dict loads; every 'step' is then a CPU float32 scalar tensor
    with torch's value (a view into the optimizer's one count tensor); the state dict saved here loads back into torch, which steps on"""
    from aspire_amd import HipAdam, HipAdagrad
    mine, theirs = (HipAdam, torch.optim.Adam) if rule == 'adam' else (HipAdagrad, torch.optim.Adagrad)
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (3, 5, 2)]
    a = theirs([{'params': ps[:2], 'lr': 0.1}, {'params': ps[2:], 'lr': 0.2}])
    for k in range(3):
        for i, p in enumerate(ps):
            p.grad = None if (i == 1 and k != 1) else torch.randn_like(p)
        a.step()
    b = mine([{'params': ps[:2]}, {'params': ps[2:]}])
    b.load_state_dict(a.state_dict())
    assert [g['lr'] for g in b.param_groups] == [0.1, 0.2]
    steps = [b.state[p]['step'] for p in ps]
    assert [float(s) for s in steps] == [3.0, 1.0, 3.0]
    assert all(s.dtype == torch.float32 and s.device.type == 'cpu' and s.dim() == 0 for s in steps)
    assert len({s.untyped_storage().data_ptr() for s in steps}) == 1 and all(s is not a.state[p]['step'] for s, p in zip(steps, ps))
    for key in ('exp_avg', 'exp_avg_sq') if rule == 'adam' else ('sum',):
        assert all(torch.equal(b.state[p][key], a.state[p][key]) for p in ps)
    sd = copy.deepcopy(b.state_dict())          # (as through torch.save: torch's load_state_dict keeps the step tensors it is given)
    assert set(sd['param_groups'][0]) == set(a.state_dict()['param_groups'][0])
    c = theirs([{'params': ps[:2]}, {'params': ps[2:]}])
    c.load_state_dict(sd)
    before = [p.detach().clone() for p in ps]
    c.step()
    assert [float(c.state[p]['step']) for p in ps] == [4.0, 1.0, 4.0]
    assert not torch.equal(ps[0].detach(), before[0]) and torch.equal(ps[1].detach(), before[1])
    # a later group rebuilds the count tensor; the counts come along
    extra = torch.nn.Parameter(torch.zeros(4))
    b.add_param_group({'params': [extra]})
    b._home_steps()
    assert [float(b.state[p]['step']) for p in ps] == [3.0, 1.0, 3.0] and extra not in b.state


def test_optimizers_refuse_what_is_not_built():
    """construction needs no GPU: the unsupported options raise NotImplementedError, torch's own value checks still apply, and the param
    groups carry every key of torch's optimizer (what makes the state dicts interchangeable)"""
    from aspire_amd import HipAdam, HipAdagrad
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True),
               dict(lr=torch.tensor(1e-3))):
        with pytest.raises(NotImplementedError):
            HipAdam(p, **kw)
    for kw in (dict(weight_decay=0.01), dict(maximize=True), dict(differentiable=True), dict(initial_accumulator_value=0.1),
               dict(lr=torch.tensor(1e-3))):
        with pytest.raises(NotImplementedError):
            HipAdagrad(p, **kw)
    with pytest.raises(ValueError):
        HipAdam(p, betas=(1.0, 0.999))
    with pytest.raises(ValueError):
        HipAdam(p, lr=-1.0)
    assert set(HipAdam(p).param_groups[0]) == set(torch.optim.Adam(p).param_groups[0])
    assert set(HipAdagrad(p).param_groups[0]) == set(torch.optim.Adagrad(p).param_groups[0])
    opt = HipAdam(p, lr=0.5)
    assert opt.param_groups[0]['lr'] == 0.5 and opt.param_groups[0]['betas'] == (0.9, 0.999) and opt.param_groups[0]['eps'] == 1e-8
    assert HipAdagrad(p).param_groups[0]['lr'] == 1e-2 and HipAdagrad(p).param_groups[0]['eps'] == 1e-10
    assert opt.step() is None and len(opt.state) == 0          # no gradient anywhere: nothing to launch, no state
    p[0].grad = torch.zeros(3)
    with pytest.raises(RuntimeError, match='GPU'):
        opt.step()
    opt.param_groups[0]['weight_decay'] = 0.1                  # edited by hand (or loaded): refused at step()
    with pytest.raises(NotImplementedError):
        opt.step()
