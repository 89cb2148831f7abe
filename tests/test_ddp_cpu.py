"""CPU: the gradient bucket's layout and the pack entry's argument checks (no device is touched), and the host logic of
aspire_amd.ddp -- GradReducer, broadcast_parameters, RankTrainerDDP -- with two ranks over gloo on CPU tensors (a small nn.Linear stack
as the encoder, a loss function and torch.optim.Adam injected, as tests/test_optim_cpu.py does for RankTrainer)."""
import ctypes
import datetime
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

TIMEOUT = datetime.timedelta(seconds=60)


# ---- the layout and the C ABI without a device ----------------------------------------------------------------------------------------
def test_layout():
    from aspire_amd import _lib, ops
    numels = [0, 1, 3, 4, 5, 4097]
    offsets, tail, total = ops.grad_bucket_layout(numels)
    assert offsets == [0, 0, 4, 8, 12, 20]
    assert all(o % 4 == 0 for o in offsets) and offsets == sorted(offsets)
    for i, (o, n) in enumerate(zip(offsets, numels)):       # the regions do not overlap and pad to the next multiple of 4
        nxt = offsets[i + 1] if i + 1 < len(offsets) else tail
        assert nxt == o + (n + 3) // 4 * 4
    assert tail == 20 + 4100 and total == tail + 8          # round_up(6, 4) floats of tail
    assert ops.grad_bucket_layout([]) == ([], 0, 0)
    assert ops.grad_bucket_layout([7]) == ([0], 8, 12)
    with pytest.raises(ValueError):
        ops.grad_bucket_layout([3, -1])
    # the entry itself: offsets may be NULL
    sizes = (ctypes.c_int64 * 6)(*numels)
    assert _lib.lib.aspire_grad_bucket_elems(sizes, 6, None) == total
    assert _lib.lib.aspire_grad_bucket_elems(sizes, -1, None) == -1 and _lib.lib.aspire_grad_bucket_elems(None, 2, None) == -1
    ws = [_lib.lib.aspire_grad_bucket_workspace_bytes(n) for n in range(0, 300)]
    assert all(w % 16 == 0 and w > 0 for w in ws) and all(a <= b for a, b in zip(ws, ws[1:])) and ws[299] > ws[1]
    assert ctypes.sizeof(_lib.GradTensor) == 16


FLAT = 1 << 20          # a made-up, 16-byte aligned device address: the checks never dereference


def _pack(tensors, n=None, scale=0.5, flat=FLAT, flat_elems=None, ws=4096, ws_bytes=1 << 16):
    from aspire_amd import _lib
    n = len(tensors) if n is None else n
    table = (_lib.GradTensor * max(len(tensors), 1))(*[_lib.GradTensor(g, k) for g, k in tensors]) if tensors is not None else None
    if flat_elems is None:
        sizes = (ctypes.c_int64 * max(len(tensors or []), 1))(*[k for _, k in tensors or []])
        flat_elems = _lib.lib.aspire_grad_bucket_elems(sizes, len(tensors or []), None)
    return _lib.lib.aspire_grad_bucket_pack_f32(table, n, scale, flat, flat_elems, ws, ws_bytes, None)


def test_pack_argument_errors_need_no_device():
    from aspire_amd import _lib
    bad, err = _lib.ASPIRE_ERR_INVALID_ARG, lambda: _lib.lib.aspire_last_error().decode()
    good = [(64, 8), (0, 5), (256, 3)]            # far below FLAT: no overlap
    assert _pack(good, n=-2, flat_elems=0) == bad and '-2' in err()
    assert _pack([(64, -5)], flat_elems=4) == bad and '-5' in err()
    assert _pack(None, n=3, flat_elems=4) == bad and 'null' in err()
    assert _pack(good, flat=None) == bad and 'flat' in err()
    assert _pack(good, flat=FLAT + 4) == bad and '16-byte' in err()
    assert _pack(good, flat_elems=24 - 4) == bad and '24' in err()            # 8 + 8 + 4 + a tail of 4
    assert _pack(good, flat_elems=24 + 4) == bad
    assert _pack([(66, 8)]) == bad and '4-byte' in err()
    for scale in (float('nan'), float('inf'), -float('inf'), 1e300):
        assert _pack(good, scale=scale) == bad and 'scale' in err()
    # a gradient that lives in the bucket: its first region, its last element, and a range that covers the whole bucket
    for g, k in ((FLAT, 8), (FLAT + 4 * 7, 1), (FLAT - 16, 64)):
        assert _pack([(g, k)]) == bad and 'overlaps' in err()
    assert _pack([(0, 8)], ws=None) == bad and 'workspace' in err()
    need = _lib.lib.aspire_grad_bucket_workspace_bytes(3)
    assert _pack(good, ws_bytes=need - 1) == bad and str(need) in err()
    assert _pack(good, ws=4096 + 8) == bad and 'workspace' in err()
    with pytest.raises(AssertionError):
        _lib.check(_pack(good, n=-1, flat_elems=0))
    # nothing to do needs no device
    assert _pack([], flat_elems=0) == _lib.ASPIRE_OK


# ---- two ranks over gloo ------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _spawn(fn, world, *args):
    ret = mp.Manager().dict()
    mp.spawn(_entry, args=(world, _free_port(), fn, ret) + args, nprocs=world, join=True)
    return dict(ret)


def _entry(rank, world, port, fn, ret, *args):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world, timeout=TIMEOUT)
    try:
        ret[rank] = fn(rank, world, *args)
    finally:
        dist.destroy_process_group()


def _encoder(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3))


def _batch(rank, it):
    return torch.randn(4, 5, generator=torch.Generator().manual_seed(100 + 10 * it + rank))


def _loss(batch, encoder):
    return encoder(batch).pow(2).sum()


def _hparams(**over):
    hp = dict(es_check_every=4, train_size=24, dev_size=2, batch_size=4, num_epochs=1, update_rule='adam', learning_rate=0.05,
              lr_decay_method='exponential', decay_lr_by=0.5, decay_lr_every=1000, num_warmup_steps=6)
    hp.update(over)
    return hp


def _state(enc, opt):
    out = {n: p.detach().clone() for n, p in enc.named_parameters()}
    for n, p in enc.named_parameters():
        for k, v in opt.state.get(p, {}).items():
            out[f'{n}/{k}'] = torch.as_tensor(v).detach().clone()
    return out


def _train_worker(rank, world, path):
    from aspire_amd import RankTrainerDDP
    enc = _encoder(7 + rank)                      # different weights per rank: the broadcast must make them rank 0's
    opt = torch.optim.Adam(enc.parameters(), lr=0.05)
    dev_calls = []

    def dev():
        dev_calls.append(1)
        return [_batch(9, 9)]

    tr = RankTrainerDDP(enc, None, _hparams(), os.path.join(path, f'rank{rank}'), lambda epoch: [_batch(rank, it) for it in range(3)],
                        dev if rank == 0 else None, optimizer=opt, loss_fn=_loss)
    derived = dict(rank=tr.rank, num_gpus=tr.num_gpus, es=tr.es_check_every, num_train=tr.num_train, num_batches=tr.num_batches,
                   total_iters=tr.total_iters)
    done = tr.train()
    files = sorted(os.listdir(tr.model_path)) if os.path.isdir(tr.model_path) else []
    return dict(derived=derived, done=done, files=files, iteration=tr.iteration, dev_iters=tr.dev_checked_iters, dev_calls=len(dev_calls),
                losses=len(tr.loss_history['loss']), state=_state(enc, opt),
                views=all(p.grad is not None and p.grad.data_ptr() % 16 == 0 and p.grad.is_contiguous() for p in enc.parameters()))


def test_two_ranks_train_to_the_bits_of_the_mean_gradient(tmp_path):
    out = _spawn(_train_worker, 2, str(tmp_path))
    for r in (0, 1):
        # es_check_every 4 // 2, num_train 24 // 2, ceil(12 / 4) batches (trainer.py:520, 770-775)
        assert out[r]['derived'] == dict(rank=r, num_gpus=2, es=2, num_train=12, num_batches=3, total_iters=3)
        assert out[r]['done'] is True and out[r]['iteration'] == 3 and out[r]['views']
    # rank 0 alone keeps the dev history, the loss history and the files; the dev pass ran once, at iteration 2
    assert out[0]['files'] == ['model_cur_best.pt', 'model_final.pt'] and out[1]['files'] == []
    assert out[0]['dev_iters'] == [2] and out[0]['dev_calls'] == 1 and out[0]['losses'] == 2
    assert out[1]['dev_iters'] == [] and out[1]['dev_calls'] == 0 and out[1]['losses'] == 0
    assert set(out[0]['state']) == set(out[1]['state']) and len(out[0]['state']) == 4 * 4
    for key, a in out[0]['state'].items():
        assert torch.equal(a, out[1]['state'][key]), key
    # one process, rank 0's start, the gradient 0.5 g_a + 0.5 g_b: at world 2 the scaling is exact and a + b commutes
    enc = _encoder(7)
    opt = torch.optim.Adam(enc.parameters(), lr=0.05)
    for it in range(3):
        grads = []
        for r in (0, 1):
            enc.zero_grad()
            _loss(_batch(r, it), enc).backward()
            grads.append([p.grad.clone() for p in enc.parameters()])
        for p, ga, gb in zip(enc.parameters(), *grads):
            p.grad = 0.5 * ga + 0.5 * gb
        opt.step()
    want = _state(enc, opt)
    for key, a in out[0]['state'].items():
        assert torch.equal(a, want[key]), key
    final = torch.load(tmp_path / 'rank0' / 'model_final.pt', weights_only=True)
    assert all(torch.equal(final[n], want[n]) for n in final)


def _partial_worker(rank, world):
    from aspire_amd import GradReducer
    torch.manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (5, 3, 6)]      # [on both ranks, on no rank, on rank 1 only]
    g = [torch.randn(5, generator=torch.Generator().manual_seed(rank)), None,
         torch.randn(6, generator=torch.Generator().manual_seed(50)) if rank == 1 else None]
    for p, gi in zip(ps, g):
        p.grad = gi
    opt = torch.optim.Adam(ps, lr=0.1)
    red = GradReducer(ps)
    red.reduce()
    got = [None if p.grad is None else p.grad.clone() for p in ps]
    opt.step()
    twice = None
    try:
        red.reduce()
    except RuntimeError as e:
        twice = str(e)
    return dict(grads=got, state=[sorted(opt.state.get(p, {})) for p in ps], twice=twice, pads=red.flat.clone(),
                layout=(red.offsets, red.tail, red.total))


def test_gradients_present_on_only_some_ranks():
    out = _spawn(_partial_worker, 2)
    g0, g1 = (torch.randn(5, generator=torch.Generator().manual_seed(r)) for r in (0, 1))
    only1 = torch.randn(6, generator=torch.Generator().manual_seed(50))
    for r in (0, 1):
        got = out[r]['grads']
        assert torch.equal(got[0], 0.5 * g0 + 0.5 * g1)
        assert got[1] is None and out[r]['state'][1] == []                        # unused everywhere: no gradient, no state
        assert torch.equal(got[2], 0.5 * only1)                                   # rank 1's alone arrives as 0.5 g on both
        assert out[r]['state'][0] == out[r]['state'][2] == ['exp_avg', 'exp_avg_sq', 'step']
        assert out[r]['twice'] is not None and 'twice' in out[r]['twice']
        offsets, tail, total = out[r]['layout']
        assert (offsets, tail, total) == ([0, 8, 12], 20, 24)
        flat = out[r]['pads']
        assert flat[5:8].eq(0).all() and flat[8:12].eq(0).all() and flat[18:20].eq(0).all()
        assert flat[tail:].tolist() == [2.0, 0.0, 1.0, 0.0]                       # ranks that had a gradient, then the tail's pad


def _mismatch_worker(rank, world):
    from aspire_amd import GradReducer
    out = {}
    for case, sizes in (('count', [(4, 2), (4, 2, 3)]), ('numel', [(4, 2), (4, 3)])):
        try:
            GradReducer([torch.nn.Parameter(torch.zeros(n)) for n in sizes[rank]])
            out[case] = None
        except RuntimeError as e:
            out[case] = str(e)
    return out


def test_layout_mismatch_raises_on_every_rank():
    """parameter lists of different lengths, then of different sizes: RuntimeError on both ranks, inside the timeout, and the process
    group is still usable for the second case"""
    out = _spawn(_mismatch_worker, 2)
    for case in ('count', 'numel'):
        assert out[0][case] is not None and out[0][case] == out[1][case]
    assert '[2, 3]' in out[0]['count']
    assert 'parameter 1' in out[0]['numel'] and '[2, 3]' in out[0]['numel']


def _short_worker(rank, world, path):
    from aspire_amd import RankTrainerDDP
    enc = _encoder(1)
    seen = []

    def loss(batch, encoder):
        seen.append(1)
        return _loss(batch, encoder)

    tr = RankTrainerDDP(enc, None, _hparams(num_epochs=2, es_check_every=1000), os.path.join(path, f'rank{rank}'),
                        lambda epoch: [_batch(rank, it) for it in range(3 - rank)], optimizer=torch.optim.Adam(enc.parameters(), lr=0.05),
                        loss_fn=loss)
    done = tr.train()
    return dict(done=done, iteration=tr.iteration, epoch=tr.epoch, seen=len(seen), state=_state(enc, tr.optimizer))


def test_short_shard_ends_the_epoch_on_every_rank(tmp_path):
    """rank 1 has two batches an epoch, rank 0 three: both run two iterations an epoch, twice, and stay in step"""
    out = _spawn(_short_worker, 2, str(tmp_path))
    for r in (0, 1):
        assert out[r]['done'] is True and out[r]['iteration'] == 4 and out[r]['epoch'] == 2 and out[r]['seen'] == 4
    for key, a in out[0]['state'].items():
        assert torch.equal(a, out[1]['state'][key]), key


def test_one_rank_needs_no_process_group(tmp_path):
    """without torch.distributed: a RankTrainer with one rank; reduce() does nothing and the gradients stay where autograd put them"""
    from aspire_amd import GradReducer, RankTrainerDDP, broadcast_parameters
    enc = _encoder(2)
    assert broadcast_parameters(enc) is enc
    tr = RankTrainerDDP(enc, None, _hparams(), str(tmp_path), lambda epoch: [_batch(0, it) for it in range(3)],
                        optimizer=torch.optim.Adam(enc.parameters(), lr=0.05), loss_fn=_loss)
    assert (tr.rank, tr.num_gpus, tr.es_check_every, tr.num_train, tr.total_iters) == (0, 1, 4, 24, 6)
    assert tr.reducer.flat is None and tr.train() is True and tr.iteration == 3
    p = torch.nn.Parameter(torch.ones(3))
    p.grad = torch.ones(3)
    keep = p.grad
    GradReducer([p]).reduce()
    assert p.grad is keep
    with pytest.raises(ValueError, match='es_check_every'):
        RankTrainerDDP(enc, None, _hparams(es_check_every=0), str(tmp_path), lambda epoch: [], loss_fn=_loss,
                       optimizer=torch.optim.Adam(enc.parameters(), lr=0.05))
