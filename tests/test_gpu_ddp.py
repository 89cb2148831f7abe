"""GPU: data-parallel training -- the gradient bucket's pack kernel against numpy bit for bit, HipAdam on views of the bucket, and
GradReducer / RankTrainerDDP with two and three ranks on cuda:0 over gloo (tests/test_gpu_parallel.py's spawn pattern: the real code
path with the collective through the host; RCCL itself needs two GPUs and has one case).

The training cases use tests/test_gpu_trainer.py's model: a random-init one-layer BertModel WITH its pooler (hidden 768, a vocabulary
of 300), B = 3 abstracts of L <= 48, explicit negatives, RankLoss with l2max, HipAdam.  The tables train through hip_embeddings=True,
so every gradient comes from a kernel documented to give the same bits on every run; at two ranks the scaling by 0.5 is exact and
a + b commutes, so a single process that steps on 0.5 g_a + 0.5 g_b must give the ranks' bits, not an approximation of them."""
import datetime
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(HERE, 'golden')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import optim_ref as orf  # noqa: E402
import readout_inputs as ri  # noqa: E402

pytestmark = pytest.mark.gpu
VOCAB = 300
WORDS = ['alpha', 'beta', 'gamma', 'delta', 'kappa', 'sigma', 'omega', 'theta', 'lambda', 'zeta', 'rho', 'tau', 'phi', 'chi', 'psi', 'mu',
         'nu', 'xi', 'pi', 'eta', 'iota', 'upsilon', 'omicron', 'epsilon']
SEED = 1234567
CHUNK = orf.CHUNK


def _max_grid():
    text = open(os.path.join(ROOT, 'aspire_amd', 'csrc', 'tuning.h')).read()
    a, b = re.search(r'constexpr int kOptimMaxGrid = (\d+) \* (\d+);', text).groups()
    return int(a) * int(b)


# ---- the pack kernel ------------------------------------------------------------------------------------------------------------------------
def _pack_case(sizes, absent, offset1, scale, seed=0):
    """-> (grads (None where absent), numels); the tensor `offset1` is a view at storage offset 1"""
    g = torch.Generator().manual_seed(seed)
    grads = []
    for i, n in enumerate(sizes):
        if i in absent:
            grads.append(None)
        elif i == offset1:
            grads.append(torch.randn(n + 1, generator=g).cuda()[1:])
        else:
            grads.append(torch.randn(n, generator=g).cuda())
    return grads, list(sizes)


def _run_pack(grads, numels, scale):
    """pack into a NaN-filled bucket between two guards of 64 floats -> (flat as numpy, the guards intact?)"""
    from aspire_amd import ops
    offsets, tail, total = ops.grad_bucket_layout(numels)
    big = torch.full((64 + total + 64,), float('nan'), device='cuda')
    big[:64] = 7.0
    big[64 + total:] = 9.0
    flat = big[64:64 + total]
    assert flat.data_ptr() % 16 == 0
    ops.grad_bucket_pack(grads, flat, scale, numels=numels)
    torch.cuda.synchronize()
    host = big.cpu().numpy()
    assert (host[:64] == 7.0).all() and (host[64 + total:] == 9.0).all(), 'a guard float changed'
    return host[64:64 + total].copy(), offsets, tail, total


def _expected(grads, numels, offsets, tail, total, scale):
    want = np.zeros(total, dtype=np.float32)
    for i, (g, n, o) in enumerate(zip(grads, numels, offsets)):
        if g is not None:
            want[o:o + n] = g.cpu().numpy().astype(np.float32) * np.float32(scale)
            want[tail + i] = 1.0
    return want


@pytest.mark.parametrize('scale', [1.0 / 3.0, 1.0])
def test_pack_equals_numpy_bit_for_bit(scale):
    sizes = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5, 7, CHUNK + 3, CHUNK + 7]
    grads, numels = _pack_case(sizes, absent={9, 10}, offset1=11, scale=scale)
    assert grads[11].data_ptr() % 16 == 4 and grads[8].data_ptr() % 16 == 0          # the scalar path and the vector path
    got, offsets, tail, total = _run_pack(grads, numels, scale)
    want = _expected(grads, numels, offsets, tail, total, scale)
    assert not np.isnan(got).any(), 'an element of the bucket was not written'
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # said again by name: the pads, the absent regions, the tail and its pad
    for i, (n, o) in enumerate(zip(numels, offsets)):
        end = offsets[i + 1] if i + 1 < len(offsets) else tail
        assert (got[o + n:end] == 0).all(), i
    assert (got[offsets[9]:offsets[9] + 8] == 0).all() and (got[offsets[10]:offsets[10] + CHUNK + 4] == 0).all()
    assert got[tail:].tolist() == [0.0 if i in (9, 10) else 1.0 for i in range(12)] and total == tail + 12
    # a second call on the same inputs: the same bits
    again, *_ = _run_pack(grads, numels, scale)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_pack_tail_pad_and_no_tensors():
    from aspire_amd import ops
    grads, numels = _pack_case([5, 2, 9, 1, 6], absent={1}, offset1=2, scale=0.25, seed=1)       # 5 tensors: a tail of 8 with 3 pad floats
    got, offsets, tail, total = _run_pack(grads, numels, 0.25)
    assert np.array_equal(got.view(np.uint32), _expected(grads, numels, offsets, tail, total, 0.25).view(np.uint32))
    assert got[tail:].tolist() == [1.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    # no tensor at all: a bucket of no elements, accepted, nothing written
    guard = torch.full((128,), 3.0, device='cuda')
    assert ops.grad_bucket_layout([]) == ([], 0, 0)
    ops.grad_bucket_pack([], guard[64:64], 0.5)
    torch.cuda.synchronize()
    assert bool((guard == 3.0).all())
    # what the binding refuses
    with pytest.raises(ValueError, match='numels'):
        ops.grad_bucket_pack([None], torch.empty(8, device='cuda'), 0.5)
    flat = torch.empty(8, device='cuda')
    with pytest.raises(AssertionError, match='overlaps'):
        ops.grad_bucket_pack([flat[:4]], flat, 0.5)
    with pytest.raises(AssertionError, match='flat_elems'):
        ops.grad_bucket_pack([torch.ones(4, device='cuda')], torch.empty(12, device='cuda'), 0.5)


def test_pack_grid_strides_over_more_chunks_than_workgroups():
    """one tensor of (kOptimMaxGrid + 1) * kOptimChunk + 1 elements (about 34 MB): every workgroup takes a second chunk, the last
    chunk holds one element and three pad floats"""
    n = (_max_grid() + 1) * CHUNK + 1
    g = torch.randn(n, generator=torch.Generator().manual_seed(2)).cuda()
    got, offsets, tail, total = _run_pack([g], [n], 1.0 / 3.0)
    want = _expected([g], [n], offsets, tail, total, 1.0 / 3.0)
    assert total == n + 3 + 4 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_adam_on_bucket_views_equals_adam_on_plain_gradients():
    from aspire_amd import HipAdam, ops
    sizes = [(3,), (5, 768), (CHUNK + 1,), (2, CHUNK), (1,)]
    numels = [int(np.prod(s)) for s in sizes]
    offsets, tail, total = ops.grad_bucket_layout(numels)
    gen = torch.Generator().manual_seed(4)
    init = [torch.randn(s, generator=gen).cuda() for s in sizes]
    sets = []
    for _ in range(2):
        ps = [torch.nn.Parameter(t.clone()) for t in init]
        sets.append((ps, HipAdam(ps, lr=1e-2)))
    flat = torch.empty(total, device='cuda')
    for step in range(2):
        grads = [torch.randn(s, generator=gen).cuda() for s in sizes]
        ops.grad_bucket_pack(grads, flat, 1.0)
        for (ps, opt), use_views in zip(sets, (True, False)):
            for p, g, o, n in zip(ps, grads, offsets, numels):
                view = flat[o:o + n].view(p.shape)
                assert view.data_ptr() % 16 == 0 and view.is_contiguous() and torch.equal(view, g)
                p.grad = view if use_views else view.clone()
            opt.step()
    for p, q in zip(sets[0][0], sets[1][0]):
        assert torch.equal(p, q)
        for key in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(sets[0][1].state[p][key], sets[1][1].state[q][key])
        assert float(sets[0][1].state[p]['step']) == 2.0


# ---- ranks on cuda:0 ------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _bert(seed, dropout=0.0):
    from transformers import BertConfig, BertModel
    torch.manual_seed(seed)
    cfg = BertConfig(vocab_size=VOCAB, hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=256,
                     max_position_embeddings=64, layer_norm_eps=1e-12, hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout,
                     attn_implementation='eager')
    return BertModel(cfg, add_pooling_layer=True)


def _abstracts(seed):
    g = torch.Generator().manual_seed(seed)

    def sent():
        return ' '.join(WORDS[int(i)] for i in torch.randint(0, len(WORDS), (int(torch.randint(3, 7, (1,), generator=g)),), generator=g)) + '.'

    return [{'TITLE': sent(), 'ABSTRACT': [sent() for _ in range(int(torch.randint(1, 4, (1,), generator=g)))]} for _ in range(3)]


def _batches(tmp, tag):
    """four rank batches with explicit negatives; rank r takes batch (2 it + r) % 4 at iteration it"""
    from transformers import BertTokenizer
    from aspire_amd import prepare_abstracts
    path = os.path.join(tmp, f'vocab_{tag}.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]', '.'] + WORDS) + '\n')
    tok = BertTokenizer(path, do_lower_case=True)
    out = []
    for base in (10, 20, 30, 40):
        batch = {}
        for key, seed in (('query', base + 1), ('pos', base + 2), ('neg', base + 3)):
            bert_batch, abs_lens, idxs = prepare_abstracts(_abstracts(seed), tok)
            assert bert_batch['tokid_tt'].shape[1] <= 48
            batch.update({key + '_bert_batch': bert_batch, key + '_abs_lens': abs_lens, key + '_senttok_idxs': idxs})
        out.append(batch)
    return out


def _hparams(dropout):
    """without dropout: one epoch of three batches at a constant lr; with: two epochs of two, the lr decaying every iteration"""
    return dict(es_check_every=1000, train_size=18 if not dropout else 12, dev_size=3, batch_size=3, num_epochs=2 if dropout else 1,
                update_rule='adam', learning_rate=1e-3, lr_decay_method='exponential', decay_lr_by=0.7,
                decay_lr_every=1 if dropout else 1000)


def _state(enc, opt):
    out = {}
    for n, p in enc.bert.named_parameters():
        out[n] = p.detach().cpu().clone()
        for k, v in opt.state.get(p, {}).items():
            out[f'{n}/{k}'] = torch.as_tensor(v).detach().cpu().clone()
    return out


def _ddp_worker(rank, world, port, out_dir, dropout, backend='gloo'):
    import torch.distributed as dist
    for p in (ROOT, HERE, os.path.join(HERE, 'golden')):
        sys.path.insert(0, p)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    if backend == 'nccl':              # one process per GPU over RCCL
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        torch.cuda.set_device(rank)
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', rank),
                                timeout=datetime.timedelta(seconds=120))
    else:
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from aspire_amd import HipAdam, HipBertTrainEncoder, RankTrainerDDP
    batches = _batches(out_dir, f'r{rank}')
    per_epoch = 2 if dropout else 3

    def make(seed, tag):
        enc = HipBertTrainEncoder(_bert(seed, 0.1 if dropout else 0.0), dropout=dropout, seed=SEED, hip_embeddings=True)
        return RankTrainerDDP(enc, ri.hparams('l2max', 0.5), _hparams(dropout), os.path.join(out_dir, f'{tag}{rank}'),
                              lambda epoch: [batches[(2 * (per_epoch * epoch + i) + rank) % 4] for i in range(per_epoch)])

    straight = make(3 + rank, 'straight')          # other weights on rank 1: the broadcast makes them rank 0's
    res = dict(seed=straight.encoder.dropout_state()[0], derived=(straight.rank, straight.num_gpus, straight.num_train, straight.total_iters),
               is_hip_adam=isinstance(straight.optimizer, HipAdam))
    res['done'] = straight.train()
    res['iteration'] = straight.iteration
    res['state'] = _state(straight.encoder, straight.optimizer)
    res['pooler'] = [(n, p.grad is None, p in straight.optimizer.state) for n, p in straight.encoder.bert.named_parameters()
                     if n.startswith('pooler.')]
    res['files'] = sorted(os.listdir(straight.model_path)) if os.path.isdir(straight.model_path) else []
    res['dropout_state'] = straight.encoder.dropout_state()
    if dropout:
        first = make(3 + rank, 'first')
        assert first.train(max_iterations=2) is False
        first.save_checkpoint(os.path.join(out_dir, f'ck{rank}.pt'))
        second = make(99 + rank, 'second')         # other weights, another dropout key: everything must come from the checkpoint
        second.encoder.set_dropout_state(1, 0)
        second.load_checkpoint(os.path.join(out_dir, f'ck{rank}.pt'))
        res['resumed_at'] = (second.iteration, second.epoch, second.batch_in_epoch)
        second.train(max_iterations=2)
        res['resumed'] = _state(second.encoder, second.optimizer)
        res['resumed_dropout_state'] = second.encoder.dropout_state()
    torch.save(res, os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


def _single_process(tmp, dropout, iters):
    """one process: every iteration's gradient formed as 0.5 g_a + 0.5 g_b (a missing one counting as zeros), HipAdam steps"""
    from aspire_amd import HipAdam, HipBertTrainEncoder, RankLoss
    batches = _batches(tmp, 'parent')
    enc = HipBertTrainEncoder(_bert(3, 0.1 if dropout else 0.0), dropout=dropout, seed=SEED, hip_embeddings=True).train()
    opt = HipAdam(enc.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.7)
    loss = RankLoss(ri.hparams('l2max', 0.5)).forward_rank
    params = list(enc.parameters())
    for it in range(iters):
        per_rank = []
        for r in (0, 1):
            opt.zero_grad()
            if dropout:
                enc.set_dropout_state(SEED + r, 3 * it)          # three training forwards an iteration: query, positive, negative
            loss(batches[(2 * it + r) % 4], enc).backward()
            per_rank.append([None if p.grad is None else p.grad.clone() for p in params])
        for p, ga, gb in zip(params, *per_rank):
            if ga is None and gb is None:
                p.grad = None
            else:
                za = ga if ga is not None else torch.zeros_like(p)
                zb = gb if gb is not None else torch.zeros_like(p)
                p.grad = 0.5 * za + 0.5 * zb
        opt.step()
        if dropout and it > 0:
            sched.step()
    return _state(enc, opt)


def _same(a, b, what):
    assert set(a) == set(b), what
    for key in a:
        assert torch.equal(a[key], b[key]), (what, key)


def _check_two_ranks(tmp_path, dropout, backend='gloo'):
    import torch.multiprocessing as mp
    iters = 4 if dropout else 3
    mp.spawn(_ddp_worker, args=(2, _free_port(), str(tmp_path), dropout, backend), nprocs=2, join=True)
    outs = [torch.load(os.path.join(str(tmp_path), f'r{r}.pt'), weights_only=False) for r in (0, 1)]
    for r, o in enumerate(outs):
        assert o['derived'] == (r, 2, (12 if dropout else 18) // 2, (2 if dropout else 1) * (2 if dropout else 3))
        assert o['is_hip_adam'] and o['done'] is True and o['iteration'] == iters
        assert o['seed'] == SEED + r                                      # identical seeds would give both ranks the same masks
        assert len(o['pooler']) == 2 and all(none and not in_state for _, none, in_state in o['pooler'])
        assert not any(k.startswith('pooler.') and '/' in k for k in o['state'])
    assert outs[0]['files'] == ['model_final.pt'] and outs[1]['files'] == []
    _same(outs[0]['state'], outs[1]['state'], 'rank 0 against rank 1')
    trained = sum(1 for k in outs[0]['state'] if k.endswith('/exp_avg'))
    assert trained == len([k for k in outs[0]['state'] if '/' not in k]) - 2          # everything but the pooler's two tensors
    want = _single_process(str(tmp_path), dropout, iters)
    _same(outs[0]['state'], want, 'the ranks against one process on the mean gradient')
    return outs


def test_two_ranks_equal_one_process_on_the_mean_gradient(tmp_path):
    from aspire_amd.encoder import HipBertEncoder
    _check_two_ranks(tmp_path, dropout=False)
    sd = torch.load(tmp_path / 'straight0' / 'model_final.pt', weights_only=True)
    cfg = _bert(0).config
    inf = HipBertEncoder.from_state_dict(cfg, {k: v.cpu() for k, v in sd.items()})
    bb = _batches(str(tmp_path), 'load')[0]['query_bert_batch']
    hidden = inf(bb['tokid_tt'], token_type_ids=bb['seg_tt'], attention_mask=bb['attnmask_tt']).last_hidden_state
    assert torch.isfinite(hidden).all()


def test_two_ranks_with_dropout_and_resume(tmp_path):
    outs = _check_two_ranks(tmp_path, dropout=True)
    for r, o in enumerate(outs):
        assert o['dropout_state'] == (SEED + r, 12) and o['resumed_dropout_state'] == (SEED + r, 12)
        assert o['resumed_at'] == (2, 1, 0)
        _same(o['resumed'], o['state'], f'rank {r}: resumed against straight')


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='RCCL needs at least two GPUs (the build boxes have one)')
def test_two_ranks_over_rccl(tmp_path):
    """the same comparison with one process per GPU, backend "nccl": the bucket is summed in place over xGMI"""
    _check_two_ranks(tmp_path, dropout=False, backend='nccl')


def _reducer_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from aspire_amd import GradReducer
    ps, grads = _reducer_case(rank)
    for p, g in zip(ps, grads):
        p.grad = g
    red = GradReducer(ps)
    red.reduce()
    torch.save([p.grad.cpu().clone() for p in ps], os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


REDUCER_SIZES = [(5,), (CHUNK + 1,), (3, 768), (1,)]


def _reducer_case(rank, device='cuda'):
    """rank 1 has no gradient for tensor 2"""
    ps = [torch.nn.Parameter(torch.zeros(s, device=device)) for s in REDUCER_SIZES]
    gen = torch.Generator().manual_seed(70 + rank)
    grads = [torch.randn(s, generator=gen).to(device) for s in REDUCER_SIZES]
    if rank == 1:
        grads[2] = None
    return ps, grads


def test_three_ranks_reduce_within_the_rounding_bound(tmp_path):
    """all ranks hold the same bits; against the float64 mean the error per element is at most (2 world - 1) 2^-24 sum_r |g_r| / world:
    one rounding per scaling and per addition (derived, not measured)"""
    import torch.multiprocessing as mp
    world = 3
    mp.spawn(_reducer_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    outs = [torch.load(os.path.join(str(tmp_path), f'r{r}.pt')) for r in range(world)]
    per_rank = [_reducer_case(r, 'cpu')[1] for r in range(world)]
    worst = 0.0
    for i in range(len(REDUCER_SIZES)):
        for o in outs[1:]:
            assert torch.equal(o[i], outs[0][i]), i
        gs = [g[i].double() if g[i] is not None else torch.zeros(REDUCER_SIZES[i], dtype=torch.float64) for g in per_rank]
        mean = sum(gs) / world
        bound = (2 * world - 1) * 2.0 ** -24 * sum(g.abs() for g in gs) / world
        err = (outs[0][i].double() - mean).abs()
        print(f'tensor {i}: largest error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), i
    assert worst > 0          # the mean of three is not exact in fp32: the bound is not vacuous
