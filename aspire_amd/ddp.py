"""Data-parallel training: the reference's ``ddp_train_model`` path (main_fsim.py; ``GenericTrainerDDP`` / ``BasicRankingTrainerDDP``,
src/learning/trainer.py:476-800: ``DistributedDataParallel(..., find_unused_parameters=True)``, one process per GPU) restated over
this project's pieces.

torch's ``DistributedDataParallel`` is not what wraps ``HipBertTrainEncoder``: its reducer hangs autograd hooks on every parameter
and copies gradients bucket by bucket, where this project's step is one launch over all 199 tensors, no atomics, the same bits on
every run.  Here the three pieces are

    GradReducer            one HIP launch packs every gradient of a step, scaled by 1 / world, into ONE flat fp32 bucket
                           (grad_bucket.hip); ONE all-reduce sums the bucket over the ranks (RCCL under "nccl"); every ``p.grad``
                           becomes a view of the bucket, which ``HipAdam`` / ``HipAdagrad`` read in place on their 16-byte path.
    broadcast_parameters   rank 0's parameters and buffers to every rank, once, at construction.
    RankTrainerDDP         ``RankTrainer`` with the reference's DDP rules.

    # one process per GPU, e.g. torch.multiprocessing.spawn(worker, nprocs=n_gpus)
    torch.cuda.set_device(rank)
    dist.init_process_group('nccl', rank=rank, world_size=n_gpus, device_id=torch.device('cuda', rank))
    trainer = RankTrainerDDP(HipBertTrainEncoder(bert, dropout=True), model_hparams, train_hparams, model_path,
                             train_batches=lambda epoch: shard_of(rank, epoch), dev_batches=dev if rank == 0 else None)
    trainer.train()

``RankTrainerDDP`` -- what differs from ``RankTrainer`` (``rank`` / ``num_gpus`` are ``parallel.rank_world(group)``):

  es_check_every, num_warmup_steps   the reference's ``// num_gpus`` (trainer.py:520, 781, 787)
  num_train                          ``train_size // num_gpus``; num_batches / total_iters formed from it (trainer.py:770-775)
  train_batches(epoch)               THIS rank's shard (the reference reads ``train-{rank}-{epoch}.jsonl``)
  the reduction                      ``GradReducer.reduce()`` immediately in front of ``optimizer.step()``.  A parameter without a gradient
                                     on ANY rank keeps ``grad is None`` (torch DDP's rule for a parameter unused everywhere), so the pooler
                                     under ``RankLoss`` never gets an optimizer state or a step count, exactly as in one process; one
                                     without a gradient on THIS rank only gets the other ranks' mean contribution (zeros from here).
  max_grad_norm                      the norm is taken AFTER the reduction, over the bucket views; every rank holds the same reduced bits
                                     and forms the same clip coefficient, so clipping adds no collective
  gradient accumulation              the reduction happens ONCE per update group, on the accumulated sums -- not once per backward as
                                     torch DDP does in the reference.  Mathematically the same mean (the scaling and the sum over ranks
                                     are linear); the rounding order differs and the traffic is 1 / update_params_every of it.
  dev pass, histories, model files   rank 0 only, no collective inside the dev pass; every rank calls ``dist.barrier()`` after a
                                     dev-check iteration (whether checks happen at all is rank 0's ``early_stop``, broadcast at construction)
  the start                          rank 0's parameters and buffers are broadcast; where the encoder has a ``dropout_state`` its seed
                                     becomes ``seed + rank`` (identical seeds would give every rank the same masks)
  a short shard                      every iteration begins with a one-element all-reduce (MIN) of "I have a batch": when any rank runs
                                     out the epoch ends on all of them, the ranks that had batches left log a warning.  (The reference
                                     assumes exactly equal shards; a short one would hang its collective.)
  checkpoints                        ``save_checkpoint`` / ``load_checkpoint`` are the base class's, called on EVERY rank with a per-rank
                                     path: the per-rank RNG and dropout state are part of the checkpoint.  ``train(max_iterations=n)``
                                     must be given the same n on every rank.

CPU tensors take a plain torch path with the same arithmetic (``g * float32(1 / world)`` into the bucket, the same layout), so the host
logic runs under gloo without a GPU, as ``RankTrainer``'s does with ``loss_fn`` / ``optimizer`` injected.
"""
import logging
import math

import torch
import torch.distributed as dist

from . import parallel
from .trainer import RankTrainer


def _collective_device(group):
    """where a small control tensor must live for a collective of `group`: on the GPU under "nccl", on the host under gloo"""
    if dist.get_backend(group) == 'nccl':
        return torch.device('cuda', torch.cuda.current_device())
    return torch.device('cpu')


def _src(group):
    return dist.get_global_rank(group, 0) if group is not None else 0


def _gather_i64(values, group, world):
    """every rank's list of int64 `values` (one length on every rank) -> [world, len] on the host"""
    dev = _collective_device(group)
    mine = torch.tensor(values, dtype=torch.int64, device=dev)
    out = torch.empty(world * mine.numel(), dtype=torch.int64, device=dev)
    if mine.numel():
        parallel.all_gather_flat(out, mine, group)
    return out.view(world, mine.numel()).cpu()


def broadcast_parameters(module, group=None):
    """Rank 0's parameters and buffers of `module` to every rank of `group`, in place (under gloo a GPU tensor goes through the host).
    Nothing to do without an initialised process group or with one rank."""
    if parallel.rank_world(group)[1] == 1:
        return module
    src = _src(group)
    with torch.no_grad():
        for t in list(module.parameters()) + list(module.buffers()):
            if parallel._through_host(t, group):
                host = t.detach().cpu()
                dist.broadcast(host, src=src, group=group)
                t.copy_(host)
            else:
                dist.broadcast(t.detach(), src=src, group=group)
    return module


class GradReducer:
    """The mean of every parameter's gradient over the ranks of `group`, through one flat bucket.

    params: every trainable parameter in the optimizer's param-group order -- the same list on every rank, fp32, on one device.  At
    construction the ranks all-gather (number of tensors, element counts); a disagreement raises RuntimeError on EVERY rank (both
    gathers complete first, so nobody is left waiting).  The bucket (ops.grad_bucket_layout) is allocated once.

    reduce():  1. packs [p.grad or None] with scale = 1 / world into the bucket (GPU: ONE aspire_grad_bucket_pack_f32 launch);
               2. parallel.all_reduce_flat over the bucket;
               3. reads the bucket's tail -- per tensor, the number of ranks that had a gradient -- only when some parameter lacks
                  a gradient here (with a gradient for everything, every count is at least 1);
               4. sets p.grad to the view of the bucket at the tensor's offset (contiguous, 16-byte aligned: the optimizer's vector
                  path, no copy back) where the count is above 0, to None where it is 0.
    Calling it again before new gradients exist finds gradients that live in the bucket and raises RuntimeError.  With one rank
    reduce() does nothing (force=True, for measurements, packs with scale 1 and hands out the views all the same)."""

    def __init__(self, params, group=None, force=False):
        self.params = list(params)
        self.group = group
        self.rank, self.world = parallel.rank_world(group)
        self.active = self.world > 1 or bool(force)
        for p in self.params:
            if p.dtype != torch.float32 or p.device != self.params[0].device or p.is_sparse:
                raise TypeError('GradReducer: every parameter must be a dense fp32 tensor on one device')
        self.numels = [p.numel() for p in self.params]
        if self.world > 1:
            counts = _gather_i64([len(self.params)], group, self.world)[:, 0].tolist()
            # (ranks that disagree on the count cannot gather equal-length lists: they gather nothing, and everyone raises below)
            same = len(set(counts)) == 1
            sizes = _gather_i64(self.numels if same else [], group, self.world).tolist()
            if not same:
                raise RuntimeError(f'GradReducer: the ranks hold different numbers of parameters: {counts}')
            if any(row != sizes[0] for row in sizes):
                bad = next(i for i in range(len(self.numels)) if len({row[i] for row in sizes}) > 1)
                raise RuntimeError(f'GradReducer: parameter {bad} has {[row[bad] for row in sizes]} elements on the ranks')
        from . import ops
        self.offsets, self.tail, self.total = ops.grad_bucket_layout(self.numels)
        self.flat, self.views = None, None
        if self.active and self.params:
            dev = self.params[0].device
            self.flat = torch.zeros(self.total, dtype=torch.float32, device=dev)
            self.views = [self.flat[o:o + n].view(p.shape) for o, n, p in zip(self.offsets, self.numels, self.params)]

    def _pack_cpu(self, grads, scale):
        """the library's arithmetic and layout on host tensors: one fp32 multiply per element, zeros elsewhere, flags in the tail"""
        self.flat.zero_()
        s = torch.tensor(scale, dtype=torch.float64).to(torch.float32)
        for i, g in enumerate(grads):
            if g is not None:
                torch.mul(g.detach().reshape(-1), s, out=self.flat[self.offsets[i]:self.offsets[i] + self.numels[i]])
                self.flat[self.tail + i] = 1.0

    @torch.no_grad()
    def reduce(self):
        if not self.active or not self.params:
            return
        grads = [p.grad for p in self.params]
        lo, hi = self.flat.data_ptr(), self.flat.data_ptr() + 4 * self.total
        for i, g in enumerate(grads):
            if g is None:
                continue
            if g.dtype != torch.float32 or g.device != self.flat.device or g.numel() != self.numels[i] or not g.is_contiguous():
                raise TypeError(f'GradReducer: the gradient of parameter {i} is not a contiguous fp32 tensor of {self.numels[i]} '
                                f'elements on {self.flat.device}')
            if g.numel() and g.data_ptr() < hi and g.data_ptr() + 4 * g.numel() > lo:
                raise RuntimeError(f'GradReducer.reduce(): the gradient of parameter {i} already lives in the bucket -- reduce() ran '
                                   'twice on the same gradients (or zero_grad(set_to_none=False) kept the views)')
        scale = 1.0 / self.world
        if self.flat.is_cuda:
            from . import ops
            ops.grad_bucket_pack(grads, self.flat, scale, numels=self.numels)
        else:
            self._pack_cpu(grads, scale)
        if self.world > 1:
            parallel.all_reduce_flat(self.flat, self.group)
        if any(g is None for g in grads):
            have = (self.flat[self.tail:self.tail + len(self.params)] > 0).tolist()
        else:
            have = [True] * len(self.params)
        for p, view, h in zip(self.params, self.views, have):
            p.grad = view if h else None


class RankTrainerDDP(RankTrainer):
    """RankTrainer under the reference's DDP rules (the module docstring lists them).  Construct it on every rank of `group` at the
    same point, after torch.distributed is initialised (without a process group it is a RankTrainer with one rank)."""

    def __init__(self, encoder, model_hparams, train_hparams, model_path, train_batches, dev_batches=None, early_stop=True,
                 optimizer=None, loss_fn=None, group=None, force_reducer=False):
        self.group = group
        self.rank, self.num_gpus = parallel.rank_world(group)
        hp = dict(train_hparams)
        hp['es_check_every'] = train_hparams['es_check_every'] // self.num_gpus
        if hp['es_check_every'] < 1:
            raise ValueError(f"es_check_every = {train_hparams['es_check_every']} // {self.num_gpus} ranks is 0")
        hp['train_size'] = train_hparams['train_size'] // self.num_gpus
        if 'num_warmup_steps' in train_hparams:
            hp['num_warmup_steps'] = train_hparams['num_warmup_steps'] // self.num_gpus
        broadcast_parameters(encoder, group)
        if hasattr(encoder, 'dropout_state'):
            seed, step = encoder.dropout_state()
            encoder.set_dropout_state(seed + self.rank, step)
        super().__init__(encoder, model_hparams, hp, model_path, train_batches, dev_batches, early_stop, optimizer, loss_fn)
        # whether dev checks happen is rank 0's decision: the other ranks need no dev_batches, but must meet rank 0 at the barrier
        wants = bool(early_stop) and (dev_batches is not None or self.rank != 0)
        if self.num_gpus > 1:
            flag = torch.tensor([int(wants)], dtype=torch.int64, device=_collective_device(group))
            dist.broadcast(flag, src=_src(group), group=group)
            wants = bool(flag.item())
        self.early_stop = wants
        self.reducer = GradReducer([p for g in self.optimizer.param_groups for p in g['params'] if p.requires_grad], group,
                                   force=force_reducer)

    # ---- rank 0 keeps the files and the histories
    def _save_model(self, suffix):
        if self.rank == 0:
            super()._save_model(suffix)

    def _record_loss(self, objective):
        if self.rank == 0:
            super()._record_loss(objective)

    def _dev_check(self, objective):
        if self.rank == 0:
            super()._dev_check(objective)

    def _step(self):
        self.reducer.reduce()
        # with max_grad_norm the norm is taken here, over the bucket views: every rank holds the same reduced bits and forms the same
        # coefficient, so no further collective is issued; a parameter without a gradient on any rank (grad None) stays out of it
        self._update()

    def _iterate(self, batch):
        checked = self.iteration % self.es_check_every == 0 and self.iteration != 0 and self.early_stop
        super()._iterate(batch)
        if checked and self.num_gpus > 1:
            dist.barrier(group=self.group)

    def _all_have(self, have):
        """one-element all-reduce (MIN) of "I have a batch": True only when every rank has one"""
        if self.num_gpus == 1:
            return have
        flag = torch.tensor([int(have)], dtype=torch.int64, device=_collective_device(self.group))
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.group)
        return bool(flag.item())

    def train(self, max_iterations=None):
        """RankTrainer.train over this rank's shard, in lockstep with the other ranks: the epoch ends for all when any rank's batches
        end.  max_iterations must be the same on every rank.  model_final.pt is written by rank 0."""
        budget = math.inf if max_iterations is None else int(max_iterations)
        end = object()
        while self.epoch < self.num_epochs:
            consumed, i = self.batch_in_epoch, 0
            batches = iter(self.train_batches(self.epoch))
            while True:
                batch = next(batches, end)
                if batch is not end and i < consumed:
                    i += 1
                    continue
                if not self._all_have(batch is not end):
                    if batch is not end:
                        logging.warning('rank %d: epoch %d ends after %d batches: another rank ran out of batches, this rank has more',
                                        self.rank, self.epoch, i)
                    break
                if budget <= 0:
                    return False
                self._iterate(batch)
                i += 1
                self.batch_in_epoch = i
                budget -= 1
            self.epoch, self.batch_in_epoch = self.epoch + 1, 0
        self._save_model('final')
        if self.rank == 0:
            logging.info('Best model; Iteration %d; Dev loss: %.4f', self.best_iter, self.best_dev_score)
        return True
