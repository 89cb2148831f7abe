"""The gradient bucket of data-parallel training (aspire_amd/ddp.py, grad_bucket.hip) on BERT-base's gradient shapes (BertConfig(): 199
tensors, 109.5 M elements, random values, nothing downloaded), by tools/optimizer_step_time.py's method: device events over windows of
about 0.2 s, the sides alternating, five windows each; one JSON line per measurement.

(a) packing one step's gradients, scaled by 1 / world, into one flat buffer:
    hip     ops.grad_bucket_pack(grads, flat, 1 / world)                          one launch of grad_bucket.hip
    torch   torch.cat([g.reshape(-1) for g in grads]).mul_(1 / world)             torch's flatten (199 copies in one cat, then a pass)
    The results are compared first (bit for bit, region by region).  GATE: the pack's median at or under torch's highest window median.
(b) one HipAdam.step() whose gradients are views of the bucket against one whose gradients are ordinary tensors.  Recorded.
(c) one full training iteration at the --shape of tools/supalign_step_time.py (10 x 256, 12 layers): RankTrainerDDP with one rank and the
    reducer forced on (pack + views, no collective) against RankTrainer.  Recorded.

One GPU: the all-reduce itself (RCCL) is not in any of these figures.

    python tools/grad_bucket_time.py [--world 8] [--shape 10x256] [--layers 12] [--windows 5] [--window-s 0.2]

Needs a GPU; there is no CPU path.
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.cls_train_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--world', type=int, default=8, help='the scale is 1 / world')
    ap.add_argument('--shape', default='10x256', help="(c)'s batch; '' skips (c)")
    ap.add_argument('--sents', type=int, default=8)
    ap.add_argument('--layers', type=int, default=12)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-s', type=float, default=0.2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from transformers import BertConfig, BertModel
    from aspire_amd import HipAdam, ops
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in BertModel(BertConfig()).parameters()]
    numels = [int(np.prod(s)) for s in shapes]
    n_elem = sum(numels)
    grads = [1e-3 * torch.randn(s, device='cuda') for s in shapes]
    offsets, tail, total = ops.grad_bucket_layout(numels)
    flat = torch.empty(total, device='cuda')
    scale = 1.0 / a.world
    out = {}

    def hip():
        ops.grad_bucket_pack(grads, flat, scale)

    def torch_side():
        out['cat'] = torch.cat([g.reshape(-1) for g in grads]).mul_(scale)

    hip()
    torch_side()
    at = 0
    for o, n in zip(offsets, numels):
        assert torch.equal(flat[o:o + n], out['cat'][at:at + n]), 'pack and torch.cat(...).mul_ disagree'
        at += n
    assert flat[tail:tail + len(shapes)].eq(1).all()
    res = dict(measure='pack', tensors=len(shapes), elements=n_elem, bucket_elements=total, world=a.world, pack_bytes=2 * 4 * n_elem)
    res.update(timed({'hip': hip, 'torch': torch_side}, a.windows, a.window_s))
    res['hip_gbps'] = round(2 * 4 * n_elem / res['hip_ms_median'] / 1e6, 1)
    res['gate_hip_median_at_or_under_torch_max'] = bool(res['hip_ms_median'] <= res['torch_ms_min_max'][1])
    print(json.dumps(res), flush=True)
    del out['cat']

    # (b) the optimizer on bucket views
    init = [0.02 * torch.randn(s, device='cuda') for s in shapes]
    views = [flat[o:o + n].view(s) for o, n, s in zip(offsets, numels, shapes)]
    sets = {}
    for name, gs in (('views', views), ('plain', [v.clone() for v in views])):
        ps = [torch.nn.Parameter(t.clone()) for t in init]
        for p, g in zip(ps, gs):
            p.grad = g
        sets[name] = (ps, HipAdam(ps, lr=2e-5))
    for _ in range(2):
        for ps, opt in sets.values():
            opt.step()
    assert all(torch.equal(p, q) for p, q in zip(sets['views'][0], sets['plain'][0])), 'a step on views differs from one on plain gradients'
    res = dict(measure='adam_step_on_views')
    res.update(timed({n: opt.step for n, (ps, opt) in sets.items()}, a.windows, a.window_s))
    print(json.dumps(res), flush=True)
    del sets, views, init, grads, flat
    torch.cuda.empty_cache()

    # (c) one iteration with and without the reducer
    if a.shape:
        from aspire_amd import HipBertTrainEncoder, RankTrainer, RankTrainerDDP
        from tools.supalign_step_time import _documents
        b, l = (int(x) for x in a.shape.split('x'))
        hp = dict(model_name='sbalisentbienc', score_aggregation='l2wasserstein', geoml_blur=0.05, geoml_scaling=0.9, sent_sm_temp=1.0,
                  abs_loss_prop=0.0, sent_loss_prop=1.0, sentsup_loss_prop=1.0)
        thp = dict(es_check_every=10 ** 9, train_size=b, batch_size=b, num_epochs=1, update_rule='adam', learning_rate=2e-5,
                   lr_decay_method='exponential', decay_lr_by=1.0, decay_lr_every=10 ** 9)
        cfg = BertConfig(vocab_size=3000, hidden_size=768, num_hidden_layers=a.layers, num_attention_heads=12, intermediate_size=3072,
                         max_position_embeddings=512, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        gen = torch.Generator().manual_seed(b * 1000 + l)
        docs = [_documents(b, l, a.sents, gen) for _ in range(2)]
        batch = {'pos_align_idxs': [[int(torch.randint(0, a.sents + 2, (1,), generator=gen)), int(torch.randint(0, a.sents + 2, (1,), generator=gen))]
                                    for _ in range(b)]}
        for key, (tok, mask, lens, idxs) in zip(('query', 'pos'), docs):
            batch.update({key + '_bert_batch': {'tokid_tt': tok, 'seg_tt': torch.zeros_like(tok), 'attnmask_tt': mask, 'seq_lens': [l] * b},
                          key + '_abs_lens': lens, key + '_senttok_idxs': idxs})
        tmp = tempfile.mkdtemp()
        plain = RankTrainer(HipBertTrainEncoder(BertModel(cfg, add_pooling_layer=False)), hp, thp, tmp, lambda epoch: [batch])
        ddp = RankTrainerDDP(HipBertTrainEncoder(BertModel(cfg, add_pooling_layer=False)), hp, thp, tmp, lambda epoch: [batch],
                             force_reducer=True)
        assert ddp.reducer.active and ddp.num_gpus == 1
        res = dict(measure='iteration', B=b, L=l, layers=a.layers, reducer_tensors=len(ddp.reducer.params))
        res.update(timed({'ddp_world1_forced': lambda: ddp._iterate(batch), 'plain': lambda: plain._iterate(batch)}, a.windows, a.window_s))
        res['peak_mem_gb'] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
