"""One training step of sbalisentbienc on this library's kernels, by tools/cls_train_time.py's method: device
events over windows of about 0.2 s, the sides alternating, five windows each; one JSON line per measurement.  Nothing is gated.

(a) one `sbalisentbienc-misup-ot` step, forward + backward (no optimizer), a 12-layer BERT-base (ffn 3072, fp32, dropout 0), B query
    and B positive abstracts of L tokens and about S sentences, in-batch negatives by a fixed permutation, score_aggregation
    'l2wasserstein', sentsup_loss_prop = sent_loss_prop = 1:
    hip     HipBertTrainEncoder + SupAlignRankLoss.forward_rank                         this project's kernels end to end
    torch   HuggingFace BertModel under torch autograd, the read-out and the loss restated in torch on the same card: the span mean
            pool as ONE torch.bmm with a [B, S, L] averaging matrix built outside the timed region, torch.cdist, the Sinkhorn
            restatement of the OT backward's tests (oracle helpers: the epsilon-scaling loop as eager torch ops, which is how
            geomloss runs it for the reference) and the aligned entries' hinge
    The two sides differ in more than kernels: the figure is the cost of a step as a user would run it either way, not a kernel
    comparison (the encoder alone: tools/encoder_backward_time.py).
(b) the cross-document distance matrix, forward + backward from a [B, S, S] gradient: torch.ops.aspire.sent_cdist against torch.cdist
    (direct differences) under autograd.  Both sides sit near the launch floor at the training shape.

    python tools/supalign_step_time.py [--shape 10x256] [--sents 8] [--layers 12] [--cdist 10x12]

Needs a GPU; there is no CPU path.
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tools.cls_train_time import timed  # noqa: E402

MARGIN = 1.0


def _documents(b, l, sents, gen):
    """-> tok [b, l], mask [b, l], abs_lens, senttok_idxs: [CLS] title [SEP] sentence ... of l tokens, `sents` +- 2 sentences"""
    tok = torch.randint(5, 3000, (b, l), generator=gen)
    lens, idxs = [], []
    for _ in range(b):
        n = int(torch.randint(max(sents - 2, 1), sents + 3, (1,), generator=gen))
        cuts = torch.linspace(6, l - 1, n + 1).long().tolist()
        idxs.append([list(range(cuts[i], cuts[i + 1])) for i in range(n)])
        lens.append(n)
    return tok, torch.ones(b, l, dtype=torch.long), lens, idxs


def _pool_matrix(idxs, lens, l):
    """[B, max_sents, l]: row (b, s) holds 1 / len(span) at sentence s's tokens, zeros for a slot the document does not have"""
    w = torch.zeros(len(idxs), max(lens), l)
    for b, spans in enumerate(idxs):
        for s, span in enumerate(spans):
            w[b, s, span] = 1.0 / len(span)
    return w


def _torch_loss(hf, q, p, perm, align, neg_align, hp):
    """the train branch of WordSentAbsSupAlignBiEnc.forward_rank in torch on the device"""
    from oracle import aspire_oracle as orc

    def reps(doc):
        tok, mask, lens, idxs, pool = doc
        return torch.bmm(pool, hf(tok, attention_mask=mask).last_hidden_state)        # [B, S, L] x [B, L, 768]: empty slots are zeros

    def ot_dist(x, y, xl, yl):
        neg = -1 * torch.cdist(x, y)
        mask = torch.full_like(neg, -10e8)
        for i, (a, b) in enumerate(zip(xl, yl)):
            mask[i, :a, :b] = 0.0
        a_w, b_w = orc.marginals(neg + mask, hp['sent_sm_temp'])
        c_xy, c_yx = orc._distances(x, y.detach()), orc._distances(y, x.detach())
        eps_s = orc.epsilon_schedule(1, orc.max_diameter(x.detach(), y.detach()), hp['geoml_blur'], hp['geoml_scaling'])
        with torch.no_grad():
            a_log, b_log = orc._log_weights(a_w.detach().clone()), orc._log_weights(b_w.detach().clone())
            g0, f0 = orc._softmin(eps_s[0], c_yx, a_log), orc._softmin(eps_s[0], c_xy, b_log)
            for eps in eps_s:
                gt, ft = orc._softmin(eps, c_yx, a_log + f0 / eps), orc._softmin(eps, c_xy, b_log + g0 / eps)
                g0, f0 = 0.5 * (g0 + gt), 0.5 * (f0 + ft)
        eps = eps_s[-1]
        g = orc._softmin(eps, c_yx, (a_log + f0 / eps).detach())
        f = orc._softmin(eps, c_xy, (b_log + g0 / eps).detach())
        return (a_w * f).sum(1) + (b_w * g).sum(1)

    def sup_dist(x, y, ali):
        ali = torch.tensor(ali, device=x.device)
        n = torch.arange(x.shape[0], device=x.device)
        return torch.cdist(x, y)[n, ali[:, 0], ali[:, 1]]

    qr, pr = reps(q), reps(p)
    nr, nl = pr[torch.tensor(perm, device=pr.device)], [p[2][i] for i in perm]
    clip = [[min(a, q[2][i] - 1), min(c, p[2][i] - 1)] for i, (a, c) in enumerate(align)]
    loss = torch.clamp_min(MARGIN + sup_dist(qr, pr, clip) - sup_dist(qr, nr, neg_align), 0).sum()
    return loss + torch.clamp_min(MARGIN + ot_dist(qr, pr, q[2], p[2]) - ot_dist(qr, nr, q[2], nl), 0).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='10x256')
    ap.add_argument('--sents', type=int, default=8)
    ap.add_argument('--layers', type=int, default=12)
    ap.add_argument('--cdist', default='10x12')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-s', type=float, default=0.2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from transformers import BertConfig, BertModel
    from aspire_amd import HipBertTrainEncoder, SupAlignRankLoss
    from aspire_amd.rank_loss import negative_align_idxs
    import aspire_amd.torch_ops  # noqa: F401
    torch.manual_seed(0)
    hp = dict(model_name='sbalisentbienc', score_aggregation='l2wasserstein', geoml_blur=0.05, geoml_scaling=0.9, sent_sm_temp=1.0,
              abs_loss_prop=0.0, sent_loss_prop=1.0, sentsup_loss_prop=1.0)
    if a.shape:
        b, l = (int(x) for x in a.shape.split('x'))
        cfg = BertConfig(vocab_size=3000, hidden_size=768, num_hidden_layers=a.layers, num_attention_heads=12, intermediate_size=3072,
                         max_position_embeddings=512, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        hf = BertModel(cfg, add_pooling_layer=False).cuda().train()
        enc = HipBertTrainEncoder(copy.deepcopy(hf)).train()
        gen = torch.Generator().manual_seed(b * 1000 + l)
        docs = [_documents(b, l, a.sents, gen) for _ in range(2)]
        dev_docs = [(t.cuda(), m.cuda(), lens, idxs, _pool_matrix(idxs, lens, l).cuda()) for t, m, lens, idxs in docs]
        perm = [(i + 1) % b for i in range(b)]
        align = [[int(torch.randint(0, a.sents + 2, (1,), generator=gen)), int(torch.randint(0, a.sents + 2, (1,), generator=gen))]
                 for _ in range(b)]
        neg_align = negative_align_idxs(align, perm, docs[0][2], docs[1][2])
        batch = {'pos_align_idxs': align}
        for key, (tok, mask, lens, idxs) in zip(('query', 'pos'), docs):
            batch.update({key + '_bert_batch': {'tokid_tt': tok, 'seg_tt': torch.zeros_like(tok), 'attnmask_tt': mask, 'seq_lens': [l] * b},
                          key + '_abs_lens': lens, key + '_senttok_idxs': idxs})
        loss_fn = SupAlignRankLoss(hp).forward_rank
        last = {}

        def hip():
            enc.zero_grad(set_to_none=True)
            last['hip'] = loss_fn(batch, enc, random_idxs=perm)
            last['hip'].backward()

        def torch_side():
            hf.zero_grad(set_to_none=True)
            last['torch'] = _torch_loss(hf, dev_docs[0], dev_docs[1], perm, align, neg_align, hp)
            last['torch'].backward()

        hip()
        torch_side()
        res = dict(step='sbalisentbienc-misup-ot', B=b, L=l, sents=a.sents, layers=a.layers, loss_hip=float(last['hip']),
                   loss_torch=float(last['torch']))
        res['loss_rel_diff'] = abs(res['loss_hip'] - res['loss_torch']) / max(1.0, abs(res['loss_torch']))     # (both sides time one loss)
        res.update(timed({'hip': hip, 'torch': torch_side}, a.windows, a.window_s))
        res['hip_over_torch'] = round(res['hip_ms_median'] / res['torch_ms_median'], 3)
        res['peak_mem_gb'] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
        print(json.dumps(res), flush=True)
    for spec in [s for s in a.cdist.split(',') if s]:
        b, s = (int(x) for x in spec.split('x'))
        gen = torch.Generator().manual_seed(b * 100 + s)
        q = torch.randn(b, s, 768, generator=gen).cuda().requires_grad_()
        c = torch.randn(b, s, 768, generator=gen).cuda().requires_grad_()
        g = torch.randn(b, s, s, generator=gen).cuda()
        lens = torch.full((b,), s, dtype=torch.int32).cuda()

        def ours():
            q.grad = c.grad = None
            (torch.ops.aspire.sent_cdist(q, lens, c, lens) * g).sum().backward()

        def theirs():
            q.grad = c.grad = None
            (torch.cdist(q, c, compute_mode='donot_use_mm_for_euclid_dist') * g).sum().backward()

        res = dict(cdist_B=b, cdist_S=s)
        res.update(timed({'ours': ours, 'torch': theirs}, a.windows, a.window_s))
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
