"""GPU: training sbalisentbienc -- the cross-document distance matrix under autograd (aspire_sent_cdist_f32 / _backward_f32,
torch.ops.aspire.sent_cdist), aspire_amd.cross_doc_l1, aspire_amd.SupAlignRankLoss.forward_rank from last_hidden_state to the loss and
back, and RankTrainer on model_name 'sbalisentbienc' down to a model_final.pt the inference side loads.  Inputs, yardsticks (float64
torch on the CPU) and cases: tests/golden/supalign_inputs.py; the reference's own fp32 figures: tests/golden/supalign.npz
(make_golden_supalign.py).

Tolerance, everywhere: trainside_inputs.bound = max(4 * ref_err, 4 * 2^-23 * max|yardstick|) per tensor.  For the distance matrix
ref_err is the deviation of fp32 torch.cdist autograd on the CPU from the float64 one (computed here, once per case); for the loss it
is the REFERENCE's fp32 deviation from the float64 yardstick as the generator recorded it, losses the same way from loss_err and |loss|.

Largest |kernel - float64| on an MI355X against its bound, per case (distance matrix: over B in {1, 3}; loss cases: the loss, then the
largest gradient error over the hidden states).  The largest ratio error / bound: 0.214 for the distance matrix (128x128, grad_c),
0.41 for a loss (l2max_train_sup), 0.24 for a hidden-state gradient (l2max_dev_a5).

    distance matrix    dist        bound        grad_q      bound        grad_c      bound
    1x1                1.877e-06   5.353e-05    9.213e-09   2.016e-07    9.213e-09   2.016e-07
    1x5                2.915e-06   5.744e-05    4.126e-08   6.598e-07    4.022e-08   6.947e-07
    5x1                2.879e-06   7.154e-05    1.586e-08   3.038e-07    4.043e-08   3.718e-07
    4x4                2.791e-06   7.017e-05    3.049e-08   6.136e-07    3.142e-08   3.042e-07
    5x3                2.779e-06   8.571e-05    3.650e-08   4.503e-07    5.656e-08   6.459e-07
    9x7 (6, 4)         3.070e-06   9.828e-05    6.905e-08   6.349e-07    9.879e-08   7.164e-07
    33x2               3.273e-06   1.172e-04    5.060e-08   9.406e-07    2.556e-07   1.948e-06
    128x128            3.797e-06   1.257e-04    1.285e-06   6.527e-06    1.072e-06   5.008e-06
    identical rows     2.249e-06   7.338e-05    3.349e-08   4.080e-07    4.215e-08   4.082e-07
    cross_doc_l1 9x7   4.390e-04   4.103e-03    1.164e-07   1.036e-06    1.369e-07   1.598e-06      (first column: the value)
    cross_doc_l1 4x4   1.854e-05   3.016e-04    3.349e-08   3.485e-07    4.138e-08   4.239e-07

    loss case                 loss error  bound        gradient error  bound
    l2max_train_sup           6.146e-07   1.505e-06    2.448e-09       3.662e-08
    l2max_train_all           7.228e-07   6.645e-06    7.957e-09       3.661e-08
    l2max_train_w             8.362e-07   8.099e-06    3.751e-09       3.661e-08
    ot_train                  1.215e-07   1.821e-06    4.949e-09       1.169e-07
    ot_train_w_a5             2.530e-07   2.912e-06    7.957e-09       8.535e-08
    l2max_dev_a0              2.189e-07   4.690e-06    9.732e-09       4.172e-08
    l2max_dev_a5              7.538e-08   5.478e-06    9.970e-09       4.172e-08
    ot_dev_a5                 2.843e-07   5.414e-06    9.970e-09       1.590e-07
    small_l2max_train_all     4.514e-07   2.759e-06    8.165e-09       4.258e-08
    small_l2max_train_w       9.110e-08   1.318e-06    2.649e-09       1.546e-08
    small_svalue              7.863e-07   6.960e-06    1.136e-08       5.670e-08      (torch's batched SVD on the device)

The trained module's eval() sentence rows and AspireConSent on model_final.pt: max |diff| 0.

Every comparison prints its figures before it asserts (pytest -s shows them).
"""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import supalign_inputs as si  # noqa: E402
import test_gpu_trainer as tg  # noqa: E402
from test_gpu_embed_train import SEED, TABLES, _trainer_runs  # noqa: E402

pytestmark = pytest.mark.gpu
D = 768


@pytest.fixture(scope='module')
def amd():
    import aspire_amd
    from aspire_amd import ops, _lib, pair_distances
    import aspire_amd.torch_ops as torch_ops
    assert torch.cuda.is_available()
    return type('NS', (), dict(pkg=aspire_amd, ops=ops, lib=_lib, to=torch_ops, pd=pair_distances))


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'supalign.npz'))


# ---- sent_cdist ---------------------------------------------------------------------------------------------------------------------------
CDIST_CASES = [(shape, b) for shape in si.CDIST_SHAPES for b in ((1, 3) if shape != '128x128' else (1,))]


@functools.lru_cache(maxsize=None)
def _cdist_case(shape, b):
    """(inputs, float64 (dist, grad_q, grad_c), the bound of each) -- computed once per case, never written to"""
    q, c, qlens, clens, g = si.cdist_case(shape, b)
    ref64 = si.cdist_ref(q, c, g, torch.float64, qlens, clens)
    ref32 = si.cdist_ref(q, c, g, torch.float32, qlens, clens)
    tols = [si.bound(np.abs(a32 - a64).max(), np.abs(a64).max()) for a32, a64 in zip(ref32, ref64)]
    return (q, c, qlens, clens, g), ref64, tols


def _lens(lens):
    return torch.tensor(lens, dtype=torch.int32).cuda()


def _abi(amd, q, c, qlens, clens, g, fill=float('nan')):
    """the C ABI through ops, the gradients into filled buffers: an element the kernel does not write shows"""
    qs, cs = amd.ops.DeviceRepSet.from_padded(torch.from_numpy(q), qlens), amd.ops.DeviceRepSet.from_padded(torch.from_numpy(c), clens)
    dist = amd.ops.sent_cdist(qs, cs)
    out = (torch.full_like(qs.rows, fill), torch.full_like(cs.rows, fill))
    gq, gc = amd.ops.sent_cdist_backward(qs, cs, torch.from_numpy(g).cuda(), out=out)
    assert gq is out[0] and gc is out[1]
    return dist.cpu().numpy(), gq.view(q.shape).cpu().numpy(), gc.view(c.shape).cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize('shape,b', CDIST_CASES)
def test_sent_cdist_forward_and_backward_match_float64(amd, shape, b):
    (q, c, qlens, clens, g), ref64, tols = _cdist_case(shape, b)
    got = _abi(amd, q, c, qlens, clens, g)
    ratios = []
    for what, a, a64, tol in zip(('dist', 'grad_q', 'grad_c'), got, ref64, tols):
        assert not np.isnan(a).any(), f'{what}: an element was not written'
        err = float(np.abs(a - a64).max())
        ratios.append(err / tol)
        print(f'[cdist {shape} B={b}] {what}: |kernel - float64| {err:.3e}, bound {tol:.3e}, ratio {err / tol:.3f}')
    assert max(ratios) <= 1.0
    dist, gq, gc = got
    for k in range(b):          # pads: the real row's norm, an exact zero against another pad; exact-zero gradient rows
        assert (dist[k, qlens[k]:, clens[k]:] == 0).all() and (gq[k, qlens[k]:] == 0).all() and (gc[k, clens[k]:] == 0).all()
        if qlens[k] < q.shape[1]:
            assert (dist[k, qlens[k]:, :clens[k]] > 1).all() and (dist[k, :qlens[k], clens[k]:] > 1).all()
    # the operator under autograd: the same bits, forward and backward
    ql, cl = _lens(qlens), _lens(clens)
    qt, ct = torch.from_numpy(q).cuda().requires_grad_(True), torch.from_numpy(c).cuda().requires_grad_(True)
    d = torch.ops.aspire.sent_cdist(qt, ql, ct, cl)
    assert d.shape == g.shape and d.requires_grad and _same_bits(d.detach().cpu().numpy(), dist)
    (d * torch.from_numpy(g).cuda()).sum().backward()
    assert _same_bits(qt.grad.cpu().numpy(), gq) and _same_bits(ct.grad.cpu().numpy(), gc)
    # a second run, into buffers filled with something else: equal bits
    again = _abi(amd, q, c, qlens, clens, g, fill=1.0)
    assert all(_same_bits(x, y) for x, y in zip(got, again))


def test_sent_cdist_pad_rows_are_zeros_and_never_read(amd):
    """what stands in a pad row of the inputs does not matter: NaN there reaches nothing"""
    (q, c, qlens, clens, g), _, _ = _cdist_case('9x7', 3)
    want = _abi(amd, q, c, qlens, clens, g)
    qn, cn = q.copy(), c.copy()
    for k in range(3):
        qn[k, qlens[k]:] = np.nan
        cn[k, clens[k]:] = np.nan
    got = _abi(amd, qn, cn, qlens, clens, g)
    assert all(_same_bits(x, y) for x, y in zip(got, want))
    assert min(qlens) < 9 and min(clens) < 7


def test_sent_cdist_identical_rows_contribute_an_exact_zero(amd):
    """d_ij == 0 (torch.cdist's backward rule): whatever G_ij is, the entry adds nothing; float64 autograd agrees"""
    q, c, qlens, clens, g = (x.copy() if isinstance(x, np.ndarray) else x for x in si.cdist_case('5x3', 3))
    c[1, 2] = q[1, 3]
    c[2, 0] = q[2, 0]
    ref64 = si.cdist_ref(q, c, g, torch.float64, qlens, clens)
    ref32 = si.cdist_ref(q, c, g, torch.float32, qlens, clens)
    got = _abi(amd, q, c, qlens, clens, g)
    assert got[0][1, 3, 2] == 0 and got[0][2, 0, 0] == 0 and ref64[0][1, 3, 2] == 0
    for what, a, a32, a64 in zip(('dist', 'grad_q', 'grad_c'), got, ref32, ref64):
        err, tol = float(np.abs(a - a64).max()), si.bound(np.abs(a32 - a64).max(), np.abs(a64).max())
        print(f'[cdist identical rows] {what}: |kernel - float64| {err:.3e}, bound {tol:.3e}')
        assert not np.isnan(a).any() and err <= tol
    g2 = g.copy()
    g2[1, 3, 2], g2[2, 0, 0] = 1e30, -7.0
    other = _abi(amd, q, c, qlens, clens, g2)
    assert all(_same_bits(x, y) for x, y in zip(got, other))


def test_sent_cdist_length_above_the_bound_poisons_that_pair_only(amd):
    (q, c, qlens, clens, g), _, _ = _cdist_case('5x3', 3)
    want = _abi(amd, q, c, qlens, clens, g)
    ql, cl = _lens([5, 6, 5]), _lens(clens)
    qt, ct, gt = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(g).cuda()
    dist = torch.ops.aspire.sent_cdist(qt, ql, ct, cl).cpu().numpy()
    gq, gc = (t.cpu().numpy() for t in torch.ops.aspire.sent_cdist_backward(gt, qt, ql, ct, cl))
    for got, ref in zip((dist, gq, gc), want):
        assert np.isnan(got[1]).all() and _same_bits(got[[0, 2]], ref[[0, 2]])


def test_sent_cdist_opcheck_and_refusals(amd):
    (q, c, qlens, clens, g), _, _ = _cdist_case('9x7', 3)
    ql, cl = _lens(qlens), _lens(clens)
    torch.library.opcheck(torch.ops.aspire.sent_cdist, (torch.from_numpy(q).cuda().requires_grad_(), ql, torch.from_numpy(c).cuda().requires_grad_(), cl))
    torch.library.opcheck(torch.ops.aspire.sent_cdist_backward, (torch.from_numpy(g).cuda(), torch.from_numpy(q).cuda(), ql, torch.from_numpy(c).cuda(), cl))
    with pytest.raises(AssertionError, match='equal batch sizes'):
        torch.ops.aspire.sent_cdist(torch.from_numpy(q).cuda(), ql, torch.from_numpy(c[:2]).cuda(), cl[:2])
    with pytest.raises(NotImplementedError, match='128'):
        torch.ops.aspire.sent_cdist(torch.zeros(1, 129, D, device='cuda'), _lens([129]), torch.zeros(1, 2, D, device='cuda'), _lens([2]))
    # the host layer: a document without rows is refused as everywhere; without grad the matrix is detached and has the same bits
    cand = amd.pd.rep_len_tup(embed=torch.from_numpy(c).permute(0, 2, 1), abs_lens=clens)
    reps = amd.pd.rep_len_tup(embed=torch.from_numpy(q).permute(0, 2, 1), abs_lens=[0] + qlens[1:])
    with pytest.raises(ValueError, match='without sentence rows'):
        amd.pd.sent_cdist(reps, cand)
    plain = amd.pd.sent_cdist(reps._replace(abs_lens=qlens), cand)
    attached = amd.pd.sent_cdist(reps._replace(embed=reps.embed.clone().requires_grad_(True), abs_lens=qlens), cand)
    assert not plain.requires_grad and attached.requires_grad and torch.equal(plain, attached.detach())


@pytest.mark.parametrize('shape,b', [('9x7', 3), ('4x4', 1)])
def test_cross_doc_l1_matches_the_reference_expression(amd, shape, b):
    """disent_models.py:655-658 in float64: linalg.norm(ord=1) of every flattened -cdist block, summed; the gradients through it"""
    (q, c, qlens, clens, _), _, _ = _cdist_case(shape, b)

    def ref(dtype):
        qt, ct = torch.tensor(q, dtype=dtype, requires_grad=True), torch.tensor(c, dtype=dtype, requires_grad=True)
        pair_sims = -1 * torch.cdist(qt, ct, compute_mode='donot_use_mm_for_euclid_dist')
        reg = torch.sum(torch.linalg.norm(pair_sims.view(b, -1), ord=1, dim=1))
        reg.backward()
        gq, gc = qt.grad.numpy(), ct.grad.numpy()
        for k in range(b):          # the pad rows are constants in the reference (its read-out's zeros): no gradient
            gq[k, qlens[k]:], gc[k, clens[k]:] = 0, 0
        return reg.item(), gq, gc

    r64, r32 = ref(torch.float64), ref(torch.float32)
    qt, ct = torch.from_numpy(q).requires_grad_(True), torch.from_numpy(c).requires_grad_(True)       # on the CPU, as the examples' are
    reg = amd.pkg.cross_doc_l1(amd.pd.rep_len_tup(embed=qt.permute(0, 2, 1), abs_lens=qlens),
                               amd.pd.rep_len_tup(embed=ct.permute(0, 2, 1), abs_lens=clens))
    assert reg.dim() == 0 and reg.requires_grad
    reg.backward()
    for what, a, a32, a64 in zip(('value', 'grad_q', 'grad_c'), (np.float64(reg.item()), qt.grad.numpy(), ct.grad.numpy()), r32, r64):
        err, tol = float(np.abs(a - a64).max()), si.bound(np.abs(np.asarray(a32) - a64).max(), np.abs(a64).max())
        print(f'[cross_doc_l1 {shape} B={b}] {what}: |kernel - float64| {err:.3e}, bound {tol:.3e}')
        assert err <= tol


# ---- SupAlignRankLoss.forward_rank -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rank_inputs(size):
    return si.rank_inputs(size)


@functools.lru_cache(maxsize=None)
def _rank_yardstick(name):
    """(float64 loss, float64 hidden-state gradients) -- computed once per case, never written to"""
    size, dev, hp = si.CASES[name]
    loss, grads, _ = si.supalign_loss64(_rank_inputs(size), dev, hp)
    return loss, grads


def _run_case(amd, name):
    size, dev, hp = si.CASES[name]
    inp = _rank_inputs(size)
    leaves, batch = {}, {}
    for w, key in (('q', 'query'), ('p', 'pos'), ('n', 'neg'))[:3 if dev else 2]:
        leaves[w] = torch.from_numpy(inp[w + '_hidden']).cuda().requires_grad_(True)
        batch[key + '_bert_batch'] = {'which': w}
        batch[key + '_abs_lens'] = list(inp[w + '_lens'])
        batch[key + '_senttok_idxs'] = inp[w + '_idxs']
    batch['pos_align_idxs'] = [list(a) for a in inp['align']]
    calls = []

    def encoder(bert_batch):
        calls.append(bert_batch['which'])
        return leaves[bert_batch['which']]

    loss = amd.pkg.SupAlignRankLoss(hp).forward_rank(batch, encoder, random_idxs=None if dev else torch.tensor(inp['perm']))
    assert calls == list(leaves) and loss.is_cuda and loss.dim() == 0
    assert batch['pos_align_idxs'] == inp['align'], 'the batch\'s alignment lists were written to'
    loss.backward()
    return inp, leaves, loss


@pytest.mark.parametrize('name', [n for n in si.CASES if n not in si.SVALUE_CASES])
def test_forward_rank_loss_and_hidden_gradients(amd, name):
    size, dev, hp = si.CASES[name]
    fx = _fixture()
    want_loss, want = _rank_yardstick(name)
    inp, leaves, loss = _run_case(amd, name)
    loss_tol = si.bound(fx[f'{name}_loss_err'], fx[f'{name}_max_loss'])
    grad_tol = si.bound(fx[f'{name}_ref_err'], fx[f'{name}_max_grad'])
    loss_err = abs(loss.item() - want_loss)
    errs = [float(np.abs(leaves[w].grad.cpu().numpy() - g).max()) for w, g in zip(leaves, want)]
    print(f'[{name}] loss {loss.item():.6f} |kernel - float64| {loss_err:.3e} bound {loss_tol:.3e} (reference {float(fx[f"{name}_loss"]):.6f}); '
          f'gradients {" ".join(f"{e:.3e}" for e in errs)} bound {grad_tol:.3e}; active {json.loads(str(fx[f"{name}_active"]))}')
    assert loss_err <= loss_tol
    if hp['score_aggregation'] != 'l2wasserstein':        # the reference's own fp32 loss sits loss_err from float64
        assert abs(loss.item() - float(fx[f'{name}_loss'])) <= loss_tol + float(fx[f'{name}_loss_err'])
    assert max(errs) <= grad_tol
    for w in leaves:
        g = leaves[w].grad.cpu().numpy()
        for b, doc in enumerate(inp[w + '_idxs']):
            free = sorted(set(range(1, inp['L'])) - {t for span in doc for t in span})
            assert free and (g[b, free] == 0).all(), 'a token of no span has a gradient'
            if hp['abs_loss_prop'] == 0:
                assert (g[b, 0] == 0).all()       # the CLS rows took no part in the loss
    if name in si.SMALL_CASES:        # the reference's stored gradients themselves
        for w in leaves:
            dev_ = float(np.abs(leaves[w].grad.cpu().numpy() - fx[f'{name}_grad_{w}']).max())
            assert dev_ <= grad_tol + float(fx[f'{name}_ref_err'])


def test_forward_rank_dev_branch_ignores_sent_loss_prop_and_the_alignments(amd):
    """disent_models.py:797: the dev loss is the sentence hinge unscaled -- RankLoss's value at sent_loss_prop 1 in every bit"""
    import readout_inputs as ri
    inp = _rank_inputs('std')
    hid = {w: torch.from_numpy(inp[w + '_hidden']).cuda() for w in 'qpn'}
    batch = {}
    for w, key in (('q', 'query'), ('p', 'pos'), ('n', 'neg')):
        batch.update({key + '_bert_batch': w, key + '_abs_lens': inp[w + '_lens'], key + '_senttok_idxs': inp[w + '_idxs']})
    hp = si.CASES['l2max_dev_a5'][2]
    assert hp['sent_loss_prop'] == 0.25
    want = amd.pkg.RankLoss(ri.hparams('l2max', 0.5)).forward_rank(batch, lambda w: hid[w])
    got = amd.pkg.SupAlignRankLoss(hp).forward_rank(batch, lambda w: hid[w])            # no 'pos_align_idxs' in the batch at all
    assert torch.equal(got, want) and not got.requires_grad
    batch['pos_align_idxs'] = [[-1, -1]] * inp['B']
    assert torch.equal(amd.pkg.SupAlignRankLoss(hp).forward_rank(batch, lambda w: hid[w]), want)
    # the train branch reads them: a missing key and a negative index are errors
    del batch['neg_bert_batch']
    with pytest.raises(ValueError, match='negative'):
        amd.pkg.SupAlignRankLoss(hp).forward_rank(batch, lambda w: hid[w], random_idxs=inp['perm'])
    del batch['pos_align_idxs']
    with pytest.raises(KeyError, match='pos_align_idxs'):
        amd.pkg.SupAlignRankLoss(hp).forward_rank(batch, lambda w: hid[w], random_idxs=inp['perm'])


@pytest.mark.parametrize('name', si.SVALUE_CASES)
def test_forward_rank_with_the_singular_value_regulariser(amd, name):
    """cd_svalue_l1_prop: torch's batched SVD on the device over -sent_cdist, against float64 on the CPU"""
    fx = _fixture()
    want_loss, want = _rank_yardstick(name)
    inp, leaves, loss = _run_case(amd, name)
    loss_tol = si.bound(fx[f'{name}_loss_err'], fx[f'{name}_max_loss'])
    grad_tol = si.bound(fx[f'{name}_ref_err'], fx[f'{name}_max_grad'])
    loss_err = abs(loss.item() - want_loss)
    errs = [float(np.abs(leaves[w].grad.cpu().numpy() - g).max()) for w, g in zip(leaves, want)]
    print(f'[{name}] loss {loss.item():.6f} |kernel - float64| {loss_err:.3e} bound {loss_tol:.3e}; '
          f'gradients {" ".join(f"{e:.3e}" for e in errs)} bound {grad_tol:.3e}')
    assert loss_err <= loss_tol and max(errs) <= grad_tol


# ---- the trainer and the model file ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _train_batches(tmp):
    """two training batches (query + positive, pre-aligned) of three abstracts each, by batch_prep.make_batch"""
    from transformers import BertTokenizer
    from aspire_amd.batch_prep import make_batch
    path = os.path.join(tmp, 'supalign_vocab.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]', '.'] + tg.WORDS) + '\n')
    tok = BertTokenizer(path, do_lower_case=True)
    out = []
    for base, align in ((10, [[0, 0], [2, 1], [1, 5]]), (20, [[1, 0], [0, 0], [4, 2]])):
        pos = [dict(ex, cc_align=a) for ex, a in zip(tg._abstracts(base + 2), align)]
        batch = make_batch({'query_texts': tg._abstracts(base + 1), 'pos_texts': pos}, tok)
        assert batch['pos_align_idxs'] == align and 'neg_bert_batch' not in batch
        assert all(batch[k + '_bert_batch']['tokid_tt'].shape == (3, batch[k + '_bert_batch']['tokid_tt'].shape[1]) and
                   batch[k + '_bert_batch']['tokid_tt'].shape[1] <= 48 for k in ('query', 'pos'))
        out.append(batch)
    return out


def test_rank_trainer_on_sbalisentbienc_repeats_resumes_and_feeds_inference(amd, tmp_path, tmp_path_factory, monkeypatch):
    """model_name 'sbalisentbienc' makes RankTrainer train SupAlignRankLoss; dropout on, the tables trained.  The in-batch permutation is
    the reference's torch.randperm on the global generator: the checkpoint carries that generator's state, so the resumed run (whose
    model was built from another seed) draws what the straight one drew.  torch.randperm is only listened to here, not replaced."""
    from transformers import BertModel
    from aspire_amd import AspireConSent, HipBertTrainEncoder, RankTrainer, SupAlignRankLoss, sent_reps_from_hidden
    batches = _train_batches(str(tmp_path_factory.getbasetemp()))
    hparams = dict(si.CASES['ot_train'][2], abs_loss_prop=0.5)
    assert hparams['model_name'] == 'sbalisentbienc'
    drawn, real_randperm = {}, torch.randperm

    def listening_randperm(n, *a, **k):
        perm = real_randperm(n, *a, **k)
        drawn[drawn['tag']].append(perm.tolist())
        return perm

    monkeypatch.setattr(torch, 'randperm', listening_randperm)

    def make(seed, tag):
        drawn['tag'] = tag
        drawn[tag] = []
        enc = HipBertTrainEncoder(tg._bert(seed, dropout=0.1), dropout=True, seed=SEED, hip_embeddings=True)
        return RankTrainer(enc, hparams, tg._train_hparams(), str(tmp_path / tag), lambda epoch: batches)

    probe = make(5, 'start')
    assert isinstance(probe.loss_fn.__self__, SupAlignRankLoss)
    start = {n: p.detach().clone() for n, p in probe.encoder.bert.named_parameters()}
    straight, trained = _trainer_runs(make, tmp_path / 'ck.pt')
    assert trained >= 19
    assert len(drawn['straight']) == 4 and drawn['again'] == drawn['straight'] and drawn['first'] + drawn['second'] == drawn['straight']
    params = dict(straight.encoder.bert.named_parameters())
    for n in TABLES:
        assert int(straight.optimizer.state[params[n]]['step']) == 4 and not torch.equal(params[n].detach(), start[n]), n
    assert np.isfinite(straight.loss_history['loss'][0]) and straight.loss_history['loss'][0] > 0
    # model_final.pt is encoder.state_dict(): it loads into the inference side, which gives the training module's eval() sentence rows
    assert straight.train() is True
    sd = torch.load(tmp_path / 'straight' / 'model_final.pt', weights_only=True)
    assert set(sd) == set(straight.encoder.bert.state_dict())
    bert = BertModel(straight.encoder.config)
    bert.load_state_dict({k: v.cpu() for k, v in sd.items()})
    inf = AspireConSent(bert_model=bert.eval())
    b = batches[0]
    cls, sent = inf.forward_device(b['pos_bert_batch'], b['pos_abs_lens'], b['pos_senttok_idxs'])
    with torch.no_grad():
        want_cls, want_sent = sent_reps_from_hidden(straight.encoder.eval()(b['pos_bert_batch']), b['pos_abs_lens'], b['pos_senttok_idxs'])
    diff = max(float((sent - want_sent.permute(0, 2, 1)).abs().max()), float((cls - want_cls).abs().max()))
    print(f'[sbalisentbienc] trained eval() sentence rows vs AspireConSent on model_final.pt: max |diff| {diff:.3e}')
    assert torch.isfinite(sent).all() and sent.shape == (3, max(b['pos_abs_lens']), D) and diff <= 1e-4
