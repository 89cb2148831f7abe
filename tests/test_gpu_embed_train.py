"""GPU: the embedding lookup under training in HIP -- aspire_bert_embed_sum_f32 / aspire_bert_embed_backward_f32, the operators over them
(torch.ops.aspire.bert_embed_sum / bert_embed_backward), HipBertTrainEncoder(hip_embeddings=True) and RankTrainer with the tables trained.

Tables: vocab 301 (not a multiple of the four rows per workgroup), max_pos 160 and 64, n_types 2 and 1.  The reference is
tests/embed_ref.py (numpy, the kernels' fp32 orders and float64), computed once per case.  Gradient rows are scaled by
10 ** randint(-3, 3), so the summation order shows in the bits.  The bound is the project's: max(4 x torch's fp32 CPU error,
4 x 2^-23 max |float64|) per tensor.
"""
import copy
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import embed_ref as er  # noqa: E402
import test_gpu_trainer as tg  # noqa: E402

pytestmark = pytest.mark.gpu
VOCAB = 301
PATTERN = 0x7FC12345        # a NaN with a payload: what the arena holds where no kernel may write


def _tables(max_pos, n_types, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, er.D)).astype(np.float32) for n in (VOCAB, max_pos, n_types)]


def _cuda(*arrays):
    return [torch.from_numpy(np.array(a)).cuda() if a is not None else None for a in arrays]


# ---- 1. forward ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b,l,max_pos,n_types,with_typ', [(1, 1, 160, 2, True), (2, 130, 160, 2, True), (3, 64, 64, 1, True),
                                                         (2, 130, 160, 2, False)])
def test_forward_gives_torchs_bits(b, l, max_pos, n_types, with_typ):
    import aspire_amd.torch_ops  # noqa: F401
    rng = np.random.default_rng(b * l)
    tok = rng.integers(0, VOCAB, size=(b, l))
    tok[0, 0], tok[-1, -1] = VOCAB - 1, 0
    if b * l == 1:
        tok[0, 0] = VOCAB - 1
    typ = rng.integers(0, n_types, size=(b, l))
    word, pos, typ_tab = _cuda(*_tables(max_pos, n_types))
    t, y = _cuda(tok, typ)
    got = torch.ops.aspire.bert_embed_sum(t, y if with_typ else None, word, pos, typ_tab, 0)
    want = (torch.nn.functional.embedding(t, word) + torch.nn.functional.embedding(y if with_typ else torch.zeros_like(t), typ_tab)) + pos[:l]
    assert got.shape == (b, l, er.D) and got.dtype == torch.float32 and torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy(), er.forward(*_tables(max_pos, n_types), tok, typ if with_typ else None))


# ---- 2. backward at the C ABI -----------------------------------------------------------------------------------------------------------------
# name -> (B, L, max_pos, n_types, padding_idx, ids, types)
CASES = {
    'distinct': (2, 130, 160, 2, 0, 'distinct', 'mixed'),
    'equal': (2, 130, 160, 2, 0, 'equal', 'ones'),
    'mixed': (2, 130, 160, 2, 0, 'mixed', 'zeros'),
    'nopad': (2, 130, 160, 2, -1, 'mixed', 'mixed'),
    'notyp': (2, 130, 160, 2, 0, 'mixed', None),
    'full': (3, 64, 64, 1, 0, 'mixed', 'zeros'),
    'one': (1, 1, 160, 2, 0, 'distinct', 'ones'),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """ids, types, gradient rows and the reference's three gradients in fp32 (the kernels' orders) and float64, torch's fp32 / float64
    CPU autograd beside them (the bound's yardstick) -- computed once per case, never written to"""
    b, l, max_pos, n_types, pad, ids, types = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if ids == 'distinct':
        tok = rng.permutation(VOCAB)[:b * l].reshape(b, l)
    elif ids == 'equal':
        tok = np.full((b, l), 7)
    else:
        tok = rng.integers(1, VOCAB, size=(b, l))
        tok[rng.random((b, l)) < 1 / 3] = 0
        tok[0, 0], tok[-1, -1] = VOCAB - 1, 0
    typ = {'mixed': rng.integers(0, n_types, size=(b, l)), 'ones': np.full((b, l), n_types - 1), 'zeros': np.zeros((b, l), dtype=np.int64),
           None: None}[types]
    tok = tok.astype(np.int64)
    typ = typ.astype(np.int64) if typ is not None else None
    grad = er.order_grads(b, l, 1000 + b * l)
    want32 = er.backward(grad, tok, typ, VOCAB, max_pos, n_types, pad=pad)
    want64 = er.backward(grad, tok, typ, VOCAB, max_pos, n_types, pad=pad, dtype=np.float64)
    torch_runs = {}
    for dt in (torch.float32, torch.float64):
        tabs = [torch.zeros(n, er.D, dtype=dt, requires_grad=True) for n in (VOCAB, max_pos, n_types)]
        t, y = torch.from_numpy(tok), torch.from_numpy(typ if typ is not None else np.zeros_like(tok))
        out = (torch.nn.functional.embedding(t, tabs[0], padding_idx=None if pad < 0 else pad)
               + torch.nn.functional.embedding(y, tabs[2])) + tabs[1][:l]
        out.backward(torch.from_numpy(grad).to(dt))
        torch_runs[dt] = [x.grad.numpy() for x in tabs]
    for a in (tok, grad) + want32 + want64:
        a.setflags(write=False)
    return tok, typ, grad, want32, want64, torch_runs


def _raw_backward(name, want=(True, True, True)):
    """one aspire_bert_embed_backward_f32 call whose three outputs and workspace are carved from ONE arena filled with PATTERN, four
    guard words around each -> the three arrays (None where not wanted); checks that no word outside them changed"""
    from aspire_amd import _lib, ops
    lib = _lib.lib
    b, l, max_pos, n_types, pad, _, _ = CASES[name]
    tok, typ, grad = _case(name)[:3]
    ws_words = lib.aspire_bert_embed_workspace_bytes(b * l, VOCAB) // 4
    sizes = [VOCAB * er.D, max_pos * er.D, n_types * er.D, ws_words]
    starts, cursor = [], 4
    for n in sizes:
        starts.append(cursor)
        cursor += (n + 3) // 4 * 4 + 4
    arena = torch.full((cursor,), PATTERN, dtype=torch.int32, device='cuda')
    inside = np.zeros(cursor, dtype=bool)
    for i, (s, n) in enumerate(zip(starts, sizes)):
        if i == 3 or want[i]:
            inside[s:s + n] = True
    assert arena.data_ptr() % 16 == 0
    ptr = [ctypes.c_void_p(arena.data_ptr() + 4 * s) for s in starts]
    t, y, g = _cuda(tok, typ, grad)
    _lib.check(lib.aspire_bert_embed_backward_f32(ops._ptr(g), ops._ptr(t), ops._ptr(y), b, l, VOCAB, max_pos, n_types, pad,
                                                     *(ptr[i] if want[i] else None for i in range(3)), ptr[3], 4 * ws_words,
                                                     ops._stream()))
    after = arena.cpu().numpy()
    assert (after[~inside] == PATTERN).all(), 'a word outside the wanted tables and the workspace changed'
    shapes = [(VOCAB, er.D), (max_pos, er.D), (n_types, er.D)]
    return [after[s:s + n].view(np.float32).reshape(shape).copy() if w else None for s, n, shape, w in zip(starts, sizes, shapes, want)]


@functools.lru_cache(maxsize=None)
def _kernel_grads(name):
    return tuple(_raw_backward(name))


@pytest.mark.parametrize('name', list(CASES))
def test_backward_gives_the_reference_orders_bits(name):
    b, l, max_pos, n_types, pad, _, _ = CASES[name]
    tok, typ, grad, want32, want64, _ = _case(name)
    got = _kernel_grads(name)
    for table, g, w in zip(('word', 'pos', 'type'), got, want32):
        assert np.isfinite(g).all(), table                  # the buffers held NaN: every row was written
        diff = np.argwhere(g != w)
        assert not len(diff), (table, len(diff), diff[:4])
    gw, gp, gt = got
    named = np.zeros(VOCAB, dtype=bool)
    named[tok.reshape(-1)] = True
    assert not gw[~named].any() and not gp[l:].any()        # exact zeros: ids no token has, position rows >= L
    if pad >= 0:
        assert named[pad] or name in ('distinct', 'equal', 'one')
        assert not gw[pad].any()
    elif named[0]:
        assert gw[0].any()                                  # padding_idx = -1: row 0 carries its sum
    if name == 'equal':
        assert named.sum() == 1 and np.abs(gw[7]).max() > 0
    if typ is None or not typ.any():
        assert not gt[1:].any()
    if name != 'one':
        assert not np.array_equal(want64[2].astype(np.float32), want32[2])      # the order does matter in these sums


@pytest.mark.parametrize('name', list(CASES))
def test_backward_lies_inside_the_bound_against_float64(name):
    _, _, _, _, want64, torch_runs = _case(name)
    for table, g, w, t32, t64 in zip(('word', 'pos', 'type'), _kernel_grads(name), want64, torch_runs[torch.float32], torch_runs[torch.float64]):
        tol = er.bound(np.abs(t32.astype(np.float64) - t64).max(), np.abs(w).max())
        err = float(np.abs(g.astype(np.float64) - w).max())
        print(f'[{name}] grad_{table}: |kernel - float64| {err:.3e}  bound {tol:.3e}')
        assert err <= tol, table


@pytest.mark.parametrize('name', ['mixed', 'equal'])
def test_two_calls_give_equal_bits(name):
    first = _kernel_grads(name)
    second = _raw_backward(name)
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize('want', [(True, False, False), (False, True, False), (False, False, True), (False, True, True)])
def test_unwanted_tables_are_not_touched(want):
    """a NULL output: nothing of it is written (the arena check inside _raw_backward) and the wanted ones keep their bits"""
    got = _raw_backward('mixed', want)
    for g, w, full in zip(got, want, _kernel_grads('mixed')):
        assert (g is None) == (not w)
        assert g is None or np.array_equal(g.view(np.int32), full.view(np.int32))


def test_nothing_wanted_launches_nothing():
    from aspire_amd import _lib, ops
    import aspire_amd.torch_ops  # noqa: F401
    tok, typ, grad = _case('mixed')[:3]
    t, y, g = _cuda(tok, typ, grad)
    assert _lib.lib.aspire_bert_embed_backward_f32(ops._ptr(g), ops._ptr(t), ops._ptr(y), 2, 130, VOCAB, 160, 2, 0, None, None,
                                                      None, None, 0, ops._stream()) == _lib.ASPIRE_OK
    assert ops.bert_embed_backward(g, t, y, VOCAB, 160, 2, 0, want=(False, False, False)) == (None, None, None)
    empty = torch.ops.aspire.bert_embed_backward(g, t, y, VOCAB, 160, 2, 0, False, False, False)
    assert [e.numel() for e in empty] == [0, 0, 0]


# ---- 3. the operator under autograd ----------------------------------------------------------------------------------------------------------
def _autograd(tok, typ, tables, grad, pad, frozen=(), hip=True):
    """-> (emb_sum, [word.grad, pos.grad, type.grad]) through the operator (hip) or torch's expression"""
    import aspire_amd.torch_ops  # noqa: F401
    word, pos, typ_tab = (torch.nn.Parameter(t.clone(), requires_grad=i not in frozen) for i, t in enumerate(tables))
    if hip:
        out = torch.ops.aspire.bert_embed_sum(tok, typ, word, pos, typ_tab, pad)
    else:
        y = typ if typ is not None else torch.zeros_like(tok)
        out = (torch.nn.functional.embedding(tok, word, padding_idx=None if pad < 0 else pad)
               + torch.nn.functional.embedding(y, typ_tab)) + pos[:tok.shape[1]]
    if out.requires_grad:
        out.backward(grad)
    return out.detach(), [p.grad for p in (word, pos, typ_tab)]


@pytest.mark.parametrize('name', ['mixed', 'nopad', 'notyp', 'full'])
def test_integer_gradients_equal_torchs_gpu_autograd(name):
    """small integers: every sum is exact in any order, so torch's atomics give the same bits"""
    b, l, max_pos, n_types, pad, _, _ = CASES[name]
    tok, typ = _case(name)[:2]
    t, y = _cuda(tok, typ)
    tables = _cuda(*_tables(max_pos, n_types))
    grad = torch.randint(-3, 4, (b, l, er.D), generator=torch.Generator().manual_seed(5)).float().cuda()
    out_h, grads_h = _autograd(t, y, tables, grad, pad)
    out_t, grads_t = _autograd(t, y, tables, grad, pad, hip=False)
    assert torch.equal(out_h, out_t)
    for table, a, w in zip(('word', 'pos', 'type'), grads_h, grads_t):
        assert a.shape == w.shape and torch.equal(a, w), table


def test_operator_gives_the_c_abis_bits_and_frozen_tables_get_none():
    b, l, max_pos, n_types, pad, _, _ = CASES['mixed']
    tok, typ, grad = _case('mixed')[:3]
    t, y, g = _cuda(tok, typ, grad)
    tables = _cuda(*_tables(max_pos, n_types))
    _, full = _autograd(t, y, tables, g, pad)
    for a, w in zip(full, _kernel_grads('mixed')):
        assert np.array_equal(a.cpu().numpy().view(np.int32), w.view(np.int32))
    for frozen in ((0,), (1,), (2,)):
        _, grads = _autograd(t, y, tables, g, pad, frozen=frozen)
        for i, (a, w) in enumerate(zip(grads, full)):
            assert a is None if i in frozen else torch.equal(a, w), (frozen, i)
    out, grads = _autograd(t, y, tables, g, pad, frozen=(0, 1, 2))
    assert not out.requires_grad and grads == [None, None, None]        # no node, no backward call


def test_opcheck():
    import aspire_amd.torch_ops  # noqa: F401
    tok, typ, grad = _case('one')[:3]
    t, y, g = _cuda(tok, typ, grad)
    word, pos, typ_tab = _cuda(*_tables(160, 2))
    word.requires_grad_(True)
    pos.requires_grad_(True)
    torch.library.opcheck(torch.ops.aspire.bert_embed_sum, (t, y, word, pos, typ_tab, 0),
                          test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration'))
    torch.library.opcheck(torch.ops.aspire.bert_embed_backward, (g, t, None, VOCAB, 160, 2, -1, True, False, True),
                          test_utils=('test_schema', 'test_faketensor'))


# ---- 4. the module ---------------------------------------------------------------------------------------------------------------------------
TABLES = ['embeddings.word_embeddings.weight', 'embeddings.position_embeddings.weight', 'embeddings.token_type_embeddings.weight']


@functools.lru_cache(maxsize=None)
def _module_case():
    """test_gpu_trainer's one-layer BertModel (vocab 300, 64 positions, padding_idx 0), a ragged (3, 37) batch whose padding is id 0, a
    gradient for last_hidden_state, a mix and a gradient for the CLS rows; the float64 and fp32 CPU BertModel's gradients for both
    read-outs -- computed once"""
    m = tg._bert(6)
    assert m.embeddings.word_embeddings.padding_idx == 0
    g = torch.Generator().manual_seed(21)
    b, l = 3, 37
    tok = torch.randint(1, tg.VOCAB, (b, l), generator=g)
    typ = torch.randint(0, 2, (b, l), generator=g)
    mask = torch.ones(b, l, dtype=torch.int64)
    mask[1, 29:] = 0
    mask[2, 12:] = 0
    tok[mask == 0] = 0
    tok[0, 0], tok[0, 1] = tg.VOCAB - 1, tok[0, 2]          # the last row of the table; an id twice in one document
    G = torch.randn(b, l, 768, generator=g)
    mix = torch.softmax(torch.randn(2, generator=g), 0)
    Gc = torch.randn(b, 768, generator=g)
    runs = {}
    for dt in (torch.float64, torch.float32):
        for kind in ('hidden', 'cls'):
            mm = copy.deepcopy(m).to(dt)
            out = mm(tok, token_type_ids=typ, attention_mask=mask, output_hidden_states=True)
            if kind == 'hidden':
                (out.last_hidden_state * G.to(dt)).sum().backward()
            else:
                cls = sum(w * h[:, 0] for w, h in zip(mix.to(dt), out.hidden_states))
                (cls * Gc.to(dt)).sum().backward()
            runs[dt, kind] = {n: p.grad for n, p in mm.named_parameters() if n in TABLES}
    return m, tok, typ, mask, G, mix, Gc, runs


def _module_run(kind, hip):
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, mix, Gc, _ = _module_case()
    enc = HipBertTrainEncoder(copy.deepcopy(m), hip_embeddings=hip).train()
    if kind == 'hidden':
        out = enc(tok, token_type_ids=typ, attention_mask=mask)
        (out * G.cuda()).sum().backward()
    else:
        out = enc.forward_cls((tok, typ, mask), mix=mix.cuda())
        (out * Gc.cuda()).sum().backward()
    return out.detach(), {n: p.grad for n, p in enc.bert.named_parameters()}


@pytest.mark.parametrize('kind', ['hidden', 'cls'])
def test_module_keyword_keeps_every_other_bit_and_the_tables_match_float64(kind):
    runs = _module_case()[-1]
    out_h, grads_h = _module_run(kind, True)
    out_t, grads_t = _module_run(kind, False)
    assert out_h.shape == ((3, 37, 768) if kind == 'hidden' else (3, 768)) and torch.equal(out_h, out_t)
    for n, g in grads_t.items():
        if n.startswith('pooler.'):
            assert g is None and grads_h[n] is None
        elif n not in TABLES:
            assert torch.equal(grads_h[n], g), n
    for n in TABLES:
        w64, w32 = runs[torch.float64, kind][n], runs[torch.float32, kind][n]
        tol = er.bound(float((w32.double() - w64).abs().max()), float(w64.abs().max()))
        err = float((grads_h[n].double().cpu() - w64).abs().max())
        err_t = float((grads_t[n].double().cpu() - w64).abs().max())
        print(f'[{kind}] {n:45s} |hip - float64| {err:.3e}  |torch - float64| {err_t:.3e}  bound {tol:.3e}')
        assert torch.isfinite(grads_h[n]).all() and err <= tol, n
    assert not grads_h[TABLES[0]][0].any()          # the padding row
    assert not grads_h[TABLES[1]][37:].any()        # positions the batch does not reach


def test_host_check_raises_before_any_launch():
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask = _module_case()[:4]
    enc = HipBertTrainEncoder(copy.deepcopy(m), hip_embeddings=True, check_ids=True).train()
    bad = tok.clone()
    bad[1, 3] = tg.VOCAB
    with pytest.raises(IndexError, match='token id'):
        enc(bad, token_type_ids=typ, attention_mask=mask)
    bad[1, 3] = -1
    with pytest.raises(IndexError, match='token id'):
        enc.forward_cls((bad, typ, mask))
    bad_typ = typ.clone()
    bad_typ[2, 0] = 2
    with pytest.raises(IndexError, match='type'):
        enc(tok, token_type_ids=bad_typ, attention_mask=mask)
    assert enc.dropout_state()[1] == 0
    assert enc.hip_embeddings and enc.check_ids and not HipBertTrainEncoder(copy.deepcopy(m)).hip_embeddings


# ---- 5. the trainer --------------------------------------------------------------------------------------------------------------------------
SEED = 0x9E3779B97F4A7C15


def _same_run(a, b):
    trained = 0
    for (n, p), (_, q) in zip(a.encoder.named_parameters(), b.encoder.named_parameters()):
        assert torch.equal(p, q), n
        sa, sb = a.optimizer.state.get(p, {}), b.optimizer.state.get(q, {})
        assert set(sa) == set(sb), n
        for key in sa:
            assert torch.equal(sa[key], sb[key]), (n, key)
        trained += bool(sa)
    return trained


def _trainer_runs(make, ck):
    """two straight runs of four iterations and one interrupted after two: equal bits in every parameter and optimizer state"""
    straight = make(5, 'straight')
    straight.train(max_iterations=4)
    again = make(5, 'again')
    again.train(max_iterations=4)
    first = make(5, 'first')
    first.train(max_iterations=2)
    first.save_checkpoint(ck)
    second = make(99, 'second')                    # other weights: everything must come from the checkpoint
    second.load_checkpoint(ck)
    second.train(max_iterations=2)
    assert again.iteration == second.iteration == straight.iteration == 4
    assert second.encoder.dropout_state() == straight.encoder.dropout_state() == again.encoder.dropout_state()
    _same_run(again, straight)
    return straight, _same_run(second, straight)


def test_rank_trainer_with_the_tables_trained_is_bitwise_reproducible(tmp_path, tmp_path_factory):
    from aspire_amd import HipBertTrainEncoder, RankTrainer
    import readout_inputs as ri
    batches = tg._batches(str(tmp_path_factory.getbasetemp()))
    hparams = ri.hparams('l2wasserstein', 0.0)

    def make(seed, tag):
        enc = HipBertTrainEncoder(tg._bert(seed, dropout=0.1), dropout=True, seed=SEED, hip_embeddings=True)
        return RankTrainer(enc, hparams, tg._train_hparams(), str(tmp_path / tag), lambda epoch: batches)

    start = {n: p.detach().clone() for n, p in make(5, 'start').encoder.bert.named_parameters()}
    straight, trained = _trainer_runs(make, tmp_path / 'ck.pt')
    assert trained >= 19            # the layer's sixteen tensors and the three tables (the embedding LayerNorm too)
    params = dict(straight.encoder.bert.named_parameters())
    for n in TABLES:
        assert params[n] in straight.optimizer.state and int(straight.optimizer.state[params[n]]['step']) == 4, n
        assert not torch.equal(params[n].detach(), start[n]), n       # the tables did train


def test_bienc_trainer_with_the_tables_trained_is_bitwise_reproducible(tmp_path, tmp_path_factory):
    from aspire_amd import BiEncTrain, ClsTripletLoss, RankTrainer
    batches = tg._batches(str(tmp_path_factory.getbasetemp()))

    def make(seed, tag):
        model = BiEncTrain(tg._bert(seed, dropout=0.1), {'fine_tune': True}, dropout=True, seed=SEED, hip_embeddings=True)
        assert model.bert_encoder.hip_embeddings
        return RankTrainer(model, {}, tg._train_hparams(), str(tmp_path / tag), lambda epoch: batches,
                           loss_fn=ClsTripletLoss().forward_rank)

    straight, trained = _trainer_runs(make, tmp_path / 'ck.pt')
    assert trained >= 20
    params = dict(straight.encoder.named_parameters())
    assert all(params['bert_encoder.bert.' + n] in straight.optimizer.state for n in TABLES)
