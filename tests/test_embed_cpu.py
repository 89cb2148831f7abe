"""CPU: the embedding entry points' argument checks (no device is touched), the workspace size, and tests/embed_ref.py against torch's
CPU autograd of the BertEmbeddings sum.  (Constructing HipBertTrainEncoder needs a GPU: its keyword is tested in
tests/test_gpu_embed_train.py.)"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_ref as er  # noqa: E402

VOCAB, MAX_POS, N_TYPES = 301, 160, 2
P = 4096        # a fake, 16-byte aligned device address: no check may follow it


def _fwd(word=P, pos=P, typ_tab=P, tok=P, typ=P, b=2, l=5, vocab=VOCAB, max_pos=MAX_POS, n_types=N_TYPES, out=P):
    from aspire_amd import _lib
    return _lib.lib.aspire_bert_embed_sum_f32(word, pos, typ_tab, tok, typ, b, l, vocab, max_pos, n_types, out, None)


def _bwd(grad=P, tok=P, typ=P, b=2, l=5, vocab=VOCAB, max_pos=MAX_POS, n_types=N_TYPES, pad=0, gw=P, gp=P, gt=P, ws=P, ws_bytes=None):
    from aspire_amd import _lib
    if ws_bytes is None:
        ws_bytes = _lib.lib.aspire_bert_embed_workspace_bytes(b * l, vocab)
    return _lib.lib.aspire_bert_embed_backward_f32(grad, tok, typ, b, l, vocab, max_pos, n_types, pad, gw, gp, gt, ws, ws_bytes, None)


def test_argument_errors_need_no_device():
    from aspire_amd import _lib
    bad, err = _lib.ASPIRE_ERR_INVALID_ARG, lambda: _lib.lib.aspire_last_error().decode()
    for name in ('word', 'pos', 'typ_tab', 'tok', 'out'):
        assert _fwd(**{name: None}) == bad and 'null' in err(), name
    assert _bwd(grad=None) == bad and 'grad_emb_sum' in err()
    assert _bwd(grad=None, gw=None, gp=None) == bad and 'grad_emb_sum' in err()        # one wanted table is enough
    assert _bwd(tok=None) == bad and 'tok' in err()
    for call in (_fwd, _bwd):
        for l in (0, -3, MAX_POS + 1):
            assert call(l=l) == bad and f'L = {l}' in err(), l
        assert call(l=MAX_POS, b=0) == _lib.ASPIRE_OK                                    # L == max_pos is inside
        for name in ('vocab', 'max_pos', 'n_types'):
            for v in (0, -7):
                assert call(**{name: v}) == bad and f'{name} = {v}' in err(), (name, v)
        assert call(b=-2) == bad and 'B = -2' in err()
    for pad in (-2, VOCAB, VOCAB + 5):
        assert _bwd(pad=pad) == bad and f'padding_idx = {pad}' in err()
    assert _bwd(ws=None) == bad and 'workspace' in err()
    need = _lib.lib.aspire_bert_embed_workspace_bytes(10, VOCAB)
    assert _bwd(ws_bytes=need - 1) == bad and str(need) in err() and str(need - 1) in err()
    assert _bwd(ws=P + 4) == bad and 'aligned' in err()
    assert _fwd(out=P + 4) == bad and 'aligned' in err()
    assert _bwd(gp=P + 8) == bad and 'aligned' in err()
    # the rank pass's limit is stated, not silently passed
    assert _bwd(b=257, l=256, max_pos=256, ws_bytes=1 << 30) == _lib.ASPIRE_ERR_UNSUPPORTED and '65792' in err()
    # nothing to do: no launch, no device
    assert _fwd(b=0) == _lib.ASPIRE_OK
    assert _bwd(b=0) == _lib.ASPIRE_OK
    assert _bwd(gw=None, gp=None, gt=None) == _lib.ASPIRE_OK
    assert _bwd(gw=None, gp=None, gt=None, grad=None, tok=None, ws=None, ws_bytes=0) == _lib.ASPIRE_OK
    assert _bwd(gw=None, ws=None, ws_bytes=0, b=0) == _lib.ASPIRE_OK                     # no word table: no workspace is asked for


def test_signatures_and_operator_names():
    from aspire_amd import _lib
    import aspire_amd.torch_ops as to
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert _lib.SIGNATURES['aspire_bert_embed_sum_f32'] == (ctypes.c_int, [vp] * 5 + [i64] * 5 + [vp, vp])
    assert _lib.SIGNATURES['aspire_bert_embed_backward_f32'] == (ctypes.c_int, [vp] * 3 + [i64] * 6 + [vp] * 4 + [ctypes.c_size_t, vp])
    assert _lib.SIGNATURES['aspire_bert_embed_workspace_bytes'] == (ctypes.c_size_t, [i64, i64])
    for name in ('bert_embed_sum', 'bert_embed_backward'):
        assert name in to.OPS and hasattr(torch.ops.aspire, name) and f'torch.ops.aspire.{name}(' in to.__doc__
    assert len(set(to.OPS)) == len(to.OPS)


def test_workspace_bytes():
    from aspire_amd import _lib
    sizes = [_lib.lib.aspire_bert_embed_workspace_bytes(m, 30522) for m in list(range(0, 300)) + [1536, 2560, 16384, 65536]]
    assert all(s % 16 == 0 and s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[299] > sizes[1] and sizes[-1] > sizes[-2] > sizes[-3]
    assert _lib.lib.aspire_bert_embed_workspace_bytes(-4, 30522) == 16


def _case(b, l, seed, pad_share=0.3):
    rng = np.random.default_rng(seed)
    tok = rng.integers(1, VOCAB, size=(b, l))
    tok[rng.random((b, l)) < pad_share] = 0
    tok[0, 0], tok[-1, -1] = VOCAB - 1, 0
    typ = rng.integers(0, N_TYPES, size=(b, l))
    tables = [rng.standard_normal((n, er.D)).astype(np.float32) for n in (VOCAB, MAX_POS, N_TYPES)]
    return tok, typ, tables, er.order_grads(b, l, seed + 1)


def _torch_grads(tables, tok, typ, grad, dtype, pad):
    word, pos, typ_tab = (torch.tensor(t, dtype=dtype, requires_grad=True) for t in tables)
    t, y = torch.from_numpy(tok), torch.from_numpy(typ)
    out = (torch.nn.functional.embedding(t, word, padding_idx=pad) + torch.nn.functional.embedding(y, typ_tab)) + pos[:tok.shape[1]]
    out.backward(torch.tensor(grad, dtype=dtype))
    return out.detach().numpy(), [x.grad.numpy() for x in (word, pos, typ_tab)]


def test_reference_equals_torch_cpu_autograd_and_a_python_loop():
    """np.add.at is sequential in index order: the fp32 word and position gradients equal torch's CPU autograd and a Python loop bit for
    bit, with the padding row zero; the forward equals torch's expression"""
    for (b, l), pad in (((2, 130), 0), ((3, 64), None), ((1, 1), 0)):
        tok, typ, tables, grad = _case(b, l, 11 * b + l)
        out, (tw, tp, tt) = _torch_grads(tables, tok, typ, grad, torch.float32, pad)
        assert np.array_equal(er.forward(*tables, tok, typ), out)
        gw, gp, gt = er.backward(grad, tok, typ, VOCAB, MAX_POS, N_TYPES, pad=-1 if pad is None else pad)
        assert np.array_equal(gw, tw) and np.array_equal(gp, tp)
        assert not gw[0].any() if pad == 0 else gw[0].any()
        assert not gp[l:].any() and gp[l - 1].any()
        loop = np.zeros_like(gw)
        for m, v in enumerate(tok.reshape(-1)):
            if v != pad:
                loop[v] = loop[v] + grad.reshape(-1, er.D)[m]
        assert np.array_equal(gw, loop)
        # the order matters with these rows: float64 rounded to fp32 is another result
        g64 = er.backward(grad, tok, typ, VOCAB, MAX_POS, N_TYPES, pad=-1 if pad is None else pad, dtype=np.float64)
        assert b * l == 1 or not np.array_equal(g64[2].astype(np.float32), gt)
        # the type table's two stages are another order than torch's, inside the bound below; with one block per row they are torch's
        if b * l <= er.TYPE_PARTS:
            assert np.array_equal(gt, tt)


def test_reference_fp32_lies_inside_the_bound_against_float64():
    for (b, l), pad in (((2, 130), 0), ((3, 64), -1)):
        tok, typ, tables, grad = _case(b, l, 7 * b + l)
        got = er.backward(grad, tok, typ, VOCAB, MAX_POS, N_TYPES, pad=pad)
        want = er.backward(grad, tok, typ, VOCAB, MAX_POS, N_TYPES, pad=pad, dtype=np.float64)
        _, t32 = _torch_grads(tables, tok, typ, grad, torch.float32, None if pad < 0 else pad)
        _, t64 = _torch_grads(tables, tok, typ, grad, torch.float64, None if pad < 0 else pad)
        for name, g, w, a, c in zip(('word', 'pos', 'type'), got, want, t32, t64):
            assert np.array_equal(w, c) or name == 'type', name         # float64: the same sequential sums
            tol = er.bound(np.abs(a.astype(np.float64) - c).max(), np.abs(w).max())
            err = float(np.abs(g.astype(np.float64) - w).max())
            print(f'{b} x {l} grad_{name}: |fp32 - float64| {err:.3e}  bound {tol:.3e}')
            assert err <= tol, name
