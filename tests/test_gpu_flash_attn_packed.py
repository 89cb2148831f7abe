"""GPU: the bare kernels of the fused training attention over PACKED rows (aspire_amd/csrc/enc_attn_train.hip's PackedDocs
instantiations) through aspire_debug_flash_attn_train_packed_f32 / aspire_debug_flash_attn_train_packed_backward_f32.

Yardstick and bound are tests/test_gpu_flash_attn_train.py's, imported: its ``_reference`` (float64 attention over the PADDED qkv with
the mask, loss = (ctx * G).sum() with G zeroed on masked rows) and trainside_inputs.bound(ref_err, max|x|) with ref_err the deviation
from float64 of the bf16 mode's emulation in fp32.  Compared on valid rows: a masked key has probability 0 and a masked query no
gradient, so the padded reference's valid rows ARE the per-document values (tests/test_packed_rows_cpu.py pins that premise).  For a
document of ONE token dQ and dK are held to that file's flash_attn_ref rule instead (they are exact zeros in the three-kernel
emulation -- bound 0 -- while the fused backward's D = rowsum(bf16(dctx) . ctx) leaves a residue of the fp32 sums' order).

Document-length triples, padded to the longest: the smallest shapes at which a tile edge, an early exit or a row offset can go wrong --
(1, 0, 5), (64, 65, 63), (128, 130, 127), (257, 3, 512), and one triple at L = 130 with the left-padding and hole patterns of
bf16_matmul_ref._mask(3, 37) and _mask(2, 130).  Outputs and the scratch are pre-filled with NaN: every element of the packed ctx,
statistics, D and dqkv must come back finite.  The dropout mask is read out of the kernels bit for bit with that file's one-hot
construction, against aspire_bert_dropout_mask_u8 over the PADDED [B, H, L, L] gathered at the tokens' positions: at (64, 65, 63)
(a prefix, L % 4 != 0: every element keyed on its own index), at (257, 3, 512) (a prefix, L % 4 == 0: one draw per four keys) and at
the hole triple (positions from row_src).  For a prefix packing the test PRINTS whether the packed rows equal the padded kernels'
rows bit for bit; that is reported, not asserted.
"""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import bf16_matmul_ref as br  # noqa: E402
import dropout_ref as dr  # noqa: E402
import flash_attn_ref as fr  # noqa: E402
import test_gpu_flash_attn_train as tf  # noqa: E402
from trainside_inputs import bound  # noqa: E402

pytestmark = pytest.mark.gpu
H, DH, D = tf.H, tf.DH, tf.D


def _prefix_mask(lens):
    l = max(lens)
    return (torch.arange(l)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64)


def _hole_mask():
    m = torch.zeros(3, 130, dtype=torch.int64)
    m[0, :37] = br._mask(3, 37)[0]          # left padding and a hole, then right padding
    m[1] = br._mask(2, 130)[1]              # left padding, a hole across the 64-key edge, one pad token
    m[2, :37] = br._mask(3, 37)[1]          # right padding alone
    return m


TRIPLES = {'1-0-5': lambda: _prefix_mask([1, 0, 5]), '64-65-63': lambda: _prefix_mask([64, 65, 63]),
           '128-130-127': lambda: _prefix_mask([128, 130, 127]), '257-3-512': lambda: _prefix_mask([257, 3, 512]), 'holes': _hole_mask,
           '12-7-16': lambda: _prefix_mask([12, 7, 16])}


# ---- the entries ------------------------------------------------------------------------------------------------------------------------
def _packing(mask):
    from aspire_amd import _lib, packed_rows
    pr = packed_rows(mask.cuda())
    pk = _lib.BertPacking(pr.rows, pr.max_len, int(pr.prefix), *(ctypes.c_void_p(t.data_ptr()) for t in (pr.doc_start, pr.row_src, pr.row_dst)))
    return pr, pk


def packed_forward(qkv_p, mask, drop=None):
    from aspire_amd import _lib, ops
    pr, pk = _packing(mask)
    b, l = mask.shape
    ctx = torch.full((pr.rows, D), float('nan'), device='cuda')
    stats = torch.full((H, pr.rows, 2), float('nan'), device='cuda')
    _lib.check(_lib.lib.aspire_debug_flash_attn_train_packed_f32(ops._ptr(qkv_p), ctypes.byref(pk), b, l,
                                                                 ctypes.byref(drop) if drop is not None else None, ops._ptr(ctx),
                                                                 ops._ptr(stats), ops._stream()))
    return ctx, stats


def packed_backward(qkv_p, mask, ctx, stats, dctx_p, drop=None, layer=0):
    from aspire_amd import _lib, ops
    pr, pk = _packing(mask)
    b, l = mask.shape
    dqkv = torch.full((pr.rows, 3 * D), float('nan'), device='cuda')
    scratch = torch.full((H, pr.rows), float('nan'), device='cuda')
    _lib.check(_lib.lib.aspire_debug_flash_attn_train_packed_backward_f32(ops._ptr(qkv_p), ctypes.byref(pk), ops._ptr(ctx), ops._ptr(stats),
                                                                          ops._ptr(dctx_p), b, l,
                                                                          ctypes.byref(drop) if drop is not None else None, layer,
                                                                          ops._ptr(scratch), ops._ptr(dqkv), ops._stream()))
    assert torch.isfinite(scratch).all()
    return dqkv


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """-> qkv, mask, G (zero on masked rows), the float64 run, the fp32 emulation, the fused emulation; computed once, never written to"""
    mask = TRIPLES[name]()
    b, l = mask.shape
    g = torch.Generator().manual_seed(5000 + l + int(mask.sum()))
    qkv = torch.randn(b, l, 3 * D, generator=g)
    G = torch.randn(b, l, D, generator=g) * mask[..., None]
    return (qkv, mask, G, tf._reference(qkv, mask, G, torch.float64, False), tf._reference(qkv, mask, G, torch.float32, True),
            fr.attention(qkv, mask, G))


def _valid_stats(x, mask):
    """[B, H, L] -> [H, R] in packed order"""
    return x.permute(1, 0, 2)[:, mask.bool()]


def _inside(tag, name, got, want, emu):
    scale = float(want.abs().max()) if want.numel() else 0.0
    tol = bound(float((emu.double() - want).abs().max()) if want.numel() else 0.0, scale)
    err = float((got.double().cpu() - want).abs().max()) if want.numel() else 0.0
    print(f'[{tag}] {name:10s} |kernel - float64| {err:.3e}  bound {tol:.3e}  ratio {err / tol if tol else 0.0:.2f}')
    return err <= tol


def _check(tag, qkv, mask, G, exact, emu32, flash, drop=None):
    v = mask.bool()
    ctx, stats = packed_forward(qkv[v].cuda(), mask, drop)
    dqkv = packed_backward(qkv[v].cuda(), mask, ctx, stats, G[v].cuda(), drop)
    assert torch.isfinite(ctx).all() and torch.isfinite(stats).all() and torch.isfinite(dqkv).all()        # every element written
    ok = _inside(tag, 'ctx', ctx, exact[0][v], emu32[0][v])
    ok &= _inside(tag, 'm', stats[..., 0], _valid_stats(exact[1], mask), _valid_stats(emu32[1], mask))
    ok &= _inside(tag, 'l', stats[..., 1], _valid_stats(exact[2], mask), _valid_stats(emu32[2], mask))
    one = (mask.sum(1) == 1)[:, None].expand_as(mask)[v]         # packed rows of one-token documents
    for i, name in enumerate(('dQ', 'dK', 'dV')):
        sl = slice(i * D, (i + 1) * D)
        got, want, emu = dqkv[:, sl], exact[3][v][:, sl], emu32[3][v][:, sl]
        if name != 'dV' and bool(one.any()):
            # a document of one token: the fused emulation's error is the rule there (flash_attn_ref.py's docstring)
            ok &= _inside(tag, name + ' len 1', got[one.cuda()], want[one], flash[3][v][:, sl][one])
            got, want, emu = got[(~one).cuda()], want[~one], emu[~one]
        ok &= _inside(tag, name, got, want, emu)
    assert ok
    return ctx, stats, dqkv


@pytest.mark.parametrize('name', ['1-0-5', '64-65-63', '128-130-127', '257-3-512', 'holes'])
def test_forward_and_backward_against_float64_on_valid_rows(name):
    qkv, mask, G, exact, emu32, flash = _case(name)
    ctx, stats, dqkv = _check(name, qkv, mask, G, exact, emu32, flash)
    if name != 'holes':
        # a prefix packing walks the same tiles as the padded kernels: reported, not asserted
        pc, ps = tf.flash_forward(qkv.cuda(), mask.cuda())
        pd = tf.flash_backward(qkv.cuda(), mask.cuda(), pc, ps, G.cuda())
        v = mask.bool().cuda()
        print(f'[{name}] packed rows equal the padded kernels\' rows bit for bit: ctx {torch.equal(pc[v], ctx)}, '
              f'dqkv {torch.equal(pd[v], dqkv)}')


def test_two_runs_give_the_same_bits():
    qkv, mask, G = _case('holes')[:3]
    v = mask.bool()
    a = packed_forward(qkv[v].cuda(), mask, tf._drop(0.1))
    b = packed_forward(qkv[v].cuda(), mask, tf._drop(0.1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    da = packed_backward(qkv[v].cuda(), mask, *a, G[v].cuda(), tf._drop(0.1))
    db = packed_backward(qkv[v].cuda(), mask, *b, G[v].cuda(), tf._drop(0.1))
    assert torch.equal(da, db) and torch.isfinite(da).all()
    plain = packed_forward(qkv[v].cuda(), mask)
    assert torch.equal(plain[1], a[1]) and not torch.equal(plain[0], a[0])      # the statistics are of the UNdropped probabilities


# ---- the dropout mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['holes', '12-7-16'])
def test_under_dropout_against_float64_under_the_same_mask(name):
    """every kernel's use of the mask by value (the dQ and dK kernels' keep . scale multiplies dP): the library's own mask of the site
    over the padded [B, H, L, L]; 'holes': keyed through row_src; '12-7-16': a prefix with L % 4 == 0, one draw per four keys"""
    qkv, mask, G = _case(name)[:3]
    p = 0.1
    b, l = mask.shape
    keep = tf._keep(p, 1, b, l).cpu()
    exact = tf._reference(qkv, mask, G, torch.float64, False, keep, dr.scale(p))
    emu32 = tf._reference(qkv, mask, G, torch.float32, True, keep, dr.scale(p))
    _check(f'dropout {name}', qkv, mask, G, exact, emu32, None, drop=tf._drop(p))


def _positions(mask):
    return [mask[i].nonzero().squeeze(1).cuda() for i in range(mask.shape[0])]


@pytest.mark.parametrize('name', ['64-65-63', '257-3-512', 'holes'])
def test_dropout_mask_read_out_of_the_forward(name):
    mask = TRIPLES[name]()
    b, l = mask.shape
    p = 0.1
    keep = tf._keep(p, 1, b, l)
    pos = _positions(mask)
    start = [0]
    for q in pos:
        start.append(start[-1] + q.numel())
    rows = start[-1]
    for w in range((max(q.numel() for q in pos) + 63) // 64):
        qkv = torch.zeros(rows, 3, H, DH, device='cuda')
        for i, q in enumerate(pos):          # V of the document's key 64 w + d one-hot at column d, in every head
            n = min(64, q.numel() - 64 * w)
            if n > 0:
                j = torch.arange(n, device='cuda')
                qkv[start[i] + 64 * w + j, 2, :, j] = 1.0
        ctx, stats = packed_forward(qkv.reshape(rows, 3 * D), mask, tf._drop(p))
        for i, q in enumerate(pos):
            n = min(64, q.numel() - 64 * w)
            if n <= 0:
                continue
            got = ctx[start[i]:start[i + 1]].reshape(-1, H, DH).permute(1, 0, 2)[..., :n] != 0        # [h, query, key of the window]
            want = keep[i][:, q][:, :, q[64 * w:64 * w + n]]
            assert torch.equal(got, want), (name, w, i)
            assert bool((stats[:, start[i]:start[i + 1], 1] == float(q.numel())).all())


@pytest.mark.parametrize('name', ['64-65-63', '257-3-512', 'holes'])
def test_dropout_mask_read_out_of_the_backward(name):
    mask = TRIPLES[name]()
    b, l = mask.shape
    p, layer = 0.1, 1
    keep = tf._keep(p, 1 + 3 * layer, b, l)
    pos = _positions(mask)
    start = [0]
    for q in pos:
        start.append(start[-1] + q.numel())
    rows = start[-1]
    qkv = torch.zeros(rows, 3, H, DH, device='cuda')
    qkv[:, 2, :, 0] = 1.0                                      # V zero except one column
    qkv = qkv.reshape(rows, 3 * D)
    ctx, stats = packed_forward(qkv, mask)
    for w in range((max(q.numel() for q in pos) + 63) // 64):
        dctx = torch.zeros(rows, H, DH, device='cuda')
        for i, q in enumerate(pos):          # the gradient of the document's query 64 w + d one-hot at column d
            n = min(64, q.numel() - 64 * w)
            if n > 0:
                j = torch.arange(n, device='cuda')
                dctx[start[i] + 64 * w + j, :, j] = 1.0
        dqkv = packed_backward(qkv, mask, ctx, stats, dctx.reshape(rows, D), tf._drop(p), layer)
        assert torch.isfinite(dqkv).all()
        for i, q in enumerate(pos):
            n = min(64, q.numel() - 64 * w)
            if n <= 0:
                continue
            dv = dqkv[start[i]:start[i + 1], 2 * D:].reshape(-1, H, DH).permute(1, 2, 0)[:, :n, :] != 0       # [h, query of the window, key]
            want = keep[i][:, q[64 * w:64 * w + n]][:, :, q]
            assert torch.equal(dv, want), (name, w, i)
