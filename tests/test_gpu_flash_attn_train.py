"""GPU: the bare kernels of the training encoder's fused attention (aspire_amd/csrc/enc_attn_train.hip) through
aspire_debug_flash_attn_train_f32 / aspire_debug_flash_attn_train_backward_f32.

1. Arithmetic.  Yardstick: attention in float64 over the same fp32 qkv -- softmax(Q K^T / 8 + (1 - mask) finfo(float32).min) V per head,
   loss = (ctx * G).sum() -- for ctx, the row statistics (m = the row maximum in log2 units, l = the row sum of exp2(s - m)) and dqkv.
   Bound per tensor: trainside_inputs.bound(ref_err, max|x|) = max(4 ref_err, 4 * 2^-23 max|x|), ref_err the deviation from float64 of
   the bf16 mode's arithmetic emulated on the CPU in fp32 (tests/bf16_matmul_ref.py's products: both operands of Q K^T, P V and the four
   backward products rounded to bf16).  At L = 1 alone, dQ and dK are held to four times the error of tests/flash_attn_ref.py instead,
   the fused arithmetic itself emulated in fp32: with one key they are exact zeros in the three-kernel emulation -- bound 0 -- while
   the fused backward's row term D = rowsum(bf16(dctx) . ctx) leaves a residue of the fp32 sums' order (flash_attn_ref.py's
   docstring); both ratios are printed there.  B = 3 at every L in {1, 5, 37, 64, 65, 128, 130, 257, 512}: two documents with
   bf16_matmul_ref._mask's patterns (or, where it has none, a full document and one with a hole and right padding) and one whose mask
   is all zero; its rows must have m == -FLT_MAX and l == L exactly.  One case with logits of about +-100 at L = 300 whose row maximum
   moves across the 64-key tiles (keys grow with their index).
2. The dropout mask, read out of the kernels exactly: Q = K = 0 makes P uniform, V one-hot per 64-key window makes ctx[i, h, d] != 0
   exactly where key 64 w + d of query i is kept; dctx one-hot per 64-query window makes dV[j, h, d] != 0 exactly where key j of query
   64 w + d is kept.  Against aspire_bert_dropout_mask_u8 over [B, H, L, L], bit for bit.  And by value: ctx and dqkv under p = 0.1
   against float64 attention under the same mask at L = 64 and 130, which holds the dQ and dK kernels' masks too.

Largest |kernel - float64| / bound per tensor on an MI355X (every comparison prints its figures before it asserts):

    tensor   error       bound       ratio  case
    ctx      5.214e-03   1.649e-02   0.32   3 x 512
    m        5.481e-03   2.193e-02   0.25   3 x 1
    l        1.369e-02   5.477e-02   0.25   3 x 5
    dQ       1.036e-02   4.144e-02   0.25   3 x 5
    dK       1.225e-02   4.899e-02   0.25   3 x 5
    dV       7.452e-03   2.981e-02   0.25   3 x 1
    dQ, dK at 3 x 1: 3.4e-07 against the fused emulation's bounds 2.3e-06 / 1.8e-06 (ratio 0.15 / 0.19); the three-kernel emulation's
    bound there is 0 (ratio infinite).
    under dropout 0.1: ctx 0.29, dQ 0.27, dK 0.19, dV 0.25 at 3 x 64; ctx 0.14, dQ 0.25, dK 0.24, dV 0.25 at 3 x 130
    logits -110.7 .. 111.6 at 2 x 300: every tensor 0.25

A ratio of 0.25 is the emulation's own error: the bound is four times it.
"""
import contextlib
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import bf16_matmul_ref as br  # noqa: E402
import flash_attn_ref as fr  # noqa: E402
from trainside_inputs import bound  # noqa: E402

pytestmark = pytest.mark.gpu
H, DH, D = 12, 64, 768
LOG2E = 1.4426950408889634
FLT_MAX = float(torch.finfo(torch.float32).max)
LENGTHS = (1, 5, 37, 64, 65, 128, 130, 257, 512)
SEED, STEP = 0x9E3779B97F4A7C15, 3


# ---- the entries ------------------------------------------------------------------------------------------------------------------------
def _drop(p, seed=SEED, step=STEP):
    from aspire_amd import _lib
    return _lib.BertDropout(0.0, p, seed, step) if p else None


def flash_forward(qkv, mask, drop=None, fill=float('nan')):
    from aspire_amd import _lib, ops
    b, l = mask.shape
    ctx = torch.full((b, l, D), fill, device='cuda')
    stats = torch.full((b, H, l, 2), fill, device='cuda')
    _lib.check(_lib.lib.aspire_debug_flash_attn_train_f32(ops._ptr(qkv), ops._ptr(mask), b, l, ctypes.byref(drop) if drop is not None else None,
                                                          ops._ptr(ctx), ops._ptr(stats), ops._stream()))
    return ctx, stats


def flash_backward(qkv, mask, ctx, stats, dctx, drop=None, layer=0):
    from aspire_amd import _lib, ops
    b, l = mask.shape
    dqkv = torch.full((b, l, 3 * D), float('nan'), device='cuda')
    scratch = torch.full((b, H, l), float('nan'), device='cuda')             # D: the entry's scratch, the caller's
    _lib.check(_lib.lib.aspire_debug_flash_attn_train_backward_f32(ops._ptr(qkv), ops._ptr(mask), ops._ptr(ctx), ops._ptr(stats), ops._ptr(dctx),
                                                                   b, l, ctypes.byref(drop) if drop is not None else None, layer,
                                                                   ops._ptr(scratch), ops._ptr(dqkv), ops._stream()))
    assert torch.isfinite(scratch).all()
    return dqkv


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
def _masks(l):
    if l in (5, 130):
        two = br._mask(2, l)
    elif l == 37:
        two = br._mask(3, 37)[:2]
    else:
        two = torch.ones(2, l, dtype=torch.int64)
        if l > 2:
            two[1, l // 2] = 0
            two[1, l - l // 4:] = 0
    return torch.cat([two, torch.zeros(1, l, dtype=torch.int64)], 0)


def _reference(qkv, mask, G, dtype, emulate, keep=None, scale=1.0):
    """-> ctx [B, L, 768], m, l [B, H, L], dqkv [B, L, 2304] in dtype; emulate: bf16_matmul_ref's products; keep [B, H, L, L] and
    scale: the probabilities' dropout, as HuggingFace applies it between the soft-max and the product with V"""
    x = qkv.to(dtype).clone().requires_grad_(True)
    b, l = mask.shape
    q, k, v = (x[..., i * D:(i + 1) * D].reshape(b, l, H, DH).transpose(1, 2) for i in range(3))
    with (br.bf16_matmul() if emulate else contextlib.nullcontext()):
        s = torch.matmul(q, k.transpose(-1, -2)) / 8 + ((1 - mask)[:, None, None, :].to(dtype) * torch.finfo(torch.float32).min)
        p = torch.softmax(s, -1)
        if keep is not None:
            p = p * (keep.to(dtype) * scale)
        ctx = torch.matmul(p, v).transpose(1, 2).reshape(b, l, D)
    (ctx * G.to(dtype)).sum().backward()
    sd = s.detach()
    m = sd.max(-1).values
    lsum = torch.exp(sd - m[..., None]).sum(-1)
    return ctx.detach(), m * LOG2E, lsum, x.grad


@functools.lru_cache(maxsize=None)
def _case(l, heavy=False):
    g = torch.Generator().manual_seed(4000 + l + (7 if heavy else 0))
    if heavy:
        b = 2
        mask = torch.ones(b, l, dtype=torch.int64)
        mask[1, :3] = 0
        mask[1, 200:230] = 0
        qkv = torch.randn(b, l, 3 * D, generator=g)
        # q . k / 8 has deviation s^2 at scale s; keys grow with their index, so the row maximum tends to sit in a later tile
        ramp = (1.0 + 0.5 * torch.arange(l) / l)[None, :, None]
        qkv[..., :D] *= 4.0
        qkv[..., D:2 * D] *= 4.0 * ramp
    else:
        mask = _masks(l)
        b = mask.shape[0]
        qkv = torch.randn(b, l, 3 * D, generator=g)
    G = torch.randn(b, l, D, generator=g)
    exact = _reference(qkv, mask, G, torch.float64, False)
    emu32 = _reference(qkv, mask, G, torch.float32, True)
    return qkv, mask, G, exact, emu32, fr.attention(qkv, mask, G)


def _compare(tag, name, got, want, emu, worst, flash=None):
    """flash: the fused arithmetic's own emulation; given, ITS error makes the bound and the three-kernel emulation's ratio is printed"""
    scale = float(want.abs().max()) if want.numel() else 0.0
    tol = bound(float((emu.double() - want).abs().max()) if want.numel() else 0.0, scale)
    err = float((got.double().cpu() - want).abs().max()) if want.numel() else 0.0
    line = f'[{tag}] {name:6s} |kernel - float64| {err:.3e}  bound {tol:.3e}  ratio {err / tol if tol else float("inf") if err else 0.0:.2f}'
    if flash is not None:
        tol = bound(float((flash.double() - want).abs().max()), scale)
        line += f'  (three-kernel emulation);  bound {tol:.3e}  ratio {err / tol if tol else 0.0:.2f}  (fused emulation: asserted)'
    print(line)
    worst.append((name, err, tol))
    return err <= tol


def _check(tag, qkv, mask, G, exact, emu32, flash=None, drop=None):
    """flash: the fused emulation's tensors where dQ and dK are held to ITS error (L = 1 alone); else every tensor is held to the
    three-kernel emulation's"""
    ctx, stats = flash_forward(qkv.cuda(), mask.cuda(), drop)
    dqkv = flash_backward(qkv.cuda(), mask.cuda(), ctx, stats, G.cuda(), drop)
    assert torch.isfinite(ctx).all() and torch.isfinite(stats).all() and torch.isfinite(dqkv).all()        # every element written
    real = mask.sum(1) > 0                         # documents with a real key; the others: m = -FLT_MAX, l = L exactly
    m, lsum = stats[..., 0].cpu(), stats[..., 1].cpu()
    if (~real).any():
        assert bool((m[~real] == -FLT_MAX).all()) and bool((lsum[~real] == float(mask.shape[1])).all())
    worst, ok = [], True
    ok &= _compare(tag, 'ctx', ctx, exact[0], emu32[0], worst)
    ok &= _compare(tag, 'm', m[real], exact[1][real], emu32[1][real], worst)
    ok &= _compare(tag, 'l', lsum[real], exact[2][real], emu32[2][real], worst)
    for i, name in enumerate(('dQ', 'dK', 'dV')):
        sl = slice(i * D, (i + 1) * D)
        ok &= _compare(tag, name, dqkv[..., sl], exact[3][..., sl], emu32[3][..., sl], worst,
                       flash[3][..., sl] if flash is not None and name != 'dV' else None)
    assert ok, [w for w in worst if not w[1] <= w[2]]


@pytest.mark.parametrize('l', LENGTHS)
def test_forward_and_backward_against_float64(l):
    qkv, mask, G, exact, emu32, flash = _case(l)
    # with one key dQ and dK are exact zeros in the three-kernel emulation (bound 0): there, and only there, the fused emulation's error
    _check(f'3 x {l}', qkv, mask, G, exact, emu32, flash if l == 1 else None)


def test_large_logits_whose_maximum_moves_across_key_tiles():
    qkv, mask, G, exact, emu32, flash = _case(300, True)
    # from the reference alone: the logits reach about +-100 and the row maximum often lies behind the first 64-key tile
    b, l = mask.shape
    q, k = (qkv[..., i * D:(i + 1) * D].reshape(b, l, H, DH).transpose(1, 2).double() for i in range(2))
    s = torch.matmul(q, k.transpose(-1, -2)) / 8
    late = float((s[0].argmax(-1) >= 64).double().mean())
    print(f'logits {float(s.min()):.1f} .. {float(s.max()):.1f}; the maximum lies behind key 63 for {late:.3f} of document 0\'s rows')
    assert float(s.abs().max()) > 80 and late > 0.5
    _check('heavy 2 x 300', qkv, mask, G, exact, emu32)


def test_two_runs_give_the_same_bits():
    qkv, mask, G = _case(130)[:3]
    a = flash_forward(qkv.cuda(), mask.cuda(), _drop(0.1))
    b = flash_forward(qkv.cuda(), mask.cuda(), _drop(0.1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    da = flash_backward(qkv.cuda(), mask.cuda(), *a, G.cuda(), _drop(0.1))
    db = flash_backward(qkv.cuda(), mask.cuda(), *b, G.cuda(), _drop(0.1))
    assert torch.equal(da, db) and torch.isfinite(da).all()
    # the statistics are of the UNdropped probabilities: the same with and without dropout
    plain = flash_forward(qkv.cuda(), mask.cuda())
    assert torch.equal(plain[1], a[1]) and not torch.equal(plain[0], a[0])


# ---- 2. the dropout mask ----------------------------------------------------------------------------------------------------------------
def _keep(p, site, b, l):
    import aspire_amd.torch_ops  # noqa: F401
    return torch.ops.aspire.bert_dropout_mask(SEED - 2 ** 64, STEP, site, p, 0, b * H * l * l).reshape(b, H, l, l).bool()


@pytest.mark.parametrize('l', [64, 130])
def test_forward_and_backward_under_dropout_against_float64_under_the_same_mask(l):
    """every kernel's use of the mask by value -- the forward, dV, and the dK and dQ kernels, whose keep . scale multiplies dP: float64
    attention under the library's own mask of the site (L = 64: one Philox block per four keys where the lane is a query; 130: every
    element keyed on its own index), bound over the three-kernel emulation under the same mask"""
    import dropout_ref as dr
    qkv, mask, G = _case(l)[:3]
    p = 0.1
    keep = _keep(p, 1, mask.shape[0], l).cpu()
    exact = _reference(qkv, mask, G, torch.float64, False, keep, dr.scale(p))
    emu32 = _reference(qkv, mask, G, torch.float32, True, keep, dr.scale(p))
    _check(f'dropout 3 x {l}', qkv, mask, G, exact, emu32, drop=_drop(p))


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('l', [37, 64, 130])
def test_dropout_mask_read_out_of_the_forward(l, p):
    b = 2
    keep = _keep(p, 1, b, l)
    mask = torch.ones(b, l, dtype=torch.int64, device='cuda')
    for w in range((l + 63) // 64):
        qkv = torch.zeros(b, l, 3, H, DH, device='cuda')
        n = min(64, l - 64 * w)
        j = torch.arange(n, device='cuda')
        qkv[:, 64 * w + j, 2, :, j] = 1.0                     # V row j one-hot at column j - 64 w, in every head
        ctx, stats = flash_forward(qkv.reshape(b, l, 3 * D), mask, _drop(p))
        got = ctx.reshape(b, l, H, DH).permute(0, 2, 1, 3)[..., :n] != 0          # [b, h, query, key of the window]
        assert torch.equal(got, keep[..., 64 * w:64 * w + n]), (l, p, w)
        assert bool((ctx.reshape(b, l, H, DH)[..., n:] == 0).all())
        assert bool((stats[..., 1] == float(l)).all()) and bool((stats[..., 0] == 0).all())
    frac = float(keep.float().mean())
    assert abs(frac - (1 - p)) < 0.02, frac


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('l', [37, 64, 130])
def test_dropout_mask_read_out_of_the_backward(l, p):
    b, layer = 2, 1
    keep = _keep(p, 1 + 3 * layer, b, l)
    mask = torch.ones(b, l, dtype=torch.int64, device='cuda')
    qkv = torch.zeros(b, l, 3, H, DH, device='cuda')
    qkv[:, :, 2, :, 0] = 1.0                                   # V zero except one column
    qkv = qkv.reshape(b, l, 3 * D)
    ctx, stats = flash_forward(qkv, mask)
    for w in range((l + 63) // 64):
        n = min(64, l - 64 * w)
        i = torch.arange(n, device='cuda')
        dctx = torch.zeros(b, l, H, DH, device='cuda')
        dctx[:, 64 * w + i, :, i] = 1.0                        # query i's gradient one-hot at column i - 64 w
        dqkv = flash_backward(qkv, mask, ctx, stats, dctx.reshape(b, l, D), _drop(p), layer)
        dv = dqkv[..., 2 * D:].reshape(b, l, H, DH).permute(0, 2, 3, 1)[:, :, :n, :] != 0       # [b, h, query of the window, key]
        assert torch.equal(dv, keep[:, :, 64 * w:64 * w + n, :]), (l, p, w)
        assert torch.isfinite(dqkv).all()
