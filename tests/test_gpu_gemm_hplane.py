"""GPU: the bare product of the inference encoder's fp16 matmul mode (aspire_amd/csrc/enc_gemm_h.hip: split_h_kernel, gemm_h_kernel)
through aspire_debug_split_hplane / aspire_debug_gemm_hplane.

Shapes (M, N, K): one row; a row tail inside one tile; exact tiles; three row tiles with a 64-wide column tail; the long contraction.
Every shape runs under the launcher's own tile choice and with both tile widths pinned (GEMM_TILE 128: 128-wide tiles + a 64-wide
tail where N % 128 == 64; 64: 64-wide tiles alone).

What is exact and why.  The split rounds once, so its output is X.half() (the weight side (64 X).half()) bit for bit.  Products of fp16
values are exact in fp32 and the accumulators are fp32, so integer operands in [-8, 8] (largest sum 3072 * 64 * 64 < 2^24, the weight's
factor 64 included) give the int64 product exactly, and with a bias and a residual that are multiples of 2^-6 every value of epilogue
(a) is an fp32 number: the float64 formula, rounded once, is met exactly.  Random operands: the fp32-sum bound of
tests/test_gpu_gemm_bf16.py, |C - float64 product of the rounded operands| <= K 2^-24 sum_k |a| |b|.  Epilogue (b) on operands whose
sums are exact (integers times a power of two): what remains is the fp32 fma with the bias (2^-24 relative on the pre-activation, far
below an fp16 ulp of the GELU for |x| <= 10), gelu_erf's own error (2.5e-7 absolute at O(1) values, relative 2e-6 in the tail) and the
one rounding to fp16 (half an ulp; 2^-25 among the subnormals): within one fp16 ulp, 2^-10 |want| + 2^-24.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp16_matmul_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64, 32), (37, 64, 32), (128, 128, 768), (300, 192, 768), (129, 768, 3072)]
TILES = [None, 128, 64]
GUARD = 8            # sentinel rows behind C's M rows
SENTINEL = -12345.0


def _split(x, weight, fill=None):
    """fp32 CPU [R, K] -> the H buffer (uint8 cuda tensor); fill: the byte every byte of the buffer holds before the split"""
    from aspire_amd import _lib, ops
    R, K = x.shape
    n = _lib.lib.aspire_debug_hplane_bytes(R, K)
    assert n == fr.h_bytes(R, K)
    buf = torch.zeros(n, dtype=torch.uint8, device='cuda') if fill is None else torch.full((n,), fill, dtype=torch.uint8, device='cuda')
    _lib.check(_lib.lib.aspire_debug_split_hplane(ops._ptr(x.cuda().contiguous()), R, K, ops._ptr(buf), int(weight), ops._stream()))
    return buf


def _gemm(ah, bh, M, N, K, bias=None, res=None, epilogue=0, tile=None):
    """-> epilogue 0: fp32 [M + GUARD, N] (the guard rows keep SENTINEL); 1: the H buffer of [M, N]"""
    from aspire_amd import _lib, ops
    c = ch = None
    if epilogue == 0:
        c = torch.full((M + GUARD, N), SENTINEL, device='cuda')
    else:
        ch = torch.zeros(_lib.lib.aspire_debug_hplane_bytes(M, N), dtype=torch.uint8, device='cuda')
    bias_d = bias.cuda() if bias is not None else None
    res_d = res.cuda().contiguous() if res is not None else None
    with _lib.pinned(**({'GEMM_TILE': tile} if tile else {})):
        _lib.check(_lib.lib.aspire_debug_gemm_hplane(ops._ptr(ah), ops._ptr(bh), ops._ptr(c), ops._ptr(ch), ops._ptr(bias_d), ops._ptr(res_d),
                                                     M, N, K, epilogue, ops._stream()))
    torch.cuda.synchronize()
    return c if epilogue == 0 else ch


@functools.lru_cache(maxsize=None)
def _ints(M, N, K):
    g = torch.Generator().manual_seed(1000 * M + N + K)
    return (torch.randint(-8, 9, (M, K), generator=g).float(), torch.randint(-8, 9, (N, K), generator=g).float())


@functools.lru_cache(maxsize=None)
def _randoms(M, N, K):
    g = torch.Generator().manual_seed(7 * M + 3 * N + K)
    a = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, K, generator=g))          # several binades per row
    b = 0.04 * torch.randn(N, K, generator=g)
    return a, b


@pytest.mark.parametrize('M,N,K', SHAPES)
def test_split_rounds_once(M, N, K):
    a, b = _randoms(M, N, K)
    got_a = fr.h_decode(_split(a, False), M, K)
    got_b = fr.h_decode(_split(b, True), N, K)
    assert np.array_equal(got_a.view(np.uint16), a.half().numpy().view(np.uint16))
    assert np.array_equal(got_b.view(np.uint16), (64.0 * b).half().numpy().view(np.uint16))


@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_integer_operands_are_exact(M, N, K, tile):
    a, b = _ints(M, N, K)
    c = _gemm(_split(a, False), _split(b, True), M, N, K, tile=tile).cpu()
    want = a.long() @ b.long().t()
    assert torch.equal(c[:M].double(), want.double())
    assert bool((c[M:] == SENTINEL).all())
    if M % 64 == 0:         # the other operand role: the same values as the weight, B's as the activation
        ct = _gemm(_split(b, False), _split(a, True), N, M, K, tile=tile).cpu()
        assert torch.equal(ct[:N].double(), want.t().double())


@pytest.mark.parametrize('tile', TILES)
def test_identity_returns_the_rounded_operand(tile):
    M, K = 300, 768
    a, _ = _randoms(M, 192, K)
    c = _gemm(_split(a, False), _split(torch.eye(K), True), M, K, K, tile=tile).cpu()
    assert torch.equal(c[:M].view(torch.int32), a.half().float().view(torch.int32))


@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_random_operands_within_the_fp32_sum_bound(M, N, K, tile):
    a, b = _randoms(M, N, K)
    c = _gemm(_split(a, False), _split(b, True), M, N, K, tile=tile).cpu()
    a16, b16 = a.half().double(), (64.0 * b).half().double() / 64.0
    want = a16 @ b16.t()
    bound = K * 2.0 ** -24 * (a16.abs() @ b16.abs().t())
    err = (c[:M].double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f'({M}, {N}, {K}) tile {tile}: max |C - float64| {float(err.max()):.3e}, largest error / bound {ratio:.3f}')
    assert bool((err <= bound).all()), ratio
    assert bool((c[M:] == SENTINEL).all())
    again = _gemm(_split(a, False), _split(b, True), M, N, K, tile=tile).cpu()          # determinism: the same bits
    assert torch.equal(again.view(torch.int32), c.view(torch.int32))


@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_bias_and_residual_exact(M, N, K, tile):
    a, b = _ints(M, N, K)
    g = torch.Generator().manual_seed(5)
    bias = torch.randint(-640, 641, (N,), generator=g).float() / 64.0                    # multiples of 2^-6: every value below is an fp32 number
    res = torch.randint(-6400, 6401, (M, N), generator=g).float() / 64.0
    ah, bh = _split(a, False), _split(b / 64.0, True)                                    # the weight int / 64: the product's values are k / 64
    want_b = (a.double() @ (b.double() / 64.0).t() + bias.double()).float()
    want_r = (a.double() @ (b.double() / 64.0).t() + bias.double() + res.double()).float()
    c = _gemm(ah, bh, M, N, K, bias=bias, tile=tile).cpu()
    assert torch.equal(c[:M].view(torch.int32), want_b.view(torch.int32))
    c = _gemm(ah, bh, M, N, K, bias=bias, res=res, tile=tile).cpu()
    assert torch.equal(c[:M].view(torch.int32), want_r.view(torch.int32))
    assert bool((c[M:] == SENTINEL).all())
    c = _gemm(ah, bh, M, N, K, res=res, tile=tile).cpu()                                 # a residual without a bias
    assert torch.equal(c[:M].double(), a.double() @ (b.double() / 64.0).t() + res.double())


@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_gelu_epilogue_writes_the_h_layout(M, N, K, tile):
    """epilogue (b): sums exact by construction (integers, the weight times a power of two that puts the pre-activations at O(1)), so the
    bound holds the bias fma, the GELU and the one rounding alone (module docstring)"""
    a, b = _ints(M, N, K)
    shift = 2.0 ** -max(1, round(np.log2(np.sqrt(K) * 24.0)))                            # sums have std sqrt(K) 24: -> about 1 (0.7 - 1.4)
    g = torch.Generator().manual_seed(6)
    bias = torch.randn(N, generator=g)
    ah, bh = _split(a, False), _split(b * shift, True)
    ch = _gemm(ah, bh, M, N, K, bias=bias, epilogue=1, tile=tile)
    got = torch.from_numpy(fr.h_decode(ch, M, N).astype(np.float64))
    x = a.double() @ (b.double() * shift).t() + bias.double()
    want = (0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))).half().double()
    assert float(x.abs().max()) < 16 and float(x.std()) > 0.5                            # inside the range gelu_erf is fitted and clamped for
    err = (got - want).abs()
    tol = 2.0 ** -10 * want.abs() + 2.0 ** -24
    print(f'({M}, {N}, {K}) tile {tile}: largest |got - want| / (one fp16 ulp) {float((err / tol).max()):.3f}')
    assert bool((err <= tol).all()), float((err / tol).max())
    again = _gemm(ah, bh, M, N, K, bias=bias, epilogue=1, tile=tile)
    assert torch.equal(again[:M * N * 2], ch[:M * N * 2])


@pytest.mark.parametrize('M,N,K', SHAPES)
def test_pad_rows_never_reach_the_output(M, N, K):
    """the whole H buffer of A 0xFF before the split: the pad rows (and everything a tail tile reads past M) are fp16 NaN"""
    a, b = _randoms(M, N, K)
    bh = _split(b, True)
    clean = _gemm(_split(a, False), bh, M, N, K).cpu()
    ah = _split(a, False, fill=0xFF)
    assert bool((ah[M * K * 2:] == 0xFF).all())
    c = _gemm(ah, bh, M, N, K).cpu()
    assert bool(torch.isfinite(c[:M]).all())
    assert torch.equal(c[:M].view(torch.int32), clean[:M].view(torch.int32))
    assert bool((c[M:] == SENTINEL).all())
    ch = _gemm(ah, bh, M, N, K, bias=torch.zeros(N), epilogue=1)
    ch0 = _gemm(_split(a, False), bh, M, N, K, bias=torch.zeros(N), epilogue=1)
    assert torch.equal(ch[:M * N * 2], ch0[:M * N * 2])
    assert bool((ch[M * N * 2:] == 0).all())                                             # nothing written behind the M rows
