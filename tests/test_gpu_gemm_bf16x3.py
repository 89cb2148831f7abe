"""GPU: the k-major bf16x3 matrix product of the training encoder's matmul mode 'bf16x3' (enc_gemm_bf16x3.hip) through
aspire_debug_gemm_bf16x3_f32, in its two forms (B_KN, TN) and its three tiles.

  identity  A . I = A and I . B = B bit for bit: random fp32 operands that use all 24 mantissa bits, mixed signs, exponents over
            thirteen binades within a row.  x3 + x2 + x1 is x exactly in fp32, so a dropped or mis-turned plane, or a wrong k map in
            one plane, changes bits.  The operand once in the A and once in the B position of each form (B_KN: B the [K, N] identity;
            TN: A [K, M] against the [K, N] identity gives A^T), by the launch rule and with each tile pinned.
  exact     integer operands: entries in [-255, 255] (one plane) for K in {1, 5, 16, 33, 100, 130}, entries in [-1023, 1023] (two
            planes) for K <= 16, M and N in {1, 5, 33, 64, 65, 130, 260}: the sum over k of (|a1| + |a2| + |a3|) (|b1| + |b2| + |b3|)
            is asserted below 2^24, so every partial sum in any order is an exact integer and the result equals the int64 product.
            By the launch rule and with each tile pinned.  Operands lie in buffers whose leading dimensions are padded, the padding
            NaN: a value read from outside an operand's extent would show.  C lies in a buffer of a sentinel with ldc > N: nothing
            outside [M, N] is written.
  rows      TN over many rows, M = N = 64, K in {255, 256, 257, 600, 5599} (the accumulators fold every 256 k; the last k tile is
            partial), and B_KN at K in {16, 37, 512}: random normal operands, |C - float64| <= trainside_inputs.bound(ref_err, max|C|)
            with ref_err the error of torch's CPU fp32 matmul on the same operands.  The same bits from a second launch.
  strides   the attention's layout: nz2 = heads, lda = Lp of the probabilities, ldb = 2304 with a head every 64 columns, per-document
            and per-head offsets, L in {5, 130}, integer operands: exact against the per-matrix float64 product.
  epilogue  alpha, bias, residual with ldr > N (exact on integers), GELU against the same fp32 formula.
  coverage  every launch's instantiation is read back (GEMM_BF16X3_LAST): all six are reached, by pin and by shape.

Largest |C - float64| on an MI355X against the bound (printed by the tests before they assert):

    form  M x N      K      error       bound       ref_err (torch's CPU fp32 matmul)
    TN    64 x 64    255    9.973e-06   7.541e-05   1.885e-05
    TN    64 x 64    256    1.125e-05   6.793e-05   1.698e-05
    TN    64 x 64    257    1.228e-05   7.918e-05   1.979e-05
    TN    64 x 64    600    1.320e-05   1.569e-04   3.923e-05
    TN    64 x 64    5599   5.180e-05   3.252e-04   8.130e-05
    B_KN  132 x 100  16     1.093e-06   9.512e-06   2.378e-06
    B_KN  132 x 100  37     2.141e-06   3.186e-05   7.965e-06
    B_KN  132 x 100  512    3.093e-05   1.301e-04   3.252e-05

(|C - the six-term product in float64| is the same figure to two digits in every row: the error is the fp32 sums', not the dropped
terms'.  With all six terms in ONE accumulator, the kernel's first form, the same rows read 2.6e-05 .. 7.3e-05 for TN and 7.5e-05 at
B_KN K = 512; the correction terms' own accumulator brought them below the CPU's.  GELU epilogue: 5.917e-07 in every form and tile.)
"""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import bf16x3_ref as x3  # noqa: E402
from trainside_inputs import bound  # noqa: E402

pytestmark = pytest.mark.gpu
BKN, TN = 1, 2
FORMS = {'B_KN': BKN, 'TN': TN}
PINS = {'': 2, '128': 0, '64': 1}        # ASPIRE_HIP_GEMM_TILE -> the tile it gives shapes of a handful of workgroups
SENTINEL = -12345.0
SIZES = (1, 5, 33, 64, 65, 130, 260)


def _last():
    from aspire_amd import _lib
    buf = ctypes.create_string_buffer(32)
    _lib.check(_lib.lib.aspire_debug_get(b'GEMM_BF16X3_LAST', buf, len(buf)))
    return int(buf.value)


def _pad4(n, extra=4):
    return (n + 3) // 4 * 4 + extra


def _store(x, ld):
    """x [..., r, c] -> a NaN-padded buffer [..., r, ld] on the GPU"""
    buf = torch.full(x.shape[:-1] + (ld,), float('nan'), dtype=torch.float32)
    buf[..., :x.shape[-1]] = x
    return buf.cuda()


def product(A, B, form, alpha=1.0, bias=None, res=None, gelu=0):
    """C [M, N] = alpha A B^T (+ bias) (+ GELU) (+ residual) for A [M, K], B [N, K] (fp32 CPU tensors), the operands laid out as `form`
    takes them -> (C on the CPU, the instantiation launched)"""
    from aspire_amd import _lib, ops
    M, K = A.shape
    N = B.shape[0]
    a = _store(A.t().contiguous() if form == TN else A, _pad4(M if form == TN else K))
    b = _store(B.t().contiguous(), _pad4(N))
    ldc = N + 3
    c = torch.full((M + 1, ldc), SENTINEL, device='cuda')
    bias_d = None if bias is None else bias.cuda()
    res_d = None if res is None else _store(res, N + 5)
    _lib.check(_lib.lib.aspire_debug_gemm_bf16x3_f32(ops._ptr(a), ops._ptr(b), ops._ptr(c), M, N, K, a.shape[-1], b.shape[-1], ldc, form, 1, 1,
                                                     0, 0, 0, 0, 0, 0, alpha, ops._ptr(bias_d), ops._ptr(res_d),
                                                     N + 5 if res is not None else 0, gelu, ops._stream()))
    out = c.cpu()
    assert bool((out[M] == SENTINEL).all()) and bool((out[:, N:] == SENTINEL).all()), 'written outside C [M, N]'
    return out[:M, :N].clone(), _last()


@functools.lru_cache(maxsize=None)
def _ints(rows, K, seed, top):
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + K + top)
    return torch.randint(-top, top + 1, (rows, K), generator=g).float()


@functools.lru_cache(maxsize=None)
def _full_mantissa(rows, cols, seed):
    """random fp32 values with all 24 mantissa bits in use, both signs, exponents over thirteen binades within every row; no zero"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-6, 7, (rows, cols), generator=g).float())
    X[X == 0] = 1.0
    assert int((X.view(torch.int32) & 0xFF).ne(0).sum()) > 0.9 * X.numel()         # the low mantissa byte is in use
    return X


@pytest.mark.parametrize('pin', list(PINS))
@pytest.mark.parametrize('position', ['A', 'B'])
@pytest.mark.parametrize('form', list(FORMS))
def test_identity_products_return_the_operand_bit_for_bit(form, position, pin):
    from aspire_amd import _lib
    f = FORMS[form]
    for rows, K in ((132, 100), (70, 37), (5, 16)):
        X = _full_mantissa(rows, K, 21 + rows)
        eye = torch.eye(K)
        with _lib.pinned(GEMM_TILE=pin):
            got, inst = product(X, eye, f) if position == 'A' else product(eye, X, f)
        got = got if position == 'A' else got.t()
        assert inst == 3 * f + PINS[pin]
        same = got.view(torch.int32) == X.view(torch.int32)
        print(f'[{form} {position} pin {pin!r} {rows} x {K}] elements whose bits differ: {int((~same).sum())}')
        assert bool(same.all()), (form, position, pin, rows, K)


@pytest.mark.parametrize('pin', list(PINS))
@pytest.mark.parametrize('form', list(FORMS))
def test_integer_products_are_exact(form, pin):
    from aspire_amd import _lib
    f = FORMS[form]
    # one plane: every K by the launch rule, with a pinned tile the K tail and several k tiles; two planes: K <= 16
    grids = [(255, (1, 5, 16, 33, 100, 130) if pin == '' else (5, 130)), (1023, (1, 5, 16) if pin == '' else (5, 16))]
    launches = 0
    with _lib.pinned(GEMM_TILE=pin):
        for top, ks in grids:
            for K in ks:
                for M in SIZES:
                    A = _ints(M, K, 1, top)
                    for N in SIZES:
                        B = _ints(N, K, 2, top)
                        assert float(x3.abs_product(A, B).max()) < 2 ** 24         # every partial sum is an exact integer
                        got, inst = product(A, B, f)
                        launches += 1
                        assert inst == 3 * f + PINS[pin], (M, N, K, inst)
                        want = (A.long() @ B.long().t())
                        assert torch.equal(got.long(), want) and torch.equal(got, want.float()), (form, pin, top, M, N, K)
    print(f'[{form} pin {pin!r}] {launches} products equal to the int64 product')


def _against_float64(form, M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    got, inst = product(A, B, FORMS[form])
    want = A.double() @ B.double().t()
    ref_err = float(((A @ B.t()).double() - want).abs().max())
    tol = bound(ref_err, float(want.abs().max()))
    err = float((got.double() - want).abs().max())
    print(f'[{form} {M} x {N} over {K}] |C - float64| {err:.3e}  bound {tol:.3e}  ref_err {ref_err:.3e}  max|C| {float(want.abs().max()):.3e}  '
          f'|C - six-term float64| {float((got.double() - x3.product(A, B)).abs().max()):.3e}')
    again, _ = product(A, B, FORMS[form])
    assert torch.equal(got, again)                         # the same bits from a second launch
    assert err <= tol
    return inst


@pytest.mark.parametrize('K', [255, 256, 257, 600, 5599])
def test_tn_over_many_rows(K):
    assert _against_float64('TN', 64, 64, K, 40 + K) == 3 * TN + 2


@pytest.mark.parametrize('K', [16, 37, 512])
def test_bkn_random_operands(K):
    assert _against_float64('B_KN', 132, 100, K, 31 + K) == 3 * BKN + 2


def _batched(form, docs, heads, L, alpha=1.0):
    """the attention's own layout: P [docs, heads, L, Lp] (pad columns NaN) against V or dctx inside a [docs L, 2304] projection, a head
    every 64 columns; C [docs L, 768] (B_KN: P V; TN: P^T dctx) -> (got, want in float64, instantiation)"""
    from aspire_amd import _lib, ops
    dh = 64
    g = torch.Generator().manual_seed(11 + form + L)
    qkv = torch.randint(-255, 256, (docs * L, 2304), generator=g).float()
    Lp = (L + 3) // 4 * 4
    P = torch.randint(-255, 256, (docs, heads, L, Lp), generator=g).float()
    P[..., L:] = float('nan')                             # pad columns: never an operand
    x = qkv.view(docs, L, 3, 12, 64)[:, :, 2, :heads].double()                     # [docs, L, heads, 64]
    Pv = P[..., :L].double()
    want = torch.einsum('bhlm,bmhd->blhd', Pv, x) if form == BKN else torch.einsum('bhml,bmhd->blhd', Pv, x)
    c = torch.full((docs, L, 768), SENTINEL, device='cuda')
    a, b = P.cuda(), qkv.cuda()[:, 1536:]
    _lib.check(_lib.lib.aspire_debug_gemm_bf16x3_f32(ops._ptr(a), ops._ptr(b), ops._ptr(c), L, dh, L, Lp, 2304, 768, form, docs * heads, heads,
                                                     heads * L * Lp, L * Lp, L * 2304, dh, L * 768, dh, alpha, None, None, 0, 0,
                                                     ops._stream()))
    inst = _last()
    out = c.cpu().view(docs, L, 12, 64)
    assert bool((out[:, :, heads:] == SENTINEL).all())
    return out[:, :, :heads], want * alpha, inst


@pytest.mark.parametrize('L', [5, 130])
@pytest.mark.parametrize('form', list(FORMS))
def test_batched_with_the_attentions_strides(form, L):
    """two documents, eleven of the twelve heads (the twelfth's columns stay the sentinel); L = 5: one partial float4 per k-slice, Lp = 8;
    L = 130: two row tiles and nine k tiles"""
    got, want, inst = _batched(FORMS[form], 2, 11, L)
    assert inst == 3 * FORMS[form] + 2
    assert float(want.abs().max()) < 2 ** 24 and torch.equal(got, want.float())


@pytest.mark.parametrize('form', list(FORMS))
def test_the_launch_rule_reaches_the_large_tiles_by_shape(form):
    """without a pin: 128 x 64 from 256 workgroups on -- C [130, 64] per head is 2 x 1 such tiles, x 132 matrices = 264; 128 x 128 from
    256 on with N >= 128 -- 64 matrices of [130, 130], 2 x 2 tiles each"""
    from aspire_amd import _lib, ops
    f = FORMS[form]
    got, want, inst = _batched(f, 11, 12, 130, alpha=0.125)
    assert inst == 3 * f + 1, inst
    assert torch.equal(got, want.float())                # (alpha = 2^-3: still exact)
    n, S, K = 64, 130, 20
    g = torch.Generator().manual_seed(17)
    A, B = torch.randint(-255, 256, (n, S, K), generator=g).float(), torch.randint(-255, 256, (n, S, K), generator=g).float()
    a = _store(A.transpose(1, 2).contiguous() if f == TN else A, _pad4(S if f == TN else K))
    b = _store(B.transpose(1, 2).contiguous(), _pad4(S))
    c = torch.full((n, S + 1, S + 3), SENTINEL, device='cuda')
    _lib.check(_lib.lib.aspire_debug_gemm_bf16x3_f32(ops._ptr(a), ops._ptr(b), ops._ptr(c), S, S, K, a.shape[-1], b.shape[-1], S + 3, f, n, 1,
                                                     a.shape[1] * a.shape[2], 0, b.shape[1] * b.shape[2], 0, (S + 1) * (S + 3), 0, 1.0, None,
                                                     None, 0, 0, ops._stream()))
    assert _last() == 3 * f + 0
    out = c.cpu()
    assert bool((out[:, S] == SENTINEL).all()) and bool((out[:, :, S:] == SENTINEL).all())
    assert torch.equal(out[:, :S, :S], torch.bmm(A.double(), B.double().transpose(1, 2)).float())


@pytest.mark.parametrize('pin', list(PINS))
@pytest.mark.parametrize('form', list(FORMS))
def test_alpha_bias_gelu_and_residual(form, pin):
    from aspire_amd import _lib
    g = torch.Generator().manual_seed(5)
    M, N, K = 65, 100, 37
    A, B = _ints(M, K, 3, 8), _ints(N, K, 4, 8)
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    res = torch.randint(-8, 9, (M, N), generator=g).float()
    with _lib.pinned(GEMM_TILE=pin):
        got, _ = product(A, B, FORMS[form], alpha=0.125, bias=bias, res=res)
        gelu, _ = product(A, B, FORMS[form], alpha=0.125, bias=bias, res=res, gelu=1)
    assert torch.equal(got, (0.125 * (A.double() @ B.double().t()) + bias.double() + res.double()).float())
    # the GELU epilogue sits between the bias and the residual, on the fp32 value
    z = 0.125 * (A.double() @ B.double().t()) + bias.double()
    want = torch.nn.functional.gelu(z) + res.double()
    err = float((gelu.double() - want).abs().max())
    print(f'[{form} pin {pin!r}] GELU epilogue |C - float64| {err:.3e}')
    assert err <= 1e-5


def test_every_instantiation_was_reached():
    """the six (form, tile) instantiations, each by a launch of this test: pinned tiles and the 64 x 64 tile by the rule"""
    from aspire_amd import _lib
    seen = set()
    A, B = _ints(65, 37, 1, 255), _ints(100, 37, 2, 255)
    for f in FORMS.values():
        for pin in PINS:
            with _lib.pinned(GEMM_TILE=pin):
                got, inst = product(A, B, f)
            assert torch.equal(got, (A.double() @ B.double().t()).float())
            seen.add(inst)
    assert seen == set(range(3, 9)), seen
