"""GPU: the bf16 matrix product of the training encoder's matmul mode (enc_gemm_bf16.hip) through aspire_debug_gemm_bf16_f32, in its
three operand forms (NT, B_KN, TN) and its three tiles.

  exact     integer operands in [-8, 8] (bf16-exact), K <= 512: every partial sum is an integer below 2^24, so the result equals the
            float64 product bit for bit in any summation order -- K in {1, 5, 16, 37, 130, 512} x M in {1, 4, 65, 132} x N in
            {4, 64, 100, 260} (every M in every form: the TN form takes any M as well), by the launch rule and with the tile pinned; one
            batched case with the attention's strides, one with alpha, bias and residual.  Operands lie in buffers whose leading
            dimensions are padded, the padding NaN: a value read from outside an operand's extent would show.  C lies in a buffer of
            a sentinel: nothing outside [M, N] is written.  Every launch's instantiation is read back (GEMM_BF16_LAST): all nine are
            reached, by pin and by shape.
  rounding  A . I = r(A) bit for bit against A.to(torch.bfloat16).float(), edge values (ties both ways, +-0, just under / over bf16's
            largest finite, +-inf) embedded in random data, the operand once in the A and once in the B position of each form.  A row
            that holds a non-finite r(A) is compared at that element alone (inf . 0 makes the rest of the row NaN on any arithmetic),
            and a zero by value: no sum that starts from the accumulator's +0 returns -0.
            Subnormals: printed, not asserted.
  random    |C - r(A) r(B)^T in float64| <= K 2^-24 (|r(A)| |r(B)|^T) elementwise, the bound of a length-K fp32 sum of exact products
            (derived, not measured); at K = 16 it rules out truncation in place of rounding.
  twice     the same bits from two calls."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
NT, BKN, TN = 0, 1, 2
FORMS = {'NT': NT, 'B_KN': BKN, 'TN': TN}
SENTINEL = -12345.0
KS, MS, NS = (1, 5, 16, 37, 130, 512), (1, 4, 65, 132), (4, 64, 100, 260)


def _last():
    from aspire_amd import _lib
    buf = ctypes.create_string_buffer(32)
    _lib.check(_lib.lib.aspire_debug_get(b'GEMM_BF16_LAST', buf, len(buf)))
    return int(buf.value)


def _pad4(n, extra=4):
    return (n + 3) // 4 * 4 + extra


def _store(x, ld):
    """x [..., r, c] -> a NaN-padded buffer [..., r, ld] on the GPU and its view of x"""
    buf = torch.full(x.shape[:-1] + (ld,), float('nan'), dtype=torch.float32)
    buf[..., :x.shape[-1]] = x
    return buf.cuda()


def product(A, B, form, alpha=1.0, bias=None, res=None, gelu=0):
    """C [M, N] = alpha A B^T (+ bias) (+ residual) for A [M, K], B [N, K] (fp32 CPU tensors), the operands laid out as `form` takes them
    -> (C on the CPU, the instantiation launched)"""
    from aspire_amd import _lib, ops
    M, K = A.shape
    N = B.shape[0]
    a = _store(A.t().contiguous() if form == TN else A, _pad4(M if form == TN else K))
    b = _store(B if form == NT else B.t().contiguous(), _pad4(K if form == NT else N))
    ldc = N + 3
    c = torch.full((M + 1, ldc), SENTINEL, device='cuda')
    bias_d = None if bias is None else bias.cuda()
    res_d = None if res is None else _store(res, N + 5)
    _lib.check(_lib.lib.aspire_debug_gemm_bf16_f32(ops._ptr(a), ops._ptr(b), ops._ptr(c), M, N, K, a.shape[-1], b.shape[-1], ldc, form, 1, 1,
                                                   0, 0, 0, 0, 0, 0, alpha, ops._ptr(bias_d), ops._ptr(res_d), N + 5 if res is not None else 0,
                                                   gelu, ops._stream()))
    out = c.cpu()
    assert bool((out[M] == SENTINEL).all()) and bool((out[:, N:] == SENTINEL).all()), 'written outside C [M, N]'
    return out[:M, :N].clone(), _last()


@functools.lru_cache(maxsize=None)
def _ints(rows, K, seed):
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + K)
    return torch.randint(-8, 9, (rows, K), generator=g).float()


@pytest.mark.parametrize('pin', ['', '128', '64'])
@pytest.mark.parametrize('form', list(FORMS))
def test_integer_products_are_exact(form, pin):
    from aspire_amd import _lib
    f = FORMS[form]
    ks = KS if pin == '' else (5, 130)                 # every K by the launch rule; with a pinned tile the K tail and two k tiles
    want_tile = {'': 2, '128': 0, '64': 1}[pin]      # (by the rule these shapes are a handful of workgroups: 64 x 64)
    with _lib.pinned(GEMM_TILE=pin):
        for K in ks:
            for M in MS:
                A = _ints(M, K, 1)
                for N in NS:
                    B = _ints(N, K, 2)
                    got, inst = product(A, B, f)
                    assert inst == 3 * f + want_tile, (M, N, K, inst)
                    assert torch.equal(got, (A.double() @ B.double().t()).float()), (form, pin, M, N, K)


def _batched(form, batch_docs, heads, L, dh, alpha=1.0):
    """the attention's own layout: operands inside a [docs L, 2304] projection, a head every 64 columns; C [docs, heads, L, Lp] (NT:
    Q K^T), or [docs L, 768] (B_KN: P V; TN: P^T dctx) -> (got, want in float64, instantiation)"""
    from aspire_amd import _lib, ops
    g = torch.Generator().manual_seed(11 + form)
    rows = batch_docs * L
    qkv = torch.randint(-8, 9, (rows, 2304), generator=g).float()
    Lp = (L + 3) // 4 * 4
    P = torch.randint(-8, 9, (batch_docs, heads, L, Lp), generator=g).float()
    P[..., L:] = float('nan')                             # pad columns: never an operand
    q4 = qkv.view(batch_docs, L, 3, 12, 64)
    if form == NT:           # scores = Q K^T
        want = torch.einsum('blhd,bmhd->bhlm', q4[:, :, 0, :heads].double(), q4[:, :, 1, :heads].double())
        c = torch.full((batch_docs, heads, L, Lp), SENTINEL, device='cuda')
        a, b = qkv.cuda(), qkv.cuda()[:, 768:]
        args = (L, L, dh, 2304, 2304, Lp)
        strides = (L * 2304, dh, L * 2304, dh, heads * L * Lp, L * Lp)
    else:
        x = q4[:, :, 2, :heads].double()                  # V (B_KN) or dctx (TN): [docs, L, heads, 64]
        Pv = P[..., :L].double()
        want = torch.einsum('bhlm,bmhd->blhd', Pv, x) if form == BKN else torch.einsum('bhml,bmhd->blhd', Pv, x)
        c = torch.full((batch_docs, L, 768), SENTINEL, device='cuda')
        a, b = P.cuda(), qkv.cuda()[:, 1536:]
        args = (L, dh, L, Lp, 2304, 768)
        strides = (heads * L * Lp, L * Lp, L * 2304, dh, L * 768, dh)
    _lib.check(_lib.lib.aspire_debug_gemm_bf16_f32(ops._ptr(a), ops._ptr(b), ops._ptr(c), *args, form, batch_docs * heads, heads, *strides,
                                                   alpha, None, None, 0, 0, ops._stream()))
    inst = _last()
    out = c.cpu()
    if form == NT:
        assert bool((out[..., L:] == SENTINEL).all())
        return out[..., :L], want * alpha, inst
    out = out.view(batch_docs, L, 12, 64)
    assert bool((out[:, :, heads:] == SENTINEL).all())
    return out[:, :, :heads], want * alpha, inst


@pytest.mark.parametrize('form', list(FORMS))
def test_batched_with_the_attentions_strides(form):
    """two documents, lda = ldb = 2304, a head every 64 columns; L = 37: the k-major forms contract over 37 rows of a 40-wide P"""
    got, want, inst = _batched(FORMS[form], 2, 12, 37, 64)
    assert inst == 3 * FORMS[form] + 2
    assert torch.equal(got, want.float())


@pytest.mark.parametrize('form', list(FORMS))
def test_the_launch_rule_reaches_the_large_tiles_by_shape(form):
    """without a pin: 128 x 128 from 256 workgroups on (N >= 128), else 128 x 64 from 256 on -- many small matrices in one launch"""
    f = FORMS[form]
    # NT scores [130, 130] per head: 2 x 2 tiles of 128 x 128, x 72 matrices = 288; the others' C is [130, 64]: 2 x 1 tiles of 128 x 64, x 132 = 264
    docs, heads = (6, 12) if f == NT else (11, 12)
    got, want, inst = _batched(f, docs, heads, 130, 64, alpha=0.125)
    assert inst == 3 * f + (0 if f == NT else 1), inst
    assert torch.equal(got, want.float())                # (alpha = 2^-3: still exact)


@pytest.mark.parametrize('form', list(FORMS))
def test_alpha_bias_and_residual(form):
    g = torch.Generator().manual_seed(5)
    M, N, K = 65, 100, 37
    A, B = _ints(M, K, 3), _ints(N, K, 4)
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    res = torch.randint(-8, 9, (M, N), generator=g).float()
    got, _ = product(A, B, FORMS[form], alpha=0.125, bias=bias, res=res)
    assert torch.equal(got, (0.125 * (A.double() @ B.double().t()) + bias.double() + res.double()).float())
    # the GELU epilogue sits between the bias and the residual, on the fp32 value
    got, _ = product(A, B, FORMS[form], alpha=0.125, bias=bias, res=res, gelu=1)
    z = 0.125 * (A.double() @ B.double().t()) + bias.double()
    want = torch.nn.functional.gelu(z) + res.double()
    assert float((got.double() - want).abs().max()) <= 1e-5


def _f(bits):
    return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)


EDGES = _f([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,       # ties: to the even neighbour below / above, both signs
            0x3F808001, 0x3F807FFF,                               # just over / under a tie
            0x00000000, 0x80000000,                               # +-0
            0x7F7F0000, 0x7F7F7FFF, 0xFF7F7FFF,                   # bf16's largest finite, and just under the tie above it
            0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0xFF7FFFFF,       # over it: inf
            0x7F800000, 0xFF800000])                              # +-inf
SUBNORMALS = _f([0x00000001, 0x00400000, 0x007FFFFF, 0x80400000, 0x00008000, 0x00010000])


def _edge_matrix(rows, cols, seed, extra=None):
    """random data with one edge value per row (so that a non-finite one spoils its own row alone), at a column that moves"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-6, 7, (rows, cols), generator=g).float())
    vals = EDGES if extra is None else extra
    where = []
    for i, v in enumerate(vals):
        r, c = (5 * i + 1) % rows, (7 * i + 3) % cols
        X[r, c] = v
        where.append((r, c))
    assert len({r for r, _ in where}) == len(where)
    return X, where


@pytest.mark.parametrize('position', ['A', 'B'])
@pytest.mark.parametrize('form', list(FORMS))
def test_operands_are_rounded_as_torch_rounds(form, position):
    f = FORMS[form]
    rows, K = 132, 100                                     # the edge matrix [rows, K] times the identity [K, K]
    X, where = _edge_matrix(rows, K, 21)
    eye = torch.eye(K)
    got, _ = product(X, eye, f) if position == 'A' else product(eye, X, f)
    got = got if position == 'A' else got.t()
    want = X.to(torch.bfloat16).float()
    finite_rows = torch.isfinite(want).all(1)
    assert int((~finite_rows).sum()) == 6                  # the four that round past the largest finite and the two infinities
    # bit for bit -- but for the sign of a zero, which no sum that starts from the accumulator's +0 can carry (-0 + +0 = +0): r(A) = +-0
    # must come back as a zero
    gf, wf = got[finite_rows], want[finite_rows]
    assert torch.equal(gf.view(torch.int32)[wf != 0], wf.view(torch.int32)[wf != 0]), (form, position)
    assert bool((gf[wf == 0] == 0).all())
    for r, c in where:
        same = got[r, c].view(torch.int32) == want[r, c].view(torch.int32) or (want[r, c] == 0 and got[r, c] == 0)
        assert same, (form, position, r, c, float(X[r, c]), float(got[r, c]))
    # subnormals: what the matrix pipe does with them is reported, not asserted
    S, swhere = _edge_matrix(rows, K, 22, extra=SUBNORMALS)
    sgot, _ = product(S, eye, f) if position == 'A' else product(eye, S, f)
    sgot = sgot if position == 'A' else sgot.t()
    for (r, c), v in zip(swhere, SUBNORMALS):
        print(f'[{form} {position}] subnormal {float(v):.6e} -> {float(sgot[r, c]):.6e} (torch bf16: {float(v.to(torch.bfloat16).float()):.6e})')


@pytest.mark.parametrize('K', [16, 37, 512])
@pytest.mark.parametrize('form', list(FORMS))
def test_random_operands_within_the_fp32_sum_bound(form, K):
    g = torch.Generator().manual_seed(31 + K)
    M, N = 132, 100
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    got, _ = product(A, B, FORMS[form])
    rA, rB = A.to(torch.bfloat16).double(), B.to(torch.bfloat16).double()
    want = rA @ rB.t()
    tol = K * 2.0 ** -24 * (rA.abs() @ rB.abs().t())
    err = (got.double() - want).abs()
    print(f'[{form} K={K}] largest |C - r(A) r(B)^T| / bound: {float((err / tol).max()):.3f}')
    assert bool((err <= tol).all())
    if K == 16:     # truncated operands would miss by ~2^-9 |a||b| per term: far outside
        tA = (A.view(torch.int32) & -65536).view(torch.float32).double()
        assert not bool(((tA @ rB.t() - want).abs() <= tol).all())
    # the same bits from a second call
    again, _ = product(A, B, FORMS[form])
    assert torch.equal(got, again)


def test_every_instantiation_was_reached():
    """the nine (form, tile) instantiations, each by a launch of this test: pinned tiles and the 64 x 64 tile by the rule"""
    from aspire_amd import _lib
    seen = set()
    A, B = _ints(65, 37, 1), _ints(100, 37, 2)
    for f in FORMS.values():
        for pin in ('', '128', '64'):
            with _lib.pinned(GEMM_TILE=pin):
                got, inst = product(A, B, f)
            assert torch.equal(got, (A.double() @ B.double().t()).float())
            seen.add(inst)
    assert seen == set(range(9)), seen
