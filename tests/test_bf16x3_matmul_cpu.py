"""CPU: the bf16x3 matmul mode without a device -- the mode's arithmetic emulated with torch.bfloat16's rounding (tests/bf16x3_ref.py),
the new entries' argument checks, the keyword and the checkpoint rule (nothing here touches a GPU).

The split: x1 + x2 + x3 == x bit for bit for every normal fp32 value whose third plane is not below bf16's range (ties both ways, +-0,
the largest magnitudes that still round to a finite bf16, random values over 60 binades).  The six-term product deviates from the
float64 product by the three dropped terms a2 b3 + a3 b2 + a3 b3: |a2| <= 2^-8 |a| and |a3| <= 2^-16 |a| (bf16 keeps 8 significant
bits and each plane rounds what the one before left), so by at most (2 * 2^-24 + 2^-32) |a| |b| -- inside the 3 * 2^-24 |a| |b| that
is asserted, and far below the 2^-8 |a| |b| of one bf16 rounding.  The largest deviation / (|a| |b|) over 2^20 random pairs, printed
by the test: 4.819e-08 = 0.81 * 2^-24."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_matmul_ref as br  # noqa: E402
import bf16x3_ref as x3  # noqa: E402
from test_bf16_matmul_cpu import _weights  # noqa: E402


def _f(bits):
    return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)


def _random(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 31, (n,), generator=g).float())


def test_the_split_adds_up_bit_for_bit():
    edges = _f([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,       # ties of the first plane: to the even neighbour below / above
                0x3F808001, 0x3F807FFF, 0x3F800001, 0x3FFFFFFF,       # just over / under a tie; 1 + 2^-23; all mantissa bits set
                0x3F808080, 0x3F80807F, 0x3F808081,                   # a tie of the second plane and its neighbours
                0x00000000, 0x80000000,                               # +-0
                0x7F7F0000, 0x7F7F7FFF, 0xFF7F7FFF,                   # bf16's largest finite, and just under the tie above it
                0x4B7FFFFF, 0xCB7FFFFF, 0x0C7FFFFF])                  # 2^24 - 1; a small number whose third plane bf16 still holds
    for x in (edges, _random(1 << 16, 1)):
        p1, p2, p3 = x3.split3(x)
        for p in (p1, p2, p3):      # every plane is a bf16 value
            assert torch.equal(p, p.to(torch.bfloat16).float())
        total = (p1.double() + p2.double() + p3.double())
        assert torch.equal(total, x.double())
        assert torch.equal(((p3 + p2) + p1).view(torch.int32)[x != 0], x.view(torch.int32)[x != 0])       # and in fp32, the kernels' order
        assert bool((p2.abs() <= 2.0 ** -8 * p1.abs()).all()) and bool((p3.abs() <= 2.0 ** -8 * p2.abs()).all())
    # a magnitude that rounds past bf16's largest finite, and an infinity, have a NaN plane (the header says so)
    for bits in (0x7F7F8000, 0x7F800000, 0xFF800000):
        assert any(bool(torch.isnan(p).any()) for p in x3.split3(_f([bits])))


def test_the_six_terms_are_within_three_roundings_of_the_exact_product():
    a, b = _random(1 << 20, 2), _random(1 << 20, 3)
    exact = a.double() * b.double()
    dev = (x3.six_terms(a, b) - exact).abs()
    scale = a.double().abs() * b.double().abs()
    print(f'largest |six terms - a b| / (|a| |b|): {float((dev / scale).max()):.3e}  (3 * 2^-24 = {3 * 2.0 ** -24:.3e}, the derived '
          f'2^-23 + 2^-32 = {2.0 ** -23 + 2.0 ** -32:.3e})')
    assert bool((dev <= 3 * 2.0 ** -24 * scale).all())
    # one plane alone (the bf16 mode) is far outside: the emulation tells the modes apart
    one = a.to(torch.bfloat16).double() * b.to(torch.bfloat16).double()
    assert float(((one - exact).abs() / scale).max()) > 2.0 ** -10
    # as a matrix product: integers that need two planes are exact
    g = torch.Generator().manual_seed(4)
    A, B = torch.randint(-1023, 1024, (7, 16), generator=g).float(), torch.randint(-1023, 1024, (5, 16), generator=g).float()
    assert torch.equal(x3.product(A, B), A.double() @ B.double().t())
    assert float(x3.abs_product(A, B).max()) < 2 ** 24


def test_prec_entries_accept_the_mode_without_a_device():
    """mode 3 passes the mode check -- the entries then fail on the next bad argument, as modes 0 and 1 do; 2, -1 and 7 stay refused"""
    from aspire_amd import _lib
    lib = _lib.lib
    bw, keep = _weights()
    B, L = 2, 5
    tape_bytes = lib.aspire_bert_tape_bytes(ctypes.byref(bw), B, L)
    ws_bytes = lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), B, L)

    def fwd(matmul, emb=16, tape=16, nbytes=tape_bytes):
        return lib.aspire_bert_layers_forward_train_prec_f32(ctypes.byref(bw), emb, 16, B, L, 16, tape, nbytes, 16, ws_bytes, None, matmul, None)

    for bad in (2, -1, 7):
        assert fwd(bad) == _lib.ASPIRE_ERR_INVALID_ARG
        err = lib.aspire_last_error()
        assert str(bad).encode() in err and b'matmul mode' in err and b'BF16X3' in err
    assert fwd(3, emb=None) == _lib.ASPIRE_ERR_INVALID_ARG and b'matmul mode' not in lib.aspire_last_error()
    assert fwd(3, tape=None) == _lib.ASPIRE_ERR_INVALID_ARG
    assert fwd(3, nbytes=tape_bytes - 1) == _lib.ASPIRE_ERR_INVALID_ARG
    assert b'tape too small' in lib.aspire_last_error()

    glayers = (_lib.BertLayerGrads * 1)()
    for f, _ in _lib.BertLayerGrads._fields_:
        setattr(glayers[0], f, ctypes.c_void_p(16))
    bg = _lib.BertGrads(ctypes.c_void_p(16), ctypes.c_void_p(16), glayers)

    def bwd(matmul, grad_hidden=16, mask=16, nbytes=tape_bytes, grad_mix=None):
        return lib.aspire_bert_layers_backward_prec_f32(ctypes.byref(bw), mask, B, L, grad_hidden, None, None, None, 16, nbytes, 16,
                                                        ctypes.byref(bg), grad_mix, 16, ws_bytes, None, matmul, None)

    for bad in (2, -1, 7):
        assert bwd(bad) == _lib.ASPIRE_ERR_INVALID_ARG
        assert str(bad).encode() in lib.aspire_last_error() and b'matmul mode' in lib.aspire_last_error()
    assert bwd(3, grad_hidden=None) == _lib.ASPIRE_ERR_INVALID_ARG and b'matmul mode' not in lib.aspire_last_error()
    assert bwd(3, mask=None) == _lib.ASPIRE_ERR_INVALID_ARG
    assert bwd(3, nbytes=tape_bytes - 1) == _lib.ASPIRE_ERR_INVALID_ARG
    assert bwd(3, grad_mix=16) == _lib.ASPIRE_ERR_INVALID_ARG
    assert _lib.lib.aspire_bert_tape_bytes(ctypes.byref(bw), B, L) == tape_bytes       # the size queries do not know the mode


def test_debug_gemm_checks_its_arguments_without_a_device():
    from aspire_amd import _lib
    lib = _lib.lib

    def gemm(A=16, B=16, C=16, M=4, N=4, K=4, lda=4, ldb=4, ldc=4, form=1, batch=1, nz2=1):
        return lib.aspire_debug_gemm_bf16x3_f32(A, B, C, M, N, K, lda, ldb, ldc, form, batch, nz2, 0, 0, 0, 0, 0, 0, 1.0, None, None, 0, 0, None)

    for kw in (dict(A=None), dict(B=None), dict(C=None), dict(M=-1), dict(N=-1), dict(K=-1), dict(batch=-1), dict(form=3), dict(form=-1),
               dict(nz2=0), dict(lda=2), dict(K=6, lda=6, ldb=6), dict(A=20), dict(form=2, M=8, lda=4), dict(form=0, K=6, lda=8, ldb=8)):
        assert gemm(**kw) == _lib.ASPIRE_ERR_INVALID_ARG, kw
    assert gemm(form=9) == _lib.ASPIRE_ERR_INVALID_ARG and b'9' in lib.aspire_last_error()
    for form in (0, 1, 2):
        for kw in (dict(M=0), dict(N=0), dict(K=0), dict(batch=0)):
            assert gemm(form=form, **kw) == _lib.ASPIRE_OK, (form, kw)              # a zero size: nothing to do, no launch
    buf = ctypes.create_string_buffer(32)
    assert lib.aspire_debug_get(b'GEMM_BF16X3_LAST', buf, len(buf)) == _lib.ASPIRE_OK
    assert int(buf.value) == -1 or 3 <= int(buf.value) < 9                         # the latest launch's instantiation: none here
    assert lib.aspire_debug_get(b'GEMM_BF16_LAST', buf, len(buf)) == _lib.ASPIRE_OK and -1 <= int(buf.value) < 9


def test_matmul_keyword_is_checked_at_construction(monkeypatch):
    from aspire_amd import BiEncTrain, HipBertTrainEncoder, IctEncTrain, SentEncTrain, ops
    monkeypatch.setattr(ops, 'require_gpu', lambda: torch.device('cpu'))            # construction alone: no kernel runs
    assert HipBertTrainEncoder.MATMUL_MODES == {'fp32': 0, 'bf16': 1, 'bf16x3': 3}
    assert HipBertTrainEncoder(br._bert(1), matmul='bf16x3').matmul == 'bf16x3'
    assert HipBertTrainEncoder(br._bert(1)).matmul == 'fp32'
    for bad in ('int8', 'bf16x2', 'BF16X3', None, 3):
        with pytest.raises(ValueError, match=r"matmul.*'fp32', 'bf16' or 'bf16x3'"):
            HipBertTrainEncoder(br._bert(1), matmul=bad)
    assert BiEncTrain(br._bert(1), matmul='bf16x3').bert_encoder.matmul == 'bf16x3'
    sent = SentEncTrain(br._bert(1), matmul='bf16x3')
    assert sent.matmul == sent.sent_encoder.matmul == 'bf16x3'
    ict = IctEncTrain(br._bert(1), br._bert(1), seed=1, matmul='bf16x3')
    assert ict.sent_encoder.matmul == ict.context_encoder.matmul == ict.matmul == 'bf16x3'
    for cls in (BiEncTrain, SentEncTrain):
        with pytest.raises(ValueError, match='matmul'):
            cls(br._bert(1), matmul='bf16x2')
    with pytest.raises(ValueError, match='matmul'):
        IctEncTrain(br._bert(1), br._bert(1), seed=1, matmul='bf16x2')


def test_checkpoint_carries_the_mode(tmp_path):
    """RankTrainer.load_checkpoint's rule on a bare state: a bf16x3 checkpoint is refused by an encoder of either other mode, and a
    bf16x3 encoder refuses theirs (and one written before the key existed, which reads as 'fp32'), each by name"""
    from aspire_amd import RankTrainer

    def trainer(mode):
        class Enc:
            matmul = mode

        tr = RankTrainer.__new__(RankTrainer)
        tr.encoder = Enc()
        return tr

    torch.save({'encoder': {}, 'matmul': 'bf16x3'}, tmp_path / 'x3.pt')
    for mine in ('fp32', 'bf16'):
        with pytest.raises(ValueError, match=f"'bf16x3'.*'{mine}'"):
            trainer(mine).load_checkpoint(tmp_path / 'x3.pt')
        torch.save({'encoder': {}, 'matmul': mine}, tmp_path / 'other.pt')
        with pytest.raises(ValueError, match=f"'{mine}'.*'bf16x3'"):
            trainer('bf16x3').load_checkpoint(tmp_path / 'other.pt')
    torch.save({'encoder': {}}, tmp_path / 'old.pt')
    with pytest.raises(ValueError, match="'fp32'.*'bf16x3'"):
        trainer('bf16x3').load_checkpoint(tmp_path / 'old.pt')
