"""CPU: the bf16 matmul mode without a device -- the rounding helper of tests/bf16_matmul_ref.py on edge values, the yardstick's own
soundness, and the new entries' argument checks (nothing here touches a GPU).

Soundness: on the cases of tests/test_gpu_encoder_backward.py the emulation accumulated in float64 lies inside
bound(ref_err, max|grad|) of the EXACT float64 model for `hidden` and every parameter, ref_err the fp32-accumulated emulation's
deviation from the exact model and bound tests/golden/trainside_inputs.bound: the bound the GPU test holds the kernels to leaves room
for another summation order of the same rounded products.  Largest error / bound over all tensors: 0.25 at 1 x (2, 5), 0.29 at
2 x (3, 37), 0.34 at 2 x (2, 130)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import bf16_matmul_ref as br  # noqa: E402
from trainside_inputs import bound  # noqa: E402


def _f(bits):
    return torch.tensor([bits - (1 << 32) if bits >= 1 << 31 else bits], dtype=torch.int32).view(torch.float32)


def _bits(x):
    return int(x.view(torch.int32)) & 0xFFFFFFFF


def test_rounding_helper_on_edge_values():
    cases = [
        (0x3F808000, 0x3F800000),       # 1 + 2^-8: a tie, the even neighbour is below
        (0x3F818000, 0x3F820000),       # 1 + 3 2^-8: a tie, the even neighbour is above
        (0x3F808001, 0x3F810000),       # just over a tie: up
        (0x3F807FFF, 0x3F800000),       # just under: down
        (0xBF808000, 0xBF800000),       # the ties with the sign set
        (0xBF818000, 0xBF820000),
        (0x00000000, 0x00000000),       # +0
        (0x80000000, 0x80000000),       # -0 keeps its sign
        (0x7F7F0000, 0x7F7F0000),       # bf16's largest finite is itself
        (0x7F7F7FFF, 0x7F7F0000),       # just under the tie above it: stays finite
        (0x7F7F8000, 0x7F800000),       # the tie rounds to even = past the largest finite: inf
        (0x7F7FFFFF, 0x7F800000),       # fp32's largest finite: inf
        (0xFF7FFFFF, 0xFF800000),
        (0x7F800000, 0x7F800000),       # inf
        (0xFF800000, 0xFF800000),
    ]
    for src, want in cases:
        got = br.round_bf16(_f(src))
        assert got.dtype == torch.float32 and _bits(got) == want, (hex(src), hex(_bits(got)), hex(want))
        assert _bits(br.round_bf16(_f(src).double()).float()) == want, hex(src)        # the same values from float64
    assert torch.isnan(br.round_bf16(torch.tensor([float('nan')])))
    # the patch is scoped
    lin, mm = torch.nn.functional.linear, torch.matmul
    with br.bf16_matmul():
        assert torch.matmul is br.matmul and torch.nn.functional.linear is br.linear
    assert torch.matmul is mm and torch.nn.functional.linear is lin


def test_emulated_products_round_both_operands_forward_and_backward():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 12, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(7, 12, generator=g, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(7, generator=g, dtype=torch.float64, requires_grad=True)
    G = torch.randn(2, 5, 7, generator=g, dtype=torch.float64)
    r = br.round_bf16
    with br.bf16_matmul():
        y = torch.nn.functional.linear(x, w, bias)
        (y * G).sum().backward()
    assert torch.equal(y.detach(), r(x.detach()) @ r(w.detach()).t() + bias.detach())
    assert torch.equal(x.grad, r(G) @ r(w.detach()))
    assert torch.equal(w.grad, r(G).reshape(-1, 7).t() @ r(x.detach()).reshape(-1, 12))
    assert torch.equal(bias.grad, G.sum((0, 1)))
    a = torch.randn(2, 3, 4, 6, generator=g, requires_grad=True)
    b = torch.randn(2, 3, 6, 5, generator=g, requires_grad=True)
    H = torch.randn(2, 3, 4, 5, generator=g)
    with br.bf16_matmul():
        c = torch.matmul(a, b)
        (c * H).sum().backward()
    assert torch.equal(c.detach(), r(a.detach()) @ r(b.detach()))
    assert torch.equal(a.grad, r(H) @ r(b.detach()).transpose(-1, -2)) and torch.equal(b.grad, r(a.detach()).transpose(-1, -2) @ r(H))


@pytest.mark.parametrize('n_layers,b,l', br.CASES)
def test_the_yardstick_is_sound(n_layers, b, l):
    m, tok, typ, mask, G, runs = br.case(n_layers, b, l)
    (h, g, _), (h64, g64, _), (h32, g32, _) = runs['exact'], runs['emu64'], runs['emu32']
    tag = f'{n_layers} x ({b}, {l})'
    tol = bound(float((h32.double() - h).abs().max()), float(h.abs().max()))
    err = float((h64 - h).abs().max())
    print(f'[{tag}] hidden |emu64 - float64| {err:.3e}  bound {tol:.3e}  (the mode\'s own error on hidden: {float((h32.double() - h).abs().max()):.3e})')
    worst = br.compare_grads(g64, g, g32, bound, tag)
    print(f'[{tag}] largest error / bound: {max([err / tol] + [e / t for e, t in worst.values() if t]):.2f}')
    assert err <= tol
    # ... and the mode is no rounding noise: it moves hidden by far more than fp32 arithmetic does
    assert float((h32.double() - h).abs().max()) > 1e-4


def _weights(n_layers=1):
    from aspire_amd import _lib
    layers = (_lib.BertLayer * n_layers)()
    for ly in layers:
        for f, _ in _lib.BertLayer._fields_:
            setattr(ly, f, ctypes.c_void_p(16))
    return _lib.BertWeights(None, None, None, ctypes.c_void_p(16), ctypes.c_void_p(16), layers, n_layers, 12, 768, 128, 0, 0, 0, 1e-12, None), layers


def test_prec_entries_check_their_arguments_without_a_device():
    from aspire_amd import _lib
    lib = _lib.lib
    bw, keep = _weights()
    B, L = 2, 5
    tape_bytes = lib.aspire_bert_tape_bytes(ctypes.byref(bw), B, L)
    ws_bytes = lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), B, L)
    assert tape_bytes > 0 and ws_bytes > 0

    def fwd(matmul, emb=16, tape=16, nbytes=tape_bytes):
        return lib.aspire_bert_layers_forward_train_prec_f32(ctypes.byref(bw), emb, 16, B, L, 16, tape, nbytes, 16, ws_bytes, None, matmul, None)

    for bad in (2, -1, 7):
        assert fwd(bad) == _lib.ASPIRE_ERR_INVALID_ARG
        assert str(bad).encode() in lib.aspire_last_error()
    for mode in (0, 1):
        assert fwd(mode, emb=None) == _lib.ASPIRE_ERR_INVALID_ARG
        assert fwd(mode, tape=None) == _lib.ASPIRE_ERR_INVALID_ARG
        assert fwd(mode, nbytes=tape_bytes - 1) == _lib.ASPIRE_ERR_INVALID_ARG
        assert b'tape too small' in lib.aspire_last_error()
    drop = _lib.BertDropout(1.0, 0.0, 0, 0)
    assert lib.aspire_bert_layers_forward_train_prec_f32(ctypes.byref(bw), 16, 16, B, L, 16, 16, tape_bytes, 16, ws_bytes, ctypes.byref(drop), 1,
                                                         None) == _lib.ASPIRE_ERR_INVALID_ARG

    glayers = (_lib.BertLayerGrads * 1)()
    for f, _ in _lib.BertLayerGrads._fields_:
        setattr(glayers[0], f, ctypes.c_void_p(16))
    bg = _lib.BertGrads(ctypes.c_void_p(16), ctypes.c_void_p(16), glayers)

    def bwd(matmul, grad_hidden=16, grad_cls=None, mask=16, nbytes=tape_bytes, grad_mix=None):
        return lib.aspire_bert_layers_backward_prec_f32(ctypes.byref(bw), mask, B, L, grad_hidden, grad_cls, None, None, 16, nbytes, 16,
                                                        ctypes.byref(bg), grad_mix, 16, ws_bytes, None, matmul, None)

    for bad in (2, -3):
        assert bwd(bad) == _lib.ASPIRE_ERR_INVALID_ARG
        assert str(bad).encode() in lib.aspire_last_error()
    for mode in (0, 1):
        assert bwd(mode, grad_hidden=None) == _lib.ASPIRE_ERR_INVALID_ARG           # no gradient source
        assert bwd(mode, mask=None) == _lib.ASPIRE_ERR_INVALID_ARG
        assert bwd(mode, nbytes=tape_bytes - 1) == _lib.ASPIRE_ERR_INVALID_ARG
        assert bwd(mode, grad_mix=16) == _lib.ASPIRE_ERR_INVALID_ARG                # grad_mix without mix / layer_cls / grad_cls
    # the size queries do not know the mode: the tape stays fp32 in the same layout
    assert lib.aspire_bert_tape_bytes(ctypes.byref(bw), B, L) == tape_bytes


def test_debug_gemm_checks_its_arguments_without_a_device():
    from aspire_amd import _lib
    lib = _lib.lib

    def gemm(A=16, B=16, C=16, M=4, N=4, K=4, lda=4, ldb=4, ldc=4, form=0, batch=1, nz2=1):
        return lib.aspire_debug_gemm_bf16_f32(A, B, C, M, N, K, lda, ldb, ldc, form, batch, nz2, 0, 0, 0, 0, 0, 0, 1.0, None, None, 0, 0, None)

    for kw in (dict(A=None), dict(B=None), dict(C=None), dict(M=-1), dict(N=-1), dict(K=-1), dict(batch=-1), dict(form=3), dict(form=-1),
               dict(nz2=0), dict(lda=2), dict(K=6, lda=6, ldb=6), dict(A=20), dict(form=2, M=8, lda=4)):
        assert gemm(**kw) == _lib.ASPIRE_ERR_INVALID_ARG, kw
    assert gemm(form=9) == _lib.ASPIRE_ERR_INVALID_ARG and b'9' in lib.aspire_last_error()
    for kw in (dict(M=0), dict(N=0), dict(K=0), dict(batch=0)):
        assert gemm(**kw) == _lib.ASPIRE_OK, kw                                    # a zero size: nothing to do, no launch
    buf = ctypes.create_string_buffer(32)
    assert lib.aspire_debug_get(b'GEMM_BF16_LAST', buf, len(buf)) == _lib.ASPIRE_OK and -1 <= int(buf.value) < 9      # the latest launch's instantiation


def test_matmul_keyword_is_checked_at_construction(monkeypatch):
    from aspire_amd import BiEncTrain, HipBertTrainEncoder, IctEncTrain, SentEncTrain, ops
    monkeypatch.setattr(ops, 'require_gpu', lambda: torch.device('cpu'))            # construction alone: no kernel runs
    assert HipBertTrainEncoder(br._bert(1)).matmul == 'fp32'
    assert HipBertTrainEncoder(br._bert(1), matmul='bf16').matmul == 'bf16'
    for bad in ('int8', 'fp16', None, 1):
        with pytest.raises(ValueError, match='matmul'):
            HipBertTrainEncoder(br._bert(1), matmul=bad)
    assert BiEncTrain(br._bert(1), matmul='bf16').bert_encoder.matmul == 'bf16'
    assert SentEncTrain(br._bert(1), matmul='bf16').matmul == 'bf16' and SentEncTrain(br._bert(1)).sent_encoder.matmul == 'fp32'
    ict = IctEncTrain(br._bert(1), br._bert(1), seed=1, matmul='bf16')
    assert ict.sent_encoder.matmul == ict.context_encoder.matmul == ict.matmul == 'bf16'
    with pytest.raises(ValueError, match='matmul'):
        SentEncTrain(br._bert(1), matmul='int8')


def test_checkpoint_carries_the_mode(tmp_path):
    """RankTrainer.load_checkpoint's rule on a bare state: a checkpoint of the other mode is refused by name, one without the key reads
    as 'fp32' (the check runs before anything of the trainer is touched)."""
    from aspire_amd import RankTrainer

    class Enc:
        matmul = 'bf16'

    tr = RankTrainer.__new__(RankTrainer)
    tr.encoder = Enc()
    torch.save({'encoder': {}, 'matmul': 'fp32'}, tmp_path / 'a.pt')
    with pytest.raises(ValueError, match="'fp32'.*'bf16'"):
        tr.load_checkpoint(tmp_path / 'a.pt')
    torch.save({'encoder': {}}, tmp_path / 'b.pt')                                    # written before the key existed
    with pytest.raises(ValueError, match="'fp32'.*'bf16'"):
        tr.load_checkpoint(tmp_path / 'b.pt')
