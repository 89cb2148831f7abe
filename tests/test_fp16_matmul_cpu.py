"""CPU: the inference encoder's fp16 matmul mode (include/aspire_hip.h A1h) without a device -- the H layout's index function, the CPU
emulation the GPU tests are held against (tests/fp16_matmul_ref.py), the argument checks of the new entry points, and the keyword's
check at construction."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp16_matmul_ref as fr  # noqa: E402


# ---- the H layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', [1, 5, 128, 300])
@pytest.mark.parametrize('K', [32, 768])
def test_piece_index_is_a_bijection(R, K):
    t = fr.h_piece_table(R, K)
    assert t.shape == (R, K // 8)
    assert sorted(t.reshape(-1).tolist()) == list(range(R * K // 8))            # onto the R K / 8 pieces, each once
    for r in (0, R // 2, R - 1):                                                # the scalar form agrees with the table
        for k in (0, 8, 24, K - 8):
            assert fr.h_piece_index(R, r, k) == t[r, k // 8] == fr.h_piece_index(R, r, k + 7)
    # within a k block a row's four pieces are its own 64 bytes, permuted by the row's bits 2..3
    for r in range(min(R, 20)):
        assert sorted(t[r, :4].tolist()) == list(range(4 * r, 4 * r + 4))
        assert [int(p) - 4 * r for p in t[r, :4]] == [q ^ ((r >> 2) & 3) for q in range(4)]
    assert R * K * 2 + fr.PAD_ROWS * K * 2 == fr.h_bytes(R, K)


@pytest.mark.parametrize('R', [128, 300])
def test_a_row_tile_of_a_k_block_is_one_contiguous_run(R):
    K = 768
    t = fr.h_piece_table(R, K)
    for kb in (0, 7, K // 32 - 1):
        for r0 in range(0, R - 127, 128):
            run = t[r0:r0 + 128, 4 * kb:4 * kb + 4].reshape(-1)
            lo = (kb * R + r0) * 4
            assert sorted(run.tolist()) == list(range(lo, lo + 512))            # 512 pieces x 16 bytes = 8 KB, nothing else in between


def test_decoder_inverts_the_index():
    R, K = 37, 64
    x = (np.arange(R * K, dtype=np.float32).reshape(R, K) % 2048).astype(np.float16)
    buf = np.zeros(fr.h_bytes(R, K), np.uint8)
    pieces = buf[:R * K * 2].view(np.float16).reshape(-1, 8)
    for r in range(R):
        for k in range(0, K, 8):
            pieces[fr.h_piece_index(R, r, k)] = x[r, k:k + 8]
    assert np.array_equal(fr.h_decode(buf, R, K), x)


# ---- the emulation -----------------------------------------------------------------------------------------------------------------
def test_emulated_linear_is_exact_on_fp16_operands_and_differs_otherwise():
    g = torch.Generator().manual_seed(3)
    lin = torch.nn.Linear(64, 32).double()
    x = torch.randn(7, 64, generator=g, dtype=torch.float64)
    with torch.no_grad():
        exact = lin(x)
        with fr.fp16_linears([lin.weight]):
            emu = lin(x)
        assert (emu - exact).abs().max() > 1e-5                                 # operands with more than 11 bits: the rounding shows
        # every operand an fp16 value already (the weight after the factor 64): the emulation IS the exact product
        lin.weight.copy_(fr.r16(64.0 * lin.weight) / 64.0)
        x16 = fr.r16(x)
        exact = lin(x16)
        with fr.fp16_linears([lin.weight]):
            emu = lin(x16)
            other = torch.nn.functional.linear(x, lin.weight.clone())           # a weight that is not listed: untouched
        assert torch.equal(emu, exact)
        assert torch.equal(other, x @ lin.weight.t())
    assert torch.nn.functional.linear is fr._linear                             # the patch is gone


def test_emulated_model_differs_from_the_exact_one_and_keeps_the_cls_tail():
    m = fr.bert(2, seed=1, intermediate_size=128, pooler=True)
    m64 = m.double()
    assert len(fr.mode_weights(m64)) == 12 and len(fr.mode_weights(m64, cls_tail=True)) == 9       # six linears a layer; the pooler never
    assert all(w is not m64.pooler.dense.weight for w in fr.mode_weights(m64))
    m.float()
    tok = torch.randint(0, fr.VOCAB, (2, 9), generator=torch.Generator().manual_seed(0))
    kw = dict(input_ids=tok, attention_mask=torch.ones_like(tok))
    exact, emu = fr.run64(m, False, **kw), fr.run64(m, True, **kw)
    d = (emu.last_hidden_state - exact.last_hidden_state).abs().max().item()
    assert 1e-5 < d < 1e-1, d
    assert torch.equal(emu.hidden_states[0], exact.hidden_states[0])            # embeddings + LayerNorm: no product of the mode


# ---- the entry points' checks --------------------------------------------------------------------------------------------------------
def _weights(n_layers=1, ffn=128):
    from aspire_amd import _lib
    layers = (_lib.BertLayer * n_layers)()
    for ly in layers:
        for f, _ in _lib.BertLayer._fields_:
            setattr(ly, f, ctypes.c_void_p(16))
    return _lib.BertWeights(ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), layers,
                            n_layers, 12, 768, ffn, 50, 512, 2, 1e-12, None), layers


def test_prec_forwards_check_their_arguments_without_a_device():
    from aspire_amd import _lib
    lib = _lib.lib
    bw, keep = _weights()
    B, L = 2, 5
    need = lib.aspire_bert_workspace_bytes_prec(ctypes.byref(bw), B, L, _lib.MATMUL_FP16)
    need_cls = lib.aspire_bert_cls_workspace_bytes_prec(ctypes.byref(bw), B, L, _lib.MATMUL_FP16)
    assert need == lib.aspire_bert_workspace_bytes(ctypes.byref(bw), B, L) > 0
    assert need_cls == lib.aspire_bert_cls_workspace_bytes(ctypes.byref(bw), B, L) > need
    assert lib.aspire_bert_workspace_bytes_prec(ctypes.byref(bw), B, L, _lib.MATMUL_FP32) == need
    for bad in (1, 2, 3, -1):                                                   # the training modes are no modes of these entries
        assert lib.aspire_bert_workspace_bytes_prec(ctypes.byref(bw), B, L, bad) == 0
        assert lib.aspire_bert_cls_workspace_bytes_prec(ctypes.byref(bw), B, L, bad) == 0

    def fwd(matmul, hp=16, tok=16, mask=16, out=16, ws=16, nbytes=need, w=bw):
        return lib.aspire_bert_forward_prec_f32(ctypes.byref(w) if w is not None else None, None, hp, matmul, tok, 16, mask, B, L, out, ws,
                                                nbytes, None)

    def cls(matmul, hp=16, tok=16, mask=16, out=16, ws=16, nbytes=need_cls, w=bw):
        return lib.aspire_bert_forward_cls_prec_f32(ctypes.byref(w) if w is not None else None, hp, matmul, tok, 16, mask, B, L, None, out,
                                                    None, ws, nbytes, None)

    for call in (fwd, cls):
        for mode in (_lib.MATMUL_FP32, _lib.MATMUL_FP16):
            for kw in (dict(tok=None), dict(mask=None), dict(out=None), dict(w=None)):
                assert call(mode, **kw) == _lib.ASPIRE_ERR_INVALID_ARG, (call.__name__, mode, kw)
                assert b'null pointer' in lib.aspire_last_error()
            assert call(mode, ws=None) == _lib.ASPIRE_ERR_INVALID_ARG
            assert call(mode, nbytes=(need if call is fwd else need_cls) - 1) == _lib.ASPIRE_ERR_INVALID_ARG
            assert b'workspace too small' in lib.aspire_last_error()
        for bad in (2, 1, 3, -4):
            assert call(bad) == _lib.ASPIRE_ERR_INVALID_ARG
            assert str(bad).encode() in lib.aspire_last_error() and b'matmul' in lib.aspire_last_error()
        assert call(_lib.MATMUL_FP16, hp=None) == _lib.ASPIRE_ERR_INVALID_ARG
        assert b'hplanes' in lib.aspire_last_error()
    # the training entries keep refusing the value
    tape, tws = lib.aspire_bert_tape_bytes(ctypes.byref(bw), B, L), lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), B, L)
    assert lib.aspire_bert_layers_forward_train_prec_f32(ctypes.byref(bw), 16, 16, B, L, 16, 16, tape, 16, tws, None, _lib.MATMUL_FP16,
                                                         None) == _lib.ASPIRE_ERR_INVALID_ARG


def test_hplane_entries_check_their_arguments_without_a_device():
    from aspire_amd import _lib
    lib = _lib.lib
    bw, keep = _weights(n_layers=2, ffn=256)
    per_layer = sum((r + 256) * k * 2 for r, k in ((2304, 768), (768, 768), (256, 768), (768, 256)))
    assert lib.aspire_bert_hplanes_bytes(ctypes.byref(bw)) == 2 * per_layer        # (every matrix a multiple of 256 bytes already)
    assert lib.aspire_bert_hplanes_bytes(None) == 0
    assert lib.aspire_bert_prepare_hplanes(ctypes.byref(bw), None, 1 << 30, None) == _lib.ASPIRE_ERR_INVALID_ARG
    assert lib.aspire_bert_prepare_hplanes(None, 16, 1 << 30, None) == _lib.ASPIRE_ERR_INVALID_ARG
    assert lib.aspire_bert_prepare_hplanes(ctypes.byref(bw), 16, 2 * per_layer - 1, None) == _lib.ASPIRE_ERR_INVALID_ARG
    assert b'too small' in lib.aspire_last_error()
    odd, keep2 = _weights(ffn=192)
    assert lib.aspire_bert_prepare_hplanes(ctypes.byref(odd), 16, 1 << 30, None) == _lib.ASPIRE_ERR_UNSUPPORTED
    assert lib.aspire_debug_hplane_bytes(300, 768) == fr.h_bytes(300, 768)
    assert lib.aspire_debug_split_hplane(None, 4, 32, 16, 0, None) == _lib.ASPIRE_ERR_INVALID_ARG
    assert lib.aspire_debug_split_hplane(16, 4, 48, 16, 0, None) == _lib.ASPIRE_ERR_UNSUPPORTED

    def gemm(Ah=16, Bh=16, C=16, Ch=None, res=None, M=4, N=64, K=32, epilogue=0):
        return lib.aspire_debug_gemm_hplane(Ah, Bh, C, Ch, None, res, M, N, K, epilogue, None)

    for kw in (dict(Ah=None), dict(Bh=None), dict(C=None), dict(epilogue=1), dict(epilogue=2), dict(M=0), dict(epilogue=1, Ch=16, res=16)):
        assert gemm(**kw) == _lib.ASPIRE_ERR_INVALID_ARG, kw
    for kw in (dict(N=32), dict(N=96), dict(K=48)):
        assert gemm(**kw) == _lib.ASPIRE_ERR_UNSUPPORTED, kw


def test_matmul_keyword_is_checked_at_construction():
    from aspire_amd.encoder import HipBertEncoder
    for bad in ('bf16', 'int8', None, 4):
        with pytest.raises(ValueError, match='matmul'):
            HipBertEncoder(fr.bert(1, intermediate_size=128), matmul=bad)
