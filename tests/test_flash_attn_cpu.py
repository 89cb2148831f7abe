"""CPU: the training encoder's fused attention mode without a device -- the new symbols, the tape's and the workspace's sizes (no L^2
term left), the refusals of the C entries, the operators and the constructors, and the checkpoint's mode key.  Nothing here touches a
GPU; the host-only size queries read the geometry of the weights struct alone."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_matmul_ref as br  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    'aspire_bert_tape_bytes_attn': 'w B L attention',
    'aspire_bert_train_workspace_bytes_attn': 'w B L attention',
    'aspire_bert_layers_forward_train_attn_f32': 'w emb_sum attn_mask B L hidden_out tape tape_bytes ws ws_bytes dropout matmul attention stream',
    'aspire_bert_layers_backward_attn_f32': 'w attn_mask B L grad_hidden grad_cls mix layer_cls tape tape_bytes grad_emb_sum grads grad_mix ws '
                                            'ws_bytes dropout matmul attention stream',
    'aspire_bert_cls_mix_train_attn_f32': 'w B L tape tape_bytes hidden_out mix cls_out layer_cls attention stream',
    'aspire_debug_flash_attn_train_f32': 'qkv mask B L dropout ctx stats stream',
    'aspire_debug_flash_attn_train_backward_f32': 'qkv mask ctx stats dctx B L dropout layer D dqkv stream',
}
GEMM, FLASH = 0, 1
SLOT = 256          # the carve's alignment: every slot of the tape and of the workspace starts on a multiple of it


# ---- 1. symbols -------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_in_the_header_the_table_and_the_library():
    from aspire_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    src = open(os.path.join(ROOT, 'include', 'aspire_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name, want in NEW.items():
        assert hasattr(raw, name), name
        res, args = _lib.SIGNATURES[name]
        m = re.search(r'\b(int|size_t)\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m, name
        params = [p.strip() for p in m.group(2).split(',')]
        assert [p.split()[-1].lstrip('*') for p in params] == want.split(), name
        assert len(args) == len(params), name
        assert res is (ctypes.c_int if m.group(1) == 'int' else ctypes.c_size_t), name
    assert re.search(r'#define\s+ASPIRE_ATTENTION_GEMM\s+0\b', hdr) and re.search(r'#define\s+ASPIRE_ATTENTION_FLASH\s+1\b', hdr)
    assert (_lib.ATTENTION_GEMM, _lib.ATTENTION_FLASH) == (GEMM, FLASH)
    assert re.search(r'#define\s+ASPIRE_ABI_VERSION\s+6\b', hdr) and _lib.lib.aspire_abi_version() == 6        # entries were only added


# ---- 2. sizes ---------------------------------------------------------------------------------------------------------------------------
def _weights(n_layers=2, ffn=128):
    from aspire_amd import _lib
    layers = (_lib.BertLayer * max(n_layers, 1))()
    for i in range(n_layers):
        for f, _ in _lib.BertLayer._fields_:
            setattr(layers[i], f, 16)
    bw = _lib.BertWeights(None, None, None, 16, 16, layers, n_layers, 12, 768, ffn, 0, 0, 0, 1e-12, None)
    bw._keep = layers
    return bw


TAPE_SLOTS, WS_SLOTS = 8, 8          # slots per layer of the tape (+ 1 for the embedding sum); slots of the workspace


@pytest.mark.parametrize('n_layers,ffn,B', [(2, 128, 1), (2, 128, 3), (12, 3072, 4), (12, 3072, 10)])
def test_tape_and_workspace_sizes(n_layers, ffn, B):
    from aspire_amd import _lib
    lib = _lib.lib
    bw = _weights(n_layers, ffn)
    w = ctypes.byref(bw)
    for b, l in ((B, 1), (B, 37), (B, 256), (B, 512)):
        assert lib.aspire_bert_tape_bytes_attn(w, b, l, GEMM) == lib.aspire_bert_tape_bytes(w, b, l) > 0
        assert lib.aspire_bert_train_workspace_bytes_attn(w, b, l, GEMM) == lib.aspire_bert_train_workspace_bytes(w, b, l) > 0
        # (at a few rows both forms round up to the same 256-byte slots; from L = 37 on the probabilities are the larger)
        assert 0 < lib.aspire_bert_tape_bytes_attn(w, b, l, FLASH) <= lib.aspire_bert_tape_bytes(w, b, l) - (l >= 37)
        assert 0 < lib.aspire_bert_train_workspace_bytes_attn(w, b, l, FLASH) <= lib.aspire_bert_train_workspace_bytes(w, b, l) - (l >= 37)
    # no L^2 term: twice the length, twice the bytes, up to the alignment of every slot
    t256, t512 = (lib.aspire_bert_tape_bytes_attn(w, B, l, FLASH) for l in (256, 512))
    w256, w512 = (lib.aspire_bert_train_workspace_bytes_attn(w, B, l, FLASH) for l in (256, 512))
    print(f'{n_layers} layers, ffn {ffn}, B {B}: flash tape {t256} / {t512} B, workspace {w256} / {w512} B at L = 256 / 512; '
          f'gemm tape {lib.aspire_bert_tape_bytes(w, B, 512)} B, workspace {lib.aspire_bert_train_workspace_bytes(w, B, 512)} B at L = 512')
    assert abs(t512 - 2 * t256) <= 2 * SLOT * (1 + TAPE_SLOTS * n_layers)
    # (the column-sum and LayerNorm partials are a ceil over row blocks: one block of each more or less)
    assert abs(w512 - 2 * w256) <= 2 * SLOT * WS_SLOTS + 4 * 2 * max(3 * 768, ffn) * 2
    # the probabilities left the tape, two statistics per row came: at least this much smaller
    gone = B * 12 * 512 * 512 * 4 - B * 12 * 512 * 8
    assert lib.aspire_bert_tape_bytes(w, B, 512) - t512 >= n_layers * gone
    # the workspace held one such buffer (dP / dS); D [B, 12, L] came
    assert lib.aspire_bert_train_workspace_bytes(w, B, 512) - w512 >= B * 12 * 512 * 512 * 4 - B * 12 * 512 * 4 - SLOT
    for bad in (2, -1):
        assert lib.aspire_bert_tape_bytes_attn(w, B, 512, bad) == 0 and lib.aspire_bert_train_workspace_bytes_attn(w, B, 512, bad) == 0


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
def test_c_entries_refuse_unknown_modes_and_flash_outside_bf16():
    from aspire_amd import _lib
    lib = _lib.lib
    bw = _weights()
    w = ctypes.byref(bw)
    B, L = 2, 5
    inval, unsup, ok = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED, _lib.ASPIRE_OK
    glayers = (_lib.BertLayerGrads * 2)()
    for i in range(2):
        for f, _ in _lib.BertLayerGrads._fields_:
            setattr(glayers[i], f, 16)
    bg = _lib.BertGrads(16, 16, glayers)

    def sizes(att):
        return lib.aspire_bert_tape_bytes_attn(w, B, L, att), lib.aspire_bert_train_workspace_bytes_attn(w, B, L, att)

    def fwd(matmul, att, b=B, tape_bytes=None):
        t, s = sizes(att if att in (GEMM, FLASH) else GEMM)
        return lib.aspire_bert_layers_forward_train_attn_f32(w, 16, 16, b, L, 16, 16, t if tape_bytes is None else tape_bytes, 16, s, None,
                                                             matmul, att, None)

    def bwd(matmul, att, b=B, ws_bytes=None):
        t, s = sizes(att if att in (GEMM, FLASH) else GEMM)
        return lib.aspire_bert_layers_backward_attn_f32(w, 16, b, L, 16, None, None, None, 16, t, 16, ctypes.byref(bg), None, 16,
                                                        s if ws_bytes is None else ws_bytes, None, matmul, att, None)

    for call in (fwd, bwd):
        for bad in (2, -1, 7):
            assert call(1, bad) == inval and str(bad).encode() in lib.aspire_last_error()
        for matmul in (0, 3):
            assert call(matmul, FLASH) == unsup and b'ASPIRE_MATMUL_BF16' in lib.aspire_last_error()
        assert call(2, FLASH) == inval                                      # an unknown matmul mode stays an invalid argument
        for matmul, att in ((0, GEMM), (1, GEMM), (3, GEMM), (1, FLASH)):
            assert call(matmul, att, b=0) == ok                             # nothing to do: no launch
    # the mode's own sizes are what the buffers are held to
    t, s = sizes(FLASH)
    assert fwd(1, FLASH, tape_bytes=t - 1) == inval and b'tape too small' in lib.aspire_last_error()
    assert bwd(1, FLASH, ws_bytes=s - 1) == inval and b'workspace too small' in lib.aspire_last_error()
    with pytest.raises(NotImplementedError, match='ASPIRE_MATMUL_BF16'):
        _lib.check(fwd(0, FLASH))
    # the CLS tap on a tape of the mode
    assert lib.aspire_bert_cls_mix_train_attn_f32(w, B, L, 16, t, 16, None, 16, None, 5, None) == inval
    assert lib.aspire_bert_cls_mix_train_attn_f32(w, B, L, 16, t - 1, 16, None, 16, None, FLASH, None) == inval
    assert lib.aspire_bert_cls_mix_train_attn_f32(w, 0, L, 16, t, 16, None, 16, None, FLASH, None) == ok
    # the bare kernels' entries
    assert lib.aspire_debug_flash_attn_train_f32(None, 16, B, L, None, 16, 16, None) == inval
    assert lib.aspire_debug_flash_attn_train_f32(16, 16, B, 513, None, 16, 16, None) == inval and b'513' in lib.aspire_last_error()
    assert lib.aspire_debug_flash_attn_train_f32(16, 16, B, 2 ** 32 + 5, None, 16, 16, None) == inval       # the int64 L is what is checked
    assert lib.aspire_debug_flash_attn_train_f32(16, 16, 0, L, None, 16, 16, None) == ok
    drop = _lib.BertDropout(0.0, 1.0, 0, 0)
    assert lib.aspire_debug_flash_attn_train_f32(16, 16, B, L, ctypes.byref(drop), 16, 16, None) == inval
    assert lib.aspire_debug_flash_attn_train_backward_f32(16, 16, 16, 16, None, B, L, None, 0, 16, 16, None) == inval
    assert lib.aspire_debug_flash_attn_train_backward_f32(16, 16, 16, 16, 16, B, L, None, 0, None, 16, None) == inval       # D is the caller's
    assert lib.aspire_debug_flash_attn_train_backward_f32(16, 16, 16, 16, 16, B, 2 ** 32 + 5, None, 0, 16, 16, None) == inval
    assert lib.aspire_debug_flash_attn_train_backward_f32(16, 16, 16, 16, 16, 0, L, None, 0, 16, 16, None) == ok


def test_attention_keyword_is_checked_at_construction(monkeypatch):
    from aspire_amd import BiEncTrain, HipBertTrainEncoder, IctEncTrain, SentEncTrain, ops
    monkeypatch.setattr(ops, 'require_gpu', lambda: torch.device('cpu'))            # construction alone: no kernel runs
    assert HipBertTrainEncoder(br._bert(1)).attention == 'gemm'
    assert HipBertTrainEncoder(br._bert(1), matmul='bf16').attention == 'gemm'
    assert HipBertTrainEncoder(br._bert(1), matmul='bf16', attention='flash').attention == 'flash'
    for bad in ('fused', 'sdpa', None, 1):
        with pytest.raises(ValueError, match='attention'):
            HipBertTrainEncoder(br._bert(1), matmul='bf16', attention=bad)
    for matmul in ('fp32', 'bf16x3'):
        with pytest.raises(NotImplementedError, match='flash'):
            HipBertTrainEncoder(br._bert(1), matmul=matmul, attention='flash')
    with pytest.raises(NotImplementedError, match='flash'):
        HipBertTrainEncoder(br._bert(1), attention='flash')
    kw = dict(matmul='bf16', attention='flash')
    assert BiEncTrain(br._bert(1), **kw).bert_encoder.attention == 'flash' and BiEncTrain(br._bert(1)).attention == 'gemm'
    assert SentEncTrain(br._bert(1), **kw).attention == 'flash' and SentEncTrain(br._bert(1)).sent_encoder.attention == 'gemm'
    ict = IctEncTrain(br._bert(1), br._bert(1), seed=1, **kw)
    assert ict.sent_encoder.attention == ict.context_encoder.attention == ict.attention == 'flash'
    with pytest.raises(NotImplementedError, match='flash'):
        SentEncTrain(br._bert(1), attention='flash')


def test_operators_exist_propagate_shapes_and_refuse_cpu_tensors():
    import aspire_amd.torch_ops as to
    from aspire_amd import _lib
    names = ('bert_layers_train_attn', 'bert_layers_backward_attn', 'bert_layers_train_cls_attn', 'bert_layers_backward_cls_attn')
    for name in names:
        assert name in to.OPS and hasattr(torch.ops.aspire, name)
    assert len(set(to.OPS)) == len(to.OPS)

    def m(*s, dt=torch.float32):
        return torch.empty(*s, device='meta', dtype=dt)

    layer = [m(2304, 768), m(2304), m(768, 768), m(768), m(768), m(768), m(128, 768), m(128), m(768, 128), m(768), m(768), m(768)]
    w = [m(768), m(768)] + layer * 2
    mask = m(3, 37, dt=torch.int64)
    key = (12, 1e-12, 0.1, 0.2, 5, 0, 1)
    bw = _weights(2)
    for att in (GEMM, FLASH):
        want = _lib.lib.aspire_bert_tape_bytes_attn(ctypes.byref(bw), 3, 37, att)
        hidden, tape = torch.ops.aspire.bert_layers_train_attn(m(3, 37, 768), mask, w, *key, att)
        assert hidden.shape == (3, 37, 768) and tape.dtype == torch.uint8 and tape.numel() == want
        ge, grads = torch.ops.aspire.bert_layers_backward_attn(m(3, 37, 768), tape, mask, w, *key, att)
        assert ge.shape == (3, 37, 768) and [g.shape for g in grads] == [t.shape for t in w]
        for mix in (m(3), None):
            cls, layer_cls, tape = torch.ops.aspire.bert_layers_train_cls_attn(m(3, 37, 768), mask, w, mix, *key, att)
            assert cls.shape == (3, 768) and layer_cls.shape == ((3, 3, 768) if mix is not None else (0,)) and tape.numel() == want
            ge, grads, gm = torch.ops.aspire.bert_layers_backward_cls_attn(m(3, 768), layer_cls, tape, mask, w, mix, *key, att)
            assert ge.shape == (3, 37, 768) and [g.shape for g in grads] == [t.shape for t in w] and gm.shape == ((3,) if mix is not None else (0,))
    # no CPU kernel behind them, as behind their siblings
    real = [torch.zeros(768), torch.zeros(768)]
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.bert_layers_train_attn(torch.zeros(1, 2, 768), torch.ones(1, 2, dtype=torch.int64), real, *key, FLASH)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.bert_layers_train_cls_attn(torch.zeros(1, 2, 768), torch.ones(1, 2, dtype=torch.int64), real, None, *key, FLASH)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.bert_layers_backward_attn(torch.zeros(1, 2, 768), torch.zeros(16, dtype=torch.uint8), torch.ones(1, 2, dtype=torch.int64),
                                                   real, *key, FLASH)
    # the operators' own check of the two modes (what the C entries refuse as well)
    with pytest.raises(AssertionError, match='attention mode 5'):
        to._check_attention(1, 5)
    for matmul in (0, 3):
        with pytest.raises(NotImplementedError, match='ASPIRE_MATMUL_BF16'):
            to._check_attention(matmul, FLASH)
    to._check_attention(1, FLASH), to._check_attention(0, GEMM)


def test_checkpoint_carries_the_attention_mode(tmp_path):
    """RankTrainer.load_checkpoint's rule on a bare state: a checkpoint of the other attention mode is refused by name, one without the
    key reads as 'gemm' (the check runs before anything of the trainer is touched)"""
    from aspire_amd import RankTrainer

    class Enc:
        matmul = 'bf16'
        attention = 'flash'

    tr = RankTrainer.__new__(RankTrainer)
    tr.encoder = Enc()
    torch.save({'encoder': {}, 'matmul': 'bf16', 'attention': 'gemm'}, tmp_path / 'a.pt')
    with pytest.raises(ValueError, match="attention='gemm'.*attention='flash'"):
        tr.load_checkpoint(tmp_path / 'a.pt')
    torch.save({'encoder': {}, 'matmul': 'bf16'}, tmp_path / 'b.pt')                  # written before the key existed
    with pytest.raises(ValueError, match="attention='gemm'.*attention='flash'"):
        tr.load_checkpoint(tmp_path / 'b.pt')
    Enc.attention = 'gemm'
    torch.save({'encoder': {}, 'matmul': 'bf16', 'attention': 'flash'}, tmp_path / 'c.pt')
    with pytest.raises(ValueError, match="attention='flash'.*attention='gemm'"):
        tr.load_checkpoint(tmp_path / 'c.pt')
