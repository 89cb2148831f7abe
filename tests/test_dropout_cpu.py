"""CPU: the training encoder's dropout without a GPU -- the numpy restatement of the generator (tests/dropout_ref.py) against Philox4x32-10's
known-answer vectors, the header's own Philox compiled for the host against the same vectors, the masks' statistics, the new C-ABI
symbols and their argument checks, and the new operators' fake kernels."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import dropout_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
NEW = ('aspire_bert_layers_forward_train_dropout_f32', 'aspire_bert_layers_backward_dropout_f32', 'aspire_bert_dropout_mask_u8')
SEED = 20240607


def test_numpy_philox_reproduces_the_known_answers():
    for counter, key, want in KAT:
        assert tuple(int(x) for x in dr.philox4x32_10(counter, key)) == want
    # ... and as arrays: the three counters under one key, element by element
    c = [np.array([k[0][i] for k in KAT]) for i in range(4)]
    got = dr.philox4x32_10(c, KAT[2][1])
    assert tuple(int(x[2]) for x in got) == KAT[2][2]


def test_header_philox_reproduces_the_known_answers(tmp_path):
    """dropout_rng.h is host code too: the function the kernels call, compiled by the host compiler"""
    src = tmp_path / 'kat.cpp'
    calls = '\n'.join(f'  show(aspire::philox4x32_10({", ".join(hex(x) + "u" for x in c + k)}));' for c, k, _ in KAT)
    src.write_text('#include <stdio.h>\n#include "dropout_rng.h"\n'
                   'static void show(aspire::Philox4 r) { printf("%08x %08x %08x %08x\\n", r.w[0], r.w[1], r.w[2], r.w[3]); }\n'
                   'int main() {\n' + calls + '\n'
                   '  aspire::DropSite d = aspire::drop_site(0x0123456789abcdefull, 7, 4, 0.1f);\n'
                   '  printf("%u %d%d%d%d%d%d\\n", d.thr, aspire::drop_keep(d, 0), aspire::drop_keep(d, 1), aspire::drop_keep(d, 2),\n'
                   '         aspire::drop_keep(d, 3), aspire::drop_keep(d, 4), aspire::drop_keep(d, (1ull << 34) + 1));\n  return 0;\n}\n')
    exe = tmp_path / 'kat'
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', f'-I{ROOT}/aspire_amd/csrc', str(src), '-o', str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split('\n')
    for line, (_, _, want) in zip(out, KAT):
        assert line == ' '.join(f'{x:08x}' for x in want)
    # the keying and the keep rule, against the numpy restatement
    keep = np.concatenate([dr.keep_mask(0x0123456789abcdef, 7, 4, 0.1, 0, 5), dr.keep_mask(0x0123456789abcdef, 7, 4, 0.1, 2 ** 34 + 1, 1)])
    assert out[3] == f'{dr.threshold(0.1)} ' + ''.join(str(int(k)) for k in keep)


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_keep_fraction(p):
    n = 2 ** 20
    frac = float(dr.keep_mask(SEED, 0, 4, p, 0, n).mean())
    tol = 5 * math.sqrt(p * (1 - p) / n)
    print(f'p = {p}: keep fraction {frac:.6f}, 1 - p = {1 - p}, bound {tol:.2e}')
    assert abs(frac - (1 - p)) <= tol


def test_masks_of_two_sites_and_two_steps_differ():
    a = dr.keep_mask(SEED, 0, 2, 0.5, 0, 4096)
    assert not np.array_equal(a, dr.keep_mask(SEED, 0, 3, 0.5, 0, 4096))
    assert not np.array_equal(a, dr.keep_mask(SEED, 1, 2, 0.5, 0, 4096))
    assert not np.array_equal(a, dr.keep_mask(SEED + 1, 0, 2, 0.5, 0, 4096))
    assert np.array_equal(a, dr.keep_mask(SEED, 0, 2, 0.5, 0, 4096))
    # a window of a mask is the mask's window, wherever it starts inside a block
    assert np.array_equal(a[3:1000], dr.keep_mask(SEED, 0, 2, 0.5, 3, 997))


def test_new_symbols_are_exported_and_bound():
    from aspire_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    # the ctypes fields are the header's, in order (test_abi_cpu.test_struct_fields_match_the_header's reading of a struct)
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'aspire_hip.h')).read(), flags=re.S)
    body = re.search(r'typedef struct \{((?:(?!typedef struct).)*?)\}\s*aspire_bert_dropout\s*;', hdr, flags=re.S).group(1)
    names = [decl.strip().split()[-1] for decl in body.split(';') if decl.strip()]
    assert [f for f, _ in _lib.BertDropout._fields_] == names == ['p_hidden', 'p_attn', 'seed', 'step']
    assert [t for _, t in _lib.BertDropout._fields_] == [ctypes.c_float, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32]
    assert _lib.lib.aspire_abi_version() == 6          # functions were only added


def _weights(n_layers=2):
    from aspire_amd import _lib
    layers = (_lib.BertLayer * n_layers)()
    for i in range(n_layers):
        for f, _ in _lib.BertLayer._fields_:
            setattr(layers[i], f, 16)
    bw = _lib.BertWeights(None, None, None, 16, 16, layers, n_layers, 12, 768, 128, 0, 0, 0, 1e-12, None)
    bw._keep = layers
    return bw


def _grads(n_layers=2):
    from aspire_amd import _lib
    layers = (_lib.BertLayerGrads * n_layers)()
    for i in range(n_layers):
        for f, _ in _lib.BertLayerGrads._fields_:
            setattr(layers[i], f, 16)
    bg = _lib.BertGrads(16, 16, layers)
    bg._keep = layers
    return bg


def test_argument_checks_stand_before_the_first_launch():
    """dummy non-null pointers, never dereferenced: every call fails, or returns, before a launch"""
    from aspire_amd import _lib
    lib = _lib.lib
    bw, bg = _weights(), _grads()
    need_t = lib.aspire_bert_tape_bytes(ctypes.byref(bw), 3, 37)
    need_w = lib.aspire_bert_train_workspace_bytes(ctypes.byref(bw), 3, 37)
    inval = _lib.ASPIRE_ERR_INVALID_ARG

    def fwd(drop, b=3, out=16, tape=16):
        return lib.aspire_bert_layers_forward_train_dropout_f32(ctypes.byref(bw), 16, 16, b, 37, out, tape, need_t, 16, need_w,
                                                                ctypes.byref(drop) if drop is not None else None, None)

    def bwd(drop, b=3, g=bg, tape=16):
        return lib.aspire_bert_layers_backward_dropout_f32(ctypes.byref(bw), 16, b, 37, 16, tape, need_t, None,
                                                           ctypes.byref(g) if g is not None else None, 16, need_w,
                                                           ctypes.byref(drop) if drop is not None else None, None)

    ok = _lib.BertDropout(0.1, 0.1, 1, 0)
    for call in (fwd, bwd):
        for bad, text in ((_lib.BertDropout(1.0, 0.1, 1, 0), b'p_hidden = 1'), (_lib.BertDropout(0.1, -0.25, 1, 0), b'p_attn = -0.25'),
                          (_lib.BertDropout(float('nan'), 0.1, 1, 0), b'p_hidden = '), (_lib.BertDropout(0.1, 1.5, 1, 0), b'p_attn = 1.5')):
            assert call(bad, b=0) == inval and text in lib.aspire_last_error(), lib.aspire_last_error()
        assert call(ok, tape=None) == inval
        for drop in (ok, None, _lib.BertDropout(0.0, 0.0, 0, 0)):
            assert call(drop, b=0) == _lib.ASPIRE_OK              # nothing to do: no launch
    assert fwd(ok, out=None) == inval and bwd(ok, g=None) == inval
    with pytest.raises(AssertionError, match='outside'):
        _lib.check(fwd(_lib.BertDropout(1.0, 0.0, 1, 0)))

    def mask(p=0.1, site=0, first=0, n=4, out=16):
        return lib.aspire_bert_dropout_mask_u8(1, 0, site, p, first, n, out, None)

    assert mask(p=1.0) == inval and b'p = 1' in lib.aspire_last_error()
    assert mask(p=float('nan')) == inval and mask(p=-0.5) == inval
    assert mask(n=-1) == inval and mask(first=-1) == inval and mask(site=-1) == inval
    assert mask(out=None) == inval and b'null' in lib.aspire_last_error()
    assert mask(n=0) == _lib.ASPIRE_OK


def test_fake_implementations_propagate_shapes():
    import aspire_amd.torch_ops as to
    for name in ('bert_layers_train_dropout', 'bert_layers_backward_dropout', 'bert_dropout_mask'):
        assert name in to.OPS and hasattr(torch.ops.aspire, name)
    assert len(set(to.OPS)) == len(to.OPS)

    def m(*s, dt=torch.float32):
        return torch.empty(*s, device='meta', dtype=dt)

    layer = [m(2304, 768), m(2304), m(768, 768), m(768), m(768), m(768), m(128, 768), m(128), m(768, 128), m(768), m(768), m(768)]
    for n in (0, 2):
        w = [m(768), m(768)] + layer * n
        hidden, tape = torch.ops.aspire.bert_layers_train_dropout(m(3, 37, 768), m(3, 37, dt=torch.int64), w, 12, 1e-12, 0.1, 0.2, 5, 0)
        assert hidden.shape == (3, 37, 768) and hidden.dtype == torch.float32
        plain = torch.ops.aspire.bert_layers_train(m(3, 37, 768), m(3, 37, dt=torch.int64), w, 12, 1e-12)[1]
        assert tape.dtype == torch.uint8 and tape.dim() == 1 and tape.numel() == plain.numel()       # the tape does not grow
        ge, grads = torch.ops.aspire.bert_layers_backward_dropout(m(3, 37, 768), tape, m(3, 37, dt=torch.int64), w, 12, 1e-12, 0.1, 0.2, 5, 0)
        assert ge.shape == (3, 37, 768) and [g.shape for g in grads] == [t.shape for t in w]
    with pytest.raises(NotImplementedError, match='CPU'):          # no CPU kernel behind them
        torch.ops.aspire.bert_layers_train_dropout(torch.zeros(1, 2, 768), torch.ones(1, 2, dtype=torch.int64),
                                                   [torch.ones(768), torch.zeros(768)], 12, 1e-12, 0.1, 0.1, 1, 0)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        keep = torch.ops.aspire.bert_dropout_mask(1, 0, 3, 0.1, 5, 11)
    assert keep.shape == (11,) and keep.dtype == torch.uint8
