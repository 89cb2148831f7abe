"""CPU: the pair arg-max entry without a GPU -- aspire_dot_argmax_f32 (aspire_amd/csrc/dot_argmax.hip) is declared, exported and
signed, its host checks return the project's codes before any launch, the torch operator has a fake and no CPU kernel, and the Python
wrapper refuses a document without rows the way numpy's argmax does."""
import ctypes
import os
import re
import types

import pytest
import torch

FAKE = 16            # a non-null, 16-byte aligned "device pointer" that no call of this file reaches
NAME = 'aspire_dot_argmax_f32'


def test_entry_is_declared_exported_and_signed():
    from aspire_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'aspire_hip.h')).read(), flags=re.S)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), f'{NAME} is not exported'
    args = [a.strip() for a in re.search(NAME + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')]
    assert args == ['const aspire_repset* q', 'const aspire_repset* c', 'int64_t D', 'int32_t* arg', 'float* best', 'void* stream']
    assert len(_lib.SIGNATURES[NAME][1]) == len(args)
    assert callable(ops.dot_argmax)
    assert os.path.exists(os.path.join(root, 'aspire_amd', 'csrc', 'dot_argmax.hip'))


def test_host_checks_without_gpu():
    from aspire_amd import _lib
    INVALID, UNSUPPORTED, OK = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED, _lib.ASPIRE_OK
    err = _lib.lib.aspire_last_error
    max_sents = _lib.lib.aspire_max_sents()

    def rs(n=3, rows=FAKE, start=FAKE, lens=FAKE, ext=0, max_len=8):
        return _lib.RepSet(rows, start, lens, n, ext, max_len, None, None)

    def status(q=None, c=None, D=768, arg=None, best=None):
        q, c = q if q is not None else rs(), c if c is not None else rs()
        return _lib.lib.aspire_dot_argmax_f32(ctypes.byref(q), ctypes.byref(c), D, arg, best, None)

    # (arg stays null in every case that passes the set checks: the call ends there, never in a launch)
    assert status() == INVALID and b'arg is null' in err()
    assert status(best=FAKE) == INVALID and b'arg is null' in err()
    assert _lib.lib.aspire_dot_argmax_f32(None, ctypes.byref(rs()), 768, FAKE, None, None) == INVALID and b'null repset' in err()
    assert _lib.lib.aspire_dot_argmax_f32(ctypes.byref(rs()), None, 768, FAKE, None, None) == INVALID and b'null repset' in err()
    assert status(D=512, arg=FAKE) == UNSUPPORTED and b'768' in err()
    assert status(q=rs(n=3), c=rs(n=4), arg=FAKE) == INVALID and b'equal batch sizes' in err()          # PAIRED only
    assert status(q=rs(rows=24), arg=FAKE) == INVALID and b'16-byte aligned' in err()
    assert status(c=rs(rows=20), arg=FAKE) == INVALID and b'16-byte aligned' in err()
    assert status(q=rs(max_len=max_sents + 1), arg=FAKE) == UNSUPPORTED and b'sentence rows' in err()
    assert status(c=rs(ext=max_sents + 1, max_len=4), arg=FAKE) == UNSUPPORTED and b'sentence rows' in err()
    assert status(q=rs(max_len=max_sents), c=rs(ext=max_sents)) == INVALID and b'arg is null' in err()     # the bound itself passes
    assert status(q=rs(max_len=-1), arg=FAKE) == INVALID
    assert status(q=rs(n=-1), c=rs(n=-1), arg=FAKE) == INVALID and b'negative' in err()
    for field in ('rows', 'start', 'lens'):
        assert status(q=rs(**{field: None}), arg=FAKE) == INVALID and b'null rows / start / len' in err()
    # P == 0: OK, nothing is touched (null everything)
    assert status(q=rs(n=0, rows=None, start=None, lens=None), c=rs(n=0, rows=None, start=None, lens=None)) == OK


def test_torch_op_has_a_fake_and_no_cpu_kernel():
    import aspire_amd.torch_ops as to
    assert 'dot_argmax' in to.OPS and hasattr(torch.ops.aspire, 'dot_argmax') and 'torch.ops.aspire.dot_argmax(' in to.__doc__
    assert len(set(to.OPS)) == len(to.OPS)
    m = lambda *s, dt=torch.float32: torch.empty(*s, device='meta', dtype=dt)
    i32 = torch.int32
    arg, best = torch.ops.aspire.dot_argmax(m(40, 768), m(5, dt=i32), m(5, dt=i32), m(70, 768), m(5, dt=i32), m(5, dt=i32), 20, 10)
    assert arg.shape == (5, 2) and arg.dtype == i32 and best.shape == (5,) and best.dtype == torch.float32
    z = torch.zeros(1, dtype=i32)
    with pytest.raises(NotImplementedError, match='CPU'):          # no CPU kernel behind the op
        torch.ops.aspire.dot_argmax(torch.zeros(2, 768), z, z + 2, torch.zeros(2, 768), z, z + 2, 2, 2)


def test_wrapper_raises_on_a_document_without_rows():
    """numpy: 'attempt to get argmax of an empty sequence' (ValueError).  The check comes before anything touches the device."""
    from aspire_amd import ops
    full = types.SimpleNamespace(n=3, lens_host=[2, 1, 4])
    hole = types.SimpleNamespace(n=3, lens_host=[2, 0, 4])
    for q, c in ((hole, full), (full, hole)):
        with pytest.raises(ValueError, match='empty'):
            ops.dot_argmax(q, c)
    with pytest.raises(AssertionError, match='equal batch sizes'):
        ops.dot_argmax(full, types.SimpleNamespace(n=2, lens_host=[1, 1]))
