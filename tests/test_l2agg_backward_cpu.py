"""CPU: the backward of the L2 aggregations without a GPU -- the C-ABI entry (declared, exported, signed), the argument checks of
aspire_l2agg_backward_f32 that return before any launch, and the fake kernels of the two new operators."""
import ctypes
import os
import re

import pytest
import torch

FAKE = 16            # a non-null, 16-byte aligned "device pointer" that no call of this file reaches
NAME = 'aspire_l2agg_backward_f32'


def test_entry_is_declared_exported_and_signed():
    from aspire_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'aspire_hip.h')).read(), flags=re.S)
    decl = [a.strip() for a in re.search(NAME + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')]
    assert decl == ['const aspire_repset* q', 'const aspire_repset* c', 'int64_t D', 'int pairing', 'int agg', 'double temp',
                    'const float* grad_scores', 'float* grad_q_rows', 'float* grad_c_rows', 'void* stream']
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), f'{NAME} is not exported'
    rs, vp = ctypes.POINTER(_lib.RepSet), ctypes.c_void_p
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, [rs, rs, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, vp, vp, vp, vp])
    assert callable(ops.l2agg_backward)


def _set(n, ext=8, max_len=8):
    from aspire_amd import _lib
    return _lib.RepSet(FAKE, FAKE, FAKE, n, ext, max_len)


def test_backward_entry_validation_without_gpu():
    from aspire_amd import _lib
    INVALID, UNSUPPORTED, OK = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED, _lib.ASPIRE_OK
    err = _lib.lib.aspire_last_error
    q, c = _set(3), _set(3)
    base = dict(D=768, pairing=_lib.PAIR_PAIRED, agg=_lib.AGG_TOP2, temp=1.0, gs=FAKE, gq=FAKE, gc=None)

    def status(q=q, c=c, **kw):
        a = dict(base, **kw)
        return _lib.lib.aspire_l2agg_backward_f32(ctypes.byref(q), ctypes.byref(c), a['D'], a['pairing'], a['agg'], a['temp'], a['gs'],
                                                  a['gq'], a['gc'], None)

    # (grad_c_rows is null in every call: a call that passed every other check ends in "is null", never in a launch)
    assert status() == INVALID and b'is null' in err()
    for agg in (_lib.AGG_MAX, _lib.AGG_TOP2, _lib.AGG_ATTENTION):
        assert status(agg=agg, temp=0.05) == INVALID and b'is null' in err()
    assert status(gs=None, gc=FAKE) == INVALID and b'is null' in err()
    assert status(gq=None, gc=FAKE) == INVALID and b'is null' in err()
    # CROSS would need an accumulation across pairs: not built, and the message says so
    assert status(pairing=_lib.PAIR_CROSS, gc=FAKE) == UNSUPPORTED and b'accumulation across pairs' in err()
    with pytest.raises(NotImplementedError, match='ASPIRE_PAIR_PAIRED'):
        _lib.check(status(pairing=_lib.PAIR_CROSS, gc=FAKE))
    assert status(pairing=2) == INVALID and b'bad pairing' in err()
    for agg in (3, 7, -1):
        assert status(agg=agg) == INVALID and b'bad aggregation' in err()
    assert status(agg=_lib.AGG_ATTENTION, temp=0.0) == INVALID and b'temperature' in err()
    assert status(agg=_lib.AGG_ATTENTION, temp=-1.0) == INVALID and b'temperature' in err()
    assert status(agg=_lib.AGG_MAX, temp=0.0) == INVALID and b'is null' in err()          # temp is ATTENTION's
    assert status(c=_set(4)) == INVALID and b'equal batch sizes' in err()
    assert status(D=512) == UNSUPPORTED and b'768' in err()
    null = _lib.lib.aspire_l2agg_backward_f32(None, ctypes.byref(c), 768, _lib.PAIR_PAIRED, _lib.AGG_MAX, 1.0, FAKE, FAKE, FAKE, None)
    assert null == INVALID and b'null repset' in err()
    # the forward's row limit, padded and CSR, either side (every pointer given: the check sits in front of the launch)
    for kw in (dict(q=_set(3, ext=129)), dict(c=_set(3, ext=129)), dict(q=_set(3, ext=0, max_len=129)), dict(c=_set(3, ext=0, max_len=129))):
        assert status(gc=FAKE, **kw) == UNSUPPORTED
        assert b'more than 128 sentence rows' in err()
    assert status(q=_set(3, ext=128), c=_set(3, ext=0, max_len=128)) == INVALID and b'is null' in err()
    # no pairs: nothing to do, no buffers needed
    assert status(q=_set(0), c=_set(0), gs=None, gq=None) == OK


def _m(*s, dt=torch.float32):
    return torch.empty(*s, device='meta', dtype=dt)


def test_fake_kernels_of_the_two_operators():
    import aspire_amd.torch_ops as to
    i32 = torch.int32
    for name in ('l2agg_pair_scores', 'l2agg_pair_backward'):
        assert name in to.OPS and hasattr(torch.ops.aspire, name)
    for agg in (0, 1, 2):
        s = torch.ops.aspire.l2agg_pair_scores(_m(4, 8, 768), _m(4, dt=i32), _m(4, 6, 768), _m(4, dt=i32), agg, 0.5)
        assert s.shape == (4,) and s.dtype == torch.float32 and s.device.type == 'meta'
        gq, gc = torch.ops.aspire.l2agg_pair_backward(_m(4), _m(4, 8, 768), _m(4, dt=i32), _m(4, 6, 768), _m(4, dt=i32), agg, 0.5)
        assert gq.shape == (4, 8, 768) and gc.shape == (4, 6, 768) and gq.dtype == gc.dtype == torch.float32
    with pytest.raises(AssertionError):      # pair_distances.py:46
        torch.ops.aspire.l2agg_pair_scores(_m(3, 8, 768), _m(3, dt=i32), _m(5, 6, 768), _m(5, dt=i32), 0, 1.0)
    # the first operator carries an autograd formula: a fake forward of inputs that require grad is attached to the graph
    q = torch.empty(2, 8, 768, device='meta', requires_grad=True)
    s = torch.ops.aspire.l2agg_pair_scores(q, _m(2, dt=i32), _m(2, 8, 768), _m(2, dt=i32), 2, 1.0)
    assert s.requires_grad and s.grad_fn is not None
    s.sum().backward()
    assert q.grad.shape == (2, 8, 768)


def test_no_cpu_kernel_behind_the_new_operators():
    import aspire_amd.torch_ops  # noqa: F401
    z, n = torch.zeros(1, 2, 768), torch.ones(1, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.l2agg_pair_scores(z, n, z, n, 0, 1.0)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.l2agg_pair_backward(torch.zeros(1), z, n, z, n, 0, 1.0)

