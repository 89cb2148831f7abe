"""CPU: the train-side distances without a GPU -- the three new C-ABI entries (aspire_jointsm_backward_f32, aspire_l2sup_scores_f32,
aspire_l2sup_backward_f32: declared, exported, signed; ABI still 6), their argument checks that return before any launch, the fake
kernels of the four new operators, the host-side checks of the two l2sup names, and the fixture tests/golden/trainside.npz held against
the yardstick the GPU tests use: the float64 closed forms of tests/golden/trainside_inputs.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import trainside_inputs as ti  # noqa: E402

FAKE = 16            # a non-null, 16-byte aligned "device pointer" that no call of this file reaches
DECLS = {
    'aspire_jointsm_backward_f32': ['const aspire_repset* q', 'const aspire_repset* c', 'int64_t D', 'int pairing',
                                    'const float* grad_scores', 'float* grad_q_rows', 'float* grad_c_rows', 'void* stream'],
    'aspire_l2sup_scores_f32': ['const aspire_repset* q', 'const aspire_repset* c', 'int64_t D', 'const int32_t* align', 'int weighted',
                                'float* scores', 'void* stream'],
    'aspire_l2sup_backward_f32': ['const aspire_repset* q', 'const aspire_repset* c', 'int64_t D', 'const int32_t* align', 'int weighted',
                                  'const float* grad_scores', 'float* grad_q_rows', 'float* grad_c_rows', 'void* stream'],
}


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'trainside.npz'))


def test_entries_are_declared_exported_and_signed():
    from aspire_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'aspire_hip.h')).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    rs, vp, i = ctypes.POINTER(_lib.RepSet), ctypes.c_void_p, ctypes.c_int
    for name, want in DECLS.items():
        decl = [a.strip() for a in re.search(name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')]
        assert decl == want, name
        assert hasattr(raw, name), f'{name} is not exported'
    assert _lib.SIGNATURES['aspire_jointsm_backward_f32'] == (i, [rs, rs, ctypes.c_int64, i, vp, vp, vp, vp])
    assert _lib.SIGNATURES['aspire_l2sup_scores_f32'] == (i, [rs, rs, ctypes.c_int64, vp, i, vp, vp])
    assert _lib.SIGNATURES['aspire_l2sup_backward_f32'] == (i, [rs, rs, ctypes.c_int64, vp, i, vp, vp, vp, vp])
    assert all(callable(getattr(ops, f)) for f in ('jointsm_backward', 'l2sup_scores', 'l2sup_backward'))
    assert _lib.lib.aspire_abi_version() == 6


def _set(n, ext=8, max_len=8):
    from aspire_amd import _lib
    return _lib.RepSet(FAKE, FAKE, FAKE, n, ext, max_len)


def _long_sets():
    """the forward's row limit, padded and CSR, either side"""
    return (dict(q=_set(3, ext=129)), dict(c=_set(3, ext=129)), dict(q=_set(3, ext=0, max_len=129)), dict(c=_set(3, ext=0, max_len=129)))


def test_jointsm_backward_validation_without_gpu():
    from aspire_amd import _lib
    INVALID, UNSUPPORTED, OK = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED, _lib.ASPIRE_OK
    err = _lib.lib.aspire_last_error
    q, c = _set(3), _set(3)
    base = dict(D=768, pairing=_lib.PAIR_PAIRED, gs=FAKE, gq=FAKE, gc=None)

    def status(q=q, c=c, **kw):
        a = dict(base, **kw)
        return _lib.lib.aspire_jointsm_backward_f32(ctypes.byref(q), ctypes.byref(c), a['D'], a['pairing'], a['gs'], a['gq'], a['gc'], None)

    # (grad_c_rows is null in every call that passes the other checks: it ends in "is null", never in a launch)
    assert status() == INVALID and b'is null' in err()
    assert status(gs=None, gc=FAKE) == INVALID and b'is null' in err()
    assert status(gq=None, gc=FAKE) == INVALID and b'is null' in err()
    assert status(pairing=_lib.PAIR_CROSS, gc=FAKE) == UNSUPPORTED and b'accumulation across pairs' in err()
    with pytest.raises(NotImplementedError, match='ASPIRE_PAIR_PAIRED'):
        _lib.check(status(pairing=_lib.PAIR_CROSS, gc=FAKE))
    assert status(pairing=2) == INVALID and b'bad pairing' in err()
    assert status(c=_set(4)) == INVALID and b'equal batch sizes' in err()
    assert status(D=512) == UNSUPPORTED and b'768' in err()
    null = _lib.lib.aspire_jointsm_backward_f32(None, ctypes.byref(c), 768, _lib.PAIR_PAIRED, FAKE, FAKE, FAKE, None)
    assert null == INVALID and b'null repset' in err()
    for kw in _long_sets():         # (every pointer given: the check sits in front of the launch)
        assert status(gc=FAKE, **kw) == UNSUPPORTED
        assert b'more than 128 sentence rows' in err()
    assert status(q=_set(3, ext=128), c=_set(3, ext=0, max_len=128)) == INVALID and b'is null' in err()
    assert status(q=_set(0), c=_set(0), gs=None, gq=None) == OK           # no pairs: nothing to do, no buffers needed


def test_l2sup_entries_validation_without_gpu():
    from aspire_amd import _lib
    INVALID, UNSUPPORTED, OK = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED, _lib.ASPIRE_OK
    err = _lib.lib.aspire_last_error
    q, c = _set(3), _set(3)

    def fwd(q=q, c=c, D=768, align=FAKE, weighted=0, scores=None):
        return _lib.lib.aspire_l2sup_scores_f32(ctypes.byref(q), ctypes.byref(c), D, align, weighted, scores, None)

    def bwd(q=q, c=c, D=768, align=FAKE, weighted=0, gs=FAKE, gq=FAKE, gc=None):
        return _lib.lib.aspire_l2sup_backward_f32(ctypes.byref(q), ctypes.byref(c), D, align, weighted, gs, gq, gc, None)

    for call, last in ((fwd, 'scores'), (bwd, 'gc')):
        assert call() == INVALID and b'is null' in err()
        assert call(weighted=1) == INVALID and b'is null' in err()
        assert call(align=None, **{last: FAKE}) == INVALID and b'is null' in err()
        assert call(c=_set(4)) == INVALID and b'equal batch sizes' in err()
        assert call(D=512) == UNSUPPORTED and b'768' in err()
        for kw in _long_sets():
            assert call(**kw, **{last: FAKE}) == UNSUPPORTED
            assert b'more than 128 sentence rows' in err()
        assert call(q=_set(3, ext=128), c=_set(3, ext=0, max_len=128)) == INVALID and b'is null' in err()
        assert call(q=_set(0), c=_set(0), align=None) == OK
    assert bwd(gs=None, gc=FAKE) == INVALID and b'is null' in err()
    assert bwd(gq=None, gc=FAKE) == INVALID and b'is null' in err()
    assert _lib.lib.aspire_l2sup_scores_f32(None, ctypes.byref(c), 768, FAKE, 0, FAKE, None) == INVALID and b'null repset' in err()
    assert _lib.lib.aspire_l2sup_backward_f32(ctypes.byref(q), None, 768, FAKE, 0, FAKE, FAKE, FAKE, None) == INVALID and b'null repset' in err()


def _m(*s, dt=torch.float32):
    return torch.empty(*s, device='meta', dtype=dt)


def test_fake_kernels_of_the_four_operators():
    import aspire_amd.torch_ops as to
    i32 = torch.int32
    for name in ('jointsm_pair_scores', 'jointsm_pair_backward', 'l2sup_pair_scores', 'l2sup_pair_backward'):
        assert name in to.OPS and hasattr(torch.ops.aspire, name)
    sets = (_m(4, 8, 768), _m(4, dt=i32), _m(4, 6, 768), _m(4, dt=i32))
    s = torch.ops.aspire.jointsm_pair_scores(*sets)
    assert s.shape == (4,) and s.dtype == torch.float32 and s.device.type == 'meta'
    gq, gc = torch.ops.aspire.jointsm_pair_backward(_m(4), *sets)
    assert gq.shape == (4, 8, 768) and gc.shape == (4, 6, 768) and gq.dtype == gc.dtype == torch.float32
    for weighted in (False, True):
        s = torch.ops.aspire.l2sup_pair_scores(*sets, _m(4, 2, dt=i32), weighted)
        assert s.shape == (4,) and s.dtype == torch.float32 and s.device.type == 'meta'
        gq, gc = torch.ops.aspire.l2sup_pair_backward(_m(4), *sets, _m(4, 2, dt=i32), weighted)
        assert gq.shape == (4, 8, 768) and gc.shape == (4, 6, 768) and gq.dtype == gc.dtype == torch.float32
    with pytest.raises(AssertionError):      # pair_distances.py:46
        torch.ops.aspire.jointsm_pair_scores(_m(3, 8, 768), _m(3, dt=i32), _m(5, 6, 768), _m(5, dt=i32))
    with pytest.raises(AssertionError):      # pair_distances.py:221
        torch.ops.aspire.l2sup_pair_scores(_m(3, 8, 768), _m(3, dt=i32), _m(5, 6, 768), _m(5, dt=i32), _m(3, 2, dt=i32), False)
    # the score operators carry an autograd formula: a fake forward of inputs that require grad is attached to the graph
    for op, extra in ((torch.ops.aspire.jointsm_pair_scores, ()), (torch.ops.aspire.l2sup_pair_scores, (_m(2, 2, dt=i32), True))):
        q = torch.empty(2, 8, 768, device='meta', requires_grad=True)
        c = torch.empty(2, 5, 768, device='meta', requires_grad=True)
        s = op(q, _m(2, dt=i32), c, _m(2, dt=i32), *extra)
        assert s.requires_grad and s.grad_fn is not None
        s.sum().backward()
        assert q.grad.shape == (2, 8, 768) and c.grad.shape == (2, 5, 768)


def test_no_cpu_kernel_behind_the_new_operators():
    import aspire_amd.torch_ops  # noqa: F401
    z, n, a = torch.zeros(1, 2, 768), torch.ones(1, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.jointsm_pair_scores(z, n, z, n)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.jointsm_pair_backward(torch.zeros(1), z, n, z, n)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.l2sup_pair_scores(z, n, z, n, a, False)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.aspire.l2sup_pair_backward(torch.zeros(1), z, n, z, n, a, True)


@pytest.mark.parametrize('fn', ['allpair_masked_dist_l2sup', 'allpair_masked_dist_l2sup_weighted'])
def test_negative_alignment_index_raises_value_error(fn):
    """align_idxs is a host list in the reference: a negative entry is refused on the host, before anything touches a GPU."""
    from aspire_amd import pair_distances as pd
    q = pd.rep_len_tup(embed=torch.zeros(2, 768, 4), abs_lens=[4, 2])
    for bad in ([[0, 1], [-1, 0]], [[0, -3], [1, 1]]):
        with pytest.raises(ValueError, match='negative'):
            getattr(pd, fn)(q, pd.rep_len_ali_tup(embed=torch.zeros(2, 768, 4), abs_lens=[4, 3], align_idxs=bad))
    assert pd.rep_len_ali_tup._fields == ('embed', 'abs_lens', 'align_idxs')


def test_fixture_is_small_and_names_every_case(fixture, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, 'trainside.npz')) < 1000 * 1000
    assert list(fixture['jointsm_cases']) == list(ti.CASES) and list(fixture['l2sup_cases']) == list(ti.L2SUP_CASES)
    for name, spec in ti.CASES.items():
        assert np.array_equal(fixture[f'jointsm_{name}_gs'], ti.jointsm_upstream(name, spec))
        assert fixture[f'jointsm_{name}_ref_err'] > 0 and fixture[f'jointsm_{name}_max_grad'] > 0
    gs = fixture['jointsm_s8_gs']
    assert (gs == 0).sum() == 1 and (gs < 0).any()


# The float64 yardstick is formed again on the machine that runs the test: its own rounding (entries of size <= 10 at 2^-53, whatever
# order the machine's BLAS sums in) may move a deviation of 1e-7 in its tenth digit, so "<= ref_err" is asked up to that.
F64_SLACK = 1e-12


def _valid_err(got, want, lens):
    return max(float(np.max(np.abs(got[b, :n] - want[b, :n]))) for b, n in enumerate(lens))


@pytest.mark.parametrize('name', ti.STORE_JOINTSM_GRADS)
def test_jointsm_yardstick_is_the_reference(fixture, name):
    """The float64 closed-form gradient the GPU test holds the kernel to sits within ref_err of the reference's stored fp32 autograd
    gradient, and the reference's pad rows are exact zeros."""
    q, c, qlens, clens = ti.case_inputs(ti.CASES[name])
    wq, wc = ti.jointsm_grad64(q, c, qlens, clens, fixture[f'jointsm_{name}_gs'])
    gq, gc = fixture[f'jointsm_{name}_grad_q'], fixture[f'jointsm_{name}_grad_c']
    assert gq.shape == q.shape and gc.shape == c.shape and gq.dtype == np.float32
    err = max(_valid_err(gq, wq, qlens), _valid_err(gc, wc, clens))
    print(f'[jointsm {name}] |float64 - reference| {err:.3e}, ref_err {float(fixture[f"jointsm_{name}_ref_err"]):.3e}')
    assert err <= float(fixture[f'jointsm_{name}_ref_err']) + F64_SLACK
    assert abs(max(np.abs(wq).max(), np.abs(wc).max()) - float(fixture[f'jointsm_{name}_max_grad'])) <= 1e-12
    for b, (ql, cl) in enumerate(zip(qlens, clens)):
        assert not gq[b, ql:].any() and not gc[b, cl:].any() and not wq[b, ql:].any() and not wc[b, cl:].any()


@pytest.mark.parametrize('weighted', [0, 1])
@pytest.mark.parametrize('name', list(ti.L2SUP_CASES))
def test_l2sup_yardstick_is_the_reference(fixture, name, weighted):
    q, c, qlens, clens, align, gs = ti.l2sup_inputs(ti.L2SUP_CASES[name])
    key = f'l2sup_{name}_w{weighted}'
    assert np.array_equal(fixture[f'l2sup_{name}_gs'], gs)
    wd, wq, wc = ti.l2sup_ref64(q, c, qlens, clens, align, weighted, gs)
    assert np.max(np.abs(fixture[f'{key}_dist'] - wd)) <= float(fixture[f'{key}_dist_err']) + F64_SLACK
    assert abs(max(np.abs(wq).max(), np.abs(wc).max()) - float(fixture[f'{key}_max_grad'])) <= 1e-12
    for p in ti.L2SUP_CASES[name]['same']:          # coincident aligned rows: distance 0 and, by torch.cdist's rule, no gradient
        assert wd[p] == 0.0 and fixture[f'{key}_dist'][p] == 0.0 and not wq[p].any() and not wc[p].any()
    if name not in ti.STORE_L2SUP_GRADS:
        return
    gq, gc = fixture[f'{key}_grad_q'], fixture[f'{key}_grad_c']
    err = max(_valid_err(gq, wq, qlens), _valid_err(gc, wc, clens))
    print(f'[{key}] |float64 - reference| {err:.3e}, ref_err {float(fixture[f"{key}_ref_err"]):.3e}')
    assert err <= float(fixture[f'{key}_ref_err']) + F64_SLACK
    for b, (ql, cl) in enumerate(zip(qlens, clens)):
        i, j = min(align[b][0], ql - 1), min(align[b][1], cl - 1)
        assert not np.delete(gq[b], i, axis=0).any() and not np.delete(gc[b], j, axis=0).any()       # one row each, pads included


def test_clipped_case_is_the_last_row_case(fixture):
    """e8clip's indices lie beyond the lengths: the reference clips them to e8last's, and gives the same numbers."""
    a, b = ti.L2SUP_CASES['e8last'], ti.L2SUP_CASES['e8clip']
    assert [[min(i, ql - 1), min(j, cl - 1)] for (i, j), ql, cl in zip(b['align'], b['qlens'], b['clens'])] == a['align']
    for w in (0, 1):
        assert np.array_equal(fixture[f'l2sup_e8last_w{w}_dist'], fixture[f'l2sup_e8clip_w{w}_dist'])
