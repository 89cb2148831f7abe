"""CPU: the batched score + rank entry of the sibling aggregations 'l2top2' / 'l2attention' without a GPU -- the two C-ABI entries
(declared, exported, signed), the METHODS rows and what _batch_call makes of them, and the argument / workspace checks of
aspire_l2agg_rank_batch_f32 (none of these calls reaches a launch)."""
import ctypes
import os
import re

import pytest

FAKE = 16            # a non-null, 16-byte aligned "device pointer" that no call of this file reaches
NEW = ('aspire_l2agg_rank_batch_workspace_bytes', 'aspire_l2agg_rank_batch_f32')


def test_new_entries_are_declared_exported_and_signed():
    from aspire_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'aspire_hip.h')).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', hdr), f'{name} is not declared in aspire_hip.h'
        assert hasattr(raw, name), f'{name} is not exported'
        assert name in _lib.SIGNATURES
    # the rank entry's parameters are aspire_l2max_rank_batch_f32's with `int agg, double temp` behind cdist_mode
    decl = lambda fn: [a.strip() for a in re.search(fn + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')]
    l2max = decl('aspire_l2max_rank_batch_f32')
    at = l2max.index('int cdist_mode') + 1
    assert decl('aspire_l2agg_rank_batch_f32') == l2max[:at] + ['int agg', 'double temp'] + l2max[at:]
    sig = _lib.SIGNATURES['aspire_l2max_rank_batch_f32'][1]
    assert _lib.SIGNATURES['aspire_l2agg_rank_batch_f32'] == (ctypes.c_int, sig[:at] + [ctypes.c_int, ctypes.c_double] + sig[at:])
    assert _lib.SIGNATURES['aspire_l2agg_rank_batch_workspace_bytes'] == _lib.SIGNATURES['aspire_l2max_rank_batch_workspace_bytes']
    assert ops._RANK_BATCH['l2agg'] == (_lib.lib.aspire_l2agg_rank_batch_f32, _lib.lib.aspire_l2agg_rank_batch_workspace_bytes)
    assert callable(ops.l2agg_rank_batch)


def test_methods_rows_and_batch_call():
    from aspire_amd import _lib, ops, scorer
    assert scorer.METHODS['l2top2'].batch({}, False) == ('l2agg', ops.l2agg_rank_batch, {'agg': _lib.AGG_TOP2})
    assert scorer.METHODS['l2attention'].batch({'cdatt_sm_temp': 0.5}, False) == (
        'l2agg', ops.l2agg_rank_batch, {'agg': _lib.AGG_ATTENTION, 'temp': 0.5})
    assert scorer.METHODS['l2attention'].batch({}, False)[2] == {'agg': _lib.AGG_ATTENTION, 'temp': 1.0}
    for name in ('l2top2', 'l2attention'):
        row = scorer.METHODS[name]
        assert name in scorer.BATCH_METHODS and name not in scorer.DOT_METHODS
        assert row.deterministic is None and row.schedule is True and callable(row.cross)
    assert scorer._batch_call(2, [5, 3], 4, {}, 'l2top2', False)[3:] == (5, 4)
    assert scorer._batch_call(2, [5, 3], None, {'cdatt_sm_temp': 0.2}, 'l2attention', False) == (
        'l2agg', ops.l2agg_rank_batch, {'agg': _lib.AGG_ATTENTION, 'temp': 0.2}, 5, 5)
    # deterministic is not built for these rows: the text rank_pool raises
    for name in ('l2top2', 'l2attention'):
        with pytest.raises(ValueError, match="deterministic=True is built for method 'ot'"):
            scorer._batch_call(2, [5, 3], 4, {}, name, True)
        with pytest.raises(ValueError, match="deterministic=True is built for method 'ot'"):
            scorer.rank_pool([], [], method=name, deterministic=True)
        with pytest.raises(ValueError, match="deterministic=True is built for method 'ot'"):
            scorer.rank_pools([[]], [[]], method=name, deterministic=True)
    # ... and the rows that have it are untouched
    assert scorer._batch_call(2, [5, 3], 4, {}, 'jointsm', True) == ('jointsm', ops.jointsm_rank_batch, {}, 5, 4)
    assert scorer._batch_call(1, [0], None, None, 'l2max', True)[2:] == ({'one_form': True}, 0, 0)
    with pytest.raises(ValueError, match='Unknown aggregation: l2top3'):
        scorer._batch_call(1, [1], None, None, 'l2top3', False)
    assert scorer.rank_pools([], [], method='l2top2') == []


def _csr(n, max_len=8):
    from aspire_amd import _lib
    return _lib.RepSet(FAKE, FAKE, FAKE, n, 0, max_len)


def test_batch_entry_validation_without_gpu():
    from aspire_amd import _lib
    INVALID, UNSUPPORTED, OK = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED, _lib.ASPIRE_OK
    err = _lib.lib.aspire_last_error
    q, c = _csr(2), _csr(30)
    ok_args = dict(D=768, job_off=FAKE, max_job=20, cdist=_lib.CDIST_AUTO, agg=_lib.AGG_TOP2, temp=1.0, scores=None, k=10,
                   top_s=FAKE, top_i=FAKE, keys=None, ws=FAKE, nbytes=1 << 20)

    def status(q=q, c=c, **kw):
        a = dict(ok_args, **kw)
        return _lib.lib.aspire_l2agg_rank_batch_f32(ctypes.byref(q), ctypes.byref(c), a['D'], a['job_off'], a['max_job'], a['cdist'],
                                                    a['agg'], a['temp'], a['scores'], a['k'], None, a['top_s'], a['top_i'], a['keys'],
                                                    a['ws'], a['nbytes'], None)

    # (scores is null in every call: a call that passed every other check ends in the preamble's "null scores", never in a launch)
    assert status() == INVALID and b'null scores' in err()
    assert status(agg=_lib.AGG_ATTENTION, temp=0.2) == INVALID and b'null scores' in err()
    for mode in (_lib.CDIST_DIRECT, _lib.CDIST_MM, _lib.CDIST_AUTO | 0x100, _lib.CDIST_MM | 0x200, _lib.CDIST_DIRECT | 0x300):
        assert status(cdist=mode) == INVALID and b'null scores' in err()           # accepted: ONE_FORM / CENTER are no-ops
    assert status(cdist=3) == INVALID and b'cdist_mode' in err()
    assert status(agg=7) == INVALID and b'bad aggregation' in err()
    assert status(agg=-1) == INVALID and b'bad aggregation' in err()
    assert status(agg=_lib.AGG_MAX) == INVALID and b'aspire_l2max_rank_batch_f32' in err()
    assert status(agg=_lib.AGG_ATTENTION, temp=0.0) == INVALID and b'temperature' in err()
    assert status(agg=_lib.AGG_ATTENTION, temp=-1.0) == INVALID and b'temperature' in err()
    assert status(agg=_lib.AGG_TOP2, temp=0.0) == INVALID and b'null scores' in err()      # temp is ATTENTION's
    padded_q, padded_c = _csr(2), _csr(30)
    padded_q.ext = 8
    padded_c.ext = 8
    assert status(q=padded_q) == INVALID and b'ext == 0' in err()
    assert status(c=padded_c) == INVALID and b'ext == 0' in err()
    assert status(c=_csr(30, max_len=129)) == UNSUPPORTED
    assert err() == b'documents with more than 128 sentence rows are not supported (got 129)'
    assert status(q=_csr(2, max_len=129)) == UNSUPPORTED
    assert status(c=_csr(30, max_len=128)) == INVALID and b'null scores' in err()
    assert status(D=512) == UNSUPPORTED and b'768' in err()
    # the preamble's own cases
    assert status(top_s=None, top_i=None) == INVALID and b'keys' in err()
    assert status(k=-1) == INVALID
    assert status(job_off=None) == INVALID and b'job_off' in err()
    assert status(max_job=31) == INVALID
    assert status(q=_csr(0), job_off=None, ws=None, nbytes=0) == OK
    assert status(q=_csr(0), k=0, top_s=None, top_i=None, job_off=None, ws=None, nbytes=0) == OK
    null = _lib.lib.aspire_l2agg_rank_batch_f32(None, ctypes.byref(c), 768, FAKE, 20, 0, _lib.AGG_TOP2, 1.0, None, 10, None, FAKE, FAKE,
                                                None, FAKE, 16, None)
    assert null == INVALID


def test_workspace_is_the_rank_scratch_only():
    from aspire_amd import _lib
    ws_bytes = _lib.lib.aspire_l2agg_rank_batch_workspace_bytes
    q, c = _csr(2), _csr(9000)
    for k in (100, 2000):
        need = ws_bytes(ctypes.byref(q), ctypes.byref(c), 5000, k)
        assert need == _lib.lib.aspire_topk_workspace_bytes(2, 5000, k) > 0 and need % 16 == 0
        args = (ctypes.byref(q), ctypes.byref(c), 768, FAKE, 5000, 0, _lib.AGG_TOP2, 1.0, FAKE, k, None, FAKE, FAKE, None)
        assert _lib.lib.aspire_l2agg_rank_batch_f32(*args, FAKE, need - 16, None) == _lib.ASPIRE_ERR_INVALID_ARG
        assert b'aspire_l2agg_rank_batch_workspace_bytes' in _lib.lib.aspire_last_error()
        assert _lib.lib.aspire_l2agg_rank_batch_f32(*args, None, need, None) == _lib.ASPIRE_ERR_INVALID_ARG
        assert _lib.lib.aspire_l2agg_rank_batch_f32(*args, 24, need + 64, None) == _lib.ASPIRE_ERR_INVALID_ARG
        assert b'aligned' in _lib.lib.aspire_last_error()
    assert ws_bytes(ctypes.byref(q), ctypes.byref(c), 4096, 100) == 0          # pools of <= 4096: none
    assert ws_bytes(ctypes.byref(q), ctypes.byref(c), 5000, 0) == 0            # k = 0: scores only
    assert ws_bytes(ctypes.byref(_csr(0)), ctypes.byref(c), 0, 10) == 0
    assert ws_bytes(ctypes.byref(q), ctypes.byref(_csr(0)), 0, 10) == 0
    assert ws_bytes(None, ctypes.byref(c), 5000, 10) == 0
