"""CPU: the argument checks the six batched rank entry points share (aspire_amd/csrc/batch_host.h: batch_preamble) and the
workspace checks each of them makes right behind it (place_scratch), through aspire_ot_rank_batch_f32, aspire_l2max_rank_batch_f32,
aspire_l2agg_rank_batch_f32, aspire_dotmax_rank_batch_f32, aspire_jointsm_rank_batch_f32 and aspire_dense_rank_batch_f32.  Every
call here returns its status before any launch: there is no GPU, the pointers are small integers that are never dereferenced
(tests/test_abi_cpu.py: test_batch_entry_validation_without_gpu shows the pattern)."""
import ctypes

import pytest

FAKE = 16            # a non-null, 16-byte aligned "device pointer" that no call of this file reaches
MISALIGNED = 24


def _entries():
    from aspire_amd import _lib
    prm = _lib.OtParams(0.05, 0.9, 1.0, 0)

    def ot(q, c, job_off, max_job, scores, k, top_s, top_i, keys, ws, nbytes):
        return _lib.lib.aspire_ot_rank_batch_f32(ctypes.byref(q), ctypes.byref(c), 768, job_off, max_job, ctypes.byref(prm),
                                                 _lib.OT_SIMILARITY, scores, k, None, top_s, top_i, keys, ws, nbytes, None)

    def l2max(q, c, job_off, max_job, scores, k, top_s, top_i, keys, ws, nbytes):
        return _lib.lib.aspire_l2max_rank_batch_f32(ctypes.byref(q), ctypes.byref(c), 768, job_off, max_job, _lib.CDIST_AUTO,
                                                    scores, k, None, top_s, top_i, keys, ws, nbytes, None)

    def dotmax(q, c, job_off, max_job, scores, k, top_s, top_i, keys, ws, nbytes):
        return _lib.lib.aspire_dotmax_rank_batch_f32(ctypes.byref(q), ctypes.byref(c), 768, job_off, max_job, _lib.SIM_COSINE,
                                                     scores, k, None, top_s, top_i, keys, ws, nbytes, None)

    def jointsm(q, c, job_off, max_job, scores, k, top_s, top_i, keys, ws, nbytes):
        return _lib.lib.aspire_jointsm_rank_batch_f32(ctypes.byref(q), ctypes.byref(c), 768, job_off, max_job, scores, k, None,
                                                      top_s, top_i, keys, ws, nbytes, None)

    def l2agg(q, c, job_off, max_job, scores, k, top_s, top_i, keys, ws, nbytes):
        return _lib.lib.aspire_l2agg_rank_batch_f32(ctypes.byref(q), ctypes.byref(c), 768, job_off, max_job, _lib.CDIST_AUTO,
                                                    _lib.AGG_TOP2, 1.0, scores, k, None, top_s, top_i, keys, ws, nbytes, None)

    # dense takes plain counts and one row matrix: the rep sets' n stand for J and C (an index list has no padded form), and
    # every check in front of the preamble passes
    def dense(q, c, job_off, max_job, scores, k, top_s, top_i, keys, ws, nbytes):
        assert q.ext == 0 and c.ext == 0
        return _lib.lib.aspire_dense_rank_batch_f32(FAKE, 1000, 768, FAKE, q.n, FAKE, c.n, job_off, max_job, _lib.DENSE_L2, scores, k,
                                                    None, top_s, top_i, keys, ws, nbytes, None)

    def dense_ws(q, c, max_job, k):
        return _lib.lib.aspire_dense_rank_batch_workspace_bytes(q._obj.n, c._obj.n, max_job, k)

    return {'ot': (ot, _lib.lib.aspire_ot_rank_batch_workspace_bytes),
            'l2max': (l2max, _lib.lib.aspire_l2max_rank_batch_workspace_bytes),
            'l2agg': (l2agg, _lib.lib.aspire_l2agg_rank_batch_workspace_bytes),
            'dotmax': (dotmax, _lib.lib.aspire_dotmax_rank_batch_workspace_bytes),
            'jointsm': (jointsm, _lib.lib.aspire_jointsm_rank_batch_workspace_bytes),
            'dense': (dense, dense_ws)}


ENTRIES = ['ot', 'l2max', 'l2agg', 'dotmax', 'jointsm', 'dense']
SCRATCH_ONLY = ('l2agg', 'dotmax', 'jointsm', 'dense')       # the workspace is the rank's multi-pass scratch and nothing else


def _csr(n, max_len=8, rows=FAKE):
    from aspire_amd import _lib
    return _lib.RepSet(rows, FAKE, FAKE, n, 0, max_len)


@pytest.mark.parametrize('entry', ENTRIES)
def test_batch_preamble_argument_errors_without_gpu(entry):
    from aspire_amd import _lib
    call, ws_bytes = _entries()[entry]
    INVALID, OK = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_OK
    q, c = _csr(2), _csr(30)
    big = 1 << 30                # more bytes than any layout of this file asks for: the workspace check is not what fails
    ok_args = dict(job_off=FAKE, max_job=20, scores=FAKE, k=10, top_s=FAKE, top_i=FAKE, keys=None, ws=FAKE, nbytes=big)

    def status(q=q, c=c, **kw):
        a = dict(ok_args, **kw)
        return call(q, c, a['job_off'], a['max_job'], a['scores'], a['k'], a['top_s'], a['top_i'], a['keys'], a['ws'], a['nbytes'])

    # padded rep sets (ext != 0), on either side
    padded_q, padded_c = _csr(2), _csr(30)
    padded_q.ext = 8
    padded_c.ext = 8
    if entry != 'dense':         # (index lists into one row matrix: no padded form to refuse)
        assert status(q=padded_q) == INVALID
        assert b'ext == 0' in _lib.lib.aspire_last_error()
        assert status(c=padded_c) == INVALID
    # k > 0 without outputs: neither (top_scores, top_idx) nor keys; half a pair; a negative k
    assert status(top_s=None, top_i=None) == INVALID
    assert b'keys' in _lib.lib.aspire_last_error()
    assert status(top_s=None) == INVALID
    assert status(top_i=None) == INVALID
    assert status(k=-1) == INVALID
    # ... which is checked before "no jobs"
    assert status(q=_csr(0), top_s=None, top_i=None) == INVALID
    # null job_off, max_job beyond the candidate count, negative max_job
    assert status(job_off=None) == INVALID
    assert b'job_off' in _lib.lib.aspire_last_error()
    assert status(max_job=31) == INVALID
    assert status(max_job=-1) == INVALID
    # null scores with candidates to score
    assert status(scores=None) == INVALID
    assert b'scores' in _lib.lib.aspire_last_error()
    # no jobs: nothing to do, whatever else is null (k > 0 with outputs, and k == 0 without)
    assert status(q=_csr(0), job_off=None, scores=None, ws=None, nbytes=0) == OK
    assert status(q=_csr(0), c=_csr(0), job_off=None, scores=None, ws=None, nbytes=0, keys=FAKE, top_s=None, top_i=None) == OK
    assert status(q=_csr(0), k=0, top_s=None, top_i=None, job_off=None, scores=None, ws=None, nbytes=0) == OK


@pytest.mark.parametrize('entry', ENTRIES)
def test_batch_workspace_checks_without_gpu(entry):
    """a pool beyond one 4096-key chunk: every entry's workspace holds the rank's multi-pass scratch (the whole of it for the four
    SCRATCH_ONLY entries); the *workspace too small* message is pinned character for character, with the entry's own query function"""
    from aspire_amd import _lib
    call, ws_bytes = _entries()[entry]
    INVALID = _lib.ASPIRE_ERR_INVALID_ARG
    q, c = _csr(2), _csr(9000)
    for k in (100, 2000):        # multi-pass winners, full sort
        need = ws_bytes(ctypes.byref(q), ctypes.byref(c), 5000, k)
        assert need >= _lib.lib.aspire_topk_workspace_bytes(2, 5000, k) > 0 and need % 16 == 0
        if entry in SCRATCH_ONLY:
            assert need == _lib.lib.aspire_topk_workspace_bytes(2, 5000, k)
        assert call(q, c, FAKE, 5000, FAKE, k, FAKE, FAKE, None, FAKE, need - 16) == INVALID
        assert _lib.lib.aspire_last_error() == (f'workspace too small: {need - 16} bytes given, '
                                                f'aspire_{entry}_rank_batch_workspace_bytes says {need}').encode()
        assert call(q, c, FAKE, 5000, FAKE, k, FAKE, FAKE, None, None, need) == INVALID
        assert call(q, c, FAKE, 5000, FAKE, k, FAKE, FAKE, None, MISALIGNED, need + 64) == INVALID
        assert b'aligned' in _lib.lib.aspire_last_error()
    # the rank scratch is asked for by max_job, not by the candidate count: short jobs need none of it
    assert _lib.lib.aspire_dotmax_rank_batch_workspace_bytes(ctypes.byref(q), ctypes.byref(c), 4096, 100) == 0
    assert ws_bytes(ctypes.byref(q), ctypes.byref(c), 4096, 100) <= ws_bytes(ctypes.byref(q), ctypes.byref(c), 5000, 100) - \
        _lib.lib.aspire_topk_workspace_bytes(2, 5000, 100)
    # no jobs or no candidates: no workspace
    assert ws_bytes(ctypes.byref(_csr(0)), ctypes.byref(c), 0, 10) == 0
    assert ws_bytes(ctypes.byref(q), ctypes.byref(_csr(0)), 0, 10) == 0
