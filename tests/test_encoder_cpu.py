"""The encoder's fall-back rule (aspire_amd/encoder.py: run_checked) without a GPU: a fake forward records the diagnostic switches
(aspire_debug_get) it runs under, fake status / range checks say what the GPU would have said."""
import ctypes
import warnings

import pytest

_KEYS = ('GEMM_LN', 'GEMM', 'ATTN')


def _switches():
    from aspire_amd import _lib
    buf = ctypes.create_string_buffer(64)
    out = {}
    for k in _KEYS:
        assert _lib.lib.aspire_debug_get(k.encode(), buf, len(buf)) == _lib.ASPIRE_OK
        out[k] = buf.value.decode()
    return out


def _rule(status_says, finite_says):
    """run_checked over a fake forward.  status_says / finite_says: what status() / outputs_finite() answer, one call each at the
    most (a further call fails).  Returns (result, the switches of every run, the order of the calls, the warning texts)."""
    from aspire_amd.encoder import run_checked
    runs, calls = [], []
    status_says, finite_says = list(status_says), list(finite_says)

    def run():
        calls.append('run')
        runs.append(_switches())
        return len(runs)

    def status():
        calls.append('status')
        return status_says.pop(0)

    def outputs_finite(r):
        assert r == len(runs)                      # the check sees the latest run's result
        calls.append('finite')
        return finite_says.pop(0)

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        out = run_checked(run, outputs_finite, 'Model.forward', status)
    assert not status_says and not finite_says     # each check consulted exactly once
    return out, runs, calls, [str(w.message) for w in caught]


LN_MSG = 'Model.forward: the fused GEMM + LayerNorm exchange timed out; encoding again with ASPIRE_HIP_GEMM_LN=off'
FR_MSG = ('Model.forward: non-finite reps on the fp16-plane encoder path (an activation beyond 65504); encoding again with '
          'ASPIRE_HIP_GEMM=bf16x3, ASPIRE_HIP_ATTN=f32')


@pytest.mark.parametrize('outer', [{}, {'GEMM': 'planes', 'GEMM_LN': 'on', 'ATTN': 'gemm'}])
def test_run_checked_reruns_once_per_rule_under_its_pin(outer):
    from aspire_amd._lib import pinned
    before = _switches()
    with pinned(**outer):
        base = _switches()
        # all well: one run, no warning
        assert _rule([0], [True]) == (1, [base], ['run', 'status', 'finite'], [])
        # the LayerNorm exchange timed out: once more with GEMM_LN=off, the rest as set around the call
        out, runs, calls, msgs = _rule([1], [True])
        assert out == 2 and runs == [base, dict(base, GEMM_LN='off')]
        assert calls == ['run', 'status', 'run', 'finite'] and msgs == [LN_MSG]
        # non-finite output: once more on the full-range kernels
        out, runs, calls, msgs = _rule([0], [False])
        assert out == 2 and runs == [base, dict(base, GEMM='bf16x3', ATTN='f32')]
        assert calls == ['run', 'status', 'finite', 'run'] and msgs == [FR_MSG]
        # both, in that order, each once: the status is not read again after the re-run, the full-range run is not checked, and it
        # runs outside the GEMM_LN pin
        out, runs, calls, msgs = _rule([1], [False])
        assert out == 3 and runs == [base, dict(base, GEMM_LN='off'), dict(base, GEMM='bf16x3', ATTN='f32')]
        assert calls == ['run', 'status', 'run', 'finite', 'run'] and msgs == [LN_MSG, FR_MSG]
        assert _switches() == base                 # every switch back to what the caller had set
    assert _switches() == before


def test_run_checked_restores_the_switches_when_a_rerun_raises():
    from aspire_amd.encoder import run_checked
    before = _switches()
    n = []

    def run():
        n.append(1)
        if len(n) > 1:
            raise RuntimeError('re-run failed')
        return None

    with pytest.warns(UserWarning, match='timed out'):
        with pytest.raises(RuntimeError):
            run_checked(run, lambda r: True, 'Model', lambda: 1)
    assert _switches() == before
