"""CPU: which kernel family a call takes.  The decision functions of aspire_amd/csrc/forms.hip are pure functions of the rep sets'
host fields, of what the call asked for and of the diagnostic switches, and aspire_debug_score_form renders their answer as text
without running anything -- so the table of tests/dispatch_cases.py is asserted here without a GPU.  The GPU tests pin forms and
compare bits; this one catches a default call that drifted onto another family."""
import ctypes
import os
import re

import pytest

import dispatch_cases as dc

SWITCHES = ('OT_FORM', 'COST_PATH', 'SINKHORN', 'GEMM', 'FUSED_VALU', 'FUSED_NOSOLVE', 'FUSED_NOSELF', 'FUSED_SOLVE16', 'COST1_BLOCKS')


def _switches():
    from aspire_amd import _lib
    buf = ctypes.create_string_buffer(64)
    out = {}
    for k in SWITCHES:
        _lib.check(_lib.lib.aspire_debug_get(k.encode(), buf, len(buf)))
        out[k] = buf.value
    return out


@pytest.mark.parametrize('case', dc.CASES, ids=[c[0] for c in dc.CASES])
def test_default_and_pinned_calls_take_the_recorded_family(case):
    _, kind, q, c, options, text = case
    before = _switches()
    assert dc.form_text(kind, q, c, options) == text
    assert _switches() == before          # every switch the case set is back


def test_case_ids_are_unique():
    ids = [c[0] for c in dc.CASES]
    assert len(ids) == len(set(ids))


def test_table_reaches_every_family_and_stage_kernel():
    """one case per branch of the entry points' switches and of the two stage launchers"""
    by_kind = {}
    for _, kind, _, _, _, text in dc.CASES:
        by_kind.setdefault(kind, set()).add(re.sub(r'^(tables\+|qbox\+)+', '', text.split()[0]))
    assert by_kind['l2agg'] >= {'generic', 'gram-planes', 'gram', 'stream16', 'fused-stream', 'tiles', 'tiles+generic'}
    assert by_kind['ot'] >= {'none', 'generic', 'fused-inbox', 'fused-qbox', 'chunk', 'chunk+generic', 'one-wave', 'tiles', 'tiles+generic'}
    assert by_kind['ot_batch'] >= {'none', 'generic', 'chunk', 'rec16', 'fused-self', 'fused-tables', 'one-wave', 'hybrid', 'tiles',
                                   'tiles+generic'}
    assert by_kind['l2max_batch'] >= {'chunk', 'rec16', 'fused-self', 'fused-tables', 'hybrid', 'stream16', 'tiles', 'generic'}
    for cost in ('gram', 'tile', 'cost1', 'tile16', 'cost1-sub', 'cost'):
        assert any(re.search(rf'cost={cost}( |$)', c[5]) for c in dc.CASES), cost
    for solve in ('wave', 'block1x8+repair', 'block4x4+repair', 'block4x4', 'block4x6+repair', 'block4x8+repair', 'block16x2+repair',
                  'block16x3+repair', 'block16x4+repair', 'block16x5+repair', 'block16x6+repair', 'block16x7+repair', 'block16x8+repair'):
        assert any(c[5].endswith('solve=' + solve) for c in dc.CASES), solve


def test_fused_solve16_does_not_change_the_family():
    """FUSED_SOLVE16 picks between two solves of ONE family (fused.hip: solve16_wanted, process state and a counter of its own)"""
    got = {dc.form_text('ot_batch', (20, 8), (20000, 8), dict(pins=p)) for p in ({}, dict(FUSED_SOLVE16=0), dict(FUSED_SOLVE16=1))}
    assert got == {'fused-self'}


def _solver_family(text):
    head = re.sub(r'^(tables\+|qbox\+)+', '', text.split()[0])
    return 'fused' if head.startswith('fused-') else head


def test_short_csr_pairs_get_one_solver_family_alone_and_in_a_batch():
    """Documents of <= 8 rows, CSR, up to kOneMaxPairs = 8192 pairs: a pool scored in a call of its own (1 x n) and as the only job
    of a batch (the same n pairs) get the same solver family -- one wave per pair while the call is latency bound, the fused
    kernel once it streams -- with ONE window where the two entry points part, recorded here as it is: a single-pool call of one
    query streams from kStreamMinGroups1 = 640 groups of four, a batch from kStreamMinGroupsBatch = 512, so n = 2045 .. 2556 is
    one-wave alone and fused in a batch.  Both thresholds are measured (forms.hip); the refactor keeps them."""
    for n in (1, 2, 50, 511, 512, 1000, 2044, 2557, 2560, 4096, 8189, 8192):
        alone = _solver_family(dc.form_text('ot', (1, 8), (n, 8), {}))
        batch = _solver_family(dc.form_text('ot_batch', (1, 8), (n, 8), {}))
        assert alone == batch == ('one-wave' if n <= 2044 else 'fused'), (n, alone, batch)
    for n in (2045, 2300, 2556):
        assert _solver_family(dc.form_text('ot', (1, 8), (n, 8), {})) == 'one-wave'
        assert _solver_family(dc.form_text('ot_batch', (1, 8), (n, 8), {})) == 'fused'
    # split into several jobs the same pairs stay below the batch threshold longer, and take the same one-wave kernel
    for jobs, n in ((2, 2000), (4, 2032), (8, 1000)):
        assert _solver_family(dc.form_text('ot_batch', (jobs, 8), (n, 8), {})) == 'one-wave'


def test_export_rejects_what_it_cannot_answer():
    from aspire_amd import _lib
    q, c = _lib.RepSet(16, 16, 16, 1, 0, 8, None, None), _lib.RepSet(16, 16, 16, 50, 0, 8, None, None)
    prm = _lib.OtParams(0.05, 0.9, 1.0, 0, 0)
    buf = ctypes.create_string_buffer(128)
    call = lambda kind, prm_ref, n: _lib.lib.aspire_debug_score_form(kind, ctypes.byref(q), ctypes.byref(c), _lib.PAIR_CROSS, prm_ref, 0, 0, buf, n)
    assert call(_lib.FORM_OT, ctypes.byref(prm), len(buf)) == _lib.ASPIRE_OK and buf.value == b'one-wave'
    assert call(_lib.FORM_L2AGG, None, len(buf)) == _lib.ASPIRE_OK and buf.value == b'tiles'       # the max-sim kinds read no params
    assert call(_lib.FORM_OT, None, len(buf)) == _lib.ASPIRE_ERR_INVALID_ARG
    assert call(7, ctypes.byref(prm), len(buf)) == _lib.ASPIRE_ERR_INVALID_ARG
    assert call(_lib.FORM_OT, ctypes.byref(prm), 4) == _lib.ASPIRE_ERR_INVALID_ARG                # "one-wave" needs 9 bytes


def test_form_switches_are_read_in_forms_hip_only():
    """the form decisions read tuning() inside forms.hip: no other unit asks for OT_FORM, COST_PATH, SINKHORN or FUSED_NOSELF"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, 'aspire_amd', 'csrc')
    for f in sorted(os.listdir(csrc)):
        if f.endswith(('.hip', '.h')) and f != 'forms.hip':
            text = open(os.path.join(csrc, f)).read()
            for field in ('ot_form', 'cost_path', 'sinkhorn_form', 'fused_noself'):
                assert not re.search(r'tuning\(\)\s*\.\s*' + field, text), (f, field)
