"""CPU: the jointsm scorer's surface without a GPU -- the three C-ABI entries (declared, exported, signed; ABI still 6), the
argument and workspace checks of aspire_jointsm_rank_batch_f32 (the cases of tests/test_batch_preamble_cpu.py), the METHODS row,
the fixture's self-check against the float64 closed form, and the host logic of aspire_amd/polyenc.py on a stubbed `ops`."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from jointsm_inputs import case_inputs, closed_form, pool_inputs, spec_of  # noqa: E402

FAKE = 16            # a non-null, 16-byte aligned "device pointer" that no call of this file reaches
MISALIGNED = 24
NEW = ('aspire_jointsm_scores_f32', 'aspire_jointsm_rank_batch_workspace_bytes', 'aspire_jointsm_rank_batch_f32')


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'jointsm.npz'))


def test_new_entries_are_declared_exported_and_signed():
    from aspire_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'aspire_hip.h')).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', hdr), f'{name} is not declared in aspire_hip.h'
        assert hasattr(raw, name), f'{name} is not exported'
        assert name in _lib.SIGNATURES
    # the rank entry's parameters are aspire_dotmax_rank_batch_f32's without `sim`
    decl = lambda fn: [a.strip() for a in re.search(fn + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')]
    assert decl('aspire_jointsm_rank_batch_f32') == [a for a in decl('aspire_dotmax_rank_batch_f32') if a != 'int sim']
    assert _lib.SIGNATURES['aspire_jointsm_rank_batch_f32'][1] == [
        a for i, a in enumerate(_lib.SIGNATURES['aspire_dotmax_rank_batch_f32'][1]) if i != 5]
    assert len(_lib.SIGNATURES['aspire_jointsm_scores_f32'][1]) == len(decl('aspire_jointsm_scores_f32')) == 7
    assert re.search(r'#define ASPIRE_ABI_VERSION 6\b', hdr) and _lib.lib.aspire_abi_version() == 6


def test_scores_entry_argument_errors_without_gpu():
    from aspire_amd import _lib
    call = _lib.lib.aspire_jointsm_scores_f32
    q, c = _lib.RepSet(FAKE, FAKE, FAKE, 2, 4, 4), _lib.RepSet(FAKE, FAKE, FAKE, 3, 4, 4)
    assert call(ctypes.byref(q), ctypes.byref(c), 768, _lib.PAIR_PAIRED, FAKE, None, None) == _lib.ASPIRE_ERR_INVALID_ARG      # 2 vs 3
    assert call(ctypes.byref(q), ctypes.byref(c), 512, _lib.PAIR_CROSS, FAKE, None, None) == _lib.ASPIRE_ERR_UNSUPPORTED
    assert b'768' in _lib.lib.aspire_last_error()
    assert call(ctypes.byref(q), ctypes.byref(c), 768, 7, FAKE, None, None) == _lib.ASPIRE_ERR_INVALID_ARG
    assert call(ctypes.byref(q), ctypes.byref(c), 768, _lib.PAIR_CROSS, None, None, None) == _lib.ASPIRE_ERR_INVALID_ARG
    assert b'scores' in _lib.lib.aspire_last_error()
    long_c = _lib.RepSet(FAKE, FAKE, FAKE, 3, 0, 129)
    assert call(ctypes.byref(q), ctypes.byref(long_c), 768, _lib.PAIR_CROSS, FAKE, None, None) == _lib.ASPIRE_ERR_UNSUPPORTED
    assert b'128' in _lib.lib.aspire_last_error()
    # pair_softmax [P, q.ext, c.ext] needs padded extents on both sides
    csr = _lib.RepSet(FAKE, FAKE, FAKE, 3, 0, 4)
    assert call(ctypes.byref(q), ctypes.byref(csr), 768, _lib.PAIR_CROSS, FAKE, FAKE, None) == _lib.ASPIRE_ERR_INVALID_ARG
    assert b'padded' in _lib.lib.aspire_last_error()
    # nothing to score: fine, whatever is null
    empty = _lib.RepSet(0, 0, 0, 0, 0, 0)
    assert call(ctypes.byref(empty), ctypes.byref(c), 768, _lib.PAIR_CROSS, None, None, None) == _lib.ASPIRE_OK


def _rank(q, c, job_off, max_job, scores, k, top_s, top_i, keys, ws, nbytes):
    from aspire_amd import _lib
    return _lib.lib.aspire_jointsm_rank_batch_f32(ctypes.byref(q), ctypes.byref(c), 768, job_off, max_job, scores, k, None, top_s,
                                                  top_i, keys, ws, nbytes, None)


def _csr(n, max_len=8, rows=FAKE):
    from aspire_amd import _lib
    return _lib.RepSet(rows, FAKE, FAKE, n, 0, max_len)


def test_batch_preamble_argument_errors_without_gpu():
    from aspire_amd import _lib
    INVALID, OK = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_OK
    q, c = _csr(2), _csr(30)
    big = 1 << 30
    ok_args = dict(job_off=FAKE, max_job=20, scores=FAKE, k=10, top_s=FAKE, top_i=FAKE, keys=None, ws=FAKE, nbytes=big)

    def status(q=q, c=c, **kw):
        a = dict(ok_args, **kw)
        return _rank(q, c, a['job_off'], a['max_job'], a['scores'], a['k'], a['top_s'], a['top_i'], a['keys'], a['ws'], a['nbytes'])

    padded_q, padded_c = _csr(2), _csr(30)
    padded_q.ext = 8
    padded_c.ext = 8
    assert status(q=padded_q) == INVALID
    assert b'ext == 0' in _lib.lib.aspire_last_error()
    assert status(c=padded_c) == INVALID
    assert status(top_s=None, top_i=None) == INVALID
    assert b'keys' in _lib.lib.aspire_last_error()
    assert status(top_s=None) == INVALID
    assert status(top_i=None) == INVALID
    assert status(k=-1) == INVALID
    assert status(q=_csr(0), top_s=None, top_i=None) == INVALID
    assert status(job_off=None) == INVALID
    assert b'job_off' in _lib.lib.aspire_last_error()
    assert status(max_job=31) == INVALID
    assert status(max_job=-1) == INVALID
    assert status(scores=None) == INVALID
    assert b'scores' in _lib.lib.aspire_last_error()
    assert status(q=_csr(0), job_off=None, scores=None, ws=None, nbytes=0) == OK
    assert status(q=_csr(0), c=_csr(0), job_off=None, scores=None, ws=None, nbytes=0, keys=FAKE, top_s=None, top_i=None) == OK
    assert status(q=_csr(0), k=0, top_s=None, top_i=None, job_off=None, scores=None, ws=None, nbytes=0) == OK
    # D != 768 and documents beyond 128 rows are refused before anything else
    assert _lib.lib.aspire_jointsm_rank_batch_f32(ctypes.byref(q), ctypes.byref(c), 512, FAKE, 20, FAKE, 10, None, FAKE, FAKE, None, FAKE,
                                                  big, None) == _lib.ASPIRE_ERR_UNSUPPORTED
    assert status(c=_csr(30, max_len=129)) == _lib.ASPIRE_ERR_UNSUPPORTED


def test_batch_workspace_checks_without_gpu():
    """a pool beyond one 4096-key chunk: the workspace is the rank's multi-pass scratch, all of it (as dotmax's)"""
    from aspire_amd import _lib
    ws_bytes = _lib.lib.aspire_jointsm_rank_batch_workspace_bytes
    INVALID = _lib.ASPIRE_ERR_INVALID_ARG
    q, c = _csr(2), _csr(9000)
    for k in (100, 2000):
        need = ws_bytes(ctypes.byref(q), ctypes.byref(c), 5000, k)
        assert need == _lib.lib.aspire_topk_workspace_bytes(2, 5000, k) > 0 and need % 16 == 0
        assert _rank(q, c, FAKE, 5000, FAKE, k, FAKE, FAKE, None, FAKE, need - 16) == INVALID
        assert b'workspace too small' in _lib.lib.aspire_last_error()
        assert _rank(q, c, FAKE, 5000, FAKE, k, FAKE, FAKE, None, None, need) == INVALID
        assert _rank(q, c, FAKE, 5000, FAKE, k, FAKE, FAKE, None, MISALIGNED, need + 64) == INVALID
        assert b'aligned' in _lib.lib.aspire_last_error()
    assert ws_bytes(ctypes.byref(q), ctypes.byref(c), 4096, 100) == 0
    assert ws_bytes(ctypes.byref(_csr(0)), ctypes.byref(c), 0, 10) == 0
    assert ws_bytes(ctypes.byref(q), ctypes.byref(_csr(0)), 0, 10) == 0
    from aspire_amd import ops
    assert ops._RANK_BATCH['jointsm'] == (_lib.lib.aspire_jointsm_rank_batch_f32, ws_bytes)


def test_methods_row():
    from aspire_amd import scorer
    row = scorer.METHODS['jointsm']
    assert 'jointsm' in scorer.BATCH_METHODS and 'jointsm' not in scorer.DOT_METHODS
    assert row.deterministic == 'any' and row.schedule is False and row.sim is None and callable(row.cross)
    entry, wrapper, kw = row.batch({}, True)
    from aspire_amd import ops
    assert entry == 'jointsm' and wrapper is ops.jointsm_rank_batch and kw == {}
    # deterministic=True is accepted by the batched call's checks ...
    assert scorer._batch_call(1, [0], None, None, 'jointsm', True) == (entry, wrapper, kw, 0, 0)
    assert scorer._batch_call(2, [5, 3], 4, {}, 'jointsm', True)[3:] == (5, 4)
    # ... and `schedule` is treated exactly as for 'cosine': an unknown one is rejected, a known non-default one ignored (both reach
    # the device upload, which is what fails here without a GPU)
    for method in ('cosine', 'jointsm'):
        for schedule, exc in (('bogus', ValueError), ('batch', None)):
            if torch.cuda.is_available():
                if exc is not None:
                    with pytest.raises(exc, match='Unknown schedule'):
                        scorer.score_pool([np.zeros((2, 768), np.float32)], [np.ones((1, 768), np.float32)], method=method, schedule=schedule)
                continue
            with pytest.raises(RuntimeError, match='no CPU fallback'):      # from_list comes first, for every method
                scorer.score_pool([np.zeros((2, 768), np.float32)], [np.ones((1, 768), np.float32)], method=method, schedule=schedule)
    assert scorer.METHODS['cosine'].schedule is False


def test_fixture_regenerates_and_reference_meets_its_own_bound(fixture):
    """the float64 closed form on the inputs regenerated from the stored seeds is within the stored reference error of the stored
    reference scores: the seeds give the generator's inputs back, and the bound the GPU tests double is the reference's own"""
    names = [str(n) for n in fixture['cases']]
    shapes = {tuple(int(x) for x in fixture[f'{n}_shape'][1:]) for n in names}
    assert {(1, 1), (8, 8), (7, 6), (20, 30), (100, 128), (128, 128)} <= shapes
    assert {float(fixture[f'{n}_scale']) for n in names} == {0.3, 0.6, 1.0}
    assert any(int(fixture[f'{n}_dup']) >= 0 for n in names)
    lo, hi = np.inf, 0.0
    for name in names:
        q, c, qlens, clens = case_inputs(spec_of(fixture, name))
        assert qlens == fixture[f'{name}_qlens'].tolist() and clens == fixture[f'{name}_clens'].tolist()
        assert all(not q[b, ql:].any() and not c[b, cl:].any() for b, (ql, cl) in enumerate(zip(qlens, clens)))      # zero pad rows
        want, want_sm = closed_form(q, c, qlens, clens)
        got = fixture[f'{name}_scores']
        err = np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))
        assert err <= float(fixture[f'{name}_ref_err']) * (1 + 1e-9) and 0 < float(fixture[f'{name}_ref_err']) < 1e-6, (name, err)
        if f'{name}_pair_sm' in fixture:
            sm = fixture[f'{name}_pair_sm']
            assert np.max(np.abs(sm - want_sm)) <= float(fixture[f'{name}_ref_err_sm']) * (1 + 1e-9) < 1e-5
            assert all(np.all(sm[b, ql:] == 0.0) and np.all(sm[b, :, cl:] == 0.0) for b, (ql, cl) in enumerate(zip(qlens, clens)))
        lo, hi = min(lo, float(got.min())), max(hi, float(got.max()))
    assert any(1 in fixture[f'{n}_qlens'] for n in names) and any(1 in fixture[f'{n}_clens'] for n in names)
    assert lo > 100 and hi > 1500          # large scores: the tolerance has to be relative
    for name in (str(n) for n in fixture['pools']):
        query, cands = pool_inputs(spec_of(fixture, name))
        want = np.array([closed_form(query[None], cd[None], [len(query)], [len(cd)])[0][0] for cd in cands])
        got = fixture[f'{name}_scores']
        assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)) <= float(fixture[f'{name}_ref_err']) * (1 + 1e-9)


class _StubOps:
    """ops as polyenc uses it, on the CPU: padded rep sets kept as arrays, jointsm_scores from the float64 closed form"""

    class DeviceRepSet:
        def __init__(self, reps, lens):
            self.reps, self.lens, self.n, self.ext = reps.numpy(), list(lens), reps.shape[0], reps.shape[1]

        @classmethod
        def from_padded(cls, reps, abs_lens):
            return cls(reps.cpu(), abs_lens)

    calls = []

    @staticmethod
    def require_gpu():
        return torch.device('cpu')

    @classmethod
    def jointsm_scores(cls, q, c, pairing, want_pair_softmax=False):
        from aspire_amd import _lib
        assert pairing == _lib.PAIR_CROSS and q.n == 1 and want_pair_softmax
        cls.calls.append(c.n)
        qq = np.repeat(q.reps, c.n, 0)
        s, soft = closed_form(qq, c.reps, q.lens * c.n, c.lens)
        soft[:, q.lens[0]:, :] = -7.0          # poison the pads: score() must cut them away
        for b, cl in enumerate(c.lens):
            soft[b, :, cl:] = -7.0
        return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(soft.astype(np.float32))


def test_polyenc_host_logic_on_stubbed_ops(monkeypatch, fixture):
    from aspire_amd import polyenc
    monkeypatch.setattr(polyenc, 'ops', _StubOps)
    _StubOps.calls.clear()
    query, cands = pool_inputs(spec_of(fixture, 'pool'))
    ret = polyenc.WordSentAlignPolyEnc.score(query_reps=query, cand_reps=cands[:9])
    assert set(ret) == {'batch_scores', 'pair_scores'}
    assert ret['batch_scores'].shape == (9,) and ret['batch_scores'].dtype == np.float32
    assert [p.shape for p in ret['pair_scores']] == [(len(query), len(cd)) for cd in cands[:9]]
    assert all((p >= 0).all() and abs(p.sum() - 1) < 1e-5 for p in ret['pair_scores'])          # un-padded: no poison, sums to 1
    model = polyenc.TrainedScoringModel('miswordpolyenc')
    with pytest.raises(ValueError, match='Unknown model'):
        polyenc.TrainedScoringModel('cospecter')
    _StubOps.calls.clear()
    pred = model.predict(query=query, cands=cands)
    assert _StubOps.calls == [len(cands)]                      # one batched call, not groups of 128
    assert set(pred) == {'cand_scores', 'pair_scores'} and isinstance(pred['cand_scores'], list) and len(pred['cand_scores']) == len(cands)
    assert np.allclose(pred['cand_scores'], fixture['pool_scores'], rtol=1e-6)
    assert np.allclose(pred['pair_scores'][149], fixture['pool_pair_scores_149'], atol=1e-5)
    assert model.predict(query=query, cands=[]) == {'cand_scores': [], 'pair_scores': []}
    # the ranking as pp_gen_nearest.py:450-456 writes it: (pid, -sim), best first, ties in pool order
    pids = [f'p{i}' for i in range(len(cands))]
    ranked = model.rank(query, cands, pids)
    sims = pred['cand_scores']
    assert ranked == [(pids[i], -sims[i]) for i in sorted(range(len(sims)), key=lambda i: sims[i], reverse=True)]
    tie = model.rank(query, [cands[3], cands[5], cands[3], cands[5]], ['a', 'b', 'c', 'd'])
    assert [p for p, _ in tie] in (['a', 'c', 'b', 'd'], ['b', 'd', 'a', 'c']) and tie[0][1] == tie[1][1] <= tie[2][1]
    with pytest.raises(ValueError, match='Unknown aggregation'):
        polyenc.WordSentAlignPolyEnc(model_hparams={'score_aggregation': 'l2max', 'base-pt-layer': 'x'})


def test_public_names():
    import aspire_amd
    from aspire_amd import ops, pair_distances, polyenc
    import aspire_amd.torch_ops as to
    assert aspire_amd.allpair_joint_sm_negscore is pair_distances.allpair_joint_sm_negscore
    assert aspire_amd.TrainedScoringModel is polyenc.TrainedScoringModel and aspire_amd.WordSentAlignPolyEnc is polyenc.WordSentAlignPolyEnc
    assert issubclass(polyenc.WordSentAlignPolyEnc, aspire_amd.AspireConSent)
    assert callable(ops.jointsm_scores) and callable(ops.jointsm_rank_batch)
    assert 'jointsm_scores' in to.OPS and hasattr(torch.ops.aspire, 'jointsm_scores')
    m = lambda *s, dt=torch.float32: torch.empty(*s, device='meta', dtype=dt)
    i32 = torch.int32
    assert torch.ops.aspire.jointsm_scores(m(3, 8, 768), m(3, dt=i32), m(5, 6, 768), m(5, dt=i32), False).shape == (15,)
    assert torch.ops.aspire.jointsm_scores(m(4, 8, 768), m(4, dt=i32), m(4, 6, 768), m(4, dt=i32), True).shape == (4,)
