"""CPU: the precomputed-embedding rankers without a GPU -- the two C-ABI entries of dense.hip (declared, exported, signed; every
argument check of aspire_dense_rank_batch_f32, none of which reaches a launch), the host logic of nearest.rank_pool /
rank_pool_faceted over a numpy stand-in for ops.dense_rank_batch, and RepStore.from_npy_sent."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

FAKE = 16            # a non-null, 16-byte aligned "device pointer" that no call of this file reaches
NEW = ('aspire_dense_rank_batch_workspace_bytes', 'aspire_dense_rank_batch_f32')


def test_new_entries_are_declared_exported_and_signed():
    from aspire_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'aspire_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', hdr), f'{name} is not declared in aspire_hip.h'
        assert hasattr(raw, name), f'{name} is not exported'
        assert name in _lib.SIGNATURES
    decl = lambda fn: [a.strip() for a in re.search(fn + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')]
    assert decl('aspire_dense_rank_batch_workspace_bytes') == ['int64_t J', 'int64_t C', 'int64_t max_job', 'int64_t k']
    args = decl('aspire_dense_rank_batch_f32')
    assert args[:7] == ['const float* rows', 'int64_t N', 'int64_t D', 'const int32_t* q_idx', 'int64_t J', 'const int32_t* cand_idx',
                        'int64_t C']
    # from job_off on: aspire_dotmax_rank_batch_f32's parameters, `int metric` in the place of `int sim`
    dotmax = decl('aspire_dotmax_rank_batch_f32')
    assert args[7:] == [a if a != 'int sim' else 'int metric' for a in dotmax[dotmax.index('const int32_t* job_off'):]]
    assert len(_lib.SIGNATURES['aspire_dense_rank_batch_f32'][1]) == len(args)
    assert _lib.SIGNATURES['aspire_dense_rank_batch_f32'][1][7:] == _lib.SIGNATURES['aspire_dotmax_rank_batch_f32'][1][3:]
    for name, value in (('ASPIRE_DENSE_L2', _lib.DENSE_L2), ('ASPIRE_DENSE_COSINE', _lib.DENSE_COSINE), ('ASPIRE_DENSE_DOT', _lib.DENSE_DOT)):
        assert int(re.search(r'#define\s+' + name + r'\s+(\d+)', hdr).group(1)) == value
    assert len({_lib.DENSE_L2, _lib.DENSE_COSINE, _lib.DENSE_DOT}) == 3
    assert callable(ops.dense_rank_batch)
    import aspire_amd.torch_ops as to
    assert 'dense_rank_batch' in to.OPS and hasattr(torch.ops.aspire, 'dense_rank_batch')
    m = lambda *s, dt=torch.float32: torch.empty(*s, device='meta', dtype=dt)
    s, ts, ti = torch.ops.aspire.dense_rank_batch(m(70, 768), m(4, dt=torch.int32), m(137, dt=torch.int32), m(5, dt=torch.int32), 67, 9, 0)
    assert s.shape == (137,) and ts.shape == (4, 9) and ti.shape == (4, 9) and ti.dtype == torch.int64
    with pytest.raises(NotImplementedError, match='CPU'):          # no CPU kernel behind the op
        torch.ops.aspire.dense_rank_batch(torch.zeros(2, 768), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                                          torch.tensor([0, 1], dtype=torch.int32), 1, 1, 0)


def test_batch_entry_validation_without_gpu():
    from aspire_amd import _lib
    INVALID, UNSUPPORTED, OK = _lib.ASPIRE_ERR_INVALID_ARG, _lib.ASPIRE_ERR_UNSUPPORTED, _lib.ASPIRE_OK
    err = _lib.lib.aspire_last_error
    ok_args = dict(rows=FAKE, N=70, D=768, q_idx=FAKE, J=2, cand_idx=FAKE, C=30, job_off=FAKE, max_job=20, metric=_lib.DENSE_L2,
                   scores=None, k=10, job_base=None, top_s=FAKE, top_i=FAKE, keys=None, ws=FAKE, nbytes=1 << 20)

    def status(**kw):
        a = dict(ok_args, **kw)
        return _lib.lib.aspire_dense_rank_batch_f32(a['rows'], a['N'], a['D'], a['q_idx'], a['J'], a['cand_idx'], a['C'], a['job_off'],
                                                    a['max_job'], a['metric'], a['scores'], a['k'], a['job_base'], a['top_s'], a['top_i'],
                                                    a['keys'], a['ws'], a['nbytes'], None)

    # (scores is null unless a case says otherwise: a call that passed every check before it ends in the preamble's "null scores",
    # and the checks behind it are reached with an argument that fails them -- never a launch)
    assert status() == INVALID and b'null scores' in err()
    for metric in (_lib.DENSE_L2, _lib.DENSE_COSINE, _lib.DENSE_DOT):
        assert status(metric=metric) == INVALID and b'null scores' in err()
    assert status(metric=3) == INVALID and b'bad metric 3' in err()
    assert status(metric=-1) == INVALID and b'bad metric' in err()
    assert status(D=512) == UNSUPPORTED and b'768' in err()
    assert status(D=0) == UNSUPPORTED
    assert status(N=-1) == INVALID and b'negative' in err()
    assert status(J=-1) == INVALID and b'negative' in err()
    assert status(C=-1) == INVALID and b'negative' in err()
    assert status(N=1 << 31) == UNSUPPORTED and b'32-bit' in err()
    assert status(N=(1 << 31) - 1) == INVALID and b'null scores' in err()
    # the preamble the batched entries share
    assert status(k=-1) == INVALID
    assert status(top_s=None, top_i=None) == INVALID and b'keys' in err()
    assert status(top_s=None) == INVALID and b'keys' in err()
    assert status(top_s=None, top_i=None, keys=FAKE) == INVALID and b'null scores' in err()
    assert status(k=0, top_s=None, top_i=None) == INVALID and b'null scores' in err()
    assert status(job_off=None) == INVALID and b'job_off' in err()
    assert status(max_job=31) == INVALID and b'max_job' in err()
    assert status(max_job=-1) == INVALID
    assert status(J=1 << 30) == UNSUPPORTED and b'too large' in err()
    assert status(C=(1 << 31) - 8, max_job=20) == UNSUPPORTED and b'too large' in err()
    assert status(J=0, job_off=None, ws=None, nbytes=0) == OK
    assert status(J=0, C=0, max_job=0, k=0, top_s=None, top_i=None, job_off=None, ws=None, nbytes=0, rows=None, q_idx=None, cand_idx=None) == OK
    # behind the preamble (scores given): the index lists, the matrix, the workspace
    assert status(scores=FAKE, q_idx=None) == INVALID and b'q_idx' in err()
    assert status(scores=FAKE, cand_idx=None) == INVALID and b'cand_idx' in err()
    assert status(scores=FAKE, rows=None) == INVALID and b'null rows' in err()
    assert status(scores=FAKE, rows=24) == INVALID and b'rows must be 16-byte aligned' in err()
    assert status(scores=FAKE, ws=24) == INVALID and b'workspace must be 16-byte aligned' in err()
    need = _lib.lib.aspire_dense_rank_batch_workspace_bytes(2, 9000, 5000, 100)
    assert need == _lib.lib.aspire_topk_workspace_bytes(2, 5000, 100) > 0 and need % 16 == 0
    big = dict(scores=FAKE, C=9000, max_job=5000, k=100)
    assert status(nbytes=need - 16, **big) == INVALID and b'aspire_dense_rank_batch_workspace_bytes' in err()
    assert status(ws=None, nbytes=need, **big) == INVALID and b'workspace too small' in err()
    assert status(ws=24, nbytes=need + 64, **big) == INVALID and b'aligned' in err()


def test_workspace_is_the_rank_scratch_only():
    from aspire_amd import _lib
    ws_bytes = _lib.lib.aspire_dense_rank_batch_workspace_bytes
    for k in (100, 2000):
        assert ws_bytes(2, 9000, 5000, k) == _lib.lib.aspire_topk_workspace_bytes(2, 5000, k) > 0
    assert ws_bytes(2, 9000, 4096, 100) == 0          # pools of <= 4096: none
    assert ws_bytes(2, 9000, 5000, 0) == 0            # k = 0: scores only
    assert ws_bytes(0, 9000, 5000, 10) == 0
    assert ws_bytes(2, 0, 0, 10) == 0
    assert ws_bytes(-1, 9000, 5000, 10) == 0


# ---- nearest.py over a numpy stand-in ---------------------------------------------------------------------------------------
def _standin(calls):
    """ops.dense_rank_batch in float64 numpy on CPU tensors: (scores, top_scores, top_idx) with the library's contract (stable
    descending rank per job, (-inf, -1) beyond a pool's size)"""
    from aspire_amd import _lib

    def dense_rank_batch(rows, q_idx, cand_idx, job_off, max_job, k, metric=_lib.DENSE_L2, **kw):
        assert not kw
        assert q_idx.dtype == cand_idx.dtype == job_off.dtype == torch.int32 and rows.dtype == torch.float32
        x, qi, ci, off = rows.numpy().astype(np.float64), q_idx.numpy(), cand_idx.numpy(), job_off.numpy()
        assert len(off) == len(qi) + 1 and off[0] == 0 and off[-1] == len(ci) and max_job == max(np.diff(off))
        assert ci.min() >= 0 and ci.max() < len(x) and qi.min() >= 0 and qi.max() < len(x)
        calls.append((qi.tolist(), ci.tolist(), off.tolist(), max_job, k, metric))
        scores = np.empty(len(ci))
        top_s, top_i = np.full((len(qi), k), -np.inf, np.float32), np.full((len(qi), k), -1, np.int64)
        for j, q in enumerate(qi):
            c = x[ci[off[j]:off[j + 1]]]
            if metric == _lib.DENSE_L2:
                s = -np.sqrt(((c - x[q]) ** 2).sum(1))
            elif metric == _lib.DENSE_COSINE:
                s = c @ x[q] / np.linalg.norm(x[q]) / np.linalg.norm(c, axis=1)
            else:
                s = c @ x[q]
            scores[off[j]:off[j + 1]] = s
            order = np.argsort(-s, kind='stable')[:k]
            top_s[j, :len(order)], top_i[j, :len(order)] = s[order], order
        return torch.from_numpy(scores.astype(np.float32)), torch.from_numpy(top_s), torch.from_numpy(top_i)
    return dense_rank_batch


@pytest.fixture
def toy(monkeypatch):
    """8 papers on a line (row r = r along the first coordinate, so distances are differences of row numbers); the map shuffles them"""
    from aspire_amd import nearest, ops
    calls = []
    monkeypatch.setattr(ops, 'dense_rank_batch', _standin(calls))
    x = np.zeros((8, 768), np.float32)
    x[:, 0] = np.arange(8)
    x[:, 1] = 1.0
    doc2idx = {'a': 3, 'b': 0, 'c': 7, 'd': 5, 'e': 1, 'f': 6, 'g': 2, 'h': 4}
    return nearest, nearest.DenseReps(x, doc2idx, device='cpu'), calls


def test_rank_pool_host_logic(toy):
    from aspire_amd import _lib
    nearest, reps, calls = toy
    qpid2pool = {'a': {'cands': ['c', 'b', 'missing', 'a', 'h', 'g'], 'relevance_adju': [0, 1, 0, 2, 0, 1]},
                 'e': ['b', 'g'],                     # a plain list of pids; b and g are both at distance 1: pool order
                 'd': {'cands': []},                  # the empty pool
                 'f': {'cands': ['nope']},            # nothing left after the skip
                 'h': {'cands': ['h']}}               # only itself
    out = nearest.rank_pool(reps, qpid2pool)
    assert type(out) is dict and list(out) == ['a', 'e']
    # 'missing' is skipped, 'a' itself is ranked (first, at 0) and left out; h and g are both at distance 1: pool order
    assert out['a'] == [('h', 1.0), ('g', 1.0), ('b', 3.0), ('c', 4.0)]
    assert out['e'] == [('b', 1.0), ('g', 1.0)]
    assert all(type(p) is str and type(d) is float and d >= 0 for r in out.values() for p, d in r)
    # ONE call for all queries; the empty pools never reach it; the query's own row does
    assert len(calls) == 1
    qi, ci, off, max_job, k, metric = calls[0]
    assert qi == [3, 1, 4] and ci == [7, 0, 3, 4, 2, 0, 2, 4] and off == [0, 5, 7, 8] and max_job == k == 5 and metric == _lib.DENSE_L2
    assert json.loads(json.dumps(out)) == {q: [list(t) for t in r] for q, r in out.items()}
    # a query the map lacks: rank_pool raises (:689), rank_pool_faceted drops it (:1148)
    with pytest.raises(KeyError):
        nearest.rank_pool(reps, {'zz': {'cands': ['a']}})
    assert nearest.rank_pool_faceted(reps, {'zz': {'cands': ['a']}, 'b': {'cands': ['e', 'b', 'c']}}) == {'b': [('e', 1.0), ('c', 7.0)]}
    # a candidate the map lacks: skipped above, KeyError here (:1175)
    with pytest.raises(KeyError):
        nearest.rank_pool_faceted(reps, {'a': {'cands': ['c', 'missing']}})
    assert nearest.rank_pool_faceted(reps, {'a': {'cands': []}}) == {} and nearest.rank_pool(reps, {}) == {}
    assert len(calls) == 2
    # the other metrics hand out ascending distances too
    cos = nearest.rank_pool(reps, {'b': ['c', 'e', 'g']}, metric='cosine')['b']
    assert [p for p, _ in cos] == ['e', 'g', 'c'] and cos[0][1] == pytest.approx(1 - 1 / np.sqrt(2)) and calls[-1][5] == _lib.DENSE_COSINE
    dot = nearest.rank_pool(reps, {'c': ['e', 'g', 'b']}, metric='dot')['c']
    assert dot == [('g', -15.0), ('e', -8.0), ('b', -1.0)] and calls[-1][5] == _lib.DENSE_DOT
    with pytest.raises(ValueError, match='Unknown metric'):
        nearest.rank_pool(reps, {'a': ['b']}, metric='l1')


def test_bad_rows_raise_index_error_before_any_call(toy):
    nearest, reps, calls = toy
    for bad in (8, -1, 1 << 40, 2.0, None, True):
        reps.doc2idx['x'] = bad
        with pytest.raises(IndexError, match="paper 'x'"):
            nearest.rank_pool(reps, {'a': ['b', 'x']})
        with pytest.raises(IndexError):
            nearest.rank_pool_faceted(reps, {'a': ['x']})
        with pytest.raises(IndexError):
            nearest.rank_pool(reps, {'x': ['a']})
    assert calls == []
    reps.doc2idx['x'] = np.int64(7)
    assert nearest.rank_pool(reps, {'a': ['x']}) == {'a': [('x', 4.0)]}


def test_dense_reps_loader(tmp_path, monkeypatch):
    from aspire_amd import nearest, ops
    import aspire_amd
    assert aspire_amd.DenseReps is nearest.DenseReps and aspire_amd.rank_pool is nearest.rank_pool
    assert aspire_amd.rank_pool_faceted is nearest.rank_pool_faceted
    x = np.random.default_rng(0).standard_normal((5, 768))             # float64 on disk: converted
    x[1, 3], x[2, 0], x[4, 767] = np.nan, np.inf, -np.inf
    np.save(tmp_path / 'toy-abstracts.npy', x)
    (tmp_path / 'pid2idx-toy-abstract.json').write_text(json.dumps({'p%d' % i: i for i in range(5)}))
    reps = nearest.DenseReps.from_npy(str(tmp_path / 'toy-abstracts.npy'), str(tmp_path / 'pid2idx-toy-abstract.json'), device='cpu')
    assert len(reps) == 5 and 'p3' in reps and 'p9' not in reps and reps.row_of('p4') == 4
    assert reps.rows.dtype == torch.float32 and tuple(reps.rows.shape) == (5, 768) and reps.rows.is_contiguous()
    # np.nan_to_num (:669): nan -> 0, +-inf -> the largest finite float32; the caller's array is not touched
    want = np.nan_to_num(x.astype(np.float32))
    assert np.array_equal(reps.rows.numpy(), want) and np.isfinite(reps.rows.numpy()).all()
    assert reps.rows[1, 3] == 0 and reps.rows[2, 0] == np.finfo(np.float32).max and reps.rows[4, 767] == np.finfo(np.float32).min
    assert np.isnan(x[1, 3])
    with pytest.raises(ValueError, match='768'):
        nearest.DenseReps(np.zeros((3, 512), np.float32), {}, device='cpu')
    if not torch.cuda.is_available():              # the matrix lives on the GPU: without one the default construction fails loudly
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            nearest.DenseReps(np.zeros((3, 768), np.float32), {})
    # the writer: what json.load gives back
    calls = []
    monkeypatch.setattr(ops, 'dense_rank_batch', _standin(calls))
    out = nearest.rank_pool(reps, {'p0': {'cands': ['p3', 'p1']}})
    nearest.write_ranked(out, str(tmp_path / 'test-pid2pool-toy-specter-ranked.json'))
    back = json.load(open(tmp_path / 'test-pid2pool-toy-specter-ranked.json'))
    assert back == {'p0': [list(t) for t in out['p0']]} and len(back['p0']) == 2


def test_repstore_from_npy_sent(tmp_path):
    from aspire_amd.repstore import RepStore
    x = np.arange(9 * 768, dtype=np.float32).reshape(9, 768)
    x[4, 5] = np.nan
    # paper 'p-1' (a pid with a dash) has three sentences stored out of order, 'q' one, '7' two; rows 2 and 6 belong to nobody
    sent2idx = {'p-1-2': 0, 'q-0': 8, 'p-1-0': 4, '7-1': 1, 'p-1-1': 3, '7-0': 5}
    np.save(tmp_path / 'toy-sent.npy', x)
    (tmp_path / 'pid2idx-toy-sent.json').write_text(json.dumps(sent2idx))
    store = RepStore.from_npy_sent(str(tmp_path / 'toy-sent.npy'), str(tmp_path / 'pid2idx-toy-sent.json'))
    assert len(store) == 3 and sorted(store.pid2reps) == ['7', 'p-1', 'q']
    want = np.nan_to_num(x)
    assert np.array_equal(store.get('p-1'), want[[4, 3, 0]]) and store.get('p-1')[0, 5] == 0
    assert np.array_equal(store.get('q'), want[[8]]) and np.array_equal(store.get('7'), want[[5, 1]])
    assert all(v.dtype == np.float32 and v.shape[1] == 768 for v in store.pid2reps.values())
    assert np.array_equal(store.faceted('7', 'all', None), want[[5, 1]])          # the store's existing access paths take it
    for bad, exc in (({'p-0': 0, 'p-2': 1}, ValueError), ({'p-0': 9}, IndexError), ({'p-0': -1}, IndexError), ({'nodash': 0}, ValueError),
                     ({'p-x': 0}, ValueError)):
        (tmp_path / 'bad.json').write_text(json.dumps(bad))
        with pytest.raises(exc):
            RepStore.from_npy_sent(str(tmp_path / 'toy-sent.npy'), str(tmp_path / 'bad.json'))
