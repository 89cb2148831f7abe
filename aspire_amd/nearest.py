"""The precomputed-embedding rankers: the `specter` / `cospecter` rows of the result tables.

Replaces src/pre_process/pp_gen_nearest.py rank_pool (:638-727) and rank_pool_faceted (:1120-1199).  Their inputs are one
[N, 768] matrix of whole-abstract reps on disk ({dataset}-{abstract|title}s.npy, written by pre_proc_buildreps.py), a
pid2idx-*.json map from paper id to matrix row, and per query a pool of candidate pids; per query the reference fancy-indexes
the pool out of the matrix and runs sklearn.neighbors.NearestNeighbors(algorithm='brute') on it.  Here the matrix is uploaded
once (`DenseReps`) and ALL queries of a call are ranked by one ops.dense_rank_batch call over row-index lists: pools overlap
heavily (the reference's own remark, :735-736) and no pool is ever copied.

    reps = DenseReps.from_npy('csfcube-abstracts.npy', 'pid2idx-csfcube-abstract.json')
    query2rankedcands = rank_pool(reps, qpid2pool)             # {qpid: [(cand_pid, distance), ...]}, ascending
    write_ranked(query2rankedcands, 'test-pid2pool-csfcube-specter-ranked.json')

The readable per-query .txt dumps of the reference are not written.
"""
import json

import numpy as np
import torch

from . import _lib, ops

# metric -> (the library's constant, similarity -> the distance handed out)
METRICS = {'l2': (_lib.DENSE_L2, lambda s: 0.0 - s),            # Euclidean distance (NearestNeighbors' default metric)
           'cosine': (_lib.DENSE_COSINE, lambda s: 1.0 - s),  # cosine distance
           'dot': (_lib.DENSE_DOT, lambda s: 0.0 - s)}       # negated dot product (0.0 - s: a zero comes out as +0.0)


class DenseReps:
    """One [N, 768] matrix of document reps, resident on the GPU, and the host-side map pid -> matrix row.

    all_doc_reps: array-like [N, 768]; copied to fp32 and passed through np.nan_to_num as the reference does (:669) before the one
    upload.  all_doc2idx: {pid: row}.  `device` is for tests of the host logic; the scoring entry takes GPU tensors only."""

    def __init__(self, all_doc_reps, all_doc2idx, device=None):
        reps = np.array(all_doc_reps, dtype=np.float32, order='C')        # (a copy: the caller's array stays as it is)
        if reps.ndim != 2 or reps.shape[1] != ops.D:
            raise ValueError(f'document reps must be [N, {ops.D}], got {reps.shape}')
        np.nan_to_num(reps, copy=False)
        self.doc2idx = dict(all_doc2idx)
        self.n = int(reps.shape[0])
        self.rows = torch.from_numpy(reps).to(ops.require_gpu() if device is None else device)

    @classmethod
    def from_npy(cls, npy_path, pid2idx_json_path, device=None):
        """The on-disk layout of pre_proc_buildreps.py: {dataset}-{abstract|title}s.npy + pid2idx-{dataset}-{...}.json"""
        with open(pid2idx_json_path, 'r', encoding='utf-8') as fp:
            doc2idx = json.load(fp)
        return cls(np.load(npy_path), doc2idx, device=device)

    def __len__(self):
        return self.n

    def __contains__(self, pid):
        return pid in self.doc2idx

    def row_of(self, pid):
        """The matrix row of `pid`: KeyError for a pid the map lacks, IndexError for a row the matrix lacks"""
        idx = self.doc2idx[pid]
        if isinstance(idx, bool) or not isinstance(idx, (int, np.integer)) or not 0 <= idx < self.n:
            raise IndexError(f'paper {pid!r} maps to row {idx!r}; the matrix has rows 0 .. {self.n - 1}')
        return int(idx)


def _cands(pool):
    return pool['cands'] if isinstance(pool, dict) else pool


def _rank_jobs(reps, jobs, metric):
    """jobs: [(qpid, query row, [cand pid], [cand row])] -> {qpid: [(cand_pid, distance), ...]} through ONE dense_rank_batch call"""
    if metric not in METRICS:
        raise ValueError(f'Unknown metric: {metric} (one of {sorted(METRICS)})')
    code, to_dist = METRICS[metric]
    jobs = [job for job in jobs if job[3]]          # an empty pool ranks nothing (sklearn refuses n_neighbors = 0)
    ranked = {}
    if not jobs:
        return ranked
    sizes = [len(job[3]) for job in jobs]
    dev = reps.rows.device
    q_idx = torch.tensor([job[1] for job in jobs], dtype=torch.int32).to(dev)
    cand_idx = torch.from_numpy(np.concatenate([np.asarray(job[3], dtype=np.int32) for job in jobs])).to(dev)
    job_off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    max_job = max(sizes)
    _, top_s, top_i = ops.dense_rank_batch(reps.rows, q_idx, cand_idx, job_off, max_job, max_job, metric=code)
    top_s, top_i = top_s.cpu().numpy(), top_i.cpu().numpy()
    for (qpid, _, pids, _), n, sims, order in zip(jobs, sizes, top_s, top_i):
        out = [(pids[i], float(to_dist(np.float64(s)))) for i, s in zip(order[:n].tolist(), sims[:n]) if pids[i] != qpid]
        if out:
            ranked[qpid] = out
    return ranked


def rank_pool(reps, qpid2pool, metric='l2'):
    """pp_gen_nearest.py rank_pool, :683-717: every query's pool re-ranked by the whole-document rep alone.

    reps: DenseReps.  qpid2pool: {qpid: {'cands': [pid, ...], ...}} (test-pid2anns-*.json as loaded; a plain list of pids per
    query is taken too).  Returns query2rankedcands {qpid: [(cand_pid, distance), ...]}: per query the pool in ascending
    distance -- with 'l2' the Euclidean distance, positive, as sklearn's brute NearestNeighbors returns it ('cosine': 1 - cos,
    'dot': the negated dot product).  As in the reference a candidate pid the map lacks is skipped (:694-698), a query pid the
    map lacks raises KeyError (:689), and a candidate equal to the query pid is ranked but left out of the list (:712-716); a
    query for which nothing is listed has no entry (the reference's defaultdict), which includes the empty pool that sklearn
    refuses.  A mapped row outside the matrix raises IndexError before anything is launched.
    TIES keep pool order: candidates at equal distance come out in the order the pool lists them (the rank is stable).
    sklearn's brute search defines no tie order; this is this project's rule.
    One departure: after a skipped candidate the reference goes on indexing the UNFILTERED pid list with positions of the
    filtered matrix (:707-711), so its labels shift by one per skip; here a distance always carries the pid of the row it was
    computed from."""
    jobs = []
    for qpid, pool in qpid2pool.items():
        qrow = reps.row_of(qpid)
        pids = [cpid for cpid in _cands(pool) if cpid in reps.doc2idx]
        jobs.append((qpid, qrow, pids, [reps.row_of(cpid) for cpid in pids]))
    return _rank_jobs(reps, jobs, metric)


def rank_pool_faceted(reps, qpid2pool, metric='l2'):
    """pp_gen_nearest.py rank_pool_faceted, :1166-1191 (qpid2pool = test-pid2anns-{dataset}-{facet}.json): as rank_pool, except
    that a query pid the map lacks is dropped (:1148) and a candidate pid the map lacks raises KeyError (:1175)."""
    jobs = []
    for qpid, pool in qpid2pool.items():
        if qpid not in reps.doc2idx:
            continue
        pids = list(_cands(pool))
        jobs.append((qpid, reps.row_of(qpid), pids, [reps.row_of(cpid) for cpid in pids]))
    return _rank_jobs(reps, jobs, metric)


def write_ranked(query2rankedcands, path):
    """test-pid2pool-{dataset}-{sent_rep_type}[-{facet}]-ranked.json, as :723-725 / :1196-1198 dump it"""
    with open(path, 'w', encoding='utf-8') as fp:
        json.dump(query2rankedcands, fp)
