"""GPU: the frame the four pair backward kernels share (aspire_amd/csrc/pair_bwd.h) -- what a pair's workgroup writes when the pair has
no gradient: a document longer than its set's host-known bound (poisoned: NaN in its valid rows up to the bound and in its partner's),
a document without rows (empty: exact zeros), and the pad rows of padded sets (exact zeros in every case).  Through ops.l2agg_backward
(three aggregations), ops.jointsm_backward, ops.ot_backward (diameter=None: every pair's own box) and ops.l2sup_backward (both forms).

The sets are built with ops.DeviceRepSet directly, without host lengths, so that the host layer's check for empty documents does not
stand in front of the kernels.  Padded: three pairs of [4, 768] blocks, lengths q = [3, 0, 5], c = [2, 3, 2], seeded normal rows,
1e30 in the pad rows (a kernel that read one would not stay finite).  Pair 0 is ordinary, pair 1 has an empty query, pair 2 a query
longer than the bound 4.  CSR (ext = 0, max_len = 4): lengths q = [3, 2, 5], c = [2, 3, 2]; the document of 5 rows is poisoned up to
the bound, its fifth row has no writer.  The output buffers are pre-filled with a sentinel: a row the kernel owns and does not write
shows, and so does a row it writes and does not own.  Every store is inside ext or min(len, bound): nothing here leaves a buffer."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
D = 768
EXT = 4
SENTINEL = -12345.0
Q_LENS, C_LENS = [3, 0, 5], [2, 3, 2]
ALIGN = [[1, 1], [0, 0], [2, 1]]

CALLS = {
    'l2max': lambda ops, lib, q, c, gs, align, out: ops.l2agg_backward(q, c, lib.AGG_MAX, gs, out=out),
    'l2top2': lambda ops, lib, q, c, gs, align, out: ops.l2agg_backward(q, c, lib.AGG_TOP2, gs, out=out),
    'l2attention': lambda ops, lib, q, c, gs, align, out: ops.l2agg_backward(q, c, lib.AGG_ATTENTION, gs, temp=2.0, out=out),
    'jointsm': lambda ops, lib, q, c, gs, align, out: ops.jointsm_backward(q, c, gs, out=out),
    'ot': lambda ops, lib, q, c, gs, align, out: ops.ot_backward(q, c, gs, diameter=None, out=out),
    'l2sup': lambda ops, lib, q, c, gs, align, out: ops.l2sup_backward(q, c, align, gs, False, out=out),
    'l2sup_weighted': lambda ops, lib, q, c, gs, align, out: ops.l2sup_backward(q, c, align, gs, True, out=out),
}


@pytest.fixture(scope='module')
def amd():
    from aspire_amd import ops, _lib
    assert torch.cuda.is_available()
    return type('NS', (), dict(ops=ops, lib=_lib))


@functools.lru_cache(maxsize=None)
def _inputs():
    """(q [3, 4, 768], c [3, 4, 768], grad_scores [3]) on the CPU, pad rows 1e30 -- made once, never written to"""
    g = torch.Generator().manual_seed(20)
    q, c, gs = torch.randn(3, EXT, D, generator=g), torch.randn(3, EXT, D, generator=g), torch.randn(3, generator=g)
    for t, lens in ((q, Q_LENS), (c, C_LENS)):
        for b, n in enumerate(lens):
            t[b, n:] = 1e30
    return q, c, gs


def _i32(values):
    return torch.tensor(values, dtype=torch.int32).cuda()


def _padded_set(amd, blocks, lens):
    n = blocks.shape[0]
    return amd.ops.DeviceRepSet(blocks.reshape(n * EXT, D).cuda(), _i32([b * EXT for b in range(n)]), _i32(lens), ext=EXT)


def _run(amd, name, qs, cs, gs, align):
    """(grad_q_rows, grad_c_rows) on the CPU, written into sentinel-filled buffers"""
    out = (torch.full_like(qs.rows, SENTINEL), torch.full_like(cs.rows, SENTINEL))
    gq, gc = CALLS[name](amd.ops, amd.lib, qs, cs, gs.cuda(), _i32(align).reshape(-1, 2), out)
    torch.cuda.synchronize()
    return gq.cpu(), gc.cpu()


def _run_padded(amd, name, pairs=slice(None)):
    q, c, gs = _inputs()
    gq, gc = _run(amd, name, _padded_set(amd, q[pairs], Q_LENS[pairs]), _padded_set(amd, c[pairs], C_LENS[pairs]), gs[pairs], ALIGN[pairs])
    return gq.view(-1, EXT, D), gc.view(-1, EXT, D)


@pytest.mark.parametrize('name', list(CALLS))
def test_padded_pairs_poisoned_empty_and_ordinary(amd, name):
    gq, gc = _run_padded(amd, name)
    assert not (gq == SENTINEL).any() and not (gc == SENTINEL).any(), 'a padded set: every row has its writer'
    # pair 1, an empty query: no gradient, exact zeros in all its 4 + 4 rows
    assert torch.count_nonzero(gq[1]) == 0 and torch.count_nonzero(gc[1]) == 0
    # pair 2, a query of 5 rows against the bound 4: NaN in its rows up to the bound and in its partner's valid rows, pads zero
    assert torch.isnan(gq[2]).all() and torch.isnan(gc[2, :2]).all() and torch.count_nonzero(gc[2, 2:]) == 0
    # pair 0, ordinary: finite, a gradient in it, pad rows exact zeros -- and what it is alone, and on a second run
    assert torch.isfinite(gq[0]).all() and torch.isfinite(gc[0]).all()
    assert torch.count_nonzero(gq[0, :3]) > 0 and torch.count_nonzero(gc[0, :2]) > 0
    assert torch.count_nonzero(gq[0, 3:]) == 0 and torch.count_nonzero(gc[0, 2:]) == 0
    alone_q, alone_c = _run_padded(amd, name, slice(0, 1))
    assert torch.equal(alone_q[0], gq[0]) and torch.equal(alone_c[0], gc[0])
    again_q, again_c = _run_padded(amd, name)
    assert torch.equal(again_q[0], gq[0]) and torch.equal(again_c[0], gc[0])
    assert torch.equal(torch.isnan(again_q), torch.isnan(gq)) and torch.equal(torch.isnan(again_c), torch.isnan(gc))


@pytest.mark.parametrize('name', list(CALLS))
def test_csr_poisoned_document_is_written_up_to_the_bound_only(amd, name):
    q, c, gs = _inputs()
    g = torch.Generator().manual_seed(21)
    q_lens, c_lens = [3, 2, 5], [2, 3, 2]
    # pair 0's valid rows are the padded pair 0's; the rest is new
    q_rows = torch.cat([q[0, :3], torch.randn(2 + 5, D, generator=g)])
    c_rows = torch.cat([c[0, :2], torch.randn(3 + 2, D, generator=g)])
    qs = amd.ops.DeviceRepSet(q_rows.cuda(), _i32([0, 3, 5]), _i32(q_lens), ext=0, max_len=4)
    cs = amd.ops.DeviceRepSet(c_rows.cuda(), _i32([0, 2, 5]), _i32(c_lens), ext=0, max_len=4)
    gq, gc = _run(amd, name, qs, cs, gs, ALIGN)
    # pairs 0 and 1, ordinary: every row written and finite; pair 0 bit for bit the padded pair 0
    assert torch.isfinite(gq[:5]).all() and torch.isfinite(gc[:5]).all()
    assert not (gq[:5] == SENTINEL).any() and not (gc[:5] == SENTINEL).any()
    pad_q, pad_c = _run_padded(amd, name, slice(0, 1))
    assert torch.equal(gq[:3], pad_q[0, :3]) and torch.equal(gc[:2], pad_c[0, :2])
    # pair 2: the query's first 4 rows and the candidate's 2 are NaN, the query's fifth row has no writer
    assert torch.isnan(gq[5:9]).all() and torch.isnan(gc[5:7]).all()
    assert (gq[9] == SENTINEL).all()


@pytest.mark.parametrize('weighted', [False, True])
def test_l2sup_negative_alignment_poisons_the_pair(amd, weighted):
    """the host layer raises on a negative index (pair_distances.py); given to the kernel it reads nothing: NaN on the valid rows"""
    q, c, gs = _inputs()
    name = 'l2sup_weighted' if weighted else 'l2sup'
    gq, gc = _run(amd, name, _padded_set(amd, q[:1], Q_LENS[:1]), _padded_set(amd, c[:1], C_LENS[:1]), gs[:1], [[-1, 0]])
    assert torch.isnan(gq[:3]).all() and torch.isnan(gc[:2]).all()
    assert torch.count_nonzero(gq[3:]) == 0 and torch.count_nonzero(gc[2:]) == 0
