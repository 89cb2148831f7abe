"""Torch-tensor front end of the C ABI: device memory and streams come from PyTorch-ROCm, every
computation happens in libaspire_hip.so.  All tensors given here must already live on the GPU."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import RepSet, OtParams, lib, check

D = 768


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError('aspire_amd needs an AMD GPU (PyTorch-ROCm sees none); there is no CPU fallback.')
    return torch.device('cuda', torch.cuda.current_device())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _f32(t, name):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), f'{name}: need contiguous fp32 GPU tensor'
    return t


def _i32(t, name):
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous(), f'{name}: need contiguous int32 GPU tensor'
    return t


# None: every rep set decides from a sample of its rows (center_hint: a few small kernels + one host sync per NEW row matrix);
# True / False: the answer for every call (set_center_hint) -- e.g. False for a process that knows its vectors are isotropic,
# True for one that scores a sentence-embedding space, so that all shards and call forms of a job use one arithmetic.
CENTER_HINT = None


def set_center_hint(mode):
    global CENTER_HINT
    assert mode in (None, True, False)
    CENTER_HINT = mode


def _rows_key(rows):
    """What a cache derived from a row matrix is valid for: the same memory, the same number of rows, not written since.  Two
    counters: the library's own generation (`_aspire_gen` on the tensor object, bumped by _rows_written: the entry points of this
    module that write rows through the C ABI report theirs) and torch's count of in-place writes (rows._version, shared by a matrix
    and its views) where torch keeps one -- a tensor made under torch.inference_mode() tracks no version (reading it raises): for
    those only the library's own writes are seen, a torch write into such a store needs drop_planes() / prepare_planes() by hand."""
    version = None if rows.is_inference() else rows._version
    return (rows.data_ptr(), int(rows.shape[0]), version, getattr(rows, '_aspire_gen', 0))


def _rows_written(t):
    """The library wrote into `t` behind torch's back (a kernel given its data pointer): caches keyed by _rows_key(t) are stale."""
    t._aspire_gen = getattr(t, '_aspire_gen', 0) + 1
    if not t.is_inference():
        torch.autograd.graph.increment_version(t)


_REBUILD_WARNED = False


def _warn_rebuild(what):
    """An automatic rebuild of a cache (planes: ~2.5 ms per GB of rows; boxes: 6 KB per document) inside a scoring call: said once."""
    global _REBUILD_WARNED
    if not _REBUILD_WARNED:
        _REBUILD_WARNED = True
        import warnings
        warnings.warn(f'aspire_amd: the rows of a resident store were written after its {what} were prepared; they are formed again '
                      'inside this scoring call (and on every call that follows a write -- torch counts writes through ANY view of the '
                      'buffer).  Prepare the caches after the last write to keep this out of the scoring path.')


def _match_planes(q, c, pairing):
    """An all-against-all call on a big pool that carries fp16 planes (DeviceRepSet.prepare_planes): the queries get
    theirs, around the pool's centre, unless they are rows of the same matrix already (then nothing happens) or carry planes the
    CALLER prepared around another store's centre (left alone: the call takes the kernels that read the fp32 rows).  Planes this
    function made earlier are kept on the query matrix and reused only while they are valid: same rows, not written since
    (_rows_key), same centre as THIS pool -- otherwise they are made again.  ~10 us for 256 query rows."""
    if pairing != _lib.PAIR_CROSS or c.planes is None or q.ext or c.ext:
        return
    slot = max(8, (c.max_len + 3) // 4 * 4)
    if c.n * slot < 128 * 128 or max(q.max_len, c.max_len) > 32:          # fewer than 128 candidate tiles: the small-pool kernels
        return
    qp = q.planes
    if qp is None or (qp.auto and qp.mu.data_ptr() != c.planes.mu.data_ptr()):
        q.prepare_planes(like=c)
        q.planes.auto = True


class RowPlanes:
    """struct aspire_rep_planes of a row matrix + the device blob it points into."""

    def __init__(self, rows, mu=None):
        _f32(rows, 'rows')
        n = int(rows.shape[0])
        nbytes = lib.aspire_rep_planes_bytes(n)
        self.blob = torch.empty(nbytes, device=rows.device, dtype=torch.uint8)
        self.mu = mu                       # tensor [768] (the store's common vector); None: formed from these rows
        self.mu_given = mu is not None
        self.auto = False                  # made by _match_planes for a call (not by the caller)
        self.key = _rows_key(rows)
        self.c = _lib.RepPlanes()
        check(lib.aspire_rep_planes_prepare(_ptr(rows), n, D, _ptr(_f32(mu, 'mu')) if mu is not None else None, _ptr(self.blob),
                                            nbytes, ctypes.byref(self.c), _stream()))
        if mu is None:
            self.mu = self.blob[:4 * D].view(torch.float32)


class DeviceRepSet:
    """Rows + CSR view of sentence reps resident in HBM (struct aspire_repset).

    rows [total, 768] fp32; start/len int32 [n]; ext > 0 marks a padded [n, ext, 768] tensor."""

    def __init__(self, rows, start, lens, ext=0, max_len=None, lens_host=None):
        self.lens_host = list(lens_host) if lens_host is not None else None      # host copy of len[], when the caller has one
        self.rows = _f32(rows, 'rows')
        assert rows.shape[-1] == D, f'encoding dim must be {D}'
        self.start = _i32(start, 'start')
        self.len = _i32(lens, 'len')
        self.n = int(start.numel())
        assert lens.numel() == self.n
        self.ext = int(ext)
        self.max_len = int(max_len if max_len is not None else (ext if ext > 0 else (int(lens.max()) if self.n else 0)))
        # A document without sentences: the reference raises (torch.max over an empty dimension, pair_distances.py:57 via
        # models.py:190-197); scored here it would come back as OT distance 0 = the best possible similarity.  Checked
        # wherever the lengths are known on the host (every constructor of the host layer passes them).
        if self.lens_host is not None and any(n <= 0 for n in self.lens_host):
            raise ValueError('a document without sentence rows cannot be scored (the reference raises on it: '
                             'pair_distances.py:57); drop it from the pool')

    @classmethod
    def from_padded(cls, reps, abs_lens):
        """reps [B, S, 768] (any device) + abs_lens list -> padded repset on the GPU."""
        dev = require_gpu()
        reps = reps.to(device=dev, dtype=torch.float32).contiguous()
        b, s, _ = reps.shape
        start = torch.arange(b, device=dev, dtype=torch.int32) * s
        lens_host = [int(n) for n in abs_lens]
        lens = torch.as_tensor(lens_host, dtype=torch.int32).to(dev)
        assert lens.numel() == b, 'abs_lens must have one entry per batch element'
        return cls(reps.view(b * s, D), start, lens, ext=s, lens_host=lens_host)

    @classmethod
    def from_list(cls, reps_list):
        """list of [S_i, 768] arrays/tensors -> CSR repset on the GPU (no padding rows)."""
        dev = require_gpu()
        ts = [torch.as_tensor(r, dtype=torch.float32) for r in reps_list]
        lens_host = [int(t.shape[0]) for t in ts]
        rows = torch.cat(ts, dim=0).to(dev).contiguous() if ts else torch.zeros(0, D, device=dev)
        lens = torch.tensor(lens_host, dtype=torch.int32)
        start = (torch.cumsum(lens, 0) - lens).to(torch.int32)
        return cls(rows, start.to(dev), lens.to(dev), ext=0, max_len=max(lens_host) if lens_host else 0, lens_host=lens_host)

    def struct(self):
        planes = self.planes                                     # kept on the matrix: index lists and slices of it share them
        return RepSet(_ptr(self.rows), _ptr(self.start), _ptr(self.len), self.n, self.ext, self.max_len,
                      ctypes.pointer(planes.c) if planes is not None else None, _ptr(self._fresh_boxes()))

    def _fresh_boxes(self):
        box = getattr(self, 'doc_box', None)
        if box is not None and getattr(self, '_doc_box_key', None) not in (None, _rows_key(self.rows)):
            self.doc_box = None                                  # the rows were written since: formed again
            _warn_rebuild('per-document boxes')
            self.prepare_boxes()
            box = self.doc_box
        return box

    def prepare_boxes(self):
        """The documents' per-coordinate bounding boxes [n, 2, 768], kept with this rep set (include/aspire_hip.h:
        aspire_repset.doc_box): the many-query otAspire calls on a resident pool then skip their pass over every candidate row
        (geomloss's diameter).  6 KB per document; formed again when the rows have been written since (_rows_key).  Returns self."""
        if self.n and getattr(self, 'doc_box', None) is None:
            box = torch.empty(self.n, 2, D, device=self.rows.device, dtype=torch.float32)
            s = RepSet(_ptr(self.rows), _ptr(self.start), _ptr(self.len), self.n, self.ext, self.max_len, None, None)
            check(lib.aspire_repset_boxes_f32(ctypes.byref(s), D, _ptr(box), _stream()))
            self.doc_box = box
            self._doc_box_key = _rows_key(self.rows)
        return self

    def slice(self, lo, hi):
        r = DeviceRepSet(self.rows, self.start[lo:hi].contiguous(), self.len[lo:hi].contiguous(), self.ext,
                         self.max_len, lens_host=self.lens_host[lo:hi] if self.lens_host is not None else None)
        if self._fresh_boxes() is not None:
            r.doc_box = self.doc_box[lo:hi]
            r._doc_box_key = self._doc_box_key
        return r

    @property
    def planes(self):
        """The matrix's fp16 planes, or None.  Planes are a cache of the rows: when the rows have been written since they were
        made (or the tensor now points elsewhere), planes the caller prepared are made again the same way (own centre / the centre
        given then), planes made for a call (_match_planes) are dropped.  The rebuild keeps the CENTRE the planes had (a copy of it):
        the shards of one pool share rank 0's centre (parallel.py), and a shard that formed a new one on its own would leave the
        bit-equality of sharded and un-sharded scores behind; any common vector serves as a centre, L2 distances do not move."""
        pl = getattr(self.rows, '_aspire_planes', None)
        if pl is not None and pl.key != _rows_key(self.rows):
            if pl.auto:
                self.rows._aspire_planes = pl = None
            else:
                _warn_rebuild('fp16 planes')
                was_given = pl.mu_given
                self.rows._aspire_planes = pl = RowPlanes(self.rows, pl.mu.clone())
                pl.mu_given = was_given
        return pl

    def prepare_planes(self, like=None, mu=None):
        """The row matrix a second time as fp16 planes (include/aspire_hip.h: aspire_rep_planes): once per resident store;
        for query sets that are not part of the store, per call with like = the store's rep set (its common vector).  The
        many-query cost tiles then run on the fp16 matrix pipe.  Returns self."""
        if like is not None:
            assert like.planes is not None, 'prepare the store\'s planes first'
            mu = like.planes.mu
        self.rows._aspire_planes = RowPlanes(self.rows, mu)
        return self

    def drop_planes(self):
        if getattr(self.rows, '_aspire_planes', None) is not None:
            self.rows._aspire_planes = None
        return self

    def center_hint(self):
        if CENTER_HINT is not None:
            return CENTER_HINT
        return self._center_hint_sampled()

    def _center_hint_sampled(self):
        """True when the rows share a large common component (|mean row|^2 > 0.25 x the mean squared norm, i.e. a mean cosine of
        roughly 0.25 between unrelated rows -- sentence-embedding spaces are usually far above that): the scoring calls then set
        ASPIRE_OT_FLAG_CENTER / ASPIRE_CDIST_CENTER (include/aspire_hip.h).  From a sample of up to 512 rows, once per rep set."""
        if getattr(self, '_center_hint', None) is None:
            hint = getattr(self.rows, '_aspire_center_hint', None)     # kept on the matrix: index lists into it share the answer
            if hint is None:
                n = int(self.rows.shape[0])
                if n == 0:
                    hint = False
                else:
                    sample = self.rows[::max(1, n // 512)][:512]
                    m = sample.mean(0)
                    hint = bool((m * m).sum() > 0.25 * (sample * sample).sum(1).mean())      # (elementwise + reductions: no rocBLAS in the product path)
                self.rows._aspire_center_hint = hint
            self._center_hint = hint
        return self._center_hint

    def host_lens(self):
        if self.lens_host is None:
            self.lens_host = self.len.cpu().tolist()
        return self.lens_host


def _npairs(q, c, pairing):
    return q.n if pairing == _lib.PAIR_PAIRED else q.n * c.n


def span_mean_pool(hidden, tok_idx, span_off, max_sents, want_cls=True):
    """A2/A3 (ex_aspire_consent.py:75-100).  hidden [B,L,768] GPU fp32 -> (cls [B,768], sent [B,S,768])."""
    _f32(hidden, 'hidden')
    b, l, d = hidden.shape
    sent = torch.empty(b, max_sents, d, device=hidden.device, dtype=torch.float32)
    cls = torch.empty(b, d, device=hidden.device, dtype=torch.float32) if want_cls else None
    check(lib.aspire_span_mean_pool_f32(_ptr(hidden), b, l, d, _ptr(_i32(tok_idx, 'tok_idx')),
                                        _ptr(_i32(span_off, 'span_off')), max_sents, _ptr(sent), _ptr(cls), _stream()))
    return cls, sent


def span_mean_pool_rows(hidden, tok_idx, span_off, max_sents, out_row, rows, cls=None):
    """The pooling written straight into a resident rep store (include/aspire_hip.h: aspire_span_mean_pool_rows_f32): slot
    (b, s) -> rows[out_row[b * S + s]] (skipped when negative); cls [B, 768] optional.  Nothing is returned: `rows` (a view
    into the store's row matrix) and `cls` are filled in place."""
    _f32(hidden, 'hidden')
    _f32(rows, 'rows')
    b, l, d = hidden.shape
    assert out_row.numel() == b * max_sents
    check(lib.aspire_span_mean_pool_rows_f32(_ptr(hidden), b, l, d, _ptr(_i32(tok_idx, 'tok_idx')), _ptr(_i32(span_off, 'span_off')),
                                             max_sents, _ptr(_i32(out_row, 'out_row')), _ptr(rows), _ptr(cls), _stream()))
    _rows_written(rows)


def span_pool_ranges(hidden, row_doc, row_start, row_len, rows=None, out_row=None, cls=None):
    """Ragged span pooling (include/aspire_hip.h: aspire_span_pool_ranges_f32; models.py:437-477): row r = the mean of
    hidden[row_doc[r], row_start[r] : row_start[r] + row_len[r]] (int32 [R] GPU tensors; the caller has checked their ranges),
    written to rows[out_row[r]] (rows[r] without out_row).  rows None: a new [R, 768] matrix.  cls [B, 768] optional, filled with
    hidden[:, 0].  Returns rows."""
    _f32(hidden, 'hidden')
    b, l, d = hidden.shape
    r = int(row_doc.numel())
    assert row_start.numel() == r and row_len.numel() == r and (out_row is None or out_row.numel() == r)
    if rows is None:
        assert out_row is None, 'out_row needs the row matrix it indexes'
        rows = torch.empty(r, d, device=hidden.device, dtype=torch.float32)
    _f32(rows, 'rows')
    if cls is not None:
        assert _f32(cls, 'cls').shape == (b, d)
    check(lib.aspire_span_pool_ranges_f32(_ptr(hidden), b, l, d, _ptr(_i32(row_doc, 'row_doc')), _ptr(_i32(row_start, 'row_start')),
                                          _ptr(_i32(row_len, 'row_len')), r, _ptr(_i32(out_row, 'out_row') if out_row is not None else None),
                                          _ptr(rows), _ptr(cls), _stream()))
    _rows_written(rows)
    return rows


def cls_l2(q_cls, c_cls, pairing=_lib.PAIR_PAIRED, eps=1e-6):
    """functional.pairwise_distance(q_cls, c_cls, p=2.0) (disent_models.py:306): ||q - c + eps||_2, [P] on the GPU."""
    _f32(q_cls, 'q_cls')
    _f32(c_cls, 'c_cls')
    qn, cn = q_cls.shape[0], c_cls.shape[0]
    out = torch.empty(cn if pairing == _lib.PAIR_PAIRED else qn * cn, device=q_cls.device, dtype=torch.float32)
    check(lib.aspire_cls_l2_f32(_ptr(q_cls), qn, _ptr(c_cls), cn, D, pairing, float(eps), _ptr(out), _stream()))
    return out


def cls_l2_backward(q_cls, c_cls, grad, eps=1e-6, out=None):
    """The gradient of the PAIRED cls_l2 distances (aspire_cls_l2_backward_f32): grad [B] = dLoss / ddist -> (grad_q, grad_c) [B, 768],
    grad_q = (q - c + eps) * grad / dist with the distance formed again as the forward forms it, grad_c = -grad_q.  out: the two
    buffers to write into instead of new ones (every row is written)."""
    _f32(q_cls, 'q_cls')
    _f32(c_cls, 'c_cls')
    assert q_cls.dim() == 2 and q_cls.shape == c_cls.shape, 'paired distances need equal batch sizes'
    grad = _f32(grad, 'grad')
    assert grad.numel() == q_cls.shape[0], 'grad: one entry per pair'
    gq, gc = out if out is not None else (torch.empty_like(q_cls), torch.empty_like(c_cls))
    assert _f32(gq, 'grad_q').shape == q_cls.shape and _f32(gc, 'grad_c').shape == c_cls.shape
    check(lib.aspire_cls_l2_backward_f32(_ptr(q_cls), q_cls.shape[0], _ptr(c_cls), c_cls.shape[0], q_cls.shape[1], _lib.PAIR_PAIRED,
                                         float(eps), _ptr(grad), _ptr(gq), _ptr(gc), _stream()))
    return gq, gc


def span_mean_pool_backward(grad_sent, grad_cls, tok_idx, span_off, B, L, max_sents, out=None):
    """The gradient of span_mean_pool with respect to hidden (aspire_span_mean_pool_backward_f32): grad_sent [B, max_sents, 768] or
    None, grad_cls [B, 768] or None (None: that output took no part in the loss) -> grad_hidden [B, L, 768] on the GPU, every element
    written by the kernel (tokens of no span: exact zeros).  out: the buffer to write into instead of a new one."""
    _i32(span_off, 'span_off')
    assert span_off.numel() == B * max_sents + 1, 'span_off: one entry per (document, slot) and the end'
    if grad_sent is not None:
        assert _f32(grad_sent, 'grad_sent').shape == (B, max_sents, D)
    if grad_cls is not None:
        assert _f32(grad_cls, 'grad_cls').shape == (B, D)
    grad_hidden = out if out is not None else torch.empty(B, L, D, device=span_off.device, dtype=torch.float32)
    assert _f32(grad_hidden, 'grad_hidden').shape == (B, L, D)
    check(lib.aspire_span_mean_pool_backward_f32(_ptr(grad_sent), _ptr(grad_cls), B, L, D, _ptr(_i32(tok_idx, 'tok_idx')), _ptr(span_off),
                                                 max_sents, _ptr(grad_hidden), _stream()))
    return grad_hidden


def bert_pooler(cls, weight, bias):
    """HF BertPooler on CLS rows (aspire_bert_pooler_f32): tanh(cls @ weight.T + bias), cls [B, 768], weight [768, 768] (nn.Linear
    layout), bias [768] -> [B, 768] on the GPU."""
    _f32(cls, 'cls')
    _f32(weight, 'weight')
    _f32(bias, 'bias')
    assert cls.dim() == 2 and tuple(weight.shape) == (cls.shape[1], cls.shape[1]) and tuple(bias.shape) == (cls.shape[1],), \
        'bert_pooler: cls [B, D], weight [D, D], bias [D]'
    out = torch.empty_like(cls)
    check(lib.aspire_bert_pooler_f32(_ptr(cls), cls.shape[0], cls.shape[1], _ptr(weight), _ptr(bias), _ptr(out), _stream()))
    return out


def token_mean_pool(hidden, mask, normalize=False):
    """sentence-transformers' Pooling(mean) [+ Normalize] (aspire_token_mean_pool_f32): hidden [B, L, 768] fp32, mask [B, L] (non-zero
    = real token) -> [B, 768] on the GPU: the masked mean of the token rows, then, with normalize, x / max(||x||, 1e-12)."""
    _f32(hidden, 'hidden')
    assert hidden.dim() == 3 and tuple(mask.shape) == tuple(hidden.shape[:2]), 'token_mean_pool: hidden [B, L, D], mask [B, L]'
    mask = mask.to(device=hidden.device, dtype=torch.int64).contiguous()
    b, l, d = hidden.shape
    out = torch.empty(b, d, device=hidden.device, dtype=torch.float32)
    check(lib.aspire_token_mean_pool_f32(_ptr(hidden), _ptr(mask), b, l, d, 1 if normalize else 0, _ptr(out), _stream()))
    return out


def _ot_params(c, blur, scaling, sent_sm_temp, cdist_mode, one_form):
    """struct aspire_ot_params of an otAspire call with its flag word: ONE_FORM as the caller asks, CENTER from the candidates' rows
    (DeviceRepSet.center_hint)."""
    return OtParams(float(blur), float(scaling), float(sent_sm_temp), cdist_mode,
                    (_lib.OT_FLAG_ONE_FORM if one_form else 0) | (_lib.OT_FLAG_CENTER if c.center_hint() else 0))


def _cdist_flags(c, cdist_mode, one_form):
    """The same two flags on the cdist_mode word of the max-sim entries (ASPIRE_CDIST_ONE_FORM / ASPIRE_CDIST_CENTER)."""
    if one_form:
        cdist_mode |= _lib.CDIST_ONE_FORM
    if c.center_hint():
        cdist_mode |= _lib.CDIST_CENTER
    return cdist_mode


def l2max_scores(q, c, pairing=_lib.PAIR_CROSS, cdist_mode=_lib.CDIST_AUTO, want_pair_sims=False, one_form=False):
    """A9 (pair_distances.py:138-186).  Returns sims [P] (and pair_sims [P, q.ext, c.ext]).  one_form: see
    include/aspire_hip.h, ASPIRE_CDIST_ONE_FORM."""
    cdist_mode = _cdist_flags(c, cdist_mode, one_form)
    p = _npairs(q, c, pairing)
    dev = q.rows.device
    scores = torch.empty(p, device=dev, dtype=torch.float32)
    pair = torch.empty(p, q.ext, c.ext, device=dev, dtype=torch.float32) if want_pair_sims else None
    _match_planes(q, c, pairing)
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_l2max_scores_f32(ctypes.byref(qs), ctypes.byref(cs), D, pairing, cdist_mode, _ptr(scores),
                                      _ptr(pair), _stream()))
    return (scores, pair) if want_pair_sims else scores


def l2agg_scores(q, c, agg, temp=1.0, pairing=_lib.PAIR_CROSS, cdist_mode=_lib.CDIST_AUTO, want_pair_sims=False):
    """Sibling aggregations of the masked -cdist block: agg = _lib.AGG_TOP2 (pair_distances.py:295-345) or
    _lib.AGG_ATTENTION (pair_distances.py:95-135; temp = cdatt_sm_temp).  Returns sims [P]; with want_pair_sims also
    pair_sims [P, q.ext, c.ext] and, for attention, pair_softmax [P, q.ext, c.ext]."""
    p = _npairs(q, c, pairing)
    dev = q.rows.device
    scores = torch.empty(p, device=dev, dtype=torch.float32)
    pair = torch.empty(p, q.ext, c.ext, device=dev, dtype=torch.float32) if want_pair_sims else None
    soft = torch.empty(p, q.ext, c.ext, device=dev, dtype=torch.float32) \
        if want_pair_sims and agg == _lib.AGG_ATTENTION else None
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_l2agg_scores_f32(ctypes.byref(qs), ctypes.byref(cs), D, pairing, cdist_mode, agg,
                                      ctypes.c_double(temp), _ptr(scores), _ptr(pair), _ptr(soft), _stream()))
    if not want_pair_sims:
        return scores
    return (scores, pair, soft) if agg == _lib.AGG_ATTENTION else (scores, pair)


def _grad_call_args(q, c, grad_scores, out):
    """What the backward entries share: the checked grad_scores [P] and the two gradient buffers laid out like q.rows / c.rows."""
    assert q.n == c.n, 'paired scoring needs equal batch sizes'      # pair_distances.py:46
    grad_scores = _f32(grad_scores, 'grad_scores')
    assert grad_scores.numel() == q.n, 'grad_scores: one entry per pair'
    gq, gc = out if out is not None else (torch.zeros_like(q.rows), torch.zeros_like(c.rows))
    assert _f32(gq, 'grad_q_rows').shape == q.rows.shape and _f32(gc, 'grad_c_rows').shape == c.rows.shape
    return grad_scores, gq, gc


def l2agg_backward(q, c, agg, grad_scores, temp=1.0, out=None):
    """The gradient of the PAIRED similarities of l2max_scores (agg = _lib.AGG_MAX) / l2agg_scores (AGG_TOP2, AGG_ATTENTION) with
    respect to the sentence rows (include/aspire_hip.h: aspire_l2agg_backward_f32).  grad_scores [P] = dLoss / dscore.  Returns
    (grad_q_rows, grad_c_rows), laid out like q.rows / c.rows: every row of every document is written by the kernel (pad rows with
    zeros); rows of the matrices that no document owns stay zero.  out: the two buffers to write into instead of new ones."""
    grad_scores, gq, gc = _grad_call_args(q, c, grad_scores, out)
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_l2agg_backward_f32(ctypes.byref(qs), ctypes.byref(cs), D, _lib.PAIR_PAIRED, agg, ctypes.c_double(temp),
                                        _ptr(grad_scores), _ptr(gq), _ptr(gc), _stream()))
    return gq, gc


def ot_backward(q, c, grad_scores, *, blur=0.05, scaling=0.9, sent_sm_temp=1.0, diameter=None, diam_group=0, want=_lib.OT_DISTANCE,
                out=None):
    """The gradient of the PAIRED otAspire scores of ot_sinkhorn (want = _lib.OT_DISTANCE or OT_SIMILARITY) with respect to the
    sentence rows (include/aspire_hip.h: aspire_ot_backward_f32 -- a restatement of geomloss's detach pattern).  grad_scores [P] =
    dLoss / dscore; diameter / diam_group: what the forward was given (None: every pair's own box).  Returns (grad_q_rows,
    grad_c_rows), laid out like q.rows / c.rows: every row of every document is written by the kernel (pad rows with zeros); rows of
    the matrices that no document owns stay zero.  out: the two buffers to write into instead of new ones."""
    grad_scores, gq, gc = _grad_call_args(q, c, grad_scores, out)
    if diameter is not None:
        assert diam_group > 0, 'diam_group must be positive'
        assert _f32(diameter, 'diameter').numel() >= (q.n + diam_group - 1) // diam_group, 'diameter: one entry per group of pairs'
    prm = OtParams(float(blur), float(scaling), float(sent_sm_temp), _lib.CDIST_AUTO, 0)      # (cdist_mode, flags: not read)
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_ot_backward_f32(ctypes.byref(qs), ctypes.byref(cs), D, _lib.PAIR_PAIRED, ctypes.byref(prm), _ptr(diameter),
                                     diam_group, want, _ptr(grad_scores), _ptr(gq), _ptr(gc), _stream()))
    return gq, gc


def group_diameter(q, c, pairing, group):
    ngroups = (c.n + group - 1) // group
    n = ngroups if pairing == _lib.PAIR_PAIRED else q.n * ngroups
    out = torch.empty(max(n, 1), device=q.rows.device, dtype=torch.float32)
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_group_diameter_f32(ctypes.byref(qs), ctypes.byref(cs), D, pairing, group, _ptr(out), _stream()))
    return out


def ot_sinkhorn(q, c, pairing=_lib.PAIR_CROSS, blur=0.05, scaling=0.9, sent_sm_temp=1.0, cdist_mode=_lib.CDIST_AUTO,
                diameter=None, diam_group=0, want=_lib.OT_DISTANCE, want_extras=False, out=None, workspace=None, one_form=False):
    """A5-A8 (pair_distances.py:21-92).  Returns scores [P]; with want_extras also
    (query_distr [P,q.ext], cand_distr [P,c.ext], pair_sims [P,q.ext,c.ext], plan [P,q.ext,c.ext])."""
    p = _npairs(q, c, pairing)
    dev = q.rows.device
    scores = out if out is not None else torch.empty(p, device=dev, dtype=torch.float32)
    assert scores.numel() >= p
    extras = [None] * 4
    if want_extras:
        extras = [torch.empty(p, q.ext, device=dev), torch.empty(p, c.ext, device=dev),
                  torch.empty(p, q.ext, c.ext, device=dev), torch.empty(p, q.ext, c.ext, device=dev)]
    prm = _ot_params(c, blur, scaling, sent_sm_temp, cdist_mode, one_form)
    _match_planes(q, c, pairing)
    qs, cs = q.struct(), c.struct()
    nbytes = lib.aspire_ot_workspace_bytes(ctypes.byref(qs), ctypes.byref(cs), pairing)
    ws = workspace if workspace is not None else torch.empty(max(nbytes, 8), device=dev, dtype=torch.uint8)
    check(lib.aspire_ot_sinkhorn_f32(ctypes.byref(qs), ctypes.byref(cs), D, pairing, ctypes.byref(prm),
                                     _ptr(diameter), diam_group, want, _ptr(scores), _ptr(extras[0]), _ptr(extras[1]),
                                     _ptr(extras[2]), _ptr(extras[3]), _ptr(ws), ws.numel(), _stream()))
    return (scores, extras) if want_extras else scores


def ot_rank(q, c, k, blur=0.05, scaling=0.9, sent_sm_temp=1.0, cdist_mode=_lib.CDIST_AUTO, diameter=None, diam_group=0,
            want=_lib.OT_DISTANCE, idx_base=0, key_form=False, one_form=False):
    """The ranking step in one call (include/aspire_hip.h: aspire_ot_rank_f32): otAspire scores [Q, C] of every
    query against every candidate and their per-query stable descending rank.  Returns (scores [Q, C], top_scores
    [Q, k], top_idx [Q, k]) -- `scores` holds the raw kernel output (positive distances for OT_DISTANCE, so the rank
    is of the OUTPUT; pass want=OT_PLAN_SIM for similarities) -- or (scores, keys [Q, k]) with key_form."""
    dev = q.rows.device
    scores = torch.empty(q.n, c.n, device=dev, dtype=torch.float32)
    prm = _ot_params(c, blur, scaling, sent_sm_temp, cdist_mode, one_form)
    _match_planes(q, c, _lib.PAIR_CROSS)
    qs, cs = q.struct(), c.struct()
    nbytes = lib.aspire_ot_rank_workspace_bytes(ctypes.byref(qs), ctypes.byref(cs), k)
    ws = torch.empty(max(nbytes, 8), device=dev, dtype=torch.uint8)
    top_s = top_i = keys = None
    if key_form:
        keys = torch.empty(q.n, k, device=dev, dtype=torch.int64)
    else:
        top_s = torch.empty(q.n, k, device=dev, dtype=torch.float32)
        top_i = torch.empty(q.n, k, device=dev, dtype=torch.int64)
    check(lib.aspire_ot_rank_f32(ctypes.byref(qs), ctypes.byref(cs), D, ctypes.byref(prm), _ptr(diameter), diam_group, want,
                                 _ptr(scores), k, idx_base, _ptr(top_s), _ptr(top_i), _ptr(keys), _ptr(ws), ws.numel(), _stream()))
    return (scores, keys) if key_form else (scores, top_s, top_i)


def _rank_outputs(J, C, k, dev, out, key_form):
    """(scores, top_scores, top_idx, keys) of a batched rank call over J jobs and C candidates: the caller's `out` taken apart, or
    fresh tensors (None for what the call does not write)."""
    if out is not None and key_form:
        scores, keys = out
        return scores, None, None, keys
    if out is not None:
        return (*out, None)
    return (torch.empty(C, device=dev, dtype=torch.float32),
            torch.empty(J, k, device=dev, dtype=torch.float32) if k > 0 and not key_form else None,
            torch.empty(J, k, device=dev, dtype=torch.int64) if k > 0 and not key_form else None,
            torch.empty(J, k, device=dev, dtype=torch.int64) if k > 0 and key_form else None)


def _rank_batch(entry, mid, q, c, job_off, max_job, k, out, workspace, job_base, key_form):
    """What the batched rank wrappers share.  `entry` names the pair of library entries (_RANK_BATCH); `mid()` gives the arguments
    that sit between max_job and scores in its C signature -- all that differs between them -- once the checks have passed."""
    call, workspace_bytes = _RANK_BATCH[entry]
    dev = q.rows.device
    _i32(job_off, 'job_off')
    assert job_off.numel() == q.n + 1, 'job_off must have one entry per job plus one'
    scores, top_s, top_i, keys = _rank_outputs(q.n, c.n, k, dev, out, key_form)
    mid = mid()
    qs, cs = q.struct(), c.struct()
    if workspace is None:
        nbytes = workspace_bytes(ctypes.byref(qs), ctypes.byref(cs), max_job, k)
        workspace = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    check(call(ctypes.byref(qs), ctypes.byref(cs), D, _ptr(job_off), max_job, *mid, _ptr(scores), k, _ptr(job_base), _ptr(top_s),
               _ptr(top_i), _ptr(keys), _ptr(workspace), workspace.numel(), _stream()))
    return (scores, keys) if key_form else (scores, top_s, top_i)


def ot_rank_batch(q, c, job_off, max_job, k, blur=0.05, scaling=0.9, sent_sm_temp=1.0, cdist_mode=_lib.CDIST_AUTO,
                  want=_lib.OT_SIMILARITY, out=None, workspace=None, job_base=None, key_form=False, one_form=False):
    """J independent (query, pool) re-ranks in ONE call (include/aspire_hip.h: aspire_ot_rank_batch_f32; the per-query
    loop of evaluate.py:58-76 batched over queries).  q: J queries; c: every job's candidates back to back; job_off int32
    GPU tensor [J + 1]; max_job: host-known bound of a pool's size.  Returns (scores [C], top_scores [J, k], top_idx [J, k])
    with top_idx = position inside the job's own pool (+ job_base[j], int32 GPU tensor [J], when this rank holds one
    block of every pool); `out` = preallocated (scores, top_scores, top_idx).  key_form: (scores, keys [J, k]) -- the
    sortable keys of topk_keys, what a shard contributes to the all-gather."""
    def mid():
        return ctypes.byref(_ot_params(c, blur, scaling, sent_sm_temp, cdist_mode, one_form)), want
    return _rank_batch('ot', mid, q, c, job_off, max_job, k, out, workspace, job_base, key_form)


def l2max_rank_batch(q, c, job_off, max_job, k, cdist_mode=_lib.CDIST_AUTO, out=None, workspace=None, job_base=None, key_form=False,
                     one_form=False):
    """tsAspire over J independent (query, pool) jobs in ONE call (include/aspire_hip.h: aspire_l2max_rank_batch_f32); arguments
    and returns as ot_rank_batch: (scores [C], top_scores [J, k], top_idx [J, k]) or (scores, keys [J, k]) with key_form."""
    cdist_mode = _cdist_flags(c, cdist_mode, one_form)
    return _rank_batch('l2max', lambda: (cdist_mode,), q, c, job_off, max_job, k, out, workspace, job_base, key_form)


def l2agg_rank_batch(q, c, job_off, max_job, k, agg, temp=1.0, cdist_mode=_lib.CDIST_AUTO, out=None, key_form=False, job_base=None,
                     workspace=None):
    """The sibling aggregations 'l2top2' (agg=AGG_TOP2) / 'l2attention' (AGG_ATTENTION, temp = cdatt_sm_temp) over J independent
    (query, pool) jobs in ONE call (include/aspire_hip.h: aspire_l2agg_rank_batch_f32); arguments and returns as l2max_rank_batch.
    One kernel form whatever the call's size: a pair's score depends on its two documents only."""
    return _rank_batch('l2agg', lambda: (cdist_mode, agg, float(temp)), q, c, job_off, max_job, k, out, workspace, job_base, key_form)


def _dot_ready(*sets):
    """The host-side contract of the dot-product max-sim entries: every document has a row (np.max over an empty similarity
    block raises in the reference) and every row is finite (sklearn's check_array raises ValueError on inf / NaN).  The finite
    check runs once per row matrix and is kept until its rows are written (_rows_key)."""
    for s in sets:
        if s.n == 0:
            continue
        if (min(s.lens_host) if s.lens_host is not None else int(s.len.min())) <= 0:
            raise ValueError('a document without sentence rows cannot be scored (np.max over an empty block raises); drop it')
        key = _rows_key(s.rows)
        if getattr(s.rows, '_aspire_finite', None) != key:
            if not bool(torch.isfinite(s.rows).all()):
                raise ValueError('Input contains NaN or infinity (sklearn.metrics.pairwise.cosine_similarity rejects it)')
            s.rows._aspire_finite = key


def dotmax_scores(q, c, pairing=_lib.PAIR_CROSS, sim=_lib.SIM_COSINE):
    """A13 (TrainedSentModel.get_similarity, models.py:602-604): sims [P] = max over the valid sentence pairs of sklearn's
    cosine similarity (sim=SIM_COSINE) or of the raw dot product (SIM_DOT, rank_pool_sent's 'dotlse')."""
    _dot_ready(q, c)
    p = _npairs(q, c, pairing)
    scores = torch.empty(p, device=q.rows.device, dtype=torch.float32)
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_dotmax_scores_f32(ctypes.byref(qs), ctypes.byref(cs), D, pairing, sim, _ptr(scores), _stream()))
    return scores


def dotmax_rank_batch(q, c, job_off, max_job, k, sim=_lib.SIM_COSINE, out=None, workspace=None, job_base=None, key_form=False):
    """The dot-product max-sim over J independent (query, pool) jobs in ONE call (include/aspire_hip.h:
    aspire_dotmax_rank_batch_f32); arguments and returns as l2max_rank_batch."""
    _dot_ready(q, c)
    return _rank_batch('dotmax', lambda: (sim,), q, c, job_off, max_job, k, out, workspace, job_base, key_form)


def dot_argmax(q, c, want_best=True, out=None):
    """A16 (pre_proc_cocits.py:487-494): for the PAIRED pairs, arg int32 [P, 2] = np.unravel_index(np.matmul(q, c.T).argmax(),
    (q_len, c_len)) with numpy's rule in full (first maximum in row-major order, +-0.0 tie, the first NaN wins) and best [P] = the
    dot product there, the bits of dotmax_scores(q, c, PAIR_PAIRED, SIM_DOT).  Non-finite rows are inside the contract; a document
    without rows raises ValueError, as numpy's argmax of an empty block does.  want_best=False passes best = NULL and returns
    (arg, None); out: the (arg, best) buffers to write into instead of new ones."""
    if q.n != c.n:
        raise AssertionError(f'paired arg-max needs equal batch sizes (query {q.n} vs cand {c.n})')
    for s in (q, c):
        if s.n and (min(s.lens_host) if s.lens_host is not None else int(s.len.min())) <= 0:
            raise ValueError('attempt to get argmax of an empty sequence: a document without sentence rows')
    dev = q.rows.device
    arg, best = out if out is not None else (torch.empty(q.n, 2, device=dev, dtype=torch.int32),
                                             torch.empty(q.n, device=dev, dtype=torch.float32) if want_best else None)
    assert _i32(arg, 'arg').numel() >= 2 * q.n and (best is None or _f32(best, 'best').numel() >= q.n)
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_dot_argmax_f32(ctypes.byref(qs), ctypes.byref(cs), D, _ptr(arg), _ptr(best), _stream()))
    return arg, best


def jointsm_scores(q, c, pairing=_lib.PAIR_CROSS, want_pair_softmax=False):
    """A14 (pair_distances.py:348-402 as WordSentAlignPolyEnc.score negates it back, disent_models.py:905-906): sims [P] =
    2 sum_ij p_ij <q_i, c_j> with p the soft-max of the scaled dot products over the pair's whole valid block.  With
    want_pair_softmax (padded rep sets) also pair_softmax [P, q.ext, c.ext]: p inside the valid block, 0.0 outside."""
    _dot_ready(q, c)
    p = _npairs(q, c, pairing)
    dev = q.rows.device
    scores = torch.empty(p, device=dev, dtype=torch.float32)
    soft = torch.empty(p, q.ext, c.ext, device=dev, dtype=torch.float32) if want_pair_softmax else None
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_jointsm_scores_f32(ctypes.byref(qs), ctypes.byref(cs), D, pairing, _ptr(scores), _ptr(soft), _stream()))
    return (scores, soft) if want_pair_softmax else scores


def jointsm_backward(q, c, grad_scores, out=None):
    """The gradient of the PAIRED similarities of jointsm_scores with respect to the sentence rows (include/aspire_hip.h:
    aspire_jointsm_backward_f32).  grad_scores [P] = dLoss / dscore.  Returns (grad_q_rows, grad_c_rows), laid out like q.rows /
    c.rows: every row of every document is written by the kernel (pad rows with zeros); rows of the matrices that no document owns
    stay zero.  out: the two buffers to write into instead of new ones."""
    grad_scores, gq, gc = _grad_call_args(q, c, grad_scores, out)
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_jointsm_backward_f32(ctypes.byref(qs), ctypes.byref(cs), D, _lib.PAIR_PAIRED, _ptr(grad_scores), _ptr(gq), _ptr(gc),
                                          _stream()))
    return gq, gc


def _align_i32(align, n):
    assert _i32(align, 'align').shape == (n, 2), 'align: int32 [P, 2] (query row, candidate row)'
    return align


def l2sup_scores(q, c, align, weighted=False):
    """pair_distances.py:189-292: sims [P] = -||q_i - c_j|| of the PAIRED pairs' pre-aligned sentences, (i, j) = align[p] clipped to
    the documents' last rows (weighted: divided by q_len * c_len).  align: int32 [P, 2] on the GPU, no negative entries
    (include/aspire_hip.h: aspire_l2sup_scores_f32)."""
    assert q.n == c.n, 'paired scoring needs equal batch sizes'      # pair_distances.py:221
    scores = torch.empty(q.n, device=q.rows.device, dtype=torch.float32)
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_l2sup_scores_f32(ctypes.byref(qs), ctypes.byref(cs), D, _ptr(_align_i32(align, q.n)), int(bool(weighted)),
                                      _ptr(scores), _stream()))
    return scores


def l2sup_backward(q, c, align, grad_scores, weighted=False, out=None):
    """The gradient of l2sup_scores with respect to the sentence rows (aspire_l2sup_backward_f32): two non-zero rows per pair, exact
    zeros in every other row of the pair's documents.  Arguments and returns as jointsm_backward."""
    grad_scores, gq, gc = _grad_call_args(q, c, grad_scores, out)
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_l2sup_backward_f32(ctypes.byref(qs), ctypes.byref(cs), D, _ptr(_align_i32(align, q.n)), int(bool(weighted)),
                                        _ptr(grad_scores), _ptr(gq), _ptr(gc), _stream()))
    return gq, gc


def sent_cdist(q, c):
    """disent_models.py:655 / :829 without the sign: dist [P, q.ext, c.ext] = ||q_i - c_j|| over the PAIRED pairs' whole zero-padded
    blocks (padded rep sets; a row at or beyond its document's length counts as zeros and is not read) -- include/aspire_hip.h:
    aspire_sent_cdist_f32."""
    assert q.n == c.n, 'paired scoring needs equal batch sizes'
    assert q.ext > 0 and c.ext > 0, 'the distance matrix needs padded rep sets'
    dist = torch.empty(q.n, q.ext, c.ext, device=q.rows.device, dtype=torch.float32)
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_sent_cdist_f32(ctypes.byref(qs), ctypes.byref(cs), D, _ptr(dist), _stream()))
    return dist


def sent_cdist_backward(q, c, grad_dist, out=None):
    """The gradient of sent_cdist with respect to the sentence rows (aspire_sent_cdist_backward_f32): grad_dist [P, q.ext, c.ext] =
    dLoss / ddist; the distances are formed again from the rows.  Returns and `out` as jointsm_backward."""
    assert q.n == c.n, 'paired scoring needs equal batch sizes'
    assert q.ext > 0 and c.ext > 0, 'the distance matrix needs padded rep sets'
    assert _f32(grad_dist, 'grad_dist').shape == (q.n, q.ext, c.ext), 'grad_dist: [P, q.ext, c.ext]'
    gq, gc = out if out is not None else (torch.zeros_like(q.rows), torch.zeros_like(c.rows))
    assert _f32(gq, 'grad_q_rows').shape == q.rows.shape and _f32(gc, 'grad_c_rows').shape == c.rows.shape
    qs, cs = q.struct(), c.struct()
    check(lib.aspire_sent_cdist_backward_f32(ctypes.byref(qs), ctypes.byref(cs), D, _ptr(grad_dist), _ptr(gq), _ptr(gc), _stream()))
    return gq, gc


def jointsm_rank_batch(q, c, job_off, max_job, k, out=None, workspace=None, job_base=None, key_form=False):
    """The joint soft-max alignment score over J independent (query, pool) jobs in ONE call (include/aspire_hip.h:
    aspire_jointsm_rank_batch_f32); arguments and returns as l2max_rank_batch."""
    _dot_ready(q, c)
    return _rank_batch('jointsm', lambda: (), q, c, job_off, max_job, k, out, workspace, job_base, key_form)


def dense_rank_batch(rows, q_idx, cand_idx, job_off, max_job, k, metric=_lib.DENSE_L2, out=None, workspace=None, job_base=None,
                     key_form=False):
    """The precomputed-embedding rankers' score + rank (include/aspire_hip.h: aspire_dense_rank_batch_f32; pp_gen_nearest.py
    rank_pool :683-717, rank_pool_faceted :1166-1191) over J (query, pool) jobs in ONE call on ONE resident matrix: rows [N, 768]
    fp32; q_idx int32 [J] = the matrix row of each job's query; cand_idx int32 [C] = every job's candidate rows back to back;
    job_off int32 [J + 1] -- all GPU tensors, nothing is gathered.  metric DENSE_L2 (-Euclidean distance), DENSE_COSINE or DENSE_DOT:
    similarities, higher is better.  max_job, k, out, workspace, job_base, key_form and the returns as l2max_rank_batch:
    (scores [C], top_scores [J, k], top_idx [J, k]) or (scores, keys [J, k]).  A row index outside [0, N) scores NaN (the kernel
    reads nothing for it); callers validate on the host (nearest.py)."""
    _f32(rows, 'rows')
    assert rows.dim() == 2 and rows.shape[1] == D, 'rows must be [N, 768]'
    _i32(q_idx, 'q_idx'), _i32(cand_idx, 'cand_idx'), _i32(job_off, 'job_off')
    J, C, dev = q_idx.numel(), cand_idx.numel(), rows.device
    assert job_off.numel() == J + 1, 'job_off must have one entry per job plus one'
    scores, top_s, top_i, keys = _rank_outputs(J, C, k, dev, out, key_form)
    if workspace is None:
        workspace = torch.empty(max(lib.aspire_dense_rank_batch_workspace_bytes(J, C, max_job, k), 16), device=dev, dtype=torch.uint8)
    check(lib.aspire_dense_rank_batch_f32(_ptr(rows), rows.shape[0], D, _ptr(q_idx), J, _ptr(cand_idx), C, _ptr(job_off), max_job,
                                          metric, _ptr(scores), k, _ptr(job_base), _ptr(top_s), _ptr(top_i), _ptr(keys),
                                          _ptr(workspace), workspace.numel(), _stream()))
    return (scores, keys) if key_form else (scores, top_s, top_i)


# <entry>_rank_batch -> (its library entry, that entry's workspace query)
_RANK_BATCH = {'ot': (lib.aspire_ot_rank_batch_f32, lib.aspire_ot_rank_batch_workspace_bytes),
               'l2max': (lib.aspire_l2max_rank_batch_f32, lib.aspire_l2max_rank_batch_workspace_bytes),
               'l2agg': (lib.aspire_l2agg_rank_batch_f32, lib.aspire_l2agg_rank_batch_workspace_bytes),
               'dotmax': (lib.aspire_dotmax_rank_batch_f32, lib.aspire_dotmax_rank_batch_workspace_bytes),
               'jointsm': (lib.aspire_jointsm_rank_batch_f32, lib.aspire_jointsm_rank_batch_workspace_bytes)}


def rank_batch_workspace_bytes(entry, q, c, max_job, k):
    """Bytes of `workspace` that <entry>_rank_batch (entry 'ot', 'l2max', 'l2agg', 'dotmax' or 'jointsm') needs for these sets: a host-side
    computation, for callers that keep one buffer over many calls."""
    qs, cs = q.struct(), c.struct()
    return _RANK_BATCH[entry][1](ctypes.byref(qs), ctypes.byref(cs), max_job, k)


def _topk_workspace(scores, k):
    qn, cn = scores.shape
    nbytes = lib.aspire_topk_workspace_bytes(qn, cn, k)
    return torch.empty(max(nbytes, 8), device=scores.device, dtype=torch.uint8), nbytes


def topk_desc(scores, k, idx_base=0):
    """A12 (evaluate.py:76): scores [Q, C] -> (top_scores [Q,k], top_idx [Q,k] int64), stable descending."""
    _f32(scores, 'scores')
    qn, cn = scores.shape
    top_s = torch.empty(qn, k, device=scores.device, dtype=torch.float32)
    top_i = torch.empty(qn, k, device=scores.device, dtype=torch.int64)
    ws, nbytes = _topk_workspace(scores, k)
    check(lib.aspire_topk_desc_f32(_ptr(scores), qn, cn, k, idx_base, _ptr(top_s), _ptr(top_i), _ptr(ws), nbytes,
                                   _stream()))
    return top_s, top_i


def topk_keys(scores, k, idx_base=0, out=None):
    """Per-query local top-k of scores [Q, C] as sortable int64 keys [Q, k] that carry the GLOBAL candidate index
    (include/aspire_hip.h: aspire_topk_keys_f32) -- what a shard contributes to the all-gather of section 8(e)."""
    _f32(scores, 'scores')
    qn, cn = scores.shape
    keys = out if out is not None else torch.empty(qn, k, device=scores.device, dtype=torch.int64)
    ws, nbytes = _topk_workspace(scores, k)
    check(lib.aspire_topk_keys_f32(_ptr(scores), qn, cn, k, idx_base, _ptr(keys), _ptr(ws), nbytes, _stream()))
    return keys


def topk_merge_keys(keys, k):
    """keys [R, Q, k_in] (R shards' blocks as an all-gather leaves them) -> (top_scores [Q, k], top_idx [Q, k])."""
    require_gpu()
    assert keys.dtype == torch.int64 and keys.dim() == 3 and keys.is_contiguous() and keys.is_cuda, 'keys: int64 [R, Q, k_in]'
    r, qn, k_in = keys.shape
    top_s = torch.empty(qn, k, device=keys.device, dtype=torch.float32)
    top_i = torch.empty(qn, k, device=keys.device, dtype=torch.int64)
    check(lib.aspire_topk_merge_keys(_ptr(keys), r, qn, k_in, k, _ptr(top_s), _ptr(top_i), _stream()))
    return top_s, top_i


def _i64_ids(t, name, shape=None):
    assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.dim() == 2, f'{name}: need contiguous int64 [B, L] on the GPU'
    assert shape is None or t.shape == shape, f'{name}: shape {tuple(t.shape)}, expected {tuple(shape)}'
    return t


def bert_embed_sum(tok, typ, word, pos, type_emb, out=None):
    """BertEmbeddings' sum (aspire_bert_embed_sum_f32): tok int64 [B, L], typ the same or None (all type 0), the three tables
    [rows, 768] fp32 -> emb_sum [B, L, 768] = (word[tok] + type_emb[typ]) + pos[:L], torch's bits.  A row whose id or type lies
    outside its table is NaN (never read).  out: the buffer to write into instead of a new one."""
    _i64_ids(tok, 'tok')
    if typ is not None:
        _i64_ids(typ, 'typ', tok.shape)
    for t, name in ((word, 'word'), (pos, 'pos'), (type_emb, 'type_emb')):
        assert _f32(t, name).dim() == 2 and t.shape[1] == D, f'{name}: need [rows, {D}]'
    b, l = tok.shape
    out = out if out is not None else torch.empty(b, l, D, device=tok.device, dtype=torch.float32)
    assert _f32(out, 'out').shape == (b, l, D)
    check(lib.aspire_bert_embed_sum_f32(_ptr(word), _ptr(pos), _ptr(type_emb), _ptr(tok), _ptr(typ), b, l, word.shape[0], pos.shape[0],
                                        type_emb.shape[0], _ptr(out), _stream()))
    return out


def bert_embed_backward(grad, tok, typ, vocab, max_pos, n_types, padding_idx=-1, want=(True, True, True), out=None):
    """The three tables' gradients (aspire_bert_embed_backward_f32): grad [B, L, 768] fp32, tok / typ as bert_embed_sum ->
    (grad_word [vocab, 768], grad_pos [max_pos, 768], grad_type [n_types, 768]), None where want says the table is not wanted
    (nothing is launched for it).  Every row of a wanted table is written by the kernels, in the fixed orders the header states: the
    same bits on every run.  out: three buffers (or None) to write into instead of new ones."""
    _i64_ids(tok, 'tok')
    if typ is not None:
        _i64_ids(typ, 'typ', tok.shape)
    b, l = tok.shape
    assert _f32(grad, 'grad').shape == (b, l, D)
    rows = (vocab, max_pos, n_types)
    outs = []
    for i, n in enumerate(rows):
        given = out[i] if out is not None else None
        if not want[i]:
            outs.append(None)
        elif given is not None:
            assert _f32(given, 'out').shape == (n, D)
            outs.append(given)
        else:
            outs.append(torch.empty(n, D, device=grad.device, dtype=torch.float32))
    if all(o is None for o in outs):
        return tuple(outs)
    ws = None
    if outs[0] is not None:
        ws = torch.empty(lib.aspire_bert_embed_workspace_bytes(b * l, vocab), device=grad.device, dtype=torch.uint8)
    check(lib.aspire_bert_embed_backward_f32(_ptr(grad), _ptr(tok), _ptr(typ), b, l, vocab, max_pos, n_types, padding_idx, _ptr(outs[0]),
                                             _ptr(outs[1]), _ptr(outs[2]), _ptr(ws), ws.numel() if ws is not None else 0, _stream()))
    return tuple(outs)


def optim_tensor_check(t, name):
    """What the optimizer kernels take: a dense, contiguous fp32 tensor on the GPU (a contiguous view at any storage offset is fine)."""
    if t.is_sparse:
        raise RuntimeError(f'{name}: sparse tensors are not supported')
    if not t.is_cuda:
        raise RuntimeError(f'{name}: need a GPU tensor (there is no CPU fallback)')
    if t.dtype != torch.float32:
        raise TypeError(f'{name}: need fp32, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name}: need a contiguous tensor')
    return t


OPTIM_TABLE = np.dtype([('param', 'u8'), ('grad', 'u8'), ('state1', 'u8'), ('state2', 'u8'), ('n', 'i8'), ('step', 'i8'), ('lr', 'f8')])
assert OPTIM_TABLE.itemsize == ctypes.sizeof(_lib.OptimTensor)
ADAMW_TABLE = np.dtype(OPTIM_TABLE.descr + [('weight_decay', 'f8')])
assert ADAMW_TABLE.itemsize == ctypes.sizeof(_lib.AdamWTensor)
_OPTIM_ENTRY = {'adam': lib.aspire_adam_step_f32, 'adagrad': lib.aspire_adagrad_step_f32}
# rule -> (entry that takes a grad_scale pointer, its table's dtype and record type)
_OPTIM_SCALED = {'adam': (lib.aspire_adam_step_scaled_f32, OPTIM_TABLE, _lib.OptimTensor),
                 'adagrad': (lib.aspire_adagrad_step_scaled_f32, OPTIM_TABLE, _lib.OptimTensor),
                 'adamw': (lib.aspire_adamw_step_f32, ADAMW_TABLE, _lib.AdamWTensor)}
_OPTIM_WS = {}      # (device index, stream handle) -> the device table of that stream's steps


def grad_scale_check(grad_scale, dev):
    """What the scaled steps read their coefficient from: a one-element fp32 tensor on the step's GPU (grad_norm()'s clip_coef)."""
    if not isinstance(grad_scale, torch.Tensor) or grad_scale.numel() != 1:
        raise ValueError('grad_scale: need a one-element tensor')
    optim_tensor_check(grad_scale, 'grad_scale')
    if grad_scale.device != dev:
        raise ValueError(f'grad_scale: on {grad_scale.device}, the step runs on {dev}')
    return grad_scale


def optim_launch(rule, table, scalars, dev, grad_scale=None):
    """One aspire_adam_step_f32 ('adam', scalars = (beta1, beta2, eps)) / aspire_adagrad_step_f32 ('adagrad', (lr_decay, eps)) call on
    dev's current stream over `table`, a numpy array of OPTIM_TABLE records (struct aspire_optim_tensor: device addresses, element
    counts, per-tensor step and lr).  The caller vouches for the addresses: adam_step / adagrad_step build a table from checked
    tensors, HipAdam / HipAdagrad keep one per set of parameters that have a gradient.
    'adamw' (scalars as 'adam'): aspire_adamw_step_f32 over ADAMW_TABLE records (struct aspire_adamw_tensor).  grad_scale: a
    one-element fp32 tensor on dev -- the step runs on every gradient times it (aspire_*_step_scaled_f32); None: the plain entries."""
    assert table.flags.c_contiguous and table.ndim == 1
    if grad_scale is None and rule in _OPTIM_ENTRY:
        entry, dtype, record, extra = _OPTIM_ENTRY[rule], OPTIM_TABLE, _lib.OptimTensor, ()
    else:
        entry, dtype, record = _OPTIM_SCALED[rule]
        extra = (grad_scale_check(grad_scale, dev).data_ptr() if grad_scale is not None else None,)
    assert table.dtype == dtype
    n = len(table)
    if n == 0:
        return
    require_gpu()
    with torch.cuda.device(dev):
        handle = torch.cuda.current_stream().cuda_stream
        key = (dev.index, handle)
        ws = _OPTIM_WS.get(key)
        if ws is None or ws.numel() < lib.aspire_optim_workspace_bytes(n):
            ws = _OPTIM_WS[key] = torch.empty(max(lib.aspire_optim_workspace_bytes(n), 16384), device=dev, dtype=torch.uint8)
        check(entry(ctypes.cast(table.ctypes.data, ctypes.POINTER(record)), n, *scalars, *extra, ws.data_ptr(), ws.numel(), handle))


def _optim_step(rule, scalars, params, grads, state1, state2, steps, lrs, weight_decays=None, grad_scale=None):
    n = len(params)
    assert len(grads) == len(state1) == len(steps) == len(lrs) == n and (state2 is None or len(state2) == n), 'one entry per tensor'
    if n == 0:
        return
    dev = params[0].device
    for i, (p, g) in enumerate(zip(params, grads)):
        s1, s2 = state1[i], state2[i] if state2 is not None else None
        for t, name in ((p, 'param'), (g, 'grad'), (s1, 'state'), (s2, 'state')):
            if t is not None:
                optim_tensor_check(t, f'{name} {i}')
        if not (g.device == dev == s1.device and p.device == dev and g.numel() == p.numel() == s1.numel()
                and (s2 is None or (s2.device == dev and s2.numel() == p.numel()))):
            raise ValueError(f'tensor {i}: param, grad and state must have one size and live on one device')
    table = np.empty(n, dtype=ADAMW_TABLE if rule == 'adamw' else OPTIM_TABLE)
    if rule == 'adamw':
        table['weight_decay'] = weight_decays
    table['param'] = [t.data_ptr() for t in params]
    table['grad'] = [t.data_ptr() for t in grads]
    table['state1'] = [t.data_ptr() for t in state1]
    table['state2'] = [t.data_ptr() for t in state2] if state2 is not None else 0
    table['n'] = [t.numel() for t in params]
    table['step'] = steps
    table['lr'] = lrs
    if grad_scale is None:
        optim_launch(rule, table, scalars, dev)
    else:
        optim_launch(rule, table, scalars, dev, grad_scale)


def adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, lrs, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=None):
    """torch.optim.Adam's update of every listed tensor in one launch (aspire_adam_step_f32), in place, on the current stream:
    params / grads / exp_avgs / exp_avg_sqs are lists of dense contiguous fp32 GPU tensors on one device (anything else raises, see
    optim_tensor_check), steps the per-tensor step numbers (>= 1, this update's), lrs the per-tensor learning rates.  grad_scale: a
    one-element fp32 GPU tensor; the update then runs on every gradient times it (aspire_adam_step_scaled_f32), the gradients in
    memory untouched."""
    _optim_step('adam', (float(beta1), float(beta2), float(eps)), params, grads, exp_avgs, exp_avg_sqs, steps, lrs, grad_scale=grad_scale)


def adagrad_step(params, grads, sums, steps, lrs, lr_decay=0.0, eps=1e-10, grad_scale=None):
    """torch.optim.Adagrad's update of every listed tensor in one launch (aspire_adagrad_step_f32); arguments as adam_step's."""
    _optim_step('adagrad', (float(lr_decay), float(eps)), params, grads, sums, None, steps, lrs, grad_scale=grad_scale)


def adamw_step(params, grads, exp_avgs, exp_avg_sqs, steps, lrs, weight_decays, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=None):
    """torch.optim.AdamW's update (decoupled decay, per-tensor weight_decays) in one launch (aspire_adamw_step_f32); else as adam_step."""
    _optim_step('adamw', (float(beta1), float(beta2), float(eps)), params, grads, exp_avgs, exp_avg_sqs, steps, lrs, weight_decays,
                grad_scale)


GRAD_TABLE = np.dtype([('grad', 'u8'), ('n', 'i8')])
assert GRAD_TABLE.itemsize == ctypes.sizeof(_lib.GradTensor)
_GRAD_WS = {}       # (device index, stream handle) -> the device table of that stream's packs


_NORM_WS = {}       # (device index, stream handle) -> the table and the partial sums of that stream's norms


def _grad_table(grads, dev, name):
    grads = [g for g in grads if g is not None and g.numel()]
    for i, g in enumerate(grads):
        optim_tensor_check(g, f'{name}: gradient {i}')
        if g.device != dev:
            raise ValueError(f'{name}: gradient {i} is on {g.device}, expected {dev}')
    table = np.zeros(len(grads), dtype=GRAD_TABLE)
    table['grad'] = [g.data_ptr() for g in grads]
    table['n'] = [g.numel() for g in grads]
    return table


def grad_norm(grads, max_norm, out=None):
    """aspire_grad_norm_f32 on the current stream of the gradients' device: -> a two-element fp32 GPU tensor, [0] the L2 norm of all
    of `grads` (dense contiguous fp32 GPU tensors on one device, optim_tensor_check; None entries stay out) viewed as one vector,
    [1] torch's clip coefficient clamp(max_norm / (norm + 1e-6), max=1).  Nothing is read back to the host."""
    grads = [g for g in grads if g is not None]
    max_norm = float(max_norm)
    if not (math.isfinite(max_norm) and max_norm > 0):
        raise ValueError(f'grad_norm: max_norm = {max_norm} must be finite and above 0')
    dev = out.device if out is not None else grads[0].device if grads else require_gpu()
    table = _grad_table(grads, dev, 'grad_norm')
    if out is None:
        out = torch.empty(2, device=dev, dtype=torch.float32)
    elif out.numel() != 2:
        raise ValueError('grad_norm: out must have two elements')
    optim_tensor_check(out, 'grad_norm: out')
    n = len(table)
    with torch.cuda.device(dev):
        handle = torch.cuda.current_stream().cuda_stream
        key = (dev.index, handle)
        sizes = np.ascontiguousarray(table['n'])        # (a column of a record array is strided: the library gets a packed copy)
        need = lib.aspire_grad_norm_workspace_bytes(sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if n else None, n)
        ws = _NORM_WS.get(key)
        if ws is None or ws.numel() < need:
            ws = _NORM_WS[key] = torch.empty(max(need, 1 << 18), device=dev, dtype=torch.uint8)
        check(lib.aspire_grad_norm_f32(ctypes.cast(table.ctypes.data, ctypes.POINTER(_lib.GradTensor)), n, max_norm, out.data_ptr(),
                                       ws.data_ptr(), ws.numel(), handle))
    return out


def grad_scale_(grads, scale):
    """aspire_grad_scale_f32: every listed gradient times `scale` (a one-element fp32 GPU tensor), in place, in one launch."""
    grads = [g for g in grads if g is not None]
    if not grads:
        return
    dev = grads[0].device
    grad_scale_check(scale, dev)
    table = _grad_table(grads, dev, 'grad_scale_')
    n = len(table)
    if n == 0:
        return
    with torch.cuda.device(dev):
        handle = torch.cuda.current_stream().cuda_stream
        key = (dev.index, handle)
        ws = _GRAD_WS.get(key)
        need = lib.aspire_grad_scale_workspace_bytes(n)
        if ws is None or ws.numel() < need:
            ws = _GRAD_WS[key] = torch.empty(max(need, 16384), device=dev, dtype=torch.uint8)
        check(lib.aspire_grad_scale_f32(ctypes.cast(table.ctypes.data, ctypes.POINTER(_lib.GradTensor)), n, scale.data_ptr(), ws.data_ptr(),
                                        ws.numel(), handle))
    for g in grads:
        if not g.is_inference():
            torch.autograd.graph.increment_version(g)


def grad_bucket_layout(numels):
    """The gradient bucket's layout for tensors of `numels` elements (aspire_grad_bucket_elems; no device is touched) ->
    (offsets, tail, total): tensor i takes [offsets[i], offsets[i] + numels[i]), every offset a multiple of 4; the tail of
    round_up(len(numels), 4) floats starts at `tail`; `total` is the bucket's length."""
    n = len(numels)
    sizes = (ctypes.c_int64 * max(n, 1))(*[int(x) for x in numels])
    offsets = (ctypes.c_int64 * max(n, 1))()
    total = lib.aspire_grad_bucket_elems(sizes, n, offsets)
    if total < 0:
        raise ValueError(f'grad_bucket_layout: a negative element count in {list(numels)}')
    return list(offsets[:n]), total - (n + 3) // 4 * 4, total


def grad_bucket_pack(grads, flat, scale, numels=None):
    """One aspire_grad_bucket_pack_f32 call on flat's device's current stream: grads[i] * scale into its region of `flat`, zeros for
    a `None`, zeros in the pads, 1 / 0 per tensor in the tail (include/aspire_hip.h).  grads: dense contiguous fp32 GPU tensors on
    flat's device (optim_tensor_check) or None; numels: every tensor's element count -- needed when a gradient is None, whose region
    keeps its size; flat: a contiguous fp32 GPU tensor of grad_bucket_layout(numels)[2] elements."""
    if numels is None:
        if any(g is None for g in grads):
            raise ValueError('grad_bucket_pack: an absent gradient keeps its region: pass numels')
        numels = [g.numel() for g in grads]
    optim_tensor_check(flat, 'flat')
    n = len(grads)
    if len(numels) != n:
        raise ValueError(f'grad_bucket_pack: {len(numels)} element counts for {n} tensors')
    for i, g in enumerate(grads):
        if g is not None:
            optim_tensor_check(g, f'grad {i}')
            if g.device != flat.device or g.numel() != numels[i]:
                raise ValueError(f'grad {i}: {g.numel()} elements on {g.device}, expected {numels[i]} on {flat.device}')
    table = np.zeros(n, dtype=GRAD_TABLE)
    table['n'] = [int(x) for x in numels]
    dev = flat.device
    with torch.cuda.device(dev):
        handle = torch.cuda.current_stream().cuda_stream
        key = (dev.index, handle)
        ws = _GRAD_WS.get(key)
        need = lib.aspire_grad_bucket_workspace_bytes(n)
        if ws is None or ws.numel() < need:
            ws = _GRAD_WS[key] = torch.empty(max(need, 16384), device=dev, dtype=torch.uint8)
        # a tensor of no elements has no storage and a null data_ptr(): where the library wants an address that is never read -- a
        # gradient of no elements that IS present, a bucket of no elements -- it gets the workspace's
        table['grad'] = [0 if g is None else (g.data_ptr() or ws.data_ptr()) for g in grads]
        check(lib.aspire_grad_bucket_pack_f32(ctypes.cast(table.ctypes.data, ctypes.POINTER(_lib.GradTensor)), n, float(scale),
                                              flat.data_ptr() or ws.data_ptr(), flat.numel(), ws.data_ptr(), ws.numel(), handle))
    return flat


def selftest_xlane():
    require_gpu()
    n = (ctypes.c_int * 16)()
    check(lib.aspire_selftest_xlane(n))
    return sum(n), list(n)


def clock_under(fn, wall_us=4000, reps=None):
    """GHz the shader engines hold while fn() runs repeatedly on the current stream (aspire_debug_clock_probe on a side stream)."""
    side = torch.cuda.Stream()
    out = torch.zeros(2, device='cuda', dtype=torch.int64)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    check(lib.aspire_debug_clock_probe(_ptr(out), int(wall_us), ctypes.c_void_p(side.cuda_stream)))
    if reps is None:
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        reps = max(2, int(1.3 * wall_us / 1e3 / max(t0.elapsed_time(t1), 1e-3)))
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ticks, wall = out.tolist()
    return ticks / max(wall, 1) * 0.1
