"""What the dropout tests measure against, written without the library: a numpy Philox4x32-10 with the keying of
include/aspire_hip.h (key = the seed's two words, counter = (block low, block high, site, step), block = e >> 2, element e takes
word e & 3, keep iff word >= floor(float32(p) * 2^32)), and a context manager that makes HuggingFace's dropout calls apply given
masks in call order."""
import contextlib

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two uint32 ints -> four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK32) for x in counter]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [x.astype(np.uint32) for x in c]


def threshold(p):
    return int(np.floor(np.float64(np.float32(p)) * 4294967296.0))


def words(seed, step, site, first, n):
    """the uint32 word of elements first .. first + n - 1 of a site"""
    e = np.arange(n, dtype=np.uint64) + np.uint64(first)
    blocks, inverse = np.unique(e >> np.uint64(2), return_inverse=True)
    out = philox4x32_10((blocks & np.uint64(MASK32), blocks >> np.uint64(32), np.full(blocks.shape, site, dtype=np.uint64),
                         np.full(blocks.shape, step & MASK32, dtype=np.uint64)), (seed & MASK32, (seed >> 32) & MASK32))
    return np.stack(out, 1)[inverse, (e & np.uint64(3)).astype(np.int64)]


def keep_mask(seed, step, site, p, first, n):
    """uint8 [n]: 1 where the element is kept"""
    return (words(seed, step, site, first, n) >= np.uint32(threshold(p)) if threshold(p) else np.ones(n, bool)).astype(np.uint8)


def scale(p):
    return float(np.float32(1) / (np.float32(1) - np.float32(p)))


@contextlib.contextmanager
def given_masks(masks):
    """masks: a list of (keep tensor or None, p) in HuggingFace's call order.  While active, torch.nn.functional.dropout(x, p, training)
    takes the next entry, asserts its shape and p, and returns x * keep * 1 / (1 - p) (fp32's 1 / (1 - p), in x's dtype); an entry with
    p == 0 expects the call and passes x through.  Every entry must have been used on exit.  (HuggingFace's eager attention calls the
    functional form, nn.Dropout.forward calls it too: patching it catches all four sites.)"""
    import torch.nn.functional as F
    real, calls = F.dropout, iter(masks)
    used = [0]

    def fake(x, p=0.5, training=True, inplace=False):
        if not training:
            return x
        keep, want_p = next(calls)
        used[0] += 1
        assert float(p) == float(want_p), (used[0], p, want_p)
        if want_p == 0:
            return x
        assert tuple(keep.shape) == tuple(x.shape), (used[0], tuple(keep.shape), tuple(x.shape))
        return x * (keep.to(x.dtype) * scale(want_p))

    F.dropout = fake
    try:
        yield
    finally:
        F.dropout = real
    assert used[0] == len(masks), (used[0], len(masks))
