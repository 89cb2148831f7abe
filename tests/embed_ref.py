"""numpy reference of the embedding lookup under training (include/aspire_hip.h: aspire_bert_embed_sum_f32 /
aspire_bert_embed_backward_f32), in the kernels' own fp32 orders and in float64.

    forward(word, pos, typ_tab, tok, typ)                   (word[tok] + typ_tab[typ]) + pos[:L], in the tables' dtype
    backward(grad, tok, typ, vocab, max_pos, n_types, pad, dtype)
        grad_word, grad_pos   np.add.at on zeros: unbuffered, one add per index in index order = ascending token row (checked in
                              tests/test_embed_cpu.py against a Python loop and torch's CPU embedding backward, bit for bit); the
                              padding row zero
        grad_type             the header's two stages: R = ceil(M / 64) rows per block, 64 partials each started at 0 and adding its
                              block's rows of type t ascending, then the partials added ascending from 0
    dtype float32 gives the kernels' bits, float64 the yardstick.
"""
import numpy as np

D = 768
TYPE_PARTS = 64


def forward(word, pos, typ_tab, tok, typ=None):
    b, l = tok.shape
    typ = np.zeros_like(tok) if typ is None else typ
    return (word[tok] + typ_tab[typ]) + pos[:l][None]


def type_grad(grad_rows, typ_rows, n_types, dtype):
    m = grad_rows.shape[0]
    g = grad_rows.astype(dtype)
    r = -(-m // TYPE_PARTS)
    out = np.zeros((n_types, g.shape[1]), dtype=dtype)
    for t in range(n_types):
        total = np.zeros(g.shape[1], dtype=dtype)
        for j in range(TYPE_PARTS):
            part = np.zeros(g.shape[1], dtype=dtype)
            for i in range(j * r, min((j + 1) * r, m)):
                if typ_rows[i] == t:
                    part = part + g[i]
            total = total + part
        out[t] = total
    return out


def backward(grad, tok, typ, vocab, max_pos, n_types, pad=-1, dtype=np.float32):
    """grad [B, L, 768], tok / typ int [B, L] (typ None: all 0) -> (grad_word, grad_pos, grad_type) in dtype"""
    b, l = tok.shape
    g = grad.reshape(b * l, -1).astype(dtype)
    ids = tok.reshape(-1)
    types = np.zeros_like(ids) if typ is None else typ.reshape(-1)
    gw = np.zeros((vocab, g.shape[1]), dtype=dtype)
    np.add.at(gw, ids, g)
    if pad >= 0:
        gw[pad] = 0
    gp = np.zeros((max_pos, g.shape[1]), dtype=dtype)
    np.add.at(gp, np.tile(np.arange(l), b), g)
    return gw, gp, type_grad(g, types, n_types, dtype)


def order_grads(b, l, seed):
    """gradient rows whose summation order matters: normal rows scaled by 10 ** randint(-3, 3)"""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.integers(-3, 4, size=(b, l, 1))
    return (rng.standard_normal((b, l, D)) * scale).astype(np.float32)


def bound(ref_err, max_ref):
    """the project's parity rule: four times the fp32 CPU reference's own error, never less than four fp32 roundings of the largest
    entry"""
    return max(4.0 * float(ref_err), 4.0 * 2.0 ** -23 * float(max_ref))
