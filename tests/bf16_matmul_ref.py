"""The yardstick of the training encoder's bf16 matmul mode (HipBertTrainEncoder(matmul='bf16'), include/aspire_hip.h:
ASPIRE_MATMUL_BF16): under ``bf16_matmul()`` every ``torch.nn.functional.linear`` and ``torch.matmul`` becomes an autograd function that
rounds BOTH operands of the forward product and of each backward product (dA = r(dC) r(B)^T, dB = r(A)^T r(dC)) with
``.to(torch.bfloat16).to(dtype)`` and multiplies in the tensors' dtype.  HuggingFace ``BertModel(attn_implementation='eager')`` run
under it is the mode's arithmetic, with fp32 or float64 accumulation; everything that is no product runs as it is.

Also here, shared by tests/test_bf16_matmul_cpu.py and tests/test_gpu_encoder_bf16.py: the models, cases and masks of
tests/test_gpu_encoder_backward.py (restated: _bert, CASES, _mask) and ``case(n_layers, b, l)``, the three CPU runs of a case --
computed once, never written to."""
import contextlib
import copy
import functools

import torch

_linear, _matmul = torch.nn.functional.linear, torch.matmul


def round_bf16(x):
    """x rounded to bf16 (round to nearest even), in x's dtype"""
    return x.to(torch.bfloat16).to(x.dtype)


def _sum_to(x, shape):
    """undo matmul's broadcast of the batch dimensions"""
    return x if x.shape == shape else x.sum_to_size(shape)


class _Bf16Product(torch.autograd.Function):
    """C = r(A) r(B) over A [..., M, K], B [..., K, N]"""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _matmul(round_bf16(a), round_bf16(b))

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        rdc = round_bf16(dc)
        da = _sum_to(_matmul(rdc, round_bf16(b).transpose(-1, -2)), a.shape)
        db = _sum_to(_matmul(round_bf16(a).transpose(-1, -2), rdc), b.shape)
        return da, db


def matmul(a, b):
    if a.dim() < 2 or b.dim() < 2:
        raise NotImplementedError('bf16_matmul_ref: matrix operands only')
    return _Bf16Product.apply(a, b)


def linear(x, weight, bias=None):
    """x [..., K] . weight [N, K]^T + bias: the token rows flattened first, so that the weight's gradient is ONE product over all rows
    (dW = r(dY)^T r(X), as the library forms it), not a sum of per-document products"""
    y = _Bf16Product.apply(x.reshape(-1, x.shape[-1]), weight.t()).reshape(*x.shape[:-1], weight.shape[0])
    return y if bias is None else y + bias


@contextlib.contextmanager
def bf16_matmul():
    torch.nn.functional.linear, torch.matmul = linear, matmul
    try:
        yield
    finally:
        torch.nn.functional.linear, torch.matmul = _linear, _matmul


# ---- the cases of tests/test_gpu_encoder_backward.py, restated -------------------------------------------------------------------------
VOCAB = 50


def _bert(n_layers, seed=0, dropout=0.0, intermediate_size=128):
    from transformers import BertConfig, BertModel
    torch.manual_seed(seed)
    cfg = BertConfig(vocab_size=VOCAB, hidden_size=768, num_hidden_layers=n_layers, num_attention_heads=12,
                     intermediate_size=intermediate_size, max_position_embeddings=512, layer_norm_eps=1e-12, hidden_dropout_prob=dropout,
                     attention_probs_dropout_prob=dropout, attn_implementation='eager')
    m = BertModel(cfg, add_pooling_layer=False).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'LayerNorm' in n or n.endswith('.bias'):
                p.add_(0.1 * torch.randn_like(p))
    return m


def _mask(b, l):
    """full / ragged right padding / left padding / a hole / (3, 37): one document whose mask is all zero"""
    m = torch.ones(b, l, dtype=torch.int64)
    if (b, l) == (2, 5):
        m[1, 3:] = 0
    elif (b, l) == (3, 37):
        m[0, :4] = 0
        m[0, 20] = 0
        m[1, 29:] = 0
        m[2] = 0
    elif (b, l) == (2, 130):
        m[1, 129:] = 0
        m[1, 64:70] = 0
        m[1, :2] = 0
    return m


CASES = [(1, 2, 5), (2, 3, 37), (2, 2, 130)]


def _run(m, dtype, emulate, tok, typ, mask, G, mix_logits=None):
    """-> (hidden or cls, parameter gradients, the mix logits' gradient or None); loss = (out * G).sum()"""
    mm = copy.deepcopy(m).to(dtype)
    logits = None if mix_logits is None else mix_logits.to(dtype).clone().requires_grad_(True)
    with (bf16_matmul() if emulate else contextlib.nullcontext()):
        out = mm(tok, token_type_ids=typ, attention_mask=mask, output_hidden_states=logits is not None)
        if logits is None:
            y = out.last_hidden_state
        else:       # MySPECTER's read-out: the CLS rows of the soft-max mix of all hidden states (the mix is no matrix product)
            y = (torch.stack(out.hidden_states, 0)[:, :, 0, :] * torch.softmax(logits, 0)[:, None, None]).sum(0)
        (y * G.to(dtype)).sum().backward()
    return y.detach(), {n: p.grad for n, p in mm.named_parameters()}, None if logits is None else logits.grad


@functools.lru_cache(maxsize=None)
def case(n_layers, b, l):
    """-> m, tok, typ, mask, G, runs; runs['exact']: the float64 model, runs['emu64'] / runs['emu32']: the emulation with float64 /
    fp32 accumulation.  Each run: (hidden, {name: grad}, None)."""
    m = _bert(n_layers, seed=10 * n_layers + b)
    g = torch.Generator().manual_seed(100 + l)
    tok = torch.randint(0, VOCAB, (b, l), generator=g)
    typ = torch.randint(0, 2, (b, l), generator=g)
    mask = _mask(b, l)
    G = torch.randn(b, l, 768, generator=g)
    runs = {'exact': _run(m, torch.float64, False, tok, typ, mask, G), 'emu64': _run(m, torch.float64, True, tok, typ, mask, G),
            'emu32': _run(m, torch.float32, True, tok, typ, mask, G)}
    return m, tok, typ, mask, G, runs


@functools.lru_cache(maxsize=None)
def cls_case(n_layers=2, b=3, l=37):
    """the CLS read-out with a learned mix: -> m, tok, typ, mask, G [b, 768], logits [n_layers + 1], runs ('exact', 'emu32')"""
    m, tok, typ, mask, _, _ = case(n_layers, b, l)
    g = torch.Generator().manual_seed(7)
    G = torch.randn(b, 768, generator=g)
    logits = torch.randn(n_layers + 1, generator=g)
    runs = {'exact': _run(m, torch.float64, False, tok, typ, mask, G, logits), 'emu32': _run(m, torch.float32, True, tok, typ, mask, G, logits)}
    return m, tok, typ, mask, G, logits, runs


def group(name):
    if name.startswith('embeddings.'):
        return 'tables' if 'LayerNorm' not in name else 'emb LayerNorm'
    return name.split('.', 3)[3]


def compare_grads(got, exact, emu32, bound, tag, report=print):
    """every gradient of `got` inside bound(|emu32 - exact|, max|exact|) of exact (the key bias, zero in exact arithmetic, scaled by the
    query bias); prints the largest error / bound per tensor group before it asserts.  -> {group: (error, bound)}"""
    worst, fails = {}, []
    for n, want in exact.items():
        ref_err = float((emu32[n].double() - want).abs().max())
        scale = float(want.abs().max())
        if n.endswith('attention.self.key.bias'):
            scale = float(exact[n.replace('key.bias', 'query.bias')].abs().max())
        tol = bound(ref_err, scale)
        err = float((got[n].double().cpu() - want).abs().max())
        k = group(n)
        if k not in worst or err * worst[k][1] > worst[k][0] * tol:
            worst[k] = (err, tol)
        if not err <= tol:
            fails.append((n, err, tol))
    for k, (err, tol) in worst.items():
        report(f'[{tag}] {k:42s} |got - float64| {err:.3e}  bound {tol:.3e}  ratio {err / tol if tol else 0.0:.2f}')
    assert not fails, fails
    return worst
