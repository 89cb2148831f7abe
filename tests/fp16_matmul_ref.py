"""CPU yardsticks of the inference encoder's fp16 matmul mode (HipBertEncoder(matmul='fp16'), include/aspire_hip.h A1h), shared by
tests/test_fp16_matmul_cpu.py, tests/test_gpu_gemm_hplane.py and tests/test_gpu_encoder_fp16.py:

  * the H layout's piece index (aspire_amd/csrc/enc_hplane.h), restated, and a decoder of an H buffer to a float array;
  * the mode emulated on a HuggingFace model in float64 -- every nn.Linear of the layer stack as F.linear(r(x), r(64 W) / 64) + b with
    r = .half().double(), everything else float64, the attention unrounded; the pooler and (cls_tail) the last layer's tail behind the
    QKV projection stay exact, as the CLS forward keeps them;
  * the exact float64 model;
  * CASES, each seeded.
"""
import contextlib
import copy
import functools

import numpy as np
import torch

PAD_ROWS = 256          # kPPadRows
WEIGHT_SCALE = 64.0     # kPWeightScale


# ---- the H layout ------------------------------------------------------------------------------------------------------------------
def h_bytes(R, K):
    return (R + PAD_ROWS) * K * 2


def h_piece_index(R, r, k):
    """index of the 16-byte piece that holds element (r, k) of X [R, K] (its 8 fp16 are k & ~7 .. + 7)"""
    kb, q = k >> 5, (k >> 3) & 3
    return (kb * R + r) * 4 + (q ^ ((r >> 2) & 3))


def h_piece_table(R, K):
    """int64 [R, K / 8]: the piece index of every (row, 8-wide k group)"""
    r = np.arange(R, dtype=np.int64)[:, None]
    k = (np.arange(K // 8, dtype=np.int64) * 8)[None, :]
    return ((k >> 5) * R + r) * 4 + (((k >> 3) & 3) ^ ((r >> 2) & 3))


def h_decode(buf, R, K):
    """an H buffer (uint8 array / tensor of >= R K 2 bytes) -> float16 array [R, K]"""
    raw = np.asarray(buf.cpu() if hasattr(buf, 'cpu') else buf, dtype=np.uint8)
    pieces = raw[:R * K * 2].view(np.float16).reshape(R * K // 8, 8)
    return pieces[h_piece_table(R, K)].reshape(R, K)


# ---- the mode's arithmetic on the CPU ----------------------------------------------------------------------------------------------
def r16(x):
    """round to fp16 once (nearest even; beyond 65504: inf), back in float64"""
    return x.half().double()


_linear = torch.nn.functional.linear


@contextlib.contextmanager
def fp16_linears(rounded_weights):
    """inside: F.linear(x, W, b) with W one of rounded_weights (by identity) is the mode's product; every other call is untouched"""
    ids = {id(w) for w in rounded_weights}

    def linear(x, weight, bias=None):
        if id(weight) not in ids:
            return _linear(x, weight, bias)
        y = _linear(r16(x.double()), r16(WEIGHT_SCALE * weight.double()) / WEIGHT_SCALE)
        return y if bias is None else y + bias.double()

    torch.nn.functional.linear = linear
    try:
        yield
    finally:
        torch.nn.functional.linear = _linear


def mode_weights(m, cls_tail=False):
    """the nn.Linear weights the mode rounds in model m: the four projections of every layer (BertModel / RobertaModel / MPNetModel);
    cls_tail: the last layer keeps only its query / key / value (the CLS forward's tail on the B CLS rows is fp32)"""
    out = []
    layers = list(m.encoder.layer)
    for i, ly in enumerate(layers):
        for name, mod in ly.named_modules():
            if isinstance(mod, torch.nn.Linear):
                is_qkv = name.split('.')[-1] in ('query', 'key', 'value', 'q', 'k', 'v')
                if cls_tail and i == len(layers) - 1 and not is_qkv:
                    continue
                out.append(mod.weight)
    return out


def run64(m, emulate, cls_tail=False, **inputs):
    """m (fp32 HF model) in float64 on the inputs -> the model's output with hidden_states; emulate: in the mode's arithmetic"""
    m64 = copy.deepcopy(m).double().eval()
    with torch.no_grad():
        if not emulate:
            return m64(output_hidden_states=True, **inputs)
        with fp16_linears(mode_weights(m64, cls_tail)):
            return m64(output_hidden_states=True, **inputs)


# ---- models and cases --------------------------------------------------------------------------------------------------------------
VOCAB = 50


def bert(n_layers, seed=0, intermediate_size=3072, pooler=False):
    from transformers import BertConfig, BertModel
    torch.manual_seed(seed)
    cfg = BertConfig(vocab_size=VOCAB, hidden_size=768, num_hidden_layers=n_layers, num_attention_heads=12,
                     intermediate_size=intermediate_size, max_position_embeddings=512, layer_norm_eps=1e-12, attn_implementation='eager')
    m = BertModel(cfg, add_pooling_layer=pooler).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'LayerNorm' in n or n.endswith('.bias'):
                p.add_(0.1 * torch.randn_like(p))
    return m


def ragged_mask(b, l):
    """full / ragged right padding / left padding / holes; (3, 37): one document whose mask is all zero; (3, 100): a one-token document"""
    m = torch.ones(b, l, dtype=torch.int64)
    if (b, l) == (2, 5):
        m[1, 3:] = 0
    elif (b, l) == (3, 37):
        m[0, 1:4] = 0
        m[0, 20] = 0
        m[1, 29:] = 0
        m[2] = 0
    elif (b, l) == (2, 130):
        m[1, 129:] = 0
        m[1, 64:70] = 0
        m[1, 1:3] = 0
    elif (b, l) == (3, 100):
        m[1, 63:] = 0
        m[2, 1:] = 0
    elif (b, l) == (4, 128):
        for i, n in enumerate((128, 97, 128, 41)):
            m[i, n:] = 0
    return m


# n_layers, B, L, intermediate_size (a multiple of 128: the mode's condition; 256: one 128-wide FFN2 k run of 8 blocks, two FFN1 column tiles)
CASES = [(1, 2, 5, 256), (2, 3, 37, 3072), (2, 2, 130, 3072), (2, 3, 100, 3072)]
HEAVY = (4, 4, 128)     # heavy_tailed_bert(4, seed=8) at 4 x 128


@functools.lru_cache(maxsize=None)
def case(n_layers, b, l, ffn=3072, pooler=False):
    """-> m, tok, typ, mask, exact, emu, emu_cls: the float64 model's output, the mode's emulation, and the emulation of the CLS forward
    (last layer's tail exact); computed once and shared, never written to"""
    m = bert(n_layers, seed=10 * n_layers + b, intermediate_size=ffn, pooler=pooler)
    g = torch.Generator().manual_seed(100 + l)
    tok = torch.randint(0, VOCAB, (b, l), generator=g)
    typ = torch.randint(0, 2, (b, l), generator=g)
    mask = ragged_mask(b, l)
    kw = dict(input_ids=tok, token_type_ids=typ, attention_mask=mask)
    return m, tok, typ, mask, run64(m, False, **kw), run64(m, True, **kw), run64(m, True, cls_tail=True, **kw)


@functools.lru_cache(maxsize=None)
def heavy_case():
    from heavy_bert import heavy_tailed_bert
    n_layers, b, l = HEAVY
    m = heavy_tailed_bert(n_layers, seed=8)
    g = torch.Generator().manual_seed(808)
    mask = ragged_mask(b, l)
    tok = torch.randint(5, 3000, (b, l), generator=g) * mask
    typ = torch.zeros_like(tok)
    kw = dict(input_ids=tok, token_type_ids=typ, attention_mask=mask)
    return m, tok, typ, mask, run64(m, False, **kw), run64(m, True, **kw), None


@functools.lru_cache(maxsize=None)
def sbert_case(kind):
    """one small RoBERTa- / MPNet-shaped model (as tests/test_gpu_sbert.py builds them) on [3, 37] right-padded ids (pad id 1)"""
    from transformers import MPNetConfig, MPNetModel, RobertaConfig, RobertaModel
    torch.manual_seed({'mpnet': 11, 'roberta': 12}[kind])
    kw = dict(vocab_size=300, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072,
              max_position_embeddings=514, layer_norm_eps=1e-5, pad_token_id=1)
    m = (MPNetModel(MPNetConfig(**kw), add_pooling_layer=False) if kind == 'mpnet'
         else RobertaModel(RobertaConfig(type_vocab_size=1, attn_implementation='eager', **kw), add_pooling_layer=False)).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'LayerNorm' in n or n.endswith('.bias'):
                p.add_(0.1 * torch.randn_like(p))
        if kind == 'mpnet':
            m.encoder.relative_attention_bias.weight.copy_(torch.randn(32, 12))
    g = torch.Generator().manual_seed(21)
    lens = torch.tensor([37, 22, 2])
    mask = (torch.arange(37)[None, :] < lens[:, None]).long()
    ids = torch.randint(5, 300, (3, 37), generator=g) * mask + (1 - mask)
    kw = dict(input_ids=ids, attention_mask=mask)
    return m, ids, mask, run64(m, False, **kw), run64(m, True, **kw)


def masked_mean(hidden, mask):
    w = mask.to(hidden.dtype)[:, :, None]
    return (hidden * w).sum(1) / w.sum(1).clamp_min(1e-9)
