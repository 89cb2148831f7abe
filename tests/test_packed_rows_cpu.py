"""CPU: the row lists of the training encoder's padding-free mode (aspire_amd.packed_rows; HipBertTrainEncoder(..., packed=True)), the
mode's refusals, and the PREMISE the mode stands on, pinned here so that the yardstick of tests/test_gpu_encoder_packed.py is in the
repository: a pad row buys nothing.

The premise, on the float64 HuggingFace model at bf16_matmul_ref.CASES: the padded batch with the loss zeroed on masked rows
(G * mask) against per-document runs over the valid tokens alone, given explicit position_ids.  ``hidden`` on valid rows and every
parameter gradient must agree to 1e-12 relative (measured: 3e-15 and 1.2e-15).  ONE tensor is excluded, by name:
``attention.self.key.bias``.  Its gradient is the column sum of dK = dS^T Q, and the rows of dS sum to zero, so it is zero in exact
arithmetic and rounding residue on both sides -- relative agreement of two residues means nothing.  That is the only exclusion.
"""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_matmul_ref as br  # noqa: E402

PATTERNS = [('(2, 5): full, right padding', br._mask(2, 5)),
            ('(3, 37): left padding + a hole, right padding, an all-zero document', br._mask(3, 37)),
            ('(2, 130): full, left padding + a hole + right padding', br._mask(2, 130)),
            ('(2, 8): full', br._mask(2, 8)),
            ('(3, 6): R == 0', torch.zeros(3, 6, dtype=torch.int64))]


@pytest.mark.parametrize('name,mask', PATTERNS, ids=[n for n, _ in PATTERNS])
def test_packed_rows_lists(name, mask):
    from aspire_amd import PackedRows, packed_rows
    pr = packed_rows(mask)
    b, l = mask.shape
    assert isinstance(pr, PackedRows)
    lens = [int(x) for x in mask.sum(1)]
    assert pr.rows == sum(lens) and pr.max_len == max(lens)
    assert pr.doc_start.dtype == pr.row_src.dtype == pr.row_dst.dtype == torch.int32
    assert pr.doc_start.tolist() == [sum(lens[:i]) for i in range(b + 1)]
    src = pr.row_src.tolist()
    assert len(src) == pr.rows and src == sorted(src) and len(set(src)) == len(src)            # ascending: document order, position order
    assert src == [i for i, v in enumerate(mask.reshape(-1).tolist()) if v]
    dst = pr.row_dst.tolist()
    assert len(dst) == b * l
    for m, p in enumerate(src):
        assert dst[p] == m
    assert all(dst[p] == -1 for p in range(b * l) if p not in set(src))
    # prefix: true exactly when every document's rows are its positions 0 .. len - 1 (right padding alone)
    want = all(mask[i].tolist() == [1] * lens[i] + [0] * (l - lens[i]) for i in range(b))
    assert pr.prefix is want
    for i in range(b):                  # a document's rows are its own tokens, in position order
        rows = src[pr.doc_start[i]:pr.doc_start[i + 1]]
        assert [p // l for p in rows] == [i] * lens[i] and [p % l for p in rows] == [j for j in range(l) if mask[i, j]]


def test_prefix_is_true_for_right_padding_only():
    from aspire_amd import packed_rows
    assert packed_rows(br._mask(2, 5)).prefix and packed_rows(br._mask(2, 8)).prefix
    assert not packed_rows(br._mask(3, 37)).prefix and not packed_rows(br._mask(2, 130)).prefix
    right = torch.ones(3, 9, dtype=torch.int64)
    right[0, 4:] = 0
    right[2] = 0                        # an all-zero document is a prefix of length 0
    assert packed_rows(right).prefix
    left = right.flip(1)
    assert not packed_rows(left).prefix
    assert packed_rows(torch.ones(2, 3, dtype=torch.bool)).rows == 6                          # any integer or bool mask
    with pytest.raises(ValueError):
        packed_rows(torch.ones(5, dtype=torch.int64))


def test_the_modes_refusals(monkeypatch):
    """packed=True exists with attention='flash' alone: NotImplementedError before any launch, worded like the other refusals; and
    forward_cls needs mask[:, 0] == 1 for every document: ValueError on the host"""
    from aspire_amd import BiEncTrain, HipBertTrainEncoder, IctEncTrain, SentEncTrain, ops
    monkeypatch.setattr(ops, 'require_gpu', lambda: torch.device('cpu'))            # construction alone: no kernel runs
    assert HipBertTrainEncoder(br._bert(1)).packed is False
    flash = dict(matmul='bf16', attention='flash')
    assert HipBertTrainEncoder(br._bert(1), **flash).packed is False
    assert HipBertTrainEncoder(br._bert(1), packed=True, **flash).packed is True
    for kw in (dict(), dict(matmul='bf16'), dict(matmul='bf16x3'), dict(matmul='bf16', attention='gemm')):
        with pytest.raises(NotImplementedError, match="packed=True is built for attention='flash' alone"):
            HipBertTrainEncoder(br._bert(1), packed=True, **kw)
    with pytest.raises(NotImplementedError, match='flash'):                         # (the older refusal comes first)
        HipBertTrainEncoder(br._bert(1), attention='flash', packed=True)
    assert BiEncTrain(br._bert(1), packed=True, **flash).bert_encoder.packed and not BiEncTrain(br._bert(1)).packed
    assert SentEncTrain(br._bert(1), packed=True, **flash).packed and not SentEncTrain(br._bert(1)).sent_encoder.packed
    ict = IctEncTrain(br._bert(1), br._bert(1), packed=True, **flash)
    assert ict.packed and ict.sent_encoder.packed and ict.context_encoder.packed
    with pytest.raises(NotImplementedError, match='packed=True'):
        SentEncTrain(br._bert(1), packed=True)
    enc = HipBertTrainEncoder(br._bert(1), packed=True, **flash).train()
    tok = torch.randint(0, br.VOCAB, (3, 37))
    with pytest.raises(ValueError, match=r'attention_mask\[:, 0\] == 1'):
        enc.forward_cls((tok, torch.zeros_like(tok), br._mask(3, 37)))


def _per_document(m, tok, typ, mask, G):
    """the float64 model on every document's valid tokens alone, with their positions -> hidden [R, 768] in packed order, summed grads"""
    mm = copy.deepcopy(m).to(torch.float64)
    rows = []
    for b in range(tok.shape[0]):
        idx = mask[b].nonzero().squeeze(1)
        if not idx.numel():
            continue
        out = mm(tok[b, idx][None], token_type_ids=typ[b, idx][None], attention_mask=torch.ones(1, idx.numel(), dtype=torch.int64),
                 position_ids=idx[None]).last_hidden_state
        (out * G[b, idx][None].to(torch.float64)).sum().backward()             # (the parameters' gradients accumulate over documents)
        rows.append(out.detach()[0])
    return torch.cat(rows, 0), {n: p.grad for n, p in mm.named_parameters()}


@pytest.mark.parametrize('n_layers,b,l', br.CASES)
def test_a_pad_row_buys_nothing(n_layers, b, l):
    m, tok, typ, mask, G, _ = br.case(n_layers, b, l)
    hidden, grads, _ = br._run(m, torch.float64, False, tok, typ, mask, G * mask[..., None])
    want_h, want_g = _per_document(m, tok, typ, mask, G)
    got_h = hidden[mask.bool()]
    err = float((got_h - want_h).abs().max()) / float(want_h.abs().max())
    print(f'[{n_layers} x ({b}, {l})] hidden on valid rows: relative {err:.2e}')
    worst, worst_name, excluded = 0.0, None, 0
    for n, g in want_g.items():
        if n.endswith('attention.self.key.bias'):
            excluded += 1
            continue
        scale = float(g.abs().max())
        e = float((grads[n] - g).abs().max())
        rel = e / scale if scale else e
        if rel > worst:
            worst, worst_name = rel, n
    print(f'[{n_layers} x ({b}, {l})] parameter gradients: largest relative {worst:.2e} ({worst_name}); excluded: {excluded} key biases')
    assert excluded == n_layers and err <= 1e-12 and worst <= 1e-12
