"""The row lists of the training encoder's padding-free mode (HipBertTrainEncoder(..., packed=True); include/aspire_hip.h: struct
aspire_bert_packing): which rows of a padded [B, L] batch are valid tokens, and where each one sits among the R = mask.sum() packed rows.
Packed rows are in document order and, inside a document, in position order; a mask with holes or left padding packs the same way as
right padding does.  Plain torch on whatever device the mask is on, with ONE host read (of the three totals); no library call."""
from typing import NamedTuple

import torch


class PackedRows(NamedTuple):
    rows: int                   # R, the valid tokens of the batch
    max_len: int                # the longest document's rows (0 iff rows == 0)
    prefix: bool                # every document's rows are its positions 0 .. len - 1 (right padding alone)
    doc_start: torch.Tensor     # int32 [B + 1]: document b's packed rows are doc_start[b] .. doc_start[b + 1] - 1
    row_src: torch.Tensor       # int32 [R]: the padded row b L + l of packed row m
    row_dst: torch.Tensor       # int32 [B L]: the packed row of a padded row, or -1


def packed_rows(mask):
    """attention mask [B, L] (nonzero = a valid token; any integer or bool dtype, any device) -> PackedRows on the mask's device"""
    if mask.dim() != 2:
        raise ValueError(f'packed_rows: the mask is [B, L]; got {tuple(mask.shape)}')
    b, l = mask.shape
    if b * l >= 2 ** 31:
        raise NotImplementedError(f'packed_rows: {b} x {l} padded token rows: the row lists are 32-bit (split the batch)')
    valid = mask != 0
    lens = valid.sum(1)
    doc_start = torch.zeros(b + 1, dtype=torch.int32, device=mask.device)
    doc_start[1:] = torch.cumsum(lens, 0)
    flat = valid.reshape(-1)
    position = torch.arange(l, device=mask.device)
    is_prefix = (valid == (position[None, :] < lens[:, None])).all() if b * l else torch.ones((), dtype=torch.bool, device=mask.device)
    longest = lens.max() if b else torch.zeros((), dtype=torch.int64, device=mask.device)
    rows, max_len, prefix = torch.stack([doc_start[-1].to(torch.int64), longest.to(torch.int64), is_prefix.to(torch.int64)]).tolist()
    # the valid padded rows in ascending order: a stable sort of "is masked" puts them first (no data-dependent shape on the device)
    row_src = torch.argsort((~flat).to(torch.uint8), stable=True)[:rows].to(torch.int32)
    row_dst = torch.where(flat, torch.cumsum(flat, 0) - 1, -1).to(torch.int32)
    return PackedRows(int(rows), int(max_len), bool(prefix), doc_start, row_src, row_dst)
