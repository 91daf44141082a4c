"""Padding masks of the Evoformer (AlphaFold 2 supplement conventions).

``msa_mask`` is (B, S, L), 1 where an MSA token is real; row 0 is the target
sequence, so ``seq_mask = msa_mask[:, 0]`` and ``pair_mask[b,i,j] =
seq_mask[b,i] * seq_mask[b,j]``.  All masks are 0/1, carry no gradient and
use the dtype of the activations.

The attention sites take the mask as an additive key mask next to their
bias (``softmax_dropout(scores, ..., mask=, bias=)``).  Its value is finite
and representable in the scores' dtype, so a fully padded row or column gives
a uniform softmax, not NaN: padded positions carry finite garbage that never
reaches a valid position.
"""

from typing import NamedTuple

import torch


def additive_mask_value(dtype) -> float:
    """The additive value of a masked key for scores of ``dtype``."""
    return -3e4 if dtype == torch.float16 else -1e9


def additive_key_mask(keep, dtype):
    """0 where ``keep`` is non-zero, ``additive_mask_value(dtype)`` elsewhere,
    in ``dtype`` and with ``keep``'s shape."""
    out = torch.zeros(keep.shape, dtype=dtype, device=keep.device)
    return out.masked_fill_(keep == 0, additive_mask_value(dtype))


class EvoformerMasks(NamedTuple):
    """Everything the blocks derive from ``msa_mask``, computed once per
    forward and shared by all blocks and recycling passes."""

    msa: torch.Tensor        # (B, S, L) 0/1
    pair: torch.Tensor       # (B, L, L) 0/1
    row_key: torch.Tensor    # (B, 1, S, 1, L) additive, MSA row attention
    col_key: torch.Tensor    # (B, L, 1, 1, S) additive, MSA column attention
    tri_start_key: torch.Tensor  # (B, 1, L, 1, L) additive, starting node
    tri_end_key: torch.Tensor    # (B, 1, L, 1, L) additive, ending node
    opm_inv_norm: torch.Tensor   # (B, L, L) fp32, 1 / (1e-3 + m^T m)


def triangle_key_mask(pair_mask, dtype, starting=True):
    """(B, 1, R, 1, T) additive key mask of a triangle attention module:
    keys k of row i are masked by pair_mask[b, i, k] around the starting
    node, by the transposed mask around the ending node."""
    pm = pair_mask if starting else pair_mask.transpose(1, 2)
    return additive_key_mask(pm, dtype)[:, None, :, None, :]


def build_evoformer_masks(msa_mask, dtype) -> EvoformerMasks:
    from .outer_product import opm_mask_inv_norm

    m = msa_mask.detach().to(dtype)
    seq = m[:, 0]
    pair = (seq[:, :, None] * seq[:, None, :]).contiguous()
    key = additive_key_mask(m, dtype)  # (B, S, L)
    return EvoformerMasks(
        msa=m,
        pair=pair,
        row_key=key[:, None, :, None, :],
        col_key=key.transpose(1, 2).contiguous()[:, :, None, None, :],
        tri_start_key=triangle_key_mask(pair, dtype, starting=True),
        tri_end_key=triangle_key_mask(pair, dtype, starting=False),
        opm_inv_norm=opm_mask_inv_norm(m),
    )
