"""Fused attention of the pair track (csrc/pair_attn.hip, head dim 64;
csrc/pair_attn_d8.hip, head dim 8 = Uni-Mol's 64 heads at embed 512): bf16,
L % 64 == 0, 64 <= L <= 512, a full per-head (B, H, L, L) bias.

    logits = bf16(fp32(q k^T) + bias)       returned: the next pair state
    o      = dropout(softmax(logits)) v

``pair_attention`` returns ``(o, logits)``, or ``None`` when the kernels do
not serve the call; ``SelfMultiheadAttention`` then runs the bmm -> add ->
``softmax_dropout`` -> bmm chain as before.

Gates: ``UNICORE_PAIR_ATTN`` for every head dim and ``UNICORE_PAIR_ATTN_D8``
for head dim 8 alone, read per call (docs/KERNELS.md, "Pair-track attention"
and "Pair-track attention, head dim 8", have the measurements behind their
defaults).
"""

import os

import torch

# default of the UNICORE_PAIR_ATTN gate: on.  Same-box figures
# (profiles/mol_pair_attn.txt): forward+backward of the module at B 32, H 8 is
# 711 -> 480 us at L 128 and 714 -> 478 us at L 256, against a spread of 16 /
# 21 us between repeated gate-0 rounds; the stress command with --coord-head
# equivariant 81.7 -> 85.3 ups.
_PAIR_ATTN_DEFAULT = "1"

# default of the UNICORE_PAIR_ATTN_D8 gate (head dim 8, csrc/pair_attn_d8.hip):
# on.  Same-box figures (profiles/mol_pair_attn_d8.txt): forward+backward of
# the module at B 32, H 64 is 789 -> 335 us at L 128 and 1862 -> 645 us at
# L 256, against a spread of 1.7 / 1.3 us between repeated gate-0 rounds; the
# stress command with --coord-head equivariant --encoder-attention-heads 64
# 20.9 -> 32.1 ups.
_PAIR_ATTN_D8_DEFAULT = "1"


class _PairAttn(torch.autograd.Function):
    """One saved (B, H, L, L) tensor, the logits that are returned anyway; P
    is recomputed from them and the LSE, the keep bits from the Philox key.
    The gradient of the bias is dS itself, in one bf16 rounding that also
    feeds the dq / dk products."""

    @staticmethod
    def forward(ctx, q, k, v, bias, p, training):
        from unicore_amd import ops

        o, logits, lse, seed = ops.pair_attn_fwd(q, k, v, bias, p, training)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, k, v, o, lse, logits)
        ctx.p = p
        ctx.dropped = training and p > 0
        ctx.seed = int(seed)
        return o, logits

    @staticmethod
    def backward(ctx, d_o, d_logits):
        from unicore_amd import ops

        q, k, v, o, lse, logits = ctx.saved_tensors
        d_o = torch.zeros_like(o) if d_o is None else _dense(d_o)
        if d_logits is not None:
            d_logits = _dense(d_logits)
        dq, dk, dv, dbias = ops.pair_attn_bwd(
            d_o, d_logits, q, k, v, o, lse, logits, ctx.p, ctx.dropped, ctx.seed
        )
        return dq, dk, dv, dbias, None, None


def _dense(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def pair_enabled() -> bool:
    return os.environ.get("UNICORE_PAIR_ATTN", _PAIR_ATTN_DEFAULT) == "1"


def pair_d8_enabled() -> bool:
    """Head dim 8 needs both gates: UNICORE_PAIR_ATTN=0 turns off every head
    dim, UNICORE_PAIR_ATTN_D8=0 this one."""
    return pair_enabled() and os.environ.get(
        "UNICORE_PAIR_ATTN_D8", _PAIR_ATTN_D8_DEFAULT) == "1"


def pair_attention(q, k, v, attn_bias, bsz, heads, p, training,
                   key_padding_mask=None):
    """q, k, v: (bsz*heads, L, D), q pre-scaled; attn_bias (bsz, heads, L, L)
    with padded keys at finfo.min.  Returns (o (bsz*heads, L, D), logits
    (bsz, heads, L, L)), or None: CPU, gate off, dtype, head dim, L, no bias
    or one that is not exactly (bsz, heads, L, L), a key padding mask, or
    tgt_len != src_len."""
    if not q.is_cuda or not pair_enabled():
        return None
    if attn_bias is None or key_padding_mask is not None:
        return None
    if q.dim() != 3 or k.shape != q.shape or v.shape != q.shape:
        return None
    L, D = q.shape[1], q.shape[2]
    if D == 8 and not pair_d8_enabled():
        return None
    if q.shape[0] != bsz * heads or tuple(attn_bias.shape) != (bsz, heads, L, L):
        return None
    if attn_bias.dtype != q.dtype or attn_bias.device != q.device:
        return None
    from unicore_amd import ops

    if not ops.gpu_kernels_available() or not ops.pair_attn_supported(
            L, D, q.dtype):
        return None
    return _PairAttn.apply(_dense(q), _dense(k), _dense(v), _dense(attn_bias),
                           float(p), bool(training))
