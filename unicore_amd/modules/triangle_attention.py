"""Triangle self-attention around the starting / ending node (AlphaFold 2
supplement, Algorithms 13 and 14), on the stored (B, I, J, C) pair layout.

    starting:  a_ijk = softmax_k(q_ij . k_ik / sqrt(c) + b_jk)
               o_ij  = g_ij * sum_k a_ijk v_ik
    ending:    a_ijk = softmax_k(q_ij . k_kj / sqrt(c) + b_ki)
               o_ij  = g_ij * sum_k a_ijk v_kj

The ending node is the starting node on the transposed pair tensor; the
transposition lives in the ``transpose`` flag of the three layout moves
below, so neither ``pair`` nor the result is ever permute-copied.

Layout moves (csrc/tri_attn.hip on GPU, the permute expression otherwise):

    pair_arrange(x, H, tr)       (B, I, J, H*D) view -> (B, H, R, T, D)
    pair_arrange_qkv(qkv, H, tr) the same for the three chunks of (.., 3*H*D)
    pair_merge(o, B, I, J, H, tr)   (B*H*R, T, D)    -> (B, I, J, H*D)
    pair_bias_arrange(lin, tr)   (B, L, L, H)        -> (B, H, L, L)

with (i, j) = (r, t), or (t, r) when ``tr`` is set.  Scores are viewed as
(B, H, R, T, T) against a (B, H, 1, T, T) bias: the broadcast that
``softmax_dropout`` addresses without materialising, with its fused
bias-gradient backward.

Gate: ``UNICORE_TRIATTN_FUSED`` (see docs/KERNELS.md, "Triangle attention
layout moves", for the measurement behind its default).  The permute
expression is used on CPU, for an unsupported head dim / head count / L, for
misaligned or oddly strided inputs, and when the gate is off.
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .gated_mul import gated_mul
from .layer_norm import LayerNorm
from .multihead_attention import qk_scores
from .padding_mask import triangle_key_mask
from .softmax_dropout import softmax_dropout

# default of the UNICORE_TRIATTN_FUSED gate: off (opt-in). Same-box figures
# (profiles/evoformer_triattn.txt): the layout entries are 1.3-2.1x faster
# than the permute copies and the module forward 2-5% faster at L=256, but
# forward+backward of the starting node is 3% slower there and the
# end-to-end difference (+0.4%) is inside the noise.
_TRIATTN_FUSED_DEFAULT = "0"

_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _fused_enabled(t) -> bool:
    if not t.is_cuda or t.dtype not in _DTYPES or t.numel() == 0:
        return False
    if os.environ.get("UNICORE_TRIATTN_FUSED", _TRIATTN_FUSED_DEFAULT) != "1":
        return False
    from unicore_amd import ops

    return ops.gpu_kernels_available() or not ops.allow_eager_on_gpu()


def _strided_ok(x) -> bool:
    # mirrors the host checks of pair_arrange in csrc/tri_attn.hip
    return (
        x.stride(3) == 1
        and all(x.size(d) == 1 or (x.stride(d) >= 0 and x.stride(d) % 8 == 0)
                for d in range(3))
        and x.data_ptr() % 16 == 0
    )


def _dense(g):
    """Contiguous and 16 B aligned; copies at most once."""
    if not g.is_contiguous():
        g = g.contiguous()
    if g.data_ptr() % 16 != 0:  # contiguous() returned it as it was
        g = g.clone()
    return g


class _PairArrange(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, heads, transpose):
        from unicore_amd import ops

        ctx.dims = (x.shape[0], x.shape[1], x.shape[2], heads, transpose)
        return ops.pair_arrange(x, heads, transpose)

    @staticmethod
    def backward(ctx, grad):
        from unicore_amd import ops

        B, I, J, H, tr = ctx.dims
        g = _dense(grad)
        g = ops.pair_merge(g.view(-1, g.shape[3], g.shape[4]), B, I, J, H, tr)
        return g, None, None


class _PairArrangeQKV(torch.autograd.Function):
    """pair_arrange of the three chunks of a fused qkv projection.  Backward
    merges the three gradients straight into one (B, I, J, 3C) buffer:
    separate Functions would return three contiguous gradients that
    autograd then concatenates, a second pass over all of them."""

    @staticmethod
    def forward(ctx, qkv, heads, transpose):
        from unicore_amd import ops

        ctx.dims = (qkv.shape[0], qkv.shape[1], qkv.shape[2], heads, transpose)
        return tuple(ops.pair_arrange(t, heads, transpose)
                     for t in qkv.chunk(3, dim=-1))

    @staticmethod
    def backward(ctx, *grads):
        from unicore_amd import ops

        B, I, J, H, tr = ctx.dims
        ref = next(g for g in grads if g is not None)
        C = H * ref.shape[4]
        d_qkv = ref.new_empty(B, I, J, 3 * C)
        for g, out in zip(grads, d_qkv.chunk(3, dim=-1)):
            if g is None:
                out.zero_()
                continue
            g = _dense(g)
            ops.pair_merge(g.view(-1, g.shape[3], g.shape[4]), B, I, J, H, tr,
                           out)
        return d_qkv, None, None


class _PairMerge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o, B, I, J, heads, transpose):
        from unicore_amd import ops

        ctx.heads, ctx.transpose, ctx.in_shape = heads, transpose, o.shape
        return ops.pair_merge(o, B, I, J, heads, transpose)

    @staticmethod
    def backward(ctx, grad):
        from unicore_amd import ops

        if not _strided_ok(grad):
            grad = _dense(grad)
        g = ops.pair_arrange(grad, ctx.heads, ctx.transpose)
        return g.view(ctx.in_shape), None, None, None, None, None


class _PairBiasArrange(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lin, transpose):
        from unicore_amd import ops

        ctx.transpose = transpose
        return ops.pair_bias_arrange(lin, transpose)

    @staticmethod
    def backward(ctx, grad):
        from unicore_amd import ops

        return ops.pair_bias_arrange_bwd(_dense(grad), ctx.transpose), None


def pair_arrange(x, heads, transpose=False):
    """(B, I, J, H*D) [contiguous channels, any spatial strides] ->
    contiguous (B, H, R, T, D): out[b,h,r,t,:] = x[b,i,j,h*D:(h+1)*D] with
    (i, j) = (t, r) if transpose else (r, t)."""
    B, I, J, C = x.shape
    D = C // heads
    if (_fused_enabled(x) and D * heads == C and D > 0 and D % 8 == 0
            and _strided_ok(x)):
        return _PairArrange.apply(x, heads, transpose)
    x5 = x.unflatten(-1, (heads, D))
    x5 = x5.permute(0, 3, 2, 1, 4) if transpose else x5.permute(0, 3, 1, 2, 4)
    return x5.contiguous()


def pair_arrange_qkv(qkv, heads, transpose=False):
    """(B, I, J, 3*H*D) fused projection -> pair_arrange of its three chunks,
    with one gradient buffer for all three in backward."""
    C3 = qkv.shape[-1]
    D = C3 // (3 * heads)
    if (_fused_enabled(qkv) and qkv.dim() == 4 and 3 * heads * D == C3
            and D > 0 and D % 8 == 0 and _strided_ok(qkv)):
        return _PairArrangeQKV.apply(qkv, heads, transpose)
    return tuple(pair_arrange(t, heads, transpose)
                 for t in qkv.chunk(3, dim=-1))


def pair_merge(o, B, I, J, heads, transpose=False):
    """Inverse of pair_arrange: (B*H*R, T, D) -> contiguous (B, I, J, H*D)."""
    D = o.shape[-1]
    if (_fused_enabled(o) and D % 8 == 0 and o.dim() == 3
            and o.is_contiguous() and o.data_ptr() % 16 == 0):
        return _PairMerge.apply(o, B, I, J, heads, transpose)
    R, T = (J, I) if transpose else (I, J)
    o5 = o.reshape(B, heads, R, T, D)
    o5 = o5.permute(0, 3, 2, 1, 4) if transpose else o5.permute(0, 2, 3, 1, 4)
    return o5.reshape(B, I, J, heads * D)


def pair_bias_arrange(lin, transpose=False):
    """(B, L, L, H) -> contiguous (B, H, L, L): out[b,h,x,y] = lin[b,x,y,h],
    or lin[b,y,x,h] if transpose."""
    if _fused_enabled(lin) and lin.dim() == 4 and lin.shape[1] == lin.shape[2]:
        from unicore_amd import ops

        if (ops.pair_bias_arrange_supported(lin.shape[3], lin.shape[1])
                and lin.is_contiguous() and lin.data_ptr() % 16 == 0):
            return _PairBiasArrange.apply(lin, transpose)
    out = lin.permute(0, 3, 2, 1) if transpose else lin.permute(0, 3, 1, 2)
    return out.contiguous()


def _fold_ok(*biases):
    # same condition as the other Evoformer modules (models/evoformer.py)
    if os.environ.get("UNICORE_FOLD_BIAS", "1") != "1":
        return False
    from unicore_amd import ops

    if not ops.gpu_kernels_available():
        return False
    return all(b is not None and ops.colsum_supported(b.numel()) for b in biases)


class TriangleAttention(nn.Module):
    """Gated triangle self-attention; ``starting=False`` is the ending node."""

    def __init__(self, d_pair, heads, dropout, starting=True):
        super().__init__()
        self.heads = heads
        self.head_dim = d_pair // heads
        self.norm = LayerNorm(d_pair)
        self.qkv = nn.Linear(d_pair, 3 * d_pair, bias=False)
        self.bias_proj = nn.Linear(d_pair, heads, bias=False)
        self.gate = nn.Linear(d_pair, d_pair)
        self.out = nn.Linear(d_pair, d_pair)
        self.dropout = dropout
        self.starting = starting
        self.scaling = self.head_dim**-0.5

    def forward(self, pair, skip_out_bias=False, p_normed=None,
                pair_mask=None, key_mask=None):
        """pair_mask: optional 0/1 (B, I, J) padding mask; its additive key
        mask (padding_mask.triangle_key_mask) may be passed as ``key_mask``
        by a caller that builds it once for many blocks."""
        B, I, J, C = pair.shape
        H, D = self.heads, self.head_dim
        tr = not self.starting
        R, T = (J, I) if tr else (I, J)
        p = self.norm(pair) if p_normed is None else p_normed
        # rows r of the (transposed) pair tensor are the attention batches,
        # heads OUTSIDE them so the (B, H, 1, T, T) bias is a contiguous-
        # block broadcast for the fused softmax kernel
        q, k, v = (t.view(B * H * R, T, D)
                   for t in pair_arrange_qkv(self.qkv(p), H, tr))
        q = q * self.scaling
        scores = qk_scores(q, k).view(B, H, R, T, T)
        bias = pair_bias_arrange(self.bias_proj(p), tr).unsqueeze(2)
        if key_mask is None and pair_mask is not None:
            key_mask = triangle_key_mask(pair_mask, scores.dtype, self.starting)
        attn = softmax_dropout(scores, self.dropout, self.training,
                               mask=key_mask, bias=bias)
        o = torch.bmm(attn.view(B * H * R, T, T), v)
        o = pair_merge(o, B, I, J, H, tr)
        if _fold_ok(self.gate.bias):
            og = gated_mul(o, F.linear(p, self.gate.weight),
                           torch.zeros_like(self.gate.bias), self.gate.bias)
        else:
            og = o * torch.sigmoid(self.gate(p))
        if skip_out_bias:
            return F.linear(og, self.out.weight)
        return self.out(og)
