"""Fused attention of the Evoformer's attention sites (csrc/evo_attn.hip):
bf16, head dim 32, T % 64 == 0, 64 <= T <= 512.

    o = dropout(softmax(q k^T + bias + mask)) v

``evo_attention`` takes the sites' batched operands and returns ``o`` as
(N, T, D), or ``None`` when the kernels do not serve the call; the caller then
runs ``qk_scores`` -> ``softmax_dropout`` -> ``bmm`` as before.

Gate: ``UNICORE_EVO_ATTN``, read per call (docs/KERNELS.md, "Evoformer
attention", has the measurement behind its default).
"""

import os

import torch

from .softmax_dropout import _broadcast_descr

# default of the UNICORE_EVO_ATTN gate: on.  Same-box figures
# (profiles/evoformer_evo_attn.txt): forward+backward of the module at msa
# 128 / residues 256 is 1.07x (both triangle nodes), 1.16x (MSA row) and
# 1.40x (MSA column) the chain, and the stress command 2.76 -> 2.92 ups.
_EVO_ATTN_DEFAULT = "1"


class _EvoAttn(torch.autograd.Function):
    """Scores never reach HBM; dropout keep bits are recomputed from the
    Philox key in backward; the bias gradient is summed over the batches
    that share a bias block inside its own kernel, in a fixed order."""

    @staticmethod
    def forward(ctx, q, k, v, bias, bias_od, mask, mask_od, p, training):
        from unicore_amd import ops

        o, lse, seed = ops.evo_attn_fwd(
            q, k, v, bias, bias_od, mask, mask_od, p, training
        )
        ctx.save_for_backward(q, k, v, o, lse,
                              bias if bias is not None else q.new_empty(0),
                              mask if mask is not None else q.new_empty(0))
        ctx.bias_od = bias_od
        ctx.mask_od = mask_od
        ctx.p = p
        ctx.dropped = training and p > 0
        ctx.seed = int(seed)
        return o

    @staticmethod
    def backward(ctx, d_out):
        from unicore_amd import ops

        q, k, v, o, lse, bias, mask = ctx.saved_tensors
        bias_t = bias if bias.numel() else None
        mask_t = mask if mask.numel() else None
        want_dbias = bias_t is not None and ctx.needs_input_grad[3]
        d_out = d_out.contiguous()
        if d_out.data_ptr() % 16 != 0:
            d_out = d_out.clone()
        grads = ops.evo_attn_bwd(
            d_out, q, k, v, o, lse, bias_t, ctx.bias_od, want_dbias, mask_t,
            ctx.mask_od, ctx.p, ctx.dropped, ctx.seed,
        )
        dbias = grads[3].to(bias_t.dtype) if want_dbias else None
        return grads[0], grads[1], grads[2], dbias, None, None, None, None, None


def _src(src, batch_dims, T, rows):
    """(tensor (nb, rows, T), outer_div) of an additive bias / mask, or None
    when its shape or broadcast pattern is outside the kernels' contract."""
    if src.dim() < 2 or src.shape[-1] != T or src.shape[-2] != rows:
        return None
    descr = _broadcast_descr(tuple(src.shape[:-2]), batch_dims)
    if descr is None:
        return None
    nb, od = descr
    n = 1
    for d in batch_dims:
        n *= d
    if n % (nb * od) != 0:
        return None
    return src.reshape(nb, rows, T), od


def _evo_plan(q, k, v, bias, mask):
    """Everything but the device and the gate: (bias, bias_od, mask, mask_od)
    in the kernels' form, or None.  q, k, v are (..., T, D) with the same
    batch dims; bias is (..., T, T), mask (..., 1, T), both broadcast against
    the batch dims by the softmax_dropout contract."""
    if q.dim() < 3 or k.shape != q.shape or v.shape != q.shape:
        return None
    T, D = q.shape[-2], q.shape[-1]
    if q.dtype != torch.bfloat16 or D != 32 or T % 64 != 0 or not 64 <= T <= 512:
        return None
    batch_dims = tuple(q.shape[:-2])
    bias_k, bias_od, mask_k, mask_od = None, 1, None, 1
    if bias is not None:
        got = None if bias.dtype != q.dtype else _src(bias, batch_dims, T, T)
        if got is None:
            return None
        bias_k, bias_od = got
    if mask is not None:
        got = None
        if mask.dtype == q.dtype and not mask.requires_grad:
            got = _src(mask, batch_dims, T, 1)
        if got is None:
            return None
        mask_k, mask_od = got
    return bias_k, bias_od, mask_k, mask_od


def _dense(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def evo_enabled() -> bool:
    return os.environ.get("UNICORE_EVO_ATTN", _EVO_ATTN_DEFAULT) == "1"


def evo_attention(q, k, v, bias, mask, p, training):
    """q, k, v: (*batch, T, D), q pre-scaled; bias (..., T, T) and additive
    key mask (..., 1, T) or None.  Returns o as (N, T, D), or None: CPU, gate
    off, dtype, head dim, T or a broadcast pattern the kernels do not take."""
    if not q.is_cuda or not evo_enabled():
        return None
    plan = _evo_plan(q, k, v, bias, mask)
    if plan is None:
        return None
    from unicore_amd import ops

    T, D = q.shape[-2], q.shape[-1]
    N = q.numel() // (T * D)
    if not ops.gpu_kernels_available() or not ops.evo_attn_supported(
            N, T, D, q.dtype):
        return None
    bias_k, bias_od, mask_k, mask_od = plan
    q, k, v = (_dense(t.reshape(N, T, D)) for t in (q, k, v))
    if bias_k is not None:
        bias_k = _dense(bias_k)
    if mask_k is not None:
        mask_k = _dense(mask_k)
    return _EvoAttn.apply(q, k, v, bias_k, bias_od, mask_k, mask_od,
                          float(p), bool(training))
