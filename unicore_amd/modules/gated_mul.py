"""Fused gated multiply: out = (x + bias_x) * sigmoid(g + bias_g).

The Evoformer/AlphaFold gating idiom.  Both projection biases ride the
kernel (their Linears run bias-free) and backward returns the bias grads
as deterministic column sums — replacing torch's sigmoid + mul kernel
pair and two activation-sized bias-grad reductions.  Eager fallback on
CPU / when the extension is absent.

``row_mask`` (one value per row of the last dim, in x's dtype; the 0/1 pair
mask of a padded batch) multiplies the result inside the same kernel, and dx,
dg and both bias gradients in backward.
"""

import torch


class _GatedMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, bias_x, bias_g):
        from unicore_amd import ops

        x = x.contiguous()
        g = g.contiguous()
        ctx.save_for_backward(x, g, bias_x, bias_g)
        return ops.gated_mul_fwd(x, g, bias_x, bias_g)

    @staticmethod
    def backward(ctx, grad):
        from unicore_amd import ops

        x, g, bias_x, bias_g = ctx.saved_tensors
        dx, dg, db = ops.gated_mul_bwd(grad, x, g, bias_x, bias_g)
        dbx = dbg = None
        if bias_x is not None:
            C = bias_x.numel()
            dbx = db[:C].to(bias_x.dtype)
            dbg = db[C:].to(bias_g.dtype)
        return dx, dg, dbx, dbg


class _GatedMulMasked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, bias_x, bias_g, row_mask):
        from unicore_amd import ops

        x = x.contiguous()
        g = g.contiguous()
        row_mask = row_mask.contiguous()
        ctx.save_for_backward(x, g, bias_x, bias_g, row_mask)
        return ops.gated_mul_masked_fwd(x, g, bias_x, bias_g, row_mask)

    @staticmethod
    def backward(ctx, grad):
        from unicore_amd import ops

        x, g, bias_x, bias_g, row_mask = ctx.saved_tensors
        dx, dg, db = ops.gated_mul_masked_bwd(grad, x, g, bias_x, bias_g,
                                              row_mask)
        dbx = dbg = None
        if bias_x is not None:
            C = bias_x.numel()
            dbx = db[:C].to(bias_x.dtype)
            dbg = db[C:].to(bias_g.dtype)
        return dx, dg, dbx, dbg, None


def gated_mul(x, g, bias_x=None, bias_g=None, row_mask=None):
    """(x + bias_x) * sigmoid(g + bias_g); biases optional (must be both
    present or both absent for the fused path).  row_mask: optional, one
    value per row (x.numel() / x.shape[-1] elements, not differentiated)."""
    if x.is_cuda and x.numel() % 8 == 0 and x.shape == g.shape:
        from unicore_amd import ops

        bias_ok = (bias_x is None) == (bias_g is None) and (
            bias_x is None
            or (ops.colsum_supported(bias_x.numel()) and x.shape[-1] == bias_x.numel())
        )
        if bias_ok and (ops.gpu_kernels_available() or not ops.allow_eager_on_gpu()):
            if row_mask is None:
                return _GatedMul.apply(x, g, bias_x, bias_g)
            # a thread's 8 elements must lie in one row
            if (x.shape[-1] % 8 == 0 and row_mask.is_cuda
                    and row_mask.dtype == x.dtype
                    and row_mask.numel() * x.shape[-1] == x.numel()):
                return _GatedMulMasked.apply(x, g, bias_x, bias_g,
                                             row_mask.detach())
    if bias_x is not None:
        x = x + bias_x
    if bias_g is not None:
        g = g + bias_g
    out = x * torch.sigmoid(g)
    if row_mask is not None:
        out = out * row_mask.reshape(*x.shape[:-1], 1).to(out.dtype)
    return out
