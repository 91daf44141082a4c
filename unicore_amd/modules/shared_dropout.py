"""Shared-axis dropout for the fused residual joins (AlphaFold 2
DropoutRowwise / DropoutColumnwise): one keep-mask per slice of a
``(B, R, T, C)`` tensor, broadcast along ``shared_dim`` (1 or 2).

``dropout_add``, ``dropout_add_ln_pre`` and ``dropout_add_ln`` route here
when their ``shared_dim`` keyword is set and dropout is active. The fused
path (csrc/shared_dropout.hip) draws the mask in-kernel and stores only the
small bitfield, ``B*T*C/8`` or ``B*R*C/8`` bytes, which backward reads back
through the same index map. The eager fallback multiplies by a broadcast
``F.dropout(ones(mask_shape))`` and hands the product to the p = 0 join.
"""

import os

import torch
import torch.nn.functional as F


def check_shared_dim(x, shared_dim):
    """Caller errors, raised on every path (not fallback cases)."""
    if shared_dim not in (1, 2):
        raise ValueError(f"shared_dim must be 1 or 2, got {shared_dim!r}")
    if x.dim() != 4:
        raise ValueError(
            "shared_dim needs a 4-D (B, R, T, C) input, got "
            f"{x.dim()}-D with shape {tuple(x.shape)}"
        )


def fused_enabled() -> bool:
    # A/B switch; docs/KERNELS.md "Shared-axis dropout" has the measurement
    # that decided the default
    return os.environ.get("UNICORE_SHARED_DROPOUT_FUSED", "1") == "1"


def fuse_ok(x, residual, bias) -> bool:
    if not (x.is_cuda and x.shape == residual.shape
            and x.dtype == residual.dtype and fused_enabled()):
        return False
    from unicore_amd import ops

    if not ops.shared_dropout_supported(x.shape, x.dtype):
        return False
    bias_ok = bias is None or (
        ops.colsum_supported(bias.numel()) and x.shape[-1] == bias.numel()
        and bias.dtype == x.dtype
    )
    return bias_ok and (ops.gpu_kernels_available()
                        or not ops.allow_eager_on_gpu())


def apply_shared_mask(x, p, shared_dim, bias=None):
    """Eager ``dropout(x + bias)`` with the keep-mask shared along
    ``shared_dim``; the caller continues with its p = 0 expression."""
    shape = list(x.shape)
    shape[shared_dim] = 1
    keep = F.dropout(torch.ones(shape, dtype=x.dtype, device=x.device), p=p)
    if bias is not None:
        x = x + bias
    return x * keep


class _SharedDropoutAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, bias, p, shared_dim):
        from unicore_amd import ops

        out, dmask = ops.shared_dropout_add_fwd(
            x.contiguous(), res.contiguous(), p, shared_dim, bias
        )
        ctx.p = p
        ctx.shared_dim = shared_dim
        ctx.bias_dim = bias.numel() if bias is not None else 0
        ctx.bias_dtype = bias.dtype if bias is not None else None
        ctx.save_for_backward(dmask)
        return out

    @staticmethod
    def backward(ctx, grad):
        from unicore_amd import ops

        (dmask,) = ctx.saved_tensors
        grad = grad.contiguous()
        dx, db = ops.shared_dropout_add_bwd(
            grad, dmask, ctx.p, ctx.shared_dim, ctx.bias_dim
        )
        dbias = db.to(ctx.bias_dtype) if ctx.bias_dim else None
        return dx, grad, dbias, None, None


class _SharedDropoutAddLN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, bias, gamma, beta, p, shared_dim, eps):
        from unicore_amd import ops

        normed, summed, dmask, mean, invvar = ops.shared_dropout_add_ln_fwd(
            x.contiguous(), res.contiguous(), bias, gamma.contiguous(),
            beta.contiguous(), p, shared_dim, eps,
        )
        ctx.save_for_backward(summed, dmask, mean, invvar, gamma)
        ctx.p = p
        ctx.shared_dim = shared_dim
        ctx.bias_dim = bias.numel() if bias is not None else 0
        ctx.bias_dtype = bias.dtype if bias is not None else None
        return normed

    @staticmethod
    def backward(ctx, d_norm):
        from unicore_amd import ops

        summed, dmask, mean, invvar, gamma = ctx.saved_tensors
        ds, dgamma, dbeta = ops.layernorm_bwd(
            d_norm.contiguous(), summed, mean, invvar, gamma
        )
        dx, db = ops.shared_dropout_add_bwd(
            ds, dmask, ctx.p, ctx.shared_dim, ctx.bias_dim
        )
        dbias = db.to(ctx.bias_dtype) if ctx.bias_dim else None
        return dx, ds, dbias, dgamma, dbeta, None, None, None


class _SharedDropoutAddLNPre(torch.autograd.Function):
    """Pre-LN chain variant (see _DropoutAddLNPre): returns the summed
    stream and the normed view, backward joins both gradients before the
    mask unmap."""

    @staticmethod
    def forward(ctx, x, res, bias, gamma, beta, p, shared_dim, eps):
        from unicore_amd import ops

        normed, summed, dmask, mean, invvar = ops.shared_dropout_add_ln_fwd(
            x.contiguous(), res.contiguous(), bias, gamma.contiguous(),
            beta.contiguous(), p, shared_dim, eps,
        )
        ctx.save_for_backward(summed, dmask, mean, invvar, gamma)
        ctx.p = p
        ctx.shared_dim = shared_dim
        ctx.bias_dim = bias.numel() if bias is not None else 0
        ctx.bias_dtype = bias.dtype if bias is not None else None
        return summed, normed

    @staticmethod
    def backward(ctx, d_sum, d_norm):
        from unicore_amd import ops

        summed, dmask, mean, invvar, gamma = ctx.saved_tensors
        if d_norm is None:
            # normed output unused downstream: only the stream grad flows
            ds = torch.zeros_like(summed)
            dgamma = torch.zeros_like(gamma)
            dbeta = torch.zeros_like(gamma)
        else:
            ds, dgamma, dbeta = ops.layernorm_bwd(
                d_norm.contiguous(), summed, mean, invvar, gamma
            )
        if d_sum is not None:
            ds = ds + d_sum
        dx, db = ops.shared_dropout_add_bwd(
            ds.contiguous(), dmask, ctx.p, ctx.shared_dim, ctx.bias_dim
        )
        dbias = db.to(ctx.bias_dtype) if ctx.bias_dim else None
        return dx, ds, dbias, dgamma, dbeta, None, None, None
