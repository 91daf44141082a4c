"""Fused dropout(x [+ bias]) + residual add: out = residual + dropout(x + b).

One HIP pass instead of torch's dropout + add pair; used at the two
residual joins of every transformer layer.  With ``bias`` the preceding
Linear runs bias-free and this op both adds the bias (free — the tensor
is already in registers) and produces its gradient as a deterministic
column sum in backward, replacing the eager per-Linear ``grad.sum(0)``
re-read of the full activation-sized grad tensor.  Eager fallback on CPU.
"""

import torch
import torch.nn.functional as F


def save_join(ctx, p, bias, shared_dim):
    ctx.p = p
    ctx.shared_dim = shared_dim
    ctx.bias_dim = bias.numel() if bias is not None else 0
    ctx.bias_dtype = bias.dtype if bias is not None else None


def unmap_grad(ctx, grad, dmask):
    """(dx, dbias) of a join from the contiguous gradient of its sum, by
    the backward entry that matches the forward's ``shared_dim``."""
    from unicore_amd import ops

    if ctx.shared_dim is not None:
        dx, db = ops.shared_dropout_add_bwd(
            grad, dmask, ctx.p, ctx.shared_dim, ctx.bias_dim
        )
    elif dmask.numel() == 0 and ctx.bias_dim == 0:
        return grad, None
    else:
        dx, db = ops.dropout_add_bwd(grad, dmask, ctx.p, ctx.bias_dim)
    return dx, db.to(ctx.bias_dtype) if ctx.bias_dim else None


class _DropoutAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, bias, p, is_training, shared_dim=None):
        from unicore_amd import ops

        if shared_dim is None:
            out, dmask = ops.dropout_add_fwd(
                x.contiguous(), res.contiguous(), p, is_training, bias
            )
        else:
            out, dmask = ops.shared_dropout_add_fwd(
                x.contiguous(), res.contiguous(), p, shared_dim, bias
            )
        save_join(ctx, p, bias, shared_dim)
        ctx.save_for_backward(dmask)
        return out

    @staticmethod
    def backward(ctx, grad):
        (dmask,) = ctx.saved_tensors
        grad = grad.contiguous()
        dx, dbias = unmap_grad(ctx, grad, dmask)
        return dx, grad, dbias, None, None, None


def dropout_add(x, residual, p, is_training, bias=None, shared_dim=None):
    """residual + dropout(x + bias, p), fused on GPU.

    ``shared_dim`` (1 or 2, 4-D input): one keep-mask per slice, broadcast
    along that axis (modules/shared_dropout.py)."""
    if shared_dim is not None:
        from unicore_amd.modules import shared_dropout as sd

        sd.check_shared_dim(x, shared_dim)
        if is_training and p > 0:
            if sd.fuse_ok(x, residual, bias):
                return _DropoutAdd.apply(x, residual, bias, p, True,
                                         shared_dim)
            x = sd.apply_shared_mask(x, p, shared_dim, bias)
            p, bias = 0.0, None
    if x.is_cuda and x.numel() % 8 == 0 and x.shape == residual.shape:
        from unicore_amd import ops

        bias_ok = bias is None or (
            ops.colsum_supported(bias.numel()) and x.shape[-1] == bias.numel()
        )
        if bias_ok and (ops.gpu_kernels_available() or not ops.allow_eager_on_gpu()):
            return _DropoutAdd.apply(x, residual, bias, p, is_training)
    if bias is not None:
        x = x + bias
    if is_training and p > 0:
        x = F.dropout(x, p=p)
    return residual + x
