"""Fused dropout(x [+ bias]) + residual add + LayerNorm (post-LN join).

One kernel computes ``LN(residual + dropout(x + bias))``, writing the
pre-norm sum once (it is both the backward input and, in post-LN stacks,
never needed again) — versus the dropout_add + LN pair, this removes a
full extra read of the hidden tensor and a kernel launch per site.

Backward chains the two existing kernels: layernorm_backward over the
saved sum yields d_sum (+ dgamma/dbeta); dropout_add_backward maps d_sum
through the keep-mask and emits the folded-bias column sum; the residual
gradient IS d_sum. Eager fallback composes F.dropout + add + F.layer_norm.
"""

import os

import torch
import torch.nn.functional as F

from unicore_amd.modules.dropout_add import save_join, unmap_grad


def _ln_fwd(ctx, x, res, bias, gamma, beta, p, is_training, eps, shared_dim):
    """Forward of both autograd functions: (normed, summed)."""
    from unicore_amd import ops

    if shared_dim is None:
        normed, summed, dmask, mean, invvar = ops.dropout_add_ln_fwd(
            x.contiguous(), res.contiguous(), bias, gamma.contiguous(),
            beta.contiguous(), p, is_training, eps,
        )
    else:
        normed, summed, dmask, mean, invvar = ops.shared_dropout_add_ln_fwd(
            x.contiguous(), res.contiguous(), bias, gamma.contiguous(),
            beta.contiguous(), p, shared_dim, eps,
        )
    ctx.save_for_backward(summed, dmask, mean, invvar, gamma)
    save_join(ctx, p, bias, shared_dim)
    return normed, summed


class _DropoutAddLN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, bias, gamma, beta, p, is_training, eps,
                shared_dim=None):
        return _ln_fwd(ctx, x, res, bias, gamma, beta, p, is_training, eps,
                       shared_dim)[0]

    @staticmethod
    def backward(ctx, d_norm):
        from unicore_amd import ops

        summed, dmask, mean, invvar, gamma = ctx.saved_tensors
        ds, dgamma, dbeta = ops.layernorm_bwd(
            d_norm.contiguous(), summed, mean, invvar, gamma
        )
        dx, dbias = unmap_grad(ctx, ds, dmask)
        return dx, ds, dbias, dgamma, dbeta, None, None, None, None


class _DropoutAddLNPre(torch.autograd.Function):
    """Pre-LN chain variant: returns BOTH the summed residual stream and
    the normed view (the next sub-module's input). Backward receives
    gradients for both; the summed grad joins the LN input grad before the
    dropout/bias unmap."""

    @staticmethod
    def forward(ctx, x, res, bias, gamma, beta, p, is_training, eps,
                shared_dim=None):
        normed, summed = _ln_fwd(ctx, x, res, bias, gamma, beta, p,
                                 is_training, eps, shared_dim)
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
        dx, dbias = unmap_grad(ctx, ds.contiguous(), dmask)
        return dx, ds, dbias, dgamma, dbeta, None, None, None, None


def _fuse_ok(x, residual, bias):
    if not (
        x.is_cuda
        and x.shape == residual.shape
        and x.shape[-1] % 8 == 0
        and x.shape[-1] <= 2048
        and os.environ.get("UNICORE_FUSED_LN_JOIN", "1") == "1"
    ):
        return False
    from unicore_amd import ops

    bias_ok = bias is None or (
        ops.colsum_supported(bias.numel()) and x.shape[-1] == bias.numel()
    )
    return bias_ok and (ops.gpu_kernels_available()
                        or not ops.allow_eager_on_gpu())


def _shared(x, residual, bias, p, is_training, shared_dim, fn, ln):
    """shared_dim handling common to both joins: returns the fused result,
    or None with (x, p, bias) rewritten for the caller's p = 0 expression."""
    from unicore_amd.modules import shared_dropout as sd

    sd.check_shared_dim(x, shared_dim)
    if not (is_training and p > 0):
        return None, x, p, bias
    if (_fuse_ok(x, residual, bias) and sd.fuse_ok(x, residual, bias)
            and ln.weight.dtype == x.dtype and ln.bias.dtype == x.dtype):
        return fn.apply(x, residual, bias, ln.weight, ln.bias, p, True,
                        ln.eps, shared_dim), x, p, bias
    return None, sd.apply_shared_mask(x, p, shared_dim, bias), 0.0, None


def dropout_add_ln_pre(x, residual, ln, p, is_training, bias=None,
                       shared_dim=None):
    """Pre-LN residual chain step: ``s = residual + dropout(x + bias)``;
    returns ``(s, ln(s))`` — *s* continues the residual stream, ``ln(s)``
    feeds the next sub-module. Fused into one kernel on GPU.

    ``shared_dim`` (1 or 2, 4-D input): one keep-mask per slice, broadcast
    along that axis (modules/shared_dropout.py)."""
    if shared_dim is not None:
        out, x, p, bias = _shared(x, residual, bias, p, is_training,
                                  shared_dim, _DropoutAddLNPre, ln)
        if out is not None:
            return out
    if _fuse_ok(x, residual, bias):
        return _DropoutAddLNPre.apply(
            x, residual, bias, ln.weight, ln.bias, p, is_training, ln.eps
        )
    if bias is not None:
        x = x + bias
    if is_training and p > 0:
        x = F.dropout(x, p=p)
    s = residual + x
    return s, ln(s)


def dropout_add_ln(x, residual, ln, p, is_training, bias=None,
                   shared_dim=None):
    """``ln(residual + dropout(x + bias, p))`` — fused on GPU.

    *ln* is the LayerNorm module whose weight/bias/eps apply;
    ``shared_dim`` as in ``dropout_add_ln_pre``.
    """
    if shared_dim is not None:
        out, x, p, bias = _shared(x, residual, bias, p, is_training,
                                  shared_dim, _DropoutAddLN, ln)
        if out is not None:
            return out
    if _fuse_ok(x, residual, bias):
        return _DropoutAddLN.apply(
            x, residual, bias, ln.weight, ln.bias, p, is_training, ln.eps
        )
    if bias is not None:
        x = x + bias
    if is_training and p > 0:
        x = F.dropout(x, p=p)
    return ln(residual + x)
