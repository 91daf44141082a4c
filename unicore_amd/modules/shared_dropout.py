"""Shared-axis dropout for the fused residual joins (AlphaFold 2
DropoutRowwise / DropoutColumnwise): one keep-mask per slice of a
``(B, R, T, C)`` tensor, broadcast along ``shared_dim`` (1 or 2).

``dropout_add``, ``dropout_add_ln_pre`` and ``dropout_add_ln`` consult the
gates here when their ``shared_dim`` keyword is set and dropout is active.
The fused path (the join kernels with the shared mask map,
csrc/dropout_mask.h) draws the mask in-kernel and stores only the small
bitfield, ``B*T*C/8`` or ``B*R*C/8`` bytes, which backward reads back
through the same index map; the joins' own autograd functions carry
``shared_dim``. The eager fallback multiplies by a broadcast
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
