"""Outer product mean of two MSA projections, in the stored pair layout.

    o[b,i,j,c*d] = (1/S) * sum_s a[b,s,i,c] * b[b,s,j,d]

The eager expression upcasts both operands to fp32, runs one fp32 GEMM that
lands in (i, c, j, d), permute-copies it to (i, j, c, d), divides by S and
casts back: three fp32 passes over a tensor of L*L*c*d elements, and the
same again in backward.  The fused path calls three bf16 MFMA contractions
(``ops.opm_fwd`` / ``opm_bwd_a`` / ``opm_bwd_b``, csrc/outer_product.hip)
that read and write the stored layouts directly, accumulate in fp32, apply
1/S in fp32 and round once.

Gate: ``UNICORE_OPM_FUSED`` (see docs/KERNELS.md, "Outer product mean", for
the measurement behind its default).  Eager fallback on CPU, for an
unsupported dtype or width, for non-contiguous or misaligned operands, and
when the gate is off.
"""

import os

import torch

# default of the UNICORE_OPM_FUSED gate: on. The same-box end-to-end A/B
# (profiles/evoformer_bs1x8_opm.txt) came out at +7.8%, above the 3% noise
# figure; the op itself runs 4.0x faster forward+backward at L=256.
_OPM_FUSED_DEFAULT = "1"


def _opm_fused_enabled() -> bool:
    return os.environ.get("UNICORE_OPM_FUSED", _OPM_FUSED_DEFAULT) == "1"


def _operand_ok(t) -> bool:
    # mirrors the host checks of csrc/outer_product.hip
    return t.is_contiguous() and t.data_ptr() % 16 == 0 and t.numel() > 0


class _OuterProductMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        from unicore_amd import ops

        ctx.save_for_backward(a, b)
        ctx.scale = 1.0 / a.shape[1]
        o = ops.opm_fwd(a, b, ctx.scale)
        return o.view(*o.shape[:3], o.shape[3] * o.shape[4])

    @staticmethod
    def backward(ctx, d_out):
        from unicore_amd import ops

        a, b = ctx.saved_tensors
        if not d_out.is_contiguous():
            d_out = d_out.contiguous()
        if d_out.data_ptr() % 16 != 0:  # contiguous() returned it as it was
            d_out = d_out.clone()
        d_o = d_out.view(*d_out.shape[:3], a.shape[-1], b.shape[-1])
        da = db = None
        if ctx.needs_input_grad[0]:
            da = ops.opm_bwd_a(d_o, b, ctx.scale)
        if ctx.needs_input_grad[1]:
            db = ops.opm_bwd_b(d_o, a, ctx.scale)
        return da, db


def _eager(a, b):
    o = torch.einsum("bsic,bsjd->bijcd", a.float(), b.float()) / a.shape[1]
    return o.reshape(*o.shape[:3], a.shape[-1] * b.shape[-1]).to(a.dtype)


def outer_product_mean(a, b):
    """a: (B, S, I, c), b: (B, S, J, d) -> (B, I, J, c*d) in a.dtype."""
    if (
        a.is_cuda
        and b.is_cuda
        and a.dim() == 4
        and b.dim() == 4
        and a.shape[:2] == b.shape[:2]
        and a.dtype == b.dtype
        and a.device == b.device
        and _opm_fused_enabled()
    ):
        from unicore_amd import ops

        if (
            ops.opm_supported(a.shape[-1], b.shape[-1], a.dtype)
            and _operand_ok(a)
            and _operand_ok(b)
            and (ops.gpu_kernels_available() or not ops.allow_eager_on_gpu())
        ):
            return _OuterProductMean.apply(a, b)
    return _eager(a, b)
