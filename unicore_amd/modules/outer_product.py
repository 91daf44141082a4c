"""Outer product mean of two MSA projections, in the stored pair layout.

    o[b,i,j,c*d] = (1/S) * sum_s a[b,s,i,c] * b[b,s,j,d]

The eager expression upcasts both operands to fp32, runs one fp32 GEMM that
lands in (i, c, j, d), permute-copies it to (i, j, c, d), divides by S and
casts back: three fp32 passes over a tensor of L*L*c*d elements, and the
same again in backward.  The fused path calls three bf16 MFMA contractions
(``ops.opm_fwd`` / ``opm_bwd_a`` / ``opm_bwd_b``, csrc/outer_product.hip)
that read and write the stored layouts directly, accumulate in fp32, apply
1/S in fp32 and round once.

Padded batches (``mask``, 1 where an MSA token is real, (B, S, L)):

    o[b,i,j] = sum_s (m_si a_si) x (m_sj b_sj) / (1e-3 + sum_s m_si m_sj)

The reciprocal normaliser ``inv_norm`` (fp32, (B, L, L)) depends on the mask
alone: ``opm_mask_inv_norm`` computes it once per forward and every block
passes it in.  The fused path multiplies the two small projections by the
mask eagerly and calls the weighted entries (``ops.opm_fwd_w`` /
``opm_bwd_a_w`` / ``opm_bwd_b_w``), which take ``inv_norm`` in place of the
scalar 1/S; no tensor of the output's size is touched outside the kernels.

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
# Masked calls (mask=) share the gate and its default: under
# --msa-padding-mask the same A/B (profiles/evoformer_padding_mask.txt) has
# the weighted entries 14-15% ahead of the masked eager expression end to
# end, and 3.7x forward+backward for the op at L=256.
_OPM_FUSED_DEFAULT = "1"

OPM_MASK_EPS = 1e-3


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


class _OuterProductMeanW(torch.autograd.Function):
    """The weighted contraction: w (fp32, (B, I, J)) in place of 1/S.  w comes
    from the 0/1 mask and gets no gradient."""

    @staticmethod
    def forward(ctx, a, b, w):
        from unicore_amd import ops

        ctx.save_for_backward(a, b, w)
        o = ops.opm_fwd_w(a, b, w)
        return o.view(*o.shape[:3], o.shape[3] * o.shape[4])

    @staticmethod
    def backward(ctx, d_out):
        from unicore_amd import ops

        a, b, w = ctx.saved_tensors
        if not d_out.is_contiguous():
            d_out = d_out.contiguous()
        if d_out.data_ptr() % 16 != 0:  # contiguous() returned it as it was
            d_out = d_out.clone()
        d_o = d_out.view(*d_out.shape[:3], a.shape[-1], b.shape[-1])
        da = db = None
        if ctx.needs_input_grad[0]:
            da = ops.opm_bwd_a_w(d_o, b, w)
        if ctx.needs_input_grad[1]:
            db = ops.opm_bwd_b_w(d_o, a, w)
        return da, db, None


def _acc_dtype(t):
    return torch.promote_types(t.dtype, torch.float32)


def opm_mask_inv_norm(mask):
    """1 / (1e-3 + sum_s m[b,s,i] m[b,s,j]) for a 0/1 mask (B, S, L): the
    reciprocal normaliser of the masked mean, (B, L, L), fp32 (float64 for a
    float64 mask).  No gradient."""
    m = mask.detach().to(_acc_dtype(mask))
    norm = torch.matmul(m.transpose(1, 2), m)
    return (1.0 / (OPM_MASK_EPS + norm)).contiguous()


def _eager_masked(a, b, mask, inv_norm):
    m = mask.unsqueeze(-1).to(a.dtype)
    acc = _acc_dtype(a)
    o = torch.einsum("bsic,bsjd->bijcd", (a * m).to(acc), (b * m).to(acc))
    o = o * inv_norm.to(acc)[..., None, None]
    return o.reshape(*o.shape[:3], a.shape[-1] * b.shape[-1]).to(a.dtype)


def _eager(a, b):
    o = torch.einsum("bsic,bsjd->bijcd", a.float(), b.float()) / a.shape[1]
    return o.reshape(*o.shape[:3], a.shape[-1] * b.shape[-1]).to(a.dtype)


def _fused_ok(a, b) -> bool:
    if not (
        a.is_cuda
        and b.is_cuda
        and a.dim() == 4
        and b.dim() == 4
        and a.shape[:2] == b.shape[:2]
        and a.dtype == b.dtype
        and a.device == b.device
        and _opm_fused_enabled()
    ):
        return False
    from unicore_amd import ops

    return (
        ops.opm_supported(a.shape[-1], b.shape[-1], a.dtype)
        and _operand_ok(a)
        and _operand_ok(b)
        and (ops.gpu_kernels_available() or not ops.allow_eager_on_gpu())
    )


def outer_product_mean(a, b, mask=None, inv_norm=None):
    """a: (B, S, I, c), b: (B, S, J, d) -> (B, I, J, c*d) in a.dtype.

    mask: optional 0/1 (B, S, L) with I == J == L, 1 where a token is real;
    inv_norm: its ``opm_mask_inv_norm`` (computed here when not given)."""
    if mask is None:
        assert inv_norm is None, "inv_norm without a mask"
        if _fused_ok(a, b):
            return _OuterProductMean.apply(a, b)
        return _eager(a, b)
    if inv_norm is None:
        inv_norm = opm_mask_inv_norm(mask)
    if _fused_ok(a, b):
        m = mask.unsqueeze(-1).to(a.dtype)
        am, bm = a * m, b * m  # the small operands; contiguous results
        w = inv_norm
        if w.dtype != torch.float32 or not w.is_contiguous():
            w = w.float().contiguous()
        if _operand_ok(am) and _operand_ok(bm):
            return _OuterProductMeanW.apply(am, bm, w)
    return _eager_masked(a, b, mask, inv_norm)
