"""Triangle multiplication contraction on channel-last pair tensors.

    outgoing: o[b,i,j,c] = sum_k a[b,i,k,c] * b[b,j,k,c]
    incoming: o[b,i,j,c] = sum_k a[b,k,i,c] * b[b,k,j,c]

Every channel is an independent L x L x L GEMM, which is the worst layout
for the library: einsum permute-copies both operands to channel-first,
runs B*C small batched GEMMs and permute-copies the result back, three
times per training step.  The fused path calls one HIP primitive
(``ops.tri_contract``: O[x,y] = sum_z A[x,z] B[y,z] with free spatial
strides) on ``transpose(1, 2)`` views, so forward and both gradients read
and write the stored layout directly:

                      result                         A (x, z)    B (y, z)
    outgoing fwd      o[i,j]  = sum_k a[i,k] b[j,k]  a           b
    outgoing da[i,k]          = sum_j do[i,j] b[j,k] do          b^T
    outgoing db[j,k]          = sum_i do[i,j] a[i,k] do^T        a^T
    incoming fwd      o[i,j]  = sum_k a[k,i] b[k,j]  a^T         b^T
    incoming da[k,i]          = sum_j b[k,j] do[i,j] b           do
    incoming db[k,j]          = sum_i a[k,i] do[i,j] a           do^T

Gate: ``UNICORE_TRI_FUSED`` (see docs/KERNELS.md, "Triangle contraction",
for the measurement behind its default).  Eager einsum fallback on CPU,
for unsupported C/dtype/strides, and when the gate is off.
"""

import os

import torch

# default of the UNICORE_TRI_FUSED gate: opt-in. The same-box end-to-end A/B
# (profiles/evoformer_bs1x8_tricontract.txt) came out at +1.2%, inside the
# +-3% noise figure, although the op itself runs 2.0-2.4x faster at L=256.
_TRI_FUSED_DEFAULT = "0"


def _tri_fused_enabled() -> bool:
    return os.environ.get("UNICORE_TRI_FUSED", _TRI_FUSED_DEFAULT) == "1"


def _operand_ok(t) -> bool:
    # mirrors the host checks of csrc/triangle.hip
    if t.stride(3) != 1 or t.data_ptr() % 16 != 0:
        return False
    return all(t.size(d) == 1 or t.stride(d) % 8 == 0 for d in range(3))


def _operand(t):
    return t if _operand_ok(t) else t.contiguous()


def _T(t):
    return t.transpose(1, 2)


class _TriangleMultiply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, outgoing):
        from unicore_amd import ops

        ctx.save_for_backward(a, b)
        ctx.outgoing = outgoing
        if outgoing:
            return ops.tri_contract(a, b)
        return ops.tri_contract(_T(a), _T(b))

    @staticmethod
    def backward(ctx, d_out):
        from unicore_amd import ops

        a, b = ctx.saved_tensors
        d_out = _operand(d_out)
        da = db = None
        if ctx.outgoing:
            if ctx.needs_input_grad[0]:
                da = ops.tri_contract(d_out, _T(b))
            if ctx.needs_input_grad[1]:
                db = ops.tri_contract(_T(d_out), _T(a))
        else:
            if ctx.needs_input_grad[0]:
                da = ops.tri_contract(b, d_out)
            if ctx.needs_input_grad[1]:
                db = ops.tri_contract(a, _T(d_out))
        return da, db, None


def _einsum(a, b, outgoing):
    if outgoing:
        return torch.einsum("bikc,bjkc->bijc", a, b)
    return torch.einsum("bkic,bkjc->bijc", a, b)


def triangle_multiply(a, b, outgoing: bool):
    """a, b: stored (B, L, L, C) pair activations -> (B, L, L, C)."""
    if (
        a.is_cuda
        and b.is_cuda
        and a.dim() == 4
        and a.shape == b.shape
        and a.dtype == b.dtype
        and a.device == b.device
        and _tri_fused_enabled()
    ):
        from unicore_amd import ops

        if (
            ops.tri_contract_supported(a.shape[-1], a.dtype)
            and _operand_ok(a)
            and _operand_ok(b)
            and (ops.gpu_kernels_available() or not ops.allow_eager_on_gpu())
        ):
            return _TriangleMultiply.apply(a, b, bool(outgoing))
    return _einsum(a, b, outgoing)
