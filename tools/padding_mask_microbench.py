#!/usr/bin/env python3
"""Time the two masked kernels of the Evoformer padding masks (bf16).

Outer product mean at (B, S, L) = (1, 128, 256), c = 32, forward alone and
forward+backward (gradients of both operands):

  unweighted  outer_product_mean(a, b): the existing fused entries, scale 1/S
  weighted    outer_product_mean(a, b, mask=, inv_norm=), UNICORE_OPM_FUSED=1:
              eager a*m and b*m, then the weighted entries
  eager       the same call with UNICORE_OPM_FUSED=0: the masked eager
              expression (fp32 GEMM, permute, weight, cast)

Row-masked gated multiply at rows x C = 256*256 x 64 with both biases,
forward alone and forward+backward:

  fused   gated_mul(..., row_mask=m)
  eager   gated_mul(...) * m[..., None]: the existing kernel and an eager
          multiply

Same process, same box: the columns are directly comparable.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd.modules import gated_mul, outer_product_mean  # noqa: E402
from unicore_amd.modules.outer_product import opm_mask_inv_norm  # noqa: E402


def _time(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters  # us


def _fwd_and_fwd_bwd(call, leaves, grad, iters=(30, 20)):
    def fwd():
        with torch.no_grad():
            call()

    def fwd_bwd():
        for t in leaves:
            t.grad = None
        call().backward(grad)

    return _time(fwd, iters[0]), _time(fwd_bwd, iters[1])


def opm():
    B, S, L = 1, 128, 256
    a = torch.randn(B, S, L, 32, device="cuda").bfloat16().requires_grad_()
    b = torch.randn(B, S, L, 32, device="cuda").bfloat16().requires_grad_()
    grad = torch.randn(B, L, L, 1024, device="cuda").bfloat16()
    mask = torch.zeros(B, S, L, device="cuda", dtype=torch.bfloat16)
    mask[:, :100, :200] = 1  # trailing padding, as a collater leaves it
    w = opm_mask_inv_norm(mask)
    cols = {}
    for col, gate, kw in (("unweighted", "1", {}),
                          ("weighted", "1", {"mask": mask, "inv_norm": w}),
                          ("eager", "0", {"mask": mask, "inv_norm": w})):
        os.environ["UNICORE_OPM_FUSED"] = gate
        cols[col] = _fwd_and_fwd_bwd(lambda: outer_product_mean(a, b, **kw),
                                     (a, b), grad)
    os.environ.pop("UNICORE_OPM_FUSED")
    (uf, ub), (wf, wb), (ef, eb) = cols["unweighted"], cols["weighted"], cols["eager"]
    print(f"outer_product_mean (1, 128, 256, 256) masked: fwd unweighted {uf:8.1f} us "
          f"weighted {wf:8.1f} us eager {ef:8.1f} us (weighted {ef / wf:4.2f}x eager, "
          f"{wf / uf:4.2f}x unweighted) | fwd+bwd unweighted {ub:8.1f} us weighted "
          f"{wb:8.1f} us eager {eb:8.1f} us (weighted {eb / wb:4.2f}x eager, "
          f"{wb / ub:4.2f}x unweighted)")


def gated():
    rows, C = 256 * 256, 64
    x = torch.randn(1, 256, 256, C, device="cuda").bfloat16().requires_grad_()
    g = torch.randn(1, 256, 256, C, device="cuda").bfloat16().requires_grad_()
    bx = torch.randn(C, device="cuda").bfloat16().requires_grad_()
    bg = torch.randn(C, device="cuda").bfloat16().requires_grad_()
    grad = torch.randn(1, 256, 256, C, device="cuda").bfloat16()
    m = (torch.rand(1, 256, 256, device="cuda") < 0.6).bfloat16()
    ff, fb = _fwd_and_fwd_bwd(lambda: gated_mul(x, g, bx, bg, row_mask=m),
                              (x, g, bx, bg), grad, iters=(50, 30))
    ef, eb = _fwd_and_fwd_bwd(lambda: gated_mul(x, g, bx, bg) * m.unsqueeze(-1),
                              (x, g, bx, bg), grad, iters=(50, 30))
    nbytes = rows * C * 2
    print(f"gated_mul row_mask ({rows}, {C}): fwd fused {ff:7.1f} us eager {ef:7.1f} us "
          f"(fused {ef / ff:4.2f}x eager, {3 * nbytes / ff / 1e3:6.1f} GB/s) | fwd+bwd "
          f"fused {fb:7.1f} us eager {eb:7.1f} us (fused {eb / fb:4.2f}x eager)")


if __name__ == "__main__":
    torch.manual_seed(0)
    opm()
    gated()
