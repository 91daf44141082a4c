#!/usr/bin/env python3
"""Time the residual joins with shared-axis dropout.

bf16, pair (1, 256, 256, 128) at p = 0.25 and MSA (1, 128, 256, 256) at
p = 0.15, with the folded bias; ``dropout_add_ln_pre`` and ``dropout_add``,
forward alone and forward+backward. Three columns per line:

  eager   UNICORE_SHARED_DROPOUT_FUSED=0: eager mask multiply, then the
          fused join at p = 0
  fused   UNICORE_SHARED_DROPOUT_FUSED=1: the join kernels, shared mask map
  unshared  the existing join at the same p (no shared_dim): the bandwidth
          yardstick, an activation-sized draw and mask

Same process, same box: the columns are directly comparable. GB/s counts
the fused path's traffic (forward: read x and residual, write the sum, and
for the LN join the normed tensor; backward of dropout_add: read g, write
dx).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd.modules import LayerNorm, dropout_add  # noqa: E402
from unicore_amd.modules.dropout_add_ln import dropout_add_ln_pre  # noqa: E402


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


def main():
    torch.manual_seed(0)
    cases = [
        ("pair", (1, 256, 256, 128), 0.25, 1),
        ("pair", (1, 256, 256, 128), 0.25, 2),
        ("msa", (1, 128, 256, 256), 0.15, 1),
    ]
    for name, shape, p, sd in cases:
        C = shape[-1]
        x = torch.randn(shape, device="cuda").bfloat16().requires_grad_()
        res = torch.randn(shape, device="cuda").bfloat16().requires_grad_()
        bias = torch.randn(C, device="cuda").bfloat16().requires_grad_()
        ln = LayerNorm(C).cuda().bfloat16()
        g1 = torch.randn(shape, device="cuda").bfloat16()
        g2 = torch.randn(shape, device="cuda").bfloat16()
        nbytes = x.numel() * 2

        def join_add(shared_dim):
            return dropout_add(x, res, p, True, bias=bias, shared_dim=shared_dim)

        def join_ln(shared_dim):
            return dropout_add_ln_pre(x, res, ln, p, True, bias=bias,
                                      shared_dim=shared_dim)

        for op, join, fwd_tensors in (("dropout_add_ln_pre", join_ln, 4),
                                      ("dropout_add", join_add, 3)):
            res_t = {}
            for col, gate, shared_dim in (("eager", "0", sd), ("fused", "1", sd),
                                          ("unshared", "1", None)):
                os.environ["UNICORE_SHARED_DROPOUT_FUSED"] = gate

                def fwd():
                    with torch.no_grad():
                        join(shared_dim)

                def fwd_bwd():
                    x.grad = res.grad = bias.grad = None
                    ln.weight.grad = ln.bias.grad = None
                    out = join(shared_dim)
                    if isinstance(out, tuple):
                        torch.autograd.backward(list(out), [g1, g2])
                    else:
                        out.backward(g1)

                res_t[col] = (_time(fwd, 50), _time(fwd_bwd, 30))
            (ef, eb), (ff, fb), (uf, ub) = (res_t["eager"], res_t["fused"],
                                            res_t["unshared"])
            print(
                f"{op} {name} {shape} p={p} shared_dim={sd}: fwd eager "
                f"{ef:7.1f} us fused {ff:7.1f} us unshared {uf:7.1f} us "
                f"(fused {ef / ff:4.2f}x eager, {fwd_tensors * nbytes / ff / 1e3:6.1f} GB/s)"
                f" | fwd+bwd eager {eb:7.1f} us fused {fb:7.1f} us unshared "
                f"{ub:7.1f} us (fused {eb / fb:4.2f}x eager, "
                f"{fb / ub:4.2f}x unshared)"
            )


if __name__ == "__main__":
    main()
