#!/usr/bin/env python3
"""Time modules.triangle_multiply, fused HIP contraction vs einsum.

bf16, B=1, C=64, L in {128, 256, 384}, both directions; forward alone and
forward+backward. One line per config. Same process, same box: the two
columns are directly comparable.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd.modules import triangle_multiply  # noqa: E402


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
    B, C = 1, 64
    for L in (128, 256, 384):
        a = torch.randn(B, L, L, C, device="cuda").bfloat16().requires_grad_()
        b = torch.randn(B, L, L, C, device="cuda").bfloat16().requires_grad_()
        d_out = torch.randn(B, L, L, C, device="cuda").bfloat16()
        for outgoing in (True, False):
            res = {}
            for gate in ("0", "1"):
                os.environ["UNICORE_TRI_FUSED"] = gate

                def fwd():
                    with torch.no_grad():
                        triangle_multiply(a, b, outgoing)

                def fwd_bwd():
                    a.grad = b.grad = None
                    triangle_multiply(a, b, outgoing).backward(d_out)

                res[gate] = (_time(fwd, 50), _time(fwd_bwd, 30))
            (ef, eb), (ff, fb) = res["0"], res["1"]
            tf = 2.0 * B * C * L ** 3 / ff / 1e6
            print(
                f"tri L={L} C={C} {'outgoing' if outgoing else 'incoming'}: "
                f"fwd einsum {ef:8.1f} us fused {ff:8.1f} us ({ef / ff:5.2f}x, "
                f"{tf:5.1f} TF) | fwd+bwd einsum {eb:8.1f} us fused {fb:8.1f} us "
                f"({eb / fb:5.2f}x)"
            )


if __name__ == "__main__":
    main()
