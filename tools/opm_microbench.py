#!/usr/bin/env python3
"""Time modules.outer_product_mean, fused HIP contractions vs the eager
fp32 einsum expression.

bf16, B=1, S=128, c=32, L in {128, 256, 384}; forward alone and
forward+backward. One line per config. Same process, same box: the two
columns are directly comparable. TF/s counts 2*S*(L*32)^2 per contraction
(one in forward, three in forward+backward).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd.modules import outer_product_mean  # noqa: E402


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
    B, S, C = 1, 128, 32
    for L in (128, 256, 384):
        a = torch.randn(B, S, L, C, device="cuda").bfloat16().requires_grad_()
        b = torch.randn(B, S, L, C, device="cuda").bfloat16().requires_grad_()
        d_out = torch.randn(B, L, L, C * C, device="cuda").bfloat16()
        res = {}
        for gate in ("0", "1"):
            os.environ["UNICORE_OPM_FUSED"] = gate

            def fwd():
                with torch.no_grad():
                    outer_product_mean(a, b)

            def fwd_bwd():
                a.grad = b.grad = None
                outer_product_mean(a, b).backward(d_out)

            res[gate] = (_time(fwd, 30), _time(fwd_bwd, 20))
        (ef, eb), (ff, fb) = res["0"], res["1"]
        flop = 2.0 * B * S * (L * C) ** 2
        print(
            f"opm L={L} S={S} c={C}: fwd eager {ef:8.1f} us fused {ff:8.1f} us "
            f"({ef / ff:5.2f}x, {flop / ff / 1e6:5.1f} TF) | fwd+bwd eager "
            f"{eb:8.1f} us fused {fb:8.1f} us ({eb / fb:5.2f}x, "
            f"{3 * flop / fb / 1e6:5.1f} TF)"
        )


if __name__ == "__main__":
    main()
