#!/usr/bin/env python3
"""Time the pair norm regulariser (modules/norm_loss.pair_norm) at 64 heads.

bf16, B = 32, at L = 128 (the stress-config shape) and L = 256, with a
padding mask; forward alone and forward+backward (gradients to pair and
bias). Two columns, timed alternately eager, fused, eager, fused
(--rounds 2):

  eager   UNICORE_PAIR_NORM=0: subtract, select, square, the sum over the
          head axis, sqrt, abs, relu, masked mean, and autograd's backward
  fused   the HIP kernels of csrc/pair_norm.hip

Same process, same box: the columns are directly comparable. The pairs are a
third each below, inside and above the tolerance band, mixed within every
8-position unit, so the backward reads nearly every unit. GB/s counts the
bytes the work requires, from the shapes: pair and bias read forward (2
tensors), pair and bias read and both gradients written backward (4). The
last lines per shape time ops.pair_norm_fwd / ops.pair_norm_bwd alone, and
the backward with every pair inside the band (nothing read, zeros written).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd import ops  # noqa: E402
from unicore_amd.modules.norm_loss import pair_norm  # noqa: E402


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    torch.manual_seed(0)
    B, H = 32, 64
    for L in (128, 256):
        mask = torch.zeros(B, L, dtype=torch.bool, device="cuda")
        mask[::2, L - 5:] = True
        fill = mask.view(B, 1, 1, L)
        fmin = torch.finfo(torch.bfloat16).min
        bias = (1.5 * torch.randn(B, H, L, L, device="cuda")).bfloat16()
        # |delta| = 8 s: 4.8 (below the band), 8 (inside), 11.2 (above)
        s = torch.tensor([0.6, 1.0, 1.4], device="cuda")[
            torch.randint(0, 3, (B, 1, L, L), device="cuda")]
        pair = (bias.float() + s * torch.randn(B, H, L, L, device="cuda")).bfloat16()
        del s
        pair = pair.masked_fill(fill, fmin).contiguous().requires_grad_()
        bias = bias.masked_fill(fill, fmin).contiguous().requires_grad_()
        nbytes = pair.numel() * 2
        fwd_bytes, bwd_bytes = 2 * nbytes, 4 * nbytes

        def fwd():
            with torch.no_grad():
                pair_norm(pair, bias, mask)

        def fwd_bwd():
            pair.grad = bias.grad = None
            pair_norm(pair, bias, mask).backward()

        res = {"eager": [], "fused": []}
        for _ in range(a.rounds):
            for col, gate in (("eager", "0"), ("fused", "1")):
                os.environ["UNICORE_PAIR_NORM"] = gate
                res[col].append((_time(fwd, 100), _time(fwd_bwd, 50)))
        (ef, eb), (ff, fb) = res["eager"][-1], res["fused"][-1]
        print(
            f"pair_norm bf16 B={B} L={L} H={H}: fwd eager {ef:8.1f} us fused "
            f"{ff:7.1f} us (fused {ef / ff:5.2f}x eager, "
            f"{fwd_bytes / ff / 1e3:6.1f} GB/s) | fwd+bwd eager {eb:8.1f} us "
            f"fused {fb:7.1f} us (fused {eb / fb:5.2f}x eager, "
            f"{(fwd_bytes + bwd_bytes) / fb / 1e3:6.1f} GB/s)"
        )
        for col in ("eager", "fused"):
            print(f"  {col} rounds, fwd / fwd+bwd us: " + ", ".join(
                f"{f:.1f} / {b:.1f}" for f, b in res[col]))

        p, q = pair.detach(), bias.detach()
        coef = ops.pair_norm_fwd(p, q, mask)[0]
        gscale = torch.full((B,), 1e-4, device="cuda")
        kf = _time(lambda: ops.pair_norm_fwd(p, q, mask), 200)
        kb = _time(lambda: ops.pair_norm_bwd(gscale, coef, p, q), 200)
        idle = torch.zeros_like(coef)
        ki = _time(lambda: ops.pair_norm_bwd(gscale, idle, p, q), 200)
        print(
            f"  kernels alone: fwd (+ row sum) {kf:7.1f} us, "
            f"{fwd_bytes / 1e6:.1f} MB, {fwd_bytes / kf / 1e3:6.1f} GB/s | bwd "
            f"{kb:7.1f} us, {bwd_bytes / 1e6:.1f} MB, "
            f"{bwd_bytes / kb / 1e3:6.1f} GB/s | bwd, all inside the band "
            f"{ki:7.1f} us, {2 * nbytes / 1e6:.1f} MB written, "
            f"{2 * nbytes / ki / 1e3:6.1f} GB/s"
        )
        del pair, bias, p, q, coef, idle


if __name__ == "__main__":
    main()
