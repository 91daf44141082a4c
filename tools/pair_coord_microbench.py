#!/usr/bin/env python3
"""Time the equivariant coordinate head (PairCoordHead).

bf16, H = 8, at the stress-config shape (B = 32, L = 128) and at L = 256;
forward alone and forward+backward (gradients to pair, pair0 and the four
parameters), with a padding mask. Two columns per line:

  eager   UNICORE_PAIR_COORD_EAGER=1: permute to channel-last, two Linears
          and a GELU over B*L*L rows, the (B, L, L, 3) product, the sum
  fused   the HIP kernels of csrc/pair_coord.hip

Same process, same box: the columns are directly comparable. GB/s counts
the fused path's minimum traffic (forward: read pair and pair0; backward:
read both twice, write dpair and dpair0).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd.modules import PairCoordHead  # noqa: E402


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
    H = 8
    for B, L in ((32, 128), (32, 256)):
        mask = torch.zeros(B, L, dtype=torch.bool, device="cuda")
        mask[::2, L - 5:] = True
        fill = torch.finfo(torch.bfloat16).min
        pair0 = torch.randn(B, H, L, L, device="cuda").bfloat16()
        pair0 = pair0.masked_fill(mask.view(B, 1, 1, L), fill)
        pair = pair0 + torch.randn(B, H, L, L, device="cuda").bfloat16()
        pair = torch.where(mask.view(B, 1, 1, L), pair0, pair)
        pair = pair.contiguous().requires_grad_()
        pair0 = pair0.requires_grad_()
        coords = torch.randn(B, L, 3, device="cuda")
        grad = torch.randn(B, L, 3, device="cuda")
        head = PairCoordHead(H).cuda()
        nbytes = pair.numel() * 2

        res = {}
        for col, gate in (("eager", "1"), ("fused", "0")):
            os.environ["UNICORE_PAIR_COORD_EAGER"] = gate

            def fwd():
                with torch.no_grad():
                    head(pair, pair0, coords, mask)

            def fwd_bwd():
                pair.grad = pair0.grad = None
                head.zero_grad(set_to_none=True)
                head(pair, pair0, coords, mask).backward(grad)

            res[col] = (_time(fwd, 50), _time(fwd_bwd, 30))
        (ef, eb), (ff, fb) = res["eager"], res["fused"]
        print(
            f"pair_coord bf16 B={B} L={L} H={H}: fwd eager {ef:8.1f} us fused "
            f"{ff:7.1f} us (fused {ef / ff:5.2f}x eager, "
            f"{2 * nbytes / ff / 1e3:6.1f} GB/s) | fwd+bwd eager {eb:8.1f} us "
            f"fused {fb:7.1f} us (fused {eb / fb:5.2f}x eager, "
            f"{8 * nbytes / fb / 1e3:6.1f} GB/s)"
        )


if __name__ == "__main__":
    main()
