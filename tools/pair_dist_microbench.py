#!/usr/bin/env python3
"""Time the pair distance head (PairDistHead) at 64 heads.

bf16, at the stress-config shape (B = 32, L = 128) and at L = 256; forward
alone and forward+backward (gradients to pair and the six parameters), with a
padding mask. Two columns, timed alternately eager, fused, eager, fused
(--rounds 2):

  eager   UNICORE_PAIR_COORD_EAGER=1: permute to channel-last, Linear, GELU,
          LayerNorm and Linear over B*L*L rows, the transpose-add
  fused   the HIP kernels of csrc/pair_dist_h64.hip

Same process, same box: the columns are directly comparable. GB/s counts the
fused path's minimum traffic (forward: read pair, write and read F, write
dist; backward: read grad, write and read dF twice, read pair twice, write
dpair). The last line per shape times ops.pair_dist_fwd / ops.pair_dist_bwd
alone (the kernels and the fold, without the module's torch ops).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd import ops  # noqa: E402
from unicore_amd.modules import PairDistHead  # noqa: E402


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
    H = 64
    os.environ["UNICORE_PAIR_DIST_H64"] = "1"
    for B, L in ((32, 128), (32, 256)):
        mask = torch.zeros(B, L, dtype=torch.bool, device="cuda")
        mask[::2, L - 5:] = True
        fill = torch.finfo(torch.bfloat16).min
        pair = torch.randn(B, H, L, L, device="cuda").bfloat16()
        pair = pair.masked_fill(mask.view(B, 1, 1, L), fill)
        pair = pair.contiguous().requires_grad_()
        grad = torch.randn(B, L, L, device="cuda")
        head = PairDistHead(H).cuda()
        nbytes = pair.numel() * 2
        sq = B * L * L * 4  # one fp32 (B, L, L) buffer
        fwd_bytes, bwd_bytes = nbytes + 3 * sq, 3 * nbytes + 4 * sq

        def fwd():
            with torch.no_grad():
                head(pair, mask)

        def fwd_bwd():
            pair.grad = None
            head.zero_grad(set_to_none=True)
            head(pair, mask).backward(grad)

        res = {"eager": [], "fused": []}
        for _ in range(a.rounds):
            for col, gate in (("eager", "1"), ("fused", "0")):
                os.environ["UNICORE_PAIR_COORD_EAGER"] = gate
                res[col].append((_time(fwd, 50), _time(fwd_bwd, 30)))
        (ef, eb), (ff, fb) = res["eager"][-1], res["fused"][-1]
        print(
            f"pair_dist bf16 B={B} L={L} H={H}: fwd eager {ef:8.1f} us fused "
            f"{ff:7.1f} us (fused {ef / ff:5.2f}x eager, "
            f"{fwd_bytes / ff / 1e3:6.1f} GB/s) | fwd+bwd eager {eb:8.1f} us "
            f"fused {fb:7.1f} us (fused {eb / fb:5.2f}x eager, "
            f"{(fwd_bytes + bwd_bytes) / fb / 1e3:6.1f} GB/s)"
        )
        for col in ("eager", "fused"):
            print(f"  {col} rounds, fwd / fwd+bwd us: " + ", ".join(
                f"{f:.1f} / {b:.1f}" for f, b in res[col]))

        w = [p.detach().float() for p in head.parameters()]
        w[4] = w[4].view(-1)
        p, eps = pair.detach(), head.layer_norm.eps
        kf = _time(lambda: ops.pair_dist_fwd(p, mask, *w, eps), 50)
        kb = _time(lambda: ops.pair_dist_bwd(grad, p, mask, *w, eps), 50)
        print(
            f"  kernels alone: fwd + sym {kf:7.1f} us, {fwd_bytes / 1e6:.1f} MB, "
            f"{fwd_bytes / kf / 1e3:6.1f} GB/s | bwd (sym + dpair + wgrad + "
            f"fold) {kb:7.1f} us, {bwd_bytes / 1e6:.1f} MB, "
            f"{bwd_bytes / kb / 1e3:6.1f} GB/s"
        )


if __name__ == "__main__":
    main()
