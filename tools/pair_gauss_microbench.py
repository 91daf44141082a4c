#!/usr/bin/env python3
"""Time the Uni-Mol pair embedding (PairGaussianEmbed) at K = 128, H = 64.

bf16, B = 32, at L = 128 (the stress-config shape) and L = 256; module forward
alone and forward+backward (gradients to all eight parameters), with a padding
mask. Two columns, timed alternately eager, fused, eager, fused (--rounds 2):

  eager   UNICORE_PAIR_GAUSS_H64=0: the (B, L, L, 128) features, two library
          GEMMs, GELU, the permute-copy and the masked_fill
  fused   the HIP kernels of csrc/pair_gauss_h64.hip

Same process, same box: the columns are directly comparable. The last line per
shape times ops.pair_gauss_fwd / ops.pair_gauss_bwd alone (the kernels and the
folds, without the module's gathers and the embedding backward).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd import ops  # noqa: E402
from unicore_amd.modules import PairGaussianEmbed  # noqa: E402


def _time(fn, iters):
    for _ in range(3):
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
    K, H, T, B = 128, 64, 32, 32
    bf16 = torch.bfloat16
    for L in (128, 256):
        mask = torch.zeros(B, L, dtype=torch.bool, device="cuda")
        mask[::2, L - 5:] = True
        coords = 2 * torch.randn(B, L, 3, device="cuda")
        tokens = torch.randint(0, T, (B, L), device="cuda")
        grad = torch.randn(B, H, L, L, device="cuda").to(bf16)
        m = PairGaussianEmbed(K, H, T).cuda().to(bf16)

        def fwd():
            with torch.no_grad():
                m(coords, tokens, mask)

        def fwd_bwd():
            m.zero_grad(set_to_none=True)
            m(coords, tokens, mask).backward(grad)

        res = {"eager": [], "fused": []}
        for _ in range(a.rounds):
            for col, gate in (("eager", "0"), ("fused", "1")):
                os.environ["UNICORE_PAIR_GAUSS_H64"] = gate
                res[col].append((_time(fwd, 20), _time(fwd_bwd, 10)))
        (ef, eb), (ff, fb) = res["eager"][-1], res["fused"][-1]
        print(
            f"pair_gauss bf16 B={B} L={L} K={K} H={H}: fwd eager {ef:8.1f} us "
            f"fused {ff:7.1f} us (fused {ef / ff:5.2f}x eager) | fwd+bwd eager "
            f"{eb:8.1f} us fused {fb:7.1f} us (fused {eb / fb:5.2f}x eager)"
        )
        for col in ("eager", "fused"):
            print(f"  {col} rounds, fwd / fwd+bwd us: " + ", ".join(
                f"{f:.1f} / {b:.1f}" for f, b in res[col]))

        t = tokens.unsqueeze(2) * T + tokens.unsqueeze(1)
        av = m.mul.weight.detach()[t].view(B, L, L).float()
        bv = m.bias.weight.detach()[t].view(B, L, L).float()
        w = (m.means.detach().float(), m.stds.detach().float(),
             m.linear1.weight.detach(), m.linear1.bias.detach(),
             m.linear2.weight.detach())
        b2, fill = m.linear2.bias.detach(), torch.finfo(bf16).min
        kf = _time(lambda: ops.pair_gauss_fwd(coords, av, bv, mask, *w, b2, fill), 20)
        kb = _time(lambda: ops.pair_gauss_bwd(grad, coords, av, bv, mask, *w), 20)
        flop = 2 * B * L * L * (K * K + K * H)
        print(
            f"  kernels alone: fwd {kf:7.1f} us ({flop / kf / 1e6:6.1f} TFLOP/s "
            f"of the MLP's products) | bwd (dx + wgrad + folds) {kb:7.1f} us"
        )


if __name__ == "__main__":
    main()
