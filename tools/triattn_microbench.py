#!/usr/bin/env python3
"""Time modules.TriangleAttention with the HIP layout moves
(UNICORE_TRIATTN_FUSED=1) against the permute chain (=0), and the four
layout entries alone against their permute expressions.

bf16, B=1, d_pair 128, H=4, L in {128, 256, 384}, starting and ending node;
forward alone and forward+backward, dropout 0.1, training mode. One line per
config. Same process, same box: the two columns are directly comparable.
GB/s of the entries counts bytes read + bytes written.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd import ops  # noqa: E402
from unicore_amd.modules import TriangleAttention  # noqa: E402

GATE = "UNICORE_TRIATTN_FUSED"


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


def bench_module(L, starting, d_pair=128, heads=4):
    torch.manual_seed(0)
    mod = TriangleAttention(d_pair, heads, 0.1, starting=starting)
    mod = mod.cuda().to(torch.bfloat16).train()
    pair = torch.randn(1, L, L, d_pair, device="cuda").bfloat16().requires_grad_()
    d_out = torch.randn(1, L, L, d_pair, device="cuda").bfloat16()
    res = {}
    for gate in ("0", "1"):
        os.environ[GATE] = gate

        def fwd():
            with torch.no_grad():
                mod(pair)

        def fwd_bwd():
            pair.grad = None
            mod.zero_grad(set_to_none=True)
            mod(pair).backward(d_out)

        res[gate] = (_time(fwd, 30), _time(fwd_bwd, 20))
    (pf, pb), (ff, fb) = res["0"], res["1"]
    node = "starting" if starting else "ending  "
    print(
        f"triattn {node} L={L} d_pair={d_pair} H={heads}: fwd permute {pf:8.1f} us "
        f"fused {ff:8.1f} us ({pf / ff:5.2f}x) | fwd+bwd permute {pb:8.1f} us "
        f"fused {fb:8.1f} us ({pb / fb:5.2f}x)"
    )


def bench_entries(L, transpose, d_pair=128, heads=4):
    B, H, C = 1, heads, d_pair
    D = C // H
    R = T = L
    q = torch.randn(B, L, L, 3 * C, device="cuda").bfloat16().chunk(3, -1)[1]
    o = torch.randn(B * H * R, T, D, device="cuda").bfloat16()
    lin = torch.randn(B, L, L, H, device="cuda").bfloat16()
    d_bias = torch.randn(B, H, L, L, device="cuda").bfloat16()
    p5 = (0, 3, 2, 1, 4) if transpose else (0, 3, 1, 2, 4)
    m5 = (0, 3, 2, 1, 4) if transpose else (0, 2, 3, 1, 4)
    pb = (0, 3, 2, 1) if transpose else (0, 3, 1, 2)
    mb = (0, 3, 2, 1) if transpose else (0, 2, 3, 1)
    cases = [
        ("pair_arrange", q.numel(),
         lambda: q.unflatten(-1, (H, D)).permute(*p5).contiguous(),
         lambda: ops.pair_arrange(q, H, transpose)),
        ("pair_merge", o.numel(),
         lambda: o.view(B, H, R, T, D).permute(*m5).reshape(B, L, L, C),
         lambda: ops.pair_merge(o, B, L, L, H, transpose)),
        ("pair_bias_arrange", lin.numel(),
         lambda: lin.permute(*pb).contiguous(),
         lambda: ops.pair_bias_arrange(lin, transpose)),
        ("pair_bias_arrange_bwd", d_bias.numel(),
         lambda: d_bias.permute(*mb).contiguous(),
         lambda: ops.pair_bias_arrange_bwd(d_bias, transpose)),
    ]
    for name, numel, eager, fused in cases:
        assert torch.equal(eager(), fused())
        te, tf = _time(eager, 50), _time(fused, 50)
        gbs = 2 * numel * 2 / tf / 1e3
        print(
            f"{name:<22} L={L} transpose={int(transpose)}: permute {te:7.1f} us "
            f"fused {tf:7.1f} us ({te / tf:5.2f}x, {gbs:6.0f} GB/s)"
        )


def main():
    for L in (128, 256, 384):
        for starting in (True, False):
            bench_module(L, starting)
    for L in (128, 256, 384):
        for transpose in (False, True):
            bench_entries(L, transpose)


if __name__ == "__main__":
    main()
