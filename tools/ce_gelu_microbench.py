#!/usr/bin/env python3
"""Time the cross-entropy and GELU-dropout kernels at the BERT bench's shapes.

bf16. Cross entropy at the masked-LM head's shape: 127 x 512 tokens, 15%
masked, padded to the 512-row bucket (10240 rows) times the synthetic
dictionary's 30528 types; `cross_entropy_fwd` and `cross_entropy_bwd` are one
kernel each (`ce_fwd_kernel`, `ce_bwd_kernel`), so the call time is the
kernel time. GELU-dropout at the FFN inner activation (127 x 512, 3072),
p = 0.1, with the folded bias.

`--kernels PATH` times another build of the extension (the parent commit's,
say) through the same Python: run the two alternately in one job on one box
and compare the medians.

  python tools/ce_gelu_microbench.py [--kernels PATH] [--tag NAME]
"""
import argparse
import importlib.util
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _load(path):
    if path is None:
        from unicore_amd import _kernels

        return _kernels
    spec = importlib.util.spec_from_file_location("_kernels", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _time(fn, iters=50, repeats=7):
    """Median over `repeats` windows of `iters` calls, us per call."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", default=None,
                    help="path of an extension build to time instead of the tree's")
    ap.add_argument("--tag", default="tree")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    k = _load(a.kernels)
    torch.manual_seed(0)

    N, V = 10240, 30528
    logits = (torch.randn(N, V, device="cuda") * 2).bfloat16()
    target = torch.randint(0, V, (N,), device="cuda")
    target[::7] = -100
    gs = torch.ones(1, device="cuda")
    loss, lse = k.cross_entropy_forward(logits, target, -100)
    nbytes = logits.numel() * 2
    med, lo, hi = _time(lambda: k.cross_entropy_forward(logits, target, -100))
    print(f"{a.tag} ce_fwd_kernel bf16 ({N}, {V}): {med:8.1f} us "
          f"[{lo:.1f}, {hi:.1f}] {nbytes / med / 1e3:7.1f} GB/s")
    med, lo, hi = _time(
        lambda: k.cross_entropy_backward(logits, target, lse, gs, -100))
    print(f"{a.tag} ce_bwd_kernel bf16 ({N}, {V}): {med:8.1f} us "
          f"[{lo:.1f}, {hi:.1f}] {2 * nbytes / med / 1e3:7.1f} GB/s")
    print(f"{a.tag} ce loss sum {loss.sum().item():.6f}")
    del logits

    rows, C, p = 127 * 512, 3072, 0.1
    x = torch.randn(rows, C, device="cuda").bfloat16()
    g = torch.randn(rows, C, device="cuda").bfloat16()
    bias = torch.randn(C, device="cuda").bfloat16()
    out, dmask = k.gelu_dropout_forward(x, bias, p, True)
    nbytes = x.numel() * 2
    med, lo, hi = _time(lambda: k.gelu_dropout_forward(x, bias, p, True))
    print(f"{a.tag} gelu_dropout fwd bf16 ({rows}, {C}) p={p} bias: {med:8.1f} us "
          f"[{lo:.1f}, {hi:.1f}] {2 * nbytes / med / 1e3:7.1f} GB/s")
    med, lo, hi = _time(lambda: k.gelu_dropout_backward(g, x, bias, dmask, p))
    print(f"{a.tag} gelu_dropout bwd bf16 ({rows}, {C}) p={p} bias: {med:8.1f} us "
          f"[{lo:.1f}, {hi:.1f}] {3 * nbytes / med / 1e3:7.1f} GB/s")


if __name__ == "__main__":
    main()
