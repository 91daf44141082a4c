#!/usr/bin/env python3
"""Time the Evoformer's attention sites with the head-dim-32 fused attention
(UNICORE_EVO_ATTN=1) against the bmm -> softmax_dropout -> bmm chain (=0).

bf16, B=1, dropout 0.1, training mode; msa depth 128, d_msa 256 / 8 heads,
d_pair 128 / 4 heads; residues L in {128, 256, 384}.  Sites: triangle
attention (starting and ending node), MSA row attention with pair bias, MSA
column attention.  Forward alone and forward+backward, one line per config.
Same process, same box: the two columns are directly comparable.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd.models.evoformer import (  # noqa: E402
    MSAColumnAttention,
    MSARowAttentionWithPairBias,
)
from unicore_amd.modules import TriangleAttention  # noqa: E402

GATE = "UNICORE_EVO_ATTN"
S, D_MSA, H_MSA, D_PAIR, H_PAIR, P = 128, 256, 8, 128, 4, 0.1


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


def _site(name, L):
    def rnd(*shape):
        return torch.randn(*shape, device="cuda").bfloat16().requires_grad_()

    if name == "msa_row":
        return MSARowAttentionWithPairBias(D_MSA, D_PAIR, H_MSA, P), [
            rnd(1, S, L, D_MSA), rnd(1, L, L, D_PAIR)]
    if name == "msa_col":
        return MSAColumnAttention(D_MSA, H_MSA, P), [rnd(1, S, L, D_MSA)]
    return TriangleAttention(D_PAIR, H_PAIR, P, starting=name == "tri_start"), [
        rnd(1, L, L, D_PAIR)]


def bench(name, L):
    torch.manual_seed(0)
    mod, args = _site(name, L)
    mod = mod.cuda().to(torch.bfloat16).train()
    d_out = torch.randn_like(args[0]).detach()

    def fwd():
        with torch.no_grad():
            mod(*args)

    def fwd_bwd():
        for a in args:
            a.grad = None
        mod.zero_grad(set_to_none=True)
        mod(*args).backward(d_out)

    # off, on, off, on: each figure is the smaller of its two rounds
    res = {"0": [1e30, 1e30], "1": [1e30, 1e30]}
    for gate in ("0", "1", "0", "1"):
        os.environ[GATE] = gate
        res[gate][0] = min(res[gate][0], _time(fwd, 30))
        res[gate][1] = min(res[gate][1], _time(fwd_bwd, 20))
    (cf, cb), (ff, fb) = res["0"], res["1"]
    print(
        f"evo_attn {name:<9} L={L} S={S}: fwd chain {cf:8.1f} us fused {ff:8.1f} us "
        f"({cf / ff:5.2f}x) | fwd+bwd chain {cb:8.1f} us fused {fb:8.1f} us "
        f"({cb / fb:5.2f}x)", flush=True
    )


def main():
    for L in (128, 256, 384):
        for name in ("tri_start", "tri_end", "msa_row", "msa_col"):
            bench(name, L)


if __name__ == "__main__":
    main()
