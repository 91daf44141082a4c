#!/usr/bin/env python3
"""Time SelfMultiheadAttention(return_logits=True) with the fused pair-track
attention (UNICORE_PAIR_ATTN=1) against the bmm -> add -> softmax_dropout ->
bmm chain (=0).

bf16, B 32, H 8 (--heads 64: head dim 8, gate UNICORE_PAIR_ATTN_D8), E 512,
dropout 0.1, training mode, L in {128, 256}; a padded
batch (finfo.min at the padded keys of the bias) and a gradient flowing into
both outputs.  Forward alone and forward+backward.  The gates alternate in one
process (0, 1, 0, 1); each figure is the smaller of its two rounds, and the
two gate-0 rounds give the spread a difference has to beat.  A second line
times the ops entries alone and prints the (B, H, L, L) traffic the kernels
must move, counted from shapes, and the rate it implies.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd.modules import SelfMultiheadAttention  # noqa: E402

B, E, P = 32, 512, 0.1


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


def bench(L, H):
    # head dim 8 (--heads 64) has a gate of its own under UNICORE_PAIR_ATTN
    gate_name = "UNICORE_PAIR_ATTN_D8" if E // H == 8 else "UNICORE_PAIR_ATTN"
    os.environ["UNICORE_PAIR_ATTN"] = "1"
    torch.manual_seed(0)
    mod = SelfMultiheadAttention(E, H, dropout=P).cuda().to(torch.bfloat16).train()
    x = torch.randn(B, L, E, device="cuda").bfloat16().requires_grad_()
    bias = torch.randn(B, H, L, L, device="cuda").bfloat16()
    n_real = torch.randint(L // 2, L + 1, (B,)).tolist()
    for b, n in enumerate(n_real):
        bias[b, :, :, n:] = torch.finfo(torch.bfloat16).min
    bias.requires_grad_()
    d_out = torch.randn_like(x).detach()
    d_logits = (torch.randn_like(bias) * 0.05).detach()

    def fwd():
        with torch.no_grad():
            mod(x, attn_bias=bias, return_logits=True)

    def fwd_bwd():
        x.grad = bias.grad = None
        mod.zero_grad(set_to_none=True)
        out, logits = mod(x, attn_bias=bias, return_logits=True)
        torch.autograd.backward([out, logits], [d_out, d_logits])

    rounds = {"0": [], "1": []}
    for gate in ("0", "1", "0", "1"):
        os.environ[gate_name] = gate
        rounds[gate].append((_time(fwd, 200), _time(fwd_bwd, 100)))
    (cf, cb), (ff, fb) = (tuple(map(min, zip(*rounds[g]))) for g in ("0", "1"))
    spread = abs(rounds["0"][0][1] - rounds["0"][1][1])
    print(
        f"pair_attn{_tag(H)} L={L}: fwd chain {cf:8.1f} us fused {ff:8.1f} us "
        f"({cf / ff:5.2f}x) | fwd+bwd chain {cb:8.1f} us fused {fb:8.1f} us "
        f"({cb / fb:5.2f}x), gate-0 rounds {rounds['0'][0][1]:.1f} / "
        f"{rounds['0'][1][1]:.1f} us (spread {spread:.1f} us))",
        flush=True
    )


def _tag(H):
    return "" if H == 8 else f" H={H}"


def kernels_alone(L, H):
    """The ops entries without the module around them: the forward moves 2
    (B, H, L, L) tensors (bias in, logits out), the backward 5 (logits and
    d_logits in, dbias out in the dq kernel; logits and dbias in in dkv) at
    head dim 64 and 3 (one kernel) at head dim 8."""
    from unicore_amd import ops

    D = E // H
    passes, what = (3, "Di + one pass") if D == 8 else (5, "Di + dq + dkv")
    q, k, v, d_o = (torch.randn(B * H, L, D, device="cuda").bfloat16()
                    for _ in range(4))
    bias = torch.randn(B, H, L, L, device="cuda").bfloat16()
    d_logits = torch.randn_like(bias) * 0.05
    o, logits, lse, seed = ops.pair_attn_fwd(q, k, v, bias, P, True)
    tf = _time(lambda: ops.pair_attn_fwd(q, k, v, bias, P, True), 200)
    tb = _time(lambda: ops.pair_attn_bwd(d_o, d_logits, q, k, v, o, lse, logits,
                                         P, True, int(seed)), 200)
    big = B * H * L * L * 2
    print(
        f"pair_attn{_tag(H)} L={L} kernels alone: fwd {tf:7.1f} us, {2 * big / 1e6:.1f} MB "
        f"= {2 * big / tf / 1e3:.0f} GB/s | bwd ({what}) {tb:7.1f} us, "
        f"{passes * big / 1e6:.1f} MB = {passes * big / tb / 1e3:.0f} GB/s",
        flush=True
    )


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--heads", type=int, default=8, choices=(8, 64),
                    help="8: head dim 64; 64: head dim 8 (Uni-Mol's shape)")
    H = ap.parse_args().heads
    for L in (128, 256):
        bench(L, H)
        kernels_alone(L, H)


if __name__ == "__main__":
    main()
