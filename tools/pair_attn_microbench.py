#!/usr/bin/env python3
"""Time SelfMultiheadAttention(return_logits=True) with the fused pair-track
attention (UNICORE_PAIR_ATTN=1) against the bmm -> add -> softmax_dropout ->
bmm chain (=0).

bf16, B 32, H 8, E 512, dropout 0.1, training mode, L in {128, 256}; a padded
batch (finfo.min at the padded keys of the bias) and a gradient flowing into
both outputs.  Forward alone and forward+backward.  The gates alternate in one
process (0, 1, 0, 1); each figure is the smaller of its two rounds, and the
two gate-0 rounds give the spread a difference has to beat.  A second line
times the ops entries alone and prints the (B, H, L, L) traffic the kernels
must move, counted from shapes, and the rate it implies.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from unicore_amd.modules import SelfMultiheadAttention  # noqa: E402

GATE = "UNICORE_PAIR_ATTN"
B, H, E, P = 32, 8, 512, 0.1


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


def bench(L):
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
        os.environ[GATE] = gate
        rounds[gate].append((_time(fwd, 200), _time(fwd_bwd, 100)))
    (cf, cb), (ff, fb) = (tuple(map(min, zip(*rounds[g]))) for g in ("0", "1"))
    spread = abs(rounds["0"][0][1] - rounds["0"][1][1])
    print(
        f"pair_attn L={L}: fwd chain {cf:8.1f} us fused {ff:8.1f} us "
        f"({cf / ff:5.2f}x) | fwd+bwd chain {cb:8.1f} us fused {fb:8.1f} us "
        f"({cb / fb:5.2f}x), gate-0 rounds {rounds['0'][0][1]:.1f} / "
        f"{rounds['0'][1][1]:.1f} us (spread {spread:.1f} us))",
        flush=True
    )


def kernels_alone(L):
    """The ops entries without the module around them: the forward moves 2
    (B, H, L, L) tensors (bias in, logits out), the backward 5 (logits and
    d_logits in, dbias out in the dq kernel; logits and dbias in in dkv)."""
    from unicore_amd import ops

    q, k, v, d_o = (torch.randn(B * H, L, 64, device="cuda").bfloat16()
                    for _ in range(4))
    bias = torch.randn(B, H, L, L, device="cuda").bfloat16()
    d_logits = torch.randn_like(bias) * 0.05
    o, logits, lse, seed = ops.pair_attn_fwd(q, k, v, bias, P, True)
    tf = _time(lambda: ops.pair_attn_fwd(q, k, v, bias, P, True), 200)
    tb = _time(lambda: ops.pair_attn_bwd(d_o, d_logits, q, k, v, o, lse, logits,
                                         P, True, int(seed)), 200)
    big = B * H * L * L * 2
    print(
        f"pair_attn L={L} kernels alone: fwd {tf:7.1f} us, {2 * big / 1e6:.1f} MB "
        f"= {2 * big / tf / 1e3:.0f} GB/s | bwd (Di + dq + dkv) {tb:7.1f} us, "
        f"{5 * big / 1e6:.1f} MB = {5 * big / tb / 1e3:.0f} GB/s", flush=True
    )


def main():
    for L in (128, 256):
        bench(L)
        kernels_alone(L)


if __name__ == "__main__":
    main()
