"""SE(3)-equivariant coordinate head on the pair track (Uni-Mol style).

    d_ij[h]  = pair[b,h,i,j] - pair0[b,h,i,j]
    w_ij     = fc2(gelu(fc1(d_ij)))           (exact erf GELU)
    w_ij     = 0 where i or j is padded
    n_b      = max(#real atoms of b - 1, 1)
    update_i = (1/n_b) * sum_j (x_j - x_i) * w_ij

``pair`` is the last layer's attention logits, ``pair0`` the gaussian pair
bias that started the track, both head-major (B, H, L, L). The update is a
weighted sum of difference vectors, so it rotates with the input and ignores
translations.

On GPU this is one HIP kernel forward and two plus the column fold backward
(csrc/pair_coord.hip): the eager chain's permute to channel-last, its two
Linears and GELU over B*L*L rows and its (B, L, L, 3) product never exist.
The eager function below is the definition, the CPU path, the path for head
counts the kernel does not serve, and what ``UNICORE_PAIR_COORD_EAGER=1``
selects.
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F


def _real_atoms(B, L, padding_mask, device):
    if padding_mask is None:
        return torch.ones(B, L, dtype=torch.bool, device=device)
    return ~padding_mask.to(torch.bool)


def _inv_count(real, dtype):
    # 1 / max(#real - 1, 1) per sample, on the device (no host sync)
    return 1.0 / (real.sum(1) - 1).clamp(min=1).to(dtype)


def pair_coord_eager(pair, pair0, coords, fc1_weight, fc1_bias, fc2_weight,
                     fc2_bias, padding_mask=None):
    """The definition above in fp32 (fp64 when ``pair`` is fp64)."""
    ct = torch.float64 if pair.dtype == torch.float64 else torch.float32
    B, H, L, _ = pair.shape
    real = _real_atoms(B, L, padding_mask, pair.device)
    valid = real.unsqueeze(2) & real.unsqueeze(1)  # (B, L, L)
    d = (pair.to(ct) - pair0.to(ct)).permute(0, 2, 3, 1)  # (B, L, L, H)
    # pads hold finfo.min: zero them before the MLP, not after
    d = d.masked_fill(~valid.unsqueeze(-1), 0.0)
    h = F.linear(d, fc1_weight.to(ct), fc1_bias.to(ct))
    w = F.linear(F.gelu(h), fc2_weight.to(ct), fc2_bias.to(ct)).squeeze(-1)
    w = w.masked_fill(~valid, 0.0)
    x = coords.to(ct)
    diff = x.unsqueeze(1) - x.unsqueeze(2)  # [b, i, j] = x_j - x_i
    update = (diff * w.unsqueeze(-1)).sum(2)
    return _inv_count(real, ct).view(B, 1, 1) * update


class _PairCoord(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pair, pair0, coords, inv_n, pad, w1, b1, w2, b2):
        from unicore_amd import ops

        out = ops.pair_coord_fwd(pair, pair0, coords, inv_n, pad, w1, b1, w2, b2)
        ctx.save_for_backward(pair, pair0, coords, inv_n, w1, b1, w2, b2)
        ctx.pad = pad
        return out

    @staticmethod
    def backward(ctx, grad):
        from unicore_amd import ops

        pair, pair0, coords, inv_n, w1, b1, w2, b2 = ctx.saved_tensors
        dpair, dw1, db1, dw2, db2 = ops.pair_coord_bwd(
            grad.float().contiguous(), pair, pair0, coords, inv_n, ctx.pad,
            w1, b1, w2, b2,
        )
        dpair0 = -dpair if ctx.needs_input_grad[1] else None
        return dpair, dpair0, None, None, None, dw1, db1, dw2, db2


def pair_coord_fused_ok(pair):
    """True if this input takes the HIP kernels."""
    if os.environ.get("UNICORE_PAIR_COORD_EAGER", "0") == "1":  # A/B benchmarking
        return False
    if not pair.is_cuda:
        return False
    from unicore_amd import ops

    return ops.pair_coord_supported(pair.size(1), pair.dtype)


def pair_coord(pair, pair0, coords, fc1_weight, fc1_bias, fc2_weight,
               fc2_bias, padding_mask=None):
    """pair, pair0 (B, H, L, L); coords (B, L, 3); padding_mask (B, L) bool,
    True = pad. Returns the (B, L, 3) coordinate update, fp32."""
    if coords.requires_grad:
        raise RuntimeError(
            "pair_coord: coords takes no gradient (the update is used as a "
            "denoising prediction); detach it"
        )
    if not pair_coord_fused_ok(pair):
        return pair_coord_eager(pair, pair0, coords, fc1_weight, fc1_bias,
                                fc2_weight, fc2_bias, padding_mask)
    B, H, L, _ = pair.shape
    pad = None
    if padding_mask is not None:
        pad = padding_mask.to(torch.bool).contiguous()
    inv_n = _inv_count(_real_atoms(B, L, pad, pair.device), torch.float32)
    # .float() keeps the parameter math fp32 under a bf16-cast module
    # (grads flow back through the casts)
    return _PairCoord.apply(
        pair, pair0, coords.float(), inv_n, pad,
        fc1_weight.float(), fc1_bias.float(),
        fc2_weight.float().view(-1), fc2_bias.float(),
    )


class PairCoordHead(nn.Module):
    """Pair track -> per-atom coordinate update, fp32 (B, L, 3)."""

    def __init__(self, heads):
        super().__init__()
        self.heads = heads
        self.fc1 = nn.Linear(heads, heads)
        self.fc2 = nn.Linear(heads, 1)

    def forward(self, pair, pair0, coords, padding_mask=None):
        return pair_coord(
            pair, pair0, coords, self.fc1.weight, self.fc1.bias,
            self.fc2.weight, self.fc2.bias, padding_mask,
        )
