"""Pairwise distance head on the pair track (Uni-Mol's DistanceHead).

    x_ij[h]  = pair[b,h,i,j]; 0 where i or j is padded
    g_ij     = gelu(dense(x_ij))                  (exact erf GELU)
    f_ij     = out_proj(layer_norm(g_ij))
    dist_ij  = 0.5 * (f_ij + f_ji); 0 where i or j is padded

``pair`` is the last layer's attention logits, head-major (B, H, L, L); padded
keys carry ``finfo.min``. The output is (B, L, L) fp32 and symmetric.

On GPU at 64 heads with L % 8 == 0 this is two HIP kernels forward and four
plus the column fold backward (the fp32-MFMA kernels of
csrc/pair_dist_h64.hip, gate ``UNICORE_PAIR_DIST_H64``): the eager chain's
permute to channel-last, its Linear, GELU, LayerNorm and Linear over B*L*L
rows never exist. The eager function below is the definition, the CPU path,
the path for head counts and lengths the kernels do not serve, and what
``UNICORE_PAIR_COORD_EAGER=1`` (the "run the pair heads eager" A/B switch,
which covers this head as well as the coordinate head) selects.
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F


# default of the UNICORE_PAIR_DIST_H64 gate (64 heads, L % 8 == 0; anything
# else runs eager): on. Same-box figures (profiles/mol_dist_head_h64.txt):
# forward+backward of the module at B 32 is 3786 -> 419 us at L 128 and
# 13099 -> 1397 us at L 256, against a spread of 3.2 / 14.5 us between the
# repeated eager rounds.
_PAIR_DIST_H64_DEFAULT = "1"


def pair_dist_eager(pair, dense_weight, dense_bias, ln_weight, ln_bias,
                    out_weight, out_bias, padding_mask=None, eps=1e-5):
    """The definition above in fp32 (fp64 when ``pair`` is fp64)."""
    ct = torch.float64 if pair.dtype == torch.float64 else torch.float32
    B, H, L, _ = pair.shape
    if padding_mask is None:
        real = torch.ones(B, L, dtype=torch.bool, device=pair.device)
    else:
        real = ~padding_mask.to(torch.bool)
    valid = real.unsqueeze(2) & real.unsqueeze(1)  # (B, L, L)
    x = pair.to(ct).permute(0, 2, 3, 1)  # (B, L, L, H)
    # pads hold finfo.min: zero them before the MLP, not after
    x = x.masked_fill(~valid.unsqueeze(-1), 0.0)
    g = F.gelu(F.linear(x, dense_weight.to(ct), dense_bias.to(ct)))
    n = F.layer_norm(g, (H,), ln_weight.to(ct), ln_bias.to(ct), eps)
    f = F.linear(n, out_weight.to(ct).view(1, H), out_bias.to(ct)).squeeze(-1)
    return (0.5 * (f + f.transpose(1, 2))).masked_fill(~valid, 0.0)


class _PairDist(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pair, pad, w1, b1, gamma, beta, w2, b2, eps):
        from unicore_amd import ops

        out = ops.pair_dist_fwd(pair, pad, w1, b1, gamma, beta, w2, b2, eps)
        ctx.save_for_backward(pair, w1, b1, gamma, beta, w2, b2)
        ctx.pad = pad
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, grad):
        from unicore_amd import ops

        pair, w1, b1, gamma, beta, w2, b2 = ctx.saved_tensors
        dpair, dw1, db1, dgamma, dbeta, dw2, db2 = ops.pair_dist_bwd(
            grad.float().contiguous(), pair, ctx.pad, w1, b1, gamma, beta, w2,
            b2, ctx.eps,
        )
        return dpair, None, dw1, db1, dgamma, dbeta, dw2, db2, None


def pair_dist_fused_ok(pair):
    """True if this input takes the HIP kernels."""
    if os.environ.get("UNICORE_PAIR_COORD_EAGER", "0") == "1":  # A/B benchmarking
        return False
    if not pair.is_cuda:
        return False
    if os.environ.get("UNICORE_PAIR_DIST_H64", _PAIR_DIST_H64_DEFAULT) != "1":
        return False
    if not pair.is_contiguous() or pair.data_ptr() % 16 != 0:
        return False
    from unicore_amd import ops

    return ops.pair_dist_supported(pair.size(1), pair.dtype, pair.size(2))


def pair_dist(pair, dense_weight, dense_bias, ln_weight, ln_bias, out_weight,
              out_bias, padding_mask=None, eps=1e-5):
    """pair (B, H, L, L); padding_mask (B, L) bool, True = pad. Returns the
    (B, L, L) distance prediction, fp32."""
    if not pair_dist_fused_ok(pair):
        return pair_dist_eager(pair, dense_weight, dense_bias, ln_weight,
                               ln_bias, out_weight, out_bias, padding_mask, eps)
    pad = None
    if padding_mask is not None:
        pad = padding_mask.to(torch.bool).contiguous()
    # .float() keeps the parameter math fp32 under a bf16-cast module
    # (grads flow back through the casts)
    return _PairDist.apply(
        pair, pad, dense_weight.float(), dense_bias.float(),
        ln_weight.float(), ln_bias.float(), out_weight.float().view(-1),
        out_bias.float(), eps,
    )


class PairDistHead(nn.Module):
    """Pair track -> pairwise distance prediction, fp32 (B, L, L)."""

    def __init__(self, heads):
        super().__init__()
        self.heads = heads
        self.dense = nn.Linear(heads, heads)
        self.layer_norm = nn.LayerNorm(heads)
        self.out_proj = nn.Linear(heads, 1)

    def forward(self, pair, padding_mask=None):
        return pair_dist(
            pair, self.dense.weight, self.dense.bias, self.layer_norm.weight,
            self.layer_norm.bias, self.out_proj.weight, self.out_proj.bias,
            padding_mask, self.layer_norm.eps,
        )
