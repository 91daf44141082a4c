"""Uni-Mol's edge-typed gaussian pair embedding (GaussianLayer + NonLinearHead).

    d_ij   = |c_i - c_j|                      fp32, exactly 0 on the diagonal
    t_ij   = tokens_i * n_types + tokens_j
    x_ij   = mul[t_ij] * d_ij + bias[t_ij]    fp32
    s_k    = |stds_k| + 1e-5
    g_ijk  = exp(-0.5 ((x_ij - means_k) / s_k)^2) / (sqrt(2 * 3.14159) * s_k)
             fp32, then cast to the model dtype
    h_ij   = gelu(linear1(g_ij))              exact erf, model dtype
    o_ij   = linear2(h_ij)                    model dtype
    out[b, :, i, j] = o_ij; finfo(dtype).min where key j is padded

The output is the pair track's first state, head-major (B, H, L, L).
Coordinates get no gradient through the fused path: distances are data here,
as in Uni-Mol. With ``coords.requires_grad`` the eager path runs, and
differentiates whatever autograd differentiates.

On GPU at K = 128, H = 64, bf16 and L % 8 == 0 this is one HIP kernel forward
and two plus the column folds backward (the bf16-MFMA kernels of
csrc/pair_gauss_h64.hip, gate ``UNICORE_PAIR_GAUSS_H64``). The module gathers
the two per-edge-type terms as (B, L, L) fp32 tensors and the kernels take it
from there; the (B, L, L, K) features, pre-activations and hidden units never
exist, forward or backward. The eager function below is the definition, the CPU
path, the path for every other shape and dtype, and what
``UNICORE_GAUSSIAN_EAGER=1`` selects.
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F


# default of the UNICORE_PAIR_GAUSS_H64 gate (K = 128, H = 64, bf16, L % 8 ==
# 0; anything else runs eager): on. Same-job figures
# (profiles/mol_pair_gauss_h64.txt): forward+backward of the module at B 32 is
# 6048 -> 1108 us at L 128 and 19932 -> 3133 us at L 256, against a spread of
# 19.1 / 4.1 us between the repeated eager rounds.
_PAIR_GAUSS_H64_DEFAULT = "1"


def pair_gauss_eager_ab(coords, a, b, means, stds, w1, b1, w2, b2,
                        padding_mask=None):
    """The definition from x_ij = a_ij d_ij + b_ij on: a and b (B, L, L) are
    the gathered per-edge-type terms. The gaussian math runs in fp32 (fp64
    when the Linear weights are fp64), the MLP in the dtype of the weights."""
    dtype = w1.dtype
    ct = torch.float64 if dtype == torch.float64 else torch.float32
    B, L = a.shape[:2]
    c = coords.to(ct)
    diff = c.unsqueeze(2) - c.unsqueeze(1)
    eye = torch.eye(L, device=c.device, dtype=ct)
    d = (diff.pow(2).sum(-1) + eye).sqrt() - eye  # (B, L, L)
    x = (a.to(ct) * d + b.to(ct)).unsqueeze(-1)
    s = stds.to(ct).abs() + 1e-5
    g = torch.exp(-0.5 * ((x - means.to(ct)) / s) ** 2) / ((2 * 3.14159) ** 0.5 * s)
    h = F.gelu(F.linear(g.to(dtype), w1, b1))
    out = F.linear(h, w2, b2).permute(0, 3, 1, 2).contiguous()
    if padding_mask is not None:
        out = out.masked_fill(
            padding_mask.to(torch.bool).view(B, 1, 1, L), torch.finfo(dtype).min
        )
    return out


def pair_gauss_eager(coords, tokens, n_types, means, stds, mul_weight,
                     bias_weight, w1, b1, w2, b2, padding_mask=None):
    """The definition above."""
    B, L = tokens.shape
    t = tokens.unsqueeze(2) * n_types + tokens.unsqueeze(1)
    a = F.embedding(t, mul_weight).view(B, L, L)
    b = F.embedding(t, bias_weight).view(B, L, L)
    return pair_gauss_eager_ab(coords, a, b, means, stds, w1, b1, w2, b2,
                               padding_mask)


class _PairGauss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, coords, pad, means, stds, w1, b1, w2, b2, fill):
        from unicore_amd import ops

        out = ops.pair_gauss_fwd(coords, a, b, pad, means, stds, w1, b1, w2,
                                 b2, fill)
        ctx.save_for_backward(a, b, coords, means, stds, w1, b1, w2)
        ctx.pad = pad
        return out

    @staticmethod
    def backward(ctx, grad):
        from unicore_amd import ops

        a, b, coords, means, stds, w1, b1, w2 = ctx.saved_tensors
        d_a, d_b, d_means, d_stds, dw1, db1, dw2, db2 = ops.pair_gauss_bwd(
            grad.contiguous(), coords, a, b, ctx.pad, means, stds, w1, b1, w2
        )
        return (d_a, d_b, None, None, d_means, d_stds, dw1.to(w1.dtype),
                db1.to(w1.dtype), dw2.to(w1.dtype), db2.to(w1.dtype), None)


def pair_gauss_fused_ok(coords, n_kernels, heads, dtype):
    """True if this input takes the HIP kernels."""
    if os.environ.get("UNICORE_GAUSSIAN_EAGER", "0") == "1":  # A/B benchmarking
        return False
    if not coords.is_cuda or coords.requires_grad:
        return False
    if os.environ.get("UNICORE_PAIR_GAUSS_H64", _PAIR_GAUSS_H64_DEFAULT) != "1":
        return False
    from unicore_amd import ops

    return ops.pair_gauss_supported(n_kernels, heads, dtype, coords.size(1))


class PairGaussianEmbed(nn.Module):
    """coords (B, L, 3), tokens (B, L) -> pair embedding (B, heads, L, L)."""

    def __init__(self, n_kernels=128, heads=64, n_types=1):
        super().__init__()
        self.n_kernels = n_kernels
        self.heads = heads
        self.n_types = n_types
        self.means = nn.Parameter(torch.empty(n_kernels).uniform_(0, 3))
        self.stds = nn.Parameter(torch.empty(n_kernels).uniform_(0, 3))
        self.mul = nn.Embedding(n_types * n_types, 1)
        self.bias = nn.Embedding(n_types * n_types, 1)
        self.linear1 = nn.Linear(n_kernels, n_kernels)
        self.linear2 = nn.Linear(n_kernels, heads)
        # Uni-Mol's start: the plain distance. Kept through a model's
        # init_bert_params pass.
        self.mul.can_global_init = False
        self.bias.can_global_init = False
        nn.init.constant_(self.mul.weight, 1.0)
        nn.init.constant_(self.bias.weight, 0.0)

    def forward(self, coords, tokens, padding_mask=None):
        dtype = self.linear1.weight.dtype
        w = (self.linear1.weight, self.linear1.bias, self.linear2.weight,
             self.linear2.bias)
        if not pair_gauss_fused_ok(coords, self.n_kernels, self.heads, dtype):
            return pair_gauss_eager(
                coords, tokens, self.n_types, self.means, self.stds,
                self.mul.weight, self.bias.weight, *w, padding_mask,
            )
        B, L = tokens.shape
        t = tokens.unsqueeze(2) * self.n_types + tokens.unsqueeze(1)
        # the scatter by edge type in the backward is torch's embedding
        # backward, as for the token embedding
        a = F.embedding(t, self.mul.weight).view(B, L, L).float()
        b = F.embedding(t, self.bias.weight).view(B, L, L).float()
        pad = None
        if padding_mask is not None:
            pad = padding_mask.to(torch.bool).contiguous()
        args = (a, b, coords.float().contiguous(), pad, self.means.float(),
                self.stds.float(), *w)
        if not all(x.is_contiguous() and x.data_ptr() % 16 == 0
                   for x in args if x is not None and x is not pad):
            return pair_gauss_eager(
                coords, tokens, self.n_types, self.means, self.stds,
                self.mul.weight, self.bias.weight, *w, padding_mask,
            )
        return _PairGauss.apply(*args, torch.finfo(dtype).min)
