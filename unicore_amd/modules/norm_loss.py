"""Uni-Mol's norm regularisers (``--x-norm-loss``,
``--delta-pair-repr-norm-loss``).

With ``C`` the reduced width, ``eps = 1e-10`` and ``tol = 1``:

    err(ss, C) = relu(|sqrt(ss + eps) - sqrt(C)| - tol)

    x_norm(x (B,L,E), padding_mask)
        = mean_b [ sum_i m_i err(sum_e x_bie^2, E) / (1e-10 + sum_i m_i) ]

    pair_norm(pair, bias (B,H,L,L), padding_mask)
        delta = pair - bias, in fp32
        e_bij = err(sum_h delta_bhij^2, H)
        = mean_b [ sum_ij m_i m_j e_bij / (1e-10 + sum_ij m_i m_j) ]

``m = ~padding_mask``. A padded position is removed by a select, not by a
multiply: it adds an exact 0 whatever the tensors hold there (``finfo.min``,
inf, NaN) and receives an exact 0 gradient. This is Uni-Mol's ``norm_loss``
and ``masked_mean``, with its "fill the -inf entries of the delta with 0"
step expressed as the select.

On GPU both run on the HIP kernels of csrc/pair_norm.hip (gate
``UNICORE_PAIR_NORM``): the pair term reads ``pair`` and ``bias`` once
forward and once backward and writes both gradients in one pass. The eager
functions below are the definition, the CPU path and the path for shapes and
dtypes the kernels do not serve.
"""

import math
import os

import torch
import torch.nn.functional as F

NORM_EPS = 1e-10
NORM_TOL = 1.0

# default of the UNICORE_PAIR_NORM gate: on. Same-box figures
# (profiles/mol_pair_norm.txt): forward+backward of pair_norm at B 32, 64
# heads is 657 -> 159 us at L 128 and 2317 -> 363 us at L 256, against a
# spread of 1.9 / 0.7 us between the repeated eager rounds.
_PAIR_NORM_DEFAULT = "1"


def _compute_dtype(t):
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def _real(padding_mask, B, L, device):
    if padding_mask is None:
        return torch.ones(B, L, dtype=torch.bool, device=device)
    return ~padding_mask.to(torch.bool)


def _err(ss, C):
    return F.relu((torch.sqrt(ss + NORM_EPS) - math.sqrt(C)).abs() - NORM_TOL)


def x_norm_eager(x, padding_mask=None):
    """The definition above in fp32 (fp64 when ``x`` is fp64)."""
    ct = _compute_dtype(x)
    B, L, E = x.shape
    real = _real(padding_mask, B, L, x.device)
    zero = torch.zeros((), dtype=ct, device=x.device)
    xs = torch.where(real.unsqueeze(-1), x.to(ct), zero)
    e = torch.where(real, _err(xs.pow(2).sum(-1), E), zero)
    return (e.sum(1) / (1e-10 + real.to(ct).sum(1))).mean()


def pair_norm_eager(pair, bias, padding_mask=None):
    """The definition above in fp32 (fp64 when ``pair`` is fp64)."""
    ct = _compute_dtype(pair)
    B, H, L, _ = pair.shape
    real = _real(padding_mask, B, L, pair.device)
    valid = real.unsqueeze(2) & real.unsqueeze(1)  # (B, L, L)
    zero = torch.zeros((), dtype=ct, device=pair.device)
    delta = torch.where(valid.unsqueeze(1), pair.to(ct) - bias.to(ct), zero)
    e = torch.where(valid, _err(delta.pow(2).sum(1), H), zero)
    n = real.to(ct).sum(1)
    return (e.sum((1, 2)) / (1e-10 + n * n)).mean()


def _count(pad, B, L, device):
    """Real atoms per sample, fp32 (B), without a host sync."""
    if pad is None:
        return torch.full((B,), float(L), device=device)
    return (~pad).sum(1).float()


class _RowNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pad):
        from unicore_amd import ops

        B, L, E = x.shape
        coef, err = ops.row_norm_fwd(
            x.view(B * L, E), None if pad is None else pad.view(-1)
        )
        n = _count(pad, B, L, x.device)
        # d loss / d err_bi, shared by the rows of a sample
        w = torch.reciprocal((1e-10 + n) * B)
        ctx.save_for_backward(x, coef, w)
        return (err.view(B, L).sum(1) * w).sum()

    @staticmethod
    def backward(ctx, grad):
        from unicore_amd import ops

        x, coef, w = ctx.saved_tensors
        B, L, E = x.shape
        g_row = (grad.float() * w).unsqueeze(1).expand(B, L).contiguous()
        dx = ops.row_norm_bwd(g_row.view(-1), coef, x.view(B * L, E))
        return dx.view(B, L, E), None


class _PairNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pair, bias, pad):
        from unicore_amd import ops

        B, L = pair.size(0), pair.size(3)
        coef, rowerr = ops.pair_norm_fwd(pair, bias, pad)
        n = _count(pad, B, L, pair.device)
        w = torch.reciprocal((1e-10 + n * n) * B)
        ctx.save_for_backward(pair, bias, coef, w)
        return (rowerr.sum(1) * w).sum()

    @staticmethod
    def backward(ctx, grad):
        from unicore_amd import ops

        pair, bias, coef, w = ctx.saved_tensors
        gscale = (grad.float() * w).contiguous()
        d_pair, d_bias = ops.pair_norm_bwd(gscale, coef, pair, bias)
        return d_pair, d_bias, None


def _gate_on(t):
    if not t.is_cuda:
        return False
    return os.environ.get("UNICORE_PAIR_NORM", _PAIR_NORM_DEFAULT) == "1"


def _dense16(t):
    return t.is_contiguous() and t.data_ptr() % 16 == 0


def x_norm_fused_ok(x):
    """True if this input takes the HIP row kernels."""
    if not _gate_on(x) or x.dim() != 3 or not _dense16(x):
        return False
    from unicore_amd import ops

    return ops.row_norm_supported(x.size(2), x.dtype)


def pair_norm_fused_ok(pair, bias):
    """True if these inputs take the HIP pair kernels."""
    if not _gate_on(pair) or pair.dim() != 4:
        return False
    if (bias.shape != pair.shape or bias.dtype != pair.dtype
            or bias.device != pair.device):
        return False
    if not _dense16(pair) or not _dense16(bias):
        return False
    from unicore_amd import ops

    return ops.pair_norm_supported(pair.size(1), pair.dtype, pair.size(3))


def _pad(padding_mask):
    if padding_mask is None:
        return None
    return padding_mask.to(torch.bool).contiguous()


def x_norm(x, padding_mask=None):
    """x (B, L, E); padding_mask (B, L) bool, True = pad. Returns the fp32
    scalar regulariser on the per-atom norm."""
    if not x_norm_fused_ok(x):
        return x_norm_eager(x, padding_mask)
    return _RowNorm.apply(x, _pad(padding_mask))


def pair_norm(pair, bias, padding_mask=None):
    """pair, bias (B, H, L, L); padding_mask (B, L) bool, True = pad. Returns
    the fp32 scalar regulariser on the per-pair norm of ``pair - bias``."""
    if not pair_norm_fused_ok(pair, bias):
        return pair_norm_eager(pair, bias, padding_mask)
    return _PairNorm.apply(pair, bias, _pad(padding_mask))
