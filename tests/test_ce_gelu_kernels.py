"""CPU checks of `tests/_ce_gelu_reference.py`, so that the GPU tests of the
cross-entropy and GELU-dropout kernels (`test_ce_gelu_kernels_gpu.py`) rest
on something checked: the float64 references against torch's own functions
and autograd, the bitfield unpacking against a hand-written pattern, the CPU
fallbacks of the two modules against the references, and every error bound
against a plain fp32 torch evaluation of the kernel's formula at the GPU
tests' inputs, which has to pass with a factor of 2 to spare."""

import math

import pytest
import torch
import torch.nn.functional as F

from _ce_gelu_reference import (
    BF16,
    CE_GRAD_SCALE,
    CE_WIDTHS,
    F16,
    F32,
    binomial_interval,
    bit_agreement_interval,
    ce_bwd_bounds,
    ce_fwd_bounds,
    ce_logits,
    ce_per_thread,
    ce_plain_fp32,
    ce_ref,
    ce_targets,
    colsum_grid,
    dbias_bound,
    dbias_depth,
    gelu_bwd_bound,
    gelu_bwd_bound32,
    gelu_eval_inputs,
    gelu_fwd_bound,
    gelu_plain_fp32,
    gelu_random,
    gelu_ref,
    keep_probability,
    unpack_keep,
)
from _optim_reference import agreement_interval

DTYPES = [F32, F16, BF16]
INF = math.inf


def _ce_special_rows():
    """Rows with -inf logits, an ignored and two out-of-range targets."""
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(7, 24, generator=gen, dtype=torch.float64) * 3
    x[0, 0] = -INF
    x[1, 8:16] = -INF
    x[2, :] = -INF
    x[2, 5] = 1.5  # every column but one
    x[3, 3] = -INF  # the target column
    t = torch.tensor([2, 20, 5, 3, -100, 24, -1])
    return x, t


def test_ce_ref_against_torch():
    x, t = _ce_special_rows()
    ref = ce_ref(x, t)
    xr = x.clone().requires_grad_()
    valid = torch.where(ref["live"], t, torch.full_like(t, -100))
    want = F.cross_entropy(xr, valid, reduction="none", ignore_index=-100)
    assert ref["live"].tolist() == [True, True, True, True, False, False, False]
    assert torch.allclose(ref["loss"], want.detach(), rtol=1e-13, atol=0)
    assert ref["loss"][3].item() == INF and want[3].item() == INF
    assert ref["loss"][2].item() == 0.0  # the one finite logit is the target
    assert (ref["loss"][4:] == 0).all() and (ref["dx"][4:] == 0).all()
    assert torch.allclose(ref["lse"], torch.logsumexp(x, 1), rtol=1e-14, atol=0)
    # dx by autograd, on the rows with a finite loss
    finite = torch.isfinite(want.detach())
    want[finite].sum().backward()
    assert torch.allclose(ref["dx"][finite], xr.grad[finite], rtol=1e-12,
                          atol=1e-15)
    assert (ref["dx"][:3][x[:3] == -INF] == 0).all()  # -inf off the target
    assert ref["dx"][3, 3].item() == -1.0  # softmax 0 minus onehot
    # a row of -inf only: non-finite, nothing more is asked
    allinf = ce_ref(torch.full((1, 8), -INF, dtype=torch.float64),
                    torch.tensor([1]))
    assert not math.isfinite(allinf["loss"].item())


def test_ce_per_thread_counts():
    assert ce_per_thread(7, False) == 1 and ce_per_thread(2049, False) == 9
    assert ce_per_thread(8, True) == 8 and ce_per_thread(2048, True) == 8
    assert ce_per_thread(2056, True) == 16 and ce_per_thread(30528, True) == 120


def test_gelu_ref_against_torch():
    x = gelu_eval_inputs(F32).double().requires_grad_()
    want = F.gelu(x)
    y, d, xb = gelu_ref(x)
    assert torch.equal(xb, x.detach())
    # both cancel in `1 + erf` far below zero: absolute in eps * |x| there
    assert ((y - want.detach()).abs() <= 1e-13 * y.abs() + 4e-16 * xb.abs()).all()
    want.sum().backward()
    assert torch.allclose(d, x.grad, rtol=1e-12, atol=1e-15)
    bias = torch.linspace(-1, 1, 8, dtype=torch.float64)
    yb, db, xbb = gelu_ref(x.detach().reshape(-1, 8), bias)
    assert torch.equal(xbb, x.detach().reshape(-1, 8) + bias)
    assert ((yb - F.gelu(xbb)).abs() <= 1e-13 * yb.abs() + 4e-16 * xbb.abs()).all()


def test_unpack_keep_bit_order():
    got = unpack_keep(torch.tensor([0x01, 0x80, 0xA5, 0x00], dtype=torch.uint8), 32)
    want = [1, 0, 0, 0, 0, 0, 0, 0,
            0, 0, 0, 0, 0, 0, 0, 1,
            1, 0, 1, 0, 0, 1, 0, 1,
            0, 0, 0, 0, 0, 0, 0, 0]
    assert got.tolist() == [bool(b) for b in want]
    with pytest.raises(AssertionError):
        unpack_keep(torch.zeros(4, dtype=torch.uint8), 24)


def test_intervals():
    assert keep_probability(0.3) == 1 - 19660 / 65536
    assert keep_probability(0.5) == 0.5
    assert keep_probability(1e-6) == 1.0 and keep_probability(1.0) == 1 / 65536
    assert binomial_interval(2**16, 1.0) == (2**16, 2**16)
    lo, hi = binomial_interval(2**16, 0.5)
    assert (lo, hi) == (2**15 - 768, 2**15 + 768)
    assert bit_agreement_interval(2**20, 0.5) == agreement_interval(2**20)
    lo, hi = bit_agreement_interval(2**15, 0.7)
    mid = 2**15 * 0.58
    assert lo < mid < hi and hi - lo < 2 * 6 * 0.5 * math.sqrt(2**15) + 1


def test_colsum_geometry():
    # mult 1, 3, 255, 3, 2 for the widths of the folded-bias test
    assert [c // math.gcd(2048, c) for c in (8, 24, 2040, 3072, 4096)] == [
        1, 3, 255, 3, 2]
    assert colsum_grid(10, 8) == 1 and colsum_grid(10**9, 8) == 2048
    assert colsum_grid(2060 * 255, 2040) == 2040  # the cap, a multiple of 255
    assert 2060 * 255 > colsum_grid(2060 * 255, 2040) * 256  # a second trip
    assert dbias_depth(2060 * 255, 2040) == 2 + 2 + 8 + 10
    assert dbias_depth(8, 8) == 1 + 256 + 1 + 10


# ---------------------------------------------------------------------------
# the CPU fallbacks of the modules
# ---------------------------------------------------------------------------


def test_fused_nll_loss_cpu_fallback():
    from unicore_amd.modules.cross_entropy import fused_nll_loss

    x = ce_logits(16, 31, F32, 4.0, seed=2).requires_grad_()
    t = ce_targets(16, 31, seed=2)
    t[3] = t[9] = -100
    ref = ce_ref(x, t)
    loss = fused_nll_loss(x, t)
    (loss * 0.5).backward()
    assert abs(loss.item() - ref["loss"].sum().item()) <= 1e-5 * 16
    assert (x.grad[3] == 0).all() and (x.grad[9] == 0).all()
    assert torch.allclose(x.grad.double(), 0.5 * ref["dx"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("with_bias", [False, True])
def test_gelu_dropout_cpu_fallback(with_bias):
    from unicore_amd.modules.gelu_dropout import gelu_dropout

    x = gelu_random((6, 24), F32, seed=3).requires_grad_()
    bias = torch.linspace(-1, 1, 24).requires_grad_() if with_bias else None
    g = gelu_random((6, 24), F32, seed=4, lo=0.5, hi=2.0)
    y_ref, d_ref, xb = gelu_ref(x, bias)
    out = gelu_dropout(x, 0.0, True, bias=bias)
    out.backward(g)
    gd = g.double()
    assert ((out.detach().double() - y_ref).abs()
            <= gelu_fwd_bound(xb, y_ref, F32, has_bias=with_bias)).all()
    assert ((x.grad.double() - gd * d_ref).abs()
            <= gelu_bwd_bound(xb, gd, d_ref, F32, has_bias=with_bias)).all()
    if with_bias:
        b32 = gelu_bwd_bound32(xb, gd, d_ref, has_bias=True)
        assert ((bias.grad.double() - (gd * d_ref).sum(0)).abs()
                <= dbias_bound(gd * d_ref, b32, 6 * 24 // 8, 24)).all()
    # eval mode ignores p
    assert torch.equal(gelu_dropout(x, 0.5, False, bias=bias), out)


# ---------------------------------------------------------------------------
# bounds against plain fp32 arithmetic: a factor of 2 to spare
# ---------------------------------------------------------------------------


def _spare(err, parts):
    """Largest `err / bound` over the elements, the bound's rounding part
    (`_ce_gelu_reference.round_half_ulp`) taken off the error first; 0 where
    error and bound are both 0."""
    bound, rounding = parts
    err = (err - rounding).clamp_min(0.0)
    ratio = torch.where(bound > 0, err / bound, (err > 0).double() * INF)
    return ratio.max().item()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1.0, 8.0])
@pytest.mark.parametrize("V", CE_WIDTHS)
def test_ce_bounds_hold_for_plain_fp32(dtype, scale, V):
    N = 16 if V < 30000 else 4  # same generator stream: the first rows
    x = ce_logits(16, V, dtype, scale, seed=V)[:N]
    t = ce_targets(16, V, seed=V)[:N]
    g = CE_GRAD_SCALE[dtype]
    ref = ce_ref(x, t)
    l32 = ref["lse"].float()
    loss, lse, dx = ce_plain_fp32(x, t, g, l32, dtype)
    for vec8 in ([False, True] if V % 8 == 0 else [False]):
        b_lse, b_loss = ce_fwd_bounds(ref, vec8, parts=True)
        assert _spare((lse.double() - ref["lse"]).abs(), b_lse) <= 0.5
        assert _spare((loss.double() - ref["loss"]).abs(), b_loss) <= 0.5
    b_dx = ce_bwd_bounds(ref, g, dtype)
    assert _spare((dx.double() - g * ref["dx"]).abs(),
                  ce_bwd_bounds(ref, g, dtype, parts=True)) <= 0.5
    # and the bound is far below what it guards (the GPU tests assert this
    # too, before they look at the kernel)
    off_target = ref["dx"] > 0
    big = (g * ref["dx"]).abs() > 4 * b_dx
    if V > 1:
        assert big[off_target].double().mean().item() >= 0.99


def test_ce_bounds_hold_for_extreme_rows():
    """Row offsets of +-1e4 and a spread of 200 inside a row, fp32."""
    x = ce_logits(6, 2056, F32, 4.0, seed=5).double()
    x[0] += 1e4
    x[1] -= 1e4
    x[2] *= 25.0
    x[3] = x[3] * 25.0 + 1e4
    x = x.float()
    t = ce_targets(6, 2056, seed=5)
    ref = ce_ref(x, t)
    loss, lse, dx = ce_plain_fp32(x, t, 0.75, ref["lse"].float(), F32)
    b_lse, b_loss = ce_fwd_bounds(ref, True, parts=True)
    assert torch.isfinite(ref["loss"]).all() and torch.isfinite(loss).all()
    assert _spare((lse.double() - ref["lse"]).abs(), b_lse) <= 0.5
    assert _spare((loss.double() - ref["loss"]).abs(), b_loss) <= 0.5
    assert _spare((dx.double() - 0.75 * ref["dx"]).abs(),
                  ce_bwd_bounds(ref, 0.75, F32, parts=True)) <= 0.5


@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_bounds_hold_for_plain_fp32_on_the_grid(dtype):
    x = gelu_eval_inputs(dtype)
    g = gelu_random(x.shape, dtype, seed=6, lo=0.5, hi=2.0)
    y_ref, d_ref, xb = gelu_ref(x)
    out, dx, _ = gelu_plain_fp32(x, None, g, 1.0, dtype)
    b_y = gelu_fwd_bound(xb, y_ref, dtype)
    b_d = gelu_bwd_bound(xb, g.double(), d_ref, dtype)
    assert _spare((out.double() - y_ref).abs(),
                  gelu_fwd_bound(xb, y_ref, dtype, parts=True)) <= 0.5
    assert _spare((dx.double() - g.double() * d_ref).abs(),
                  gelu_bwd_bound(xb, g.double(), d_ref, dtype, parts=True)) <= 0.5
    assert (y_ref.abs() > 4 * b_y).double().mean().item() >= 0.9
    assert ((g.double() * d_ref).abs() > 4 * b_d).double().mean().item() >= 0.9
    # the cancelling tail: the bound is absolute, about 2 * ERF_ULPS * u * |x| / 2
    tail = xb < -8
    assert (b_y[tail] > 2.0**-24 * xb[tail].abs()).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("C", [24, 2040])
def test_gelu_bias_bounds_hold_for_plain_fp32(dtype, p, C):
    rows = 40
    scale = float(torch.tensor(1.0 / (1.0 - p), dtype=F32)) if p else 1.0
    x = gelu_random((rows, C), dtype, seed=C)
    bias = gelu_random((C,), dtype, seed=C + 1, lo=0.05, hi=1.0)
    g = gelu_random((rows, C), dtype, seed=C + 2, lo=0.5, hi=2.0)
    y_ref, d_ref, xb = gelu_ref(x, bias)
    out, dx, dx32 = gelu_plain_fp32(x, bias, g, scale, dtype)
    gd = g.double()
    assert _spare((out.double() - y_ref * scale).abs(),
                  gelu_fwd_bound(xb, y_ref, dtype, scale, True, parts=True)) <= 0.5
    assert _spare((dx.double() - gd * scale * d_ref).abs(),
                  gelu_bwd_bound(xb, gd, d_ref, dtype, scale, True, parts=True)) <= 0.5
    terms = gd * scale * d_ref
    b32 = gelu_bwd_bound32(xb, gd, d_ref, scale, True)
    dbias = dx32.sum(0)  # fp32 sum of the unrounded terms, torch's order
    bound = dbias_bound(terms, b32, rows * C // 8, C)
    assert _spare((dbias.double() - terms.sum(0)).abs(),
                  (bound, torch.zeros_like(bound))) <= 0.5
