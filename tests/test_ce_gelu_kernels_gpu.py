"""The loss and the FFN's inner activation against float64 (MI355X):
`cross_entropy_fwd / _bwd` (`csrc/cross_entropy.hip`) and
`gelu_dropout_fwd / _bwd` (`csrc/gelu_dropout.hip`). References, bounds and
inputs come from `_ce_gelu_reference.py`, which `test_ce_gelu_kernels.py`
validates on the CPU, where a plain fp32 evaluation has to meet every bound
with a factor of 2 to spare.

Every tolerance is a rounding-error bound, `u = 2**-24`. The accuracy of the
device intrinsics is ASSUMED (`_ce_gelu_reference.EXP2_ULPS`, `LOG2_ULPS`,
`ERF_ULPS`: 1, 1 and 4 ulps): nobody has measured it on gfx950 and the
toolchain's documentation does not state it. `__expf(d)` is
`v_exp_f32(d * log2e)`: the rounded product and the rounded constant move the
result by `1.25u * |d|`, the instruction by 1 ulp (`2u`). A result that is
subnormal may be flushed: `2**-126` absolute everywhere.

Each bound is an arithmetic part plus a rounding part. The rounding part is
the single roundings of values that are stored or handed over (the returned
fp32 number, the 2-byte output, the lse given to the backward): half an ulp
each, which a correct kernel uses up now and then. The margin of 2 that the
CPU tests ask is on the arithmetic part.

Cross entropy, forward. A thread folds its `T` elements into an online
state `(m, s)`, 6 shuffle steps and 3 block combines merge the states. Every
term `exp(x_i - max)` reaches `s` as a product of at most `T + 9` factors
`exp(a_k)`, `a_k <= 0`, whose exponents telescope to `x_i - max`. Each factor
costs `__expf`'s error at a rounded difference, a product and an addition:
`s` is off by `u * (sum_i p_i * 2.25 * |x_i - max| + 5 * (T + 9))`,
relative. All terms are positive, so nothing cancels. `lse = max +
__logf(s)`: the error of `s` is absolute in the logarithm; `__logf` is
`v_log_f32(s) * ln 2`, one ulp of `max(|log2 s|, 1)` and `2u * |log s|`;
the sum rounds (half an ulp of lse, rounding part). `loss = lse - x_t` rounds
once more. Rows with an ignored or out-of-range target are exactly 0.

Cross entropy, backward, `dx_i = g * (exp(x_i - l) - [i == t])`, with `l` the
float64 lse rounded to fp32 so that the forward's error stays out:
`|g| * p_i * (2.25 * |x_i - lse| + 3) * u` arithmetic; half an ulp of lse
times `|g| * p_i`, half an fp32 ulp and half an output ulp of `dx` rounding.

GELU, `y = 0.5 * x * (1 + erff(x * 0.70710678f))`: `1 + erf` is off by
`2 * ERF_ULPS * u * |erf|` (erff), `1.3u * |z| * erf'(z)` (the rounded
argument) and `u * (1 + erf)` (the sum), all absolute. Far below zero
`1 + erf` cancels to a few `u` while its error stays `2 * ERF_ULPS * u`: THE
BOUND THERE IS ABSOLUTE, `0.5 * |x| * 2 * ERF_ULPS * u`, not relative to the
tiny result; the eval-mode grid keeps such points under 10% so that the
non-vacuity condition can hold. `2u * |y|` for the products, with dropout
`2u` more for `1 / (1 - p)` and its product, with a bias `max|gelu'| * u *
|x + bias|` for the rounded sum. The derivative `0.5 * (1 + erf) + x * pdf`
adds `|x| * pdf * (2.25 * x*x/2 + 4.3) * u` for `pdf = 0.3989..f *
__expf(-0.5 * x * x)` and `4u` for the products with `g` and the scale.

Bias gradient: the column sum of the unrounded fp32 `dx`. Any order of `k`
additions is within `k * u * sum |terms|`; `k` is the longest chain of the
kernel's geometry (`dbias_depth`), at most the row count.

Non-vacuity: each parity test first asserts on the reference that the values
it guards exceed 4x their bound (99% of the off-target `dx` of live rows; 90%
of GELU values and derivatives), so that a kernel that dropped the term
could not pass. fp16 cannot hold the softmax of a 30k vocabulary (entries of
3e-5 against a spacing of 6e-8): its `grad_scale` is a loss scale, 12288.
"""

import functools
import math

import numpy as np
import pytest
import torch

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
    ce_ref,
    ce_targets,
    colsum_grid,
    dbias_bound,
    gelu_bwd_bound,
    gelu_bwd_bound32,
    gelu_eval_inputs,
    gelu_fwd_bound,
    gelu_random,
    gelu_ref,
    keep_probability,
    unpack_keep,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)

DTYPES = [F32, F16, BF16]
INF = math.inf
GRID_UNITS = 2048 * 256  # units of 8 elements one grid-stride trip covers


def _kernels():
    from unicore_amd import ops

    assert ops.has_kernels(), "HIP extension must be built/loaded on a GPU box"
    return ops


def _view(t, off):
    """`t` as a contiguous view `off` elements into a larger device buffer."""
    flat = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
    out = flat[off : off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous()
    assert out.data_ptr() == flat.data_ptr() + off * t.element_size()
    return out


def _assert_within(name, got, ref, bound, where=None):
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    ok = err <= bound
    if where is not None:
        ok = ok | ~where
        err = torch.where(where, err, torch.zeros_like(err))
    worst = torch.where(ok, torch.zeros_like(err), err - bound).argmax().item()
    print(f"{name}: max err/bound "
          f"{torch.where(bound > 0, err / bound, torch.zeros_like(err)).max().item():.3f}")
    assert ok.all(), (
        f"{name}: |err| {err.reshape(-1)[worst].item():.3e} > bound "
        f"{bound.reshape(-1)[worst].item():.3e} at element {worst} (ref "
        f"{ref.reshape(-1)[worst].item():.6e}, got {got.reshape(-1)[worst].item():.6e}); "
        f"{int((~ok).sum())} of {ok.numel()} outside"
    )


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------


def _ce_vacuity(ref, g, b_dx):
    """Off-target |dx_ref| above 4x its bound on 99% of the live rows'
    entries: a backward without the softmax term cannot pass."""
    off_target = (ref["dx"] > 0) & ref["live"].unsqueeze(1)
    if off_target.any():
        big = (g * ref["dx"]).abs() > 4 * b_dx
        assert big[off_target].double().mean().item() >= 0.99


def _ce_run(x, t, g, ignore_index=-100, off=0, vacuity=True):
    """Forward and backward of the kernel on CPU tensors `x` (N, V) and `t`,
    against the reference. The backward gets the float64 lse rounded to
    fp32. Rows whose reference loss is not finite are the caller's to judge.
    Returns (ref, loss, lse, dx) with the results on the CPU."""
    ops = _kernels()
    dtype = x.dtype
    N, V = x.shape
    ref = ce_ref(x, t, ignore_index)
    esize = x.element_size()
    vec8 = V % 8 == 0 and (off * esize) % 16 == 0
    finite = torch.isfinite(ref["loss"]) & torch.isfinite(ref["lse"])
    b_lse, b_loss = ce_fwd_bounds(ref, vec8)
    b_dx = ce_bwd_bounds(ref, g, dtype)
    if vacuity:
        _ce_vacuity(ref, g, b_dx)

    xs = _view(x, off) if off else x.cuda()
    td = t.cuda()
    loss, lse = ops.cross_entropy_fwd(xs, td, ignore_index)
    assert loss.dtype == F32 and lse.dtype == F32
    assert loss.shape == (N,) and lse.shape == (N,)
    _assert_within("lse", lse, ref["lse"], b_lse, finite)
    _assert_within("loss", loss, ref["loss"], b_loss, finite)
    dead = ~ref["live"]
    assert (loss.cpu()[dead] == 0).all()

    l32 = ref["lse"].float().cuda()
    gs = torch.tensor([g], dtype=F32, device="cuda")
    dx = ops.cross_entropy_bwd(xs, td, l32, gs, ignore_index)
    assert dx.dtype == dtype and dx.shape == (N, V)
    rows = finite.unsqueeze(1).expand(N, V)
    _assert_within("dx", dx, g * ref["dx"], b_dx, rows)
    assert (dx.cpu()[dead & finite] == 0).all()
    torch.cuda.synchronize()
    return ref, loss.cpu(), lse.cpu(), dx.cpu()


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1.0, 8.0])
@pytest.mark.parametrize("V", CE_WIDTHS)
def test_ce_widths(dtype, scale, V):
    """Scalar kernel: fewer columns than threads (1, 7), several trips (2047,
    2049, 30523). Vector kernel: idle threads (8, 24), exactly one trip
    (2048), one trip and one thread's second (2056), two and fifteen trips
    (4096, 30528). Targets at column 0, V - 1, a thread's last lane element
    and in the last vector (`ce_targets`)."""
    x = ce_logits(16, V, dtype, scale, seed=V)
    t = ce_targets(16, V, seed=V)
    ref, loss, _, dx = _ce_run(x, t, CE_GRAD_SCALE[dtype])
    if V == 1:
        assert (loss == 0).all() and (dx == 0).all()


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [24, 31])
def test_ce_grid_stride(dtype, V):
    """2051 rows on 2048 blocks: blocks 0..2 take a second row and reuse
    their LDS partials. Rows 2048.. are 51 times wider than the rows the
    same blocks handled first, so a stale partial shows."""
    N = 2048 + 3
    x = ce_logits(N, V, F32, 0.1, seed=V).double()
    x = (x * (1 + 50 * (torch.arange(N) // 2048)).unsqueeze(1)).to(dtype)
    t = ce_targets(N, V, seed=V)
    ref, loss, lse, dx = _ce_run(x, t, CE_GRAD_SCALE[dtype])
    # the rows of the second trip one by one, and far from their first-trip
    # partners' values
    b_lse, b_loss = ce_fwd_bounds(ref, V % 8 == 0)
    for r in range(2048, N):
        assert abs(lse[r].item() - ref["lse"][r].item()) <= b_lse[r].item()
        assert abs(loss[r].item() - ref["loss"][r].item()) <= b_loss[r].item()
        assert abs(ref["lse"][r] - ref["lse"][r - 2048]).item() > 100 * b_lse[r].item()
        assert dx[r].abs().sum().item() > 0


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [24, 31])
def test_ce_ignored_and_out_of_range_targets(dtype, V):
    """Interior rows with target -100 (ignore_index), -1, V and V + 1000:
    loss and dx row exactly 0, lse still right, neighbours untouched."""
    x = ce_logits(16, V, dtype, 4.0, seed=V + 1)
    t = ce_targets(16, V, seed=V + 1)
    bad = {3: -100, 6: -1, 9: V, 12: V + 1000}
    for r, v in bad.items():
        t[r] = v
    ref, loss, lse, dx = _ce_run(x, t, CE_GRAD_SCALE[dtype])
    assert ref["live"].sum().item() == 12
    for r in bad:
        assert loss[r].item() == 0.0 and (dx[r] == 0).all()
        assert math.isfinite(lse[r].item())
    # the same rows with good targets give the same neighbours, bitwise
    t2 = ce_targets(16, V, seed=V + 1)
    _, loss2, lse2, dx2 = _ce_run(x, t2, CE_GRAD_SCALE[dtype])
    good = ref["live"]
    assert torch.equal(loss[good], loss2[good]) and torch.equal(lse, lse2)
    assert torch.equal(dx[good], dx2[good])
    # another ignore_index: that one is ignored, -100 is merely out of range
    t3 = t2.clone()
    t3[5] = 2
    _, loss3, _, dx3 = _ce_run(x, t3, CE_GRAD_SCALE[dtype], ignore_index=2)
    assert loss3[5].item() == 0.0 and (dx3[5] == 0).all()


@requires_gpu
@pytest.mark.parametrize("V", [1, 31, 2056])
def test_ce_extreme_logits_fp32(V):
    """Row offsets of +1e4 and -1e4, a spread of 200 inside a row, both at
    once: no overflow, and the bound holds with |lse| large. V = 1: loss and
    dx exactly 0 whatever the logit."""
    x = ce_logits(6, V, F32, 4.0, seed=5).double()
    x[0] += 1e4
    x[1] -= 1e4
    x[2] *= 25.0
    x[3] = x[3] * 25.0 + 1e4
    x = x.float()
    t = ce_targets(6, V, seed=5)
    ref, loss, lse, dx = _ce_run(x, t, 0.75, vacuity=False)
    assert torch.isfinite(loss).all() and torch.isfinite(dx).all()
    assert abs(lse[0].item()) > 9e3 and abs(lse[1].item()) > 9e3
    if V == 1:
        assert (loss == 0).all() and (dx == 0).all()
    else:
        assert (x[2].max() - x[2].min()).item() > 150


def _neg_inf_rows(V, dtype):
    """Rows with -inf logits where the online state meets them first; the
    targets sit on finite logits except in row 5."""
    x = ce_logits(8, V, dtype, 3.0, seed=V + 2)
    t = torch.full((8,), V - 2, dtype=torch.int64)
    x[0, 0] = -INF  # the first element thread 0 sees
    for tid in (1, 2):
        if 8 * tid < V - 2:
            x[1, 8 * tid] = -INF  # the first element of a thread's vector
    x[2, 8:16] = -INF  # thread 1's whole first vector
    x[3, :] = -INF
    x[3, V - 2] = 1.25  # every column but one
    x[4, :V - 2] = -INF  # finite only in the last two columns
    x[5, V - 2] = -INF  # the target column: +inf
    x[6, :] = -INF  # nothing finite: only "non-finite" is asked
    return x, t


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [24, 31, 2049, 2056])
def test_ce_neg_inf_logits(dtype, V):
    """A -inf logit adds nothing to the sum and gets dx == 0 exactly; the row
    stays finite (the bounds are those of the finite rows); a target on a
    -inf logit costs +inf, as in `F.cross_entropy`. Both kernels (24, 2056
    vector; 31, 2049 scalar)."""
    x, t = _neg_inf_rows(V, dtype)
    ref, loss, lse, dx = _ce_run(x, t, CE_GRAD_SCALE[dtype], vacuity=False)
    finite_rows = [0, 1, 2, 3, 4, 7]
    assert torch.isfinite(ref["loss"][finite_rows]).all()
    assert torch.isfinite(loss[finite_rows]).all(), loss
    assert torch.isfinite(lse[finite_rows + [5]]).all(), lse
    assert loss[3].item() == 0.0 and lse[3].item() == 1.25
    assert loss[5].item() == INF and ref["loss"][5].item() == INF
    assert not math.isfinite(loss[6].item())
    for r in finite_rows:
        assert (dx[r][x[r] == -INF] == 0).all()
        assert torch.isfinite(dx[r]).all()


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [24, 31, 2049, 2056])
@pytest.mark.parametrize("bad", [INF, math.nan], ids=["inf", "nan"])
def test_ce_non_finite_logits_reach_the_loss(dtype, V, bad):
    """+inf or NaN anywhere in a row (the only element a thread sees, the
    first and the last of a vector, the ragged tail) makes that row's loss
    non-finite: the loss scaler has nothing else to go by. The other rows
    stay within their bounds."""
    x = ce_logits(8, V, dtype, 3.0, seed=V + 3)
    t = ce_targets(8, V, seed=V + 3)
    places = {1: 0, 3: 8, 4: 15, 6: V - 1}
    for r, c in places.items():
        x[r, c] = bad
    ref, loss, lse, dx = _ce_run(x, t, CE_GRAD_SCALE[dtype], vacuity=False)
    for r in range(8):
        assert math.isfinite(loss[r].item()) == (r not in places), (r, loss)
        assert math.isfinite(ref["loss"][r].item()) == (r not in places)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [24, 2056])
def test_ce_misaligned_views(dtype, V):
    """`V % 8 == 0` but the logits start 1..3 (fp32) or 1..7 (2-byte)
    elements into a buffer: no 16-byte load may touch them, the host has to
    take the scalar kernel. Same bounds, and the aligned call's results
    within them."""
    x = ce_logits(16, V, dtype, 4.0, seed=V + 4)
    t = ce_targets(16, V, seed=V + 4)
    g = CE_GRAD_SCALE[dtype]
    ref, loss0, lse0, dx0 = _ce_run(x, t, g)
    b_lse, b_loss = ce_fwd_bounds(ref, False)
    b_dx = ce_bwd_bounds(ref, g, dtype)
    for off in range(1, 4 if dtype == F32 else 8):
        _, loss, lse, dx = _ce_run(x, t, g, off=off)
        assert ((loss.double() - loss0.double()).abs() <= 2 * b_loss).all()
        assert ((lse.double() - lse0.double()).abs() <= 2 * b_lse).all()
        assert ((dx.double() - dx0.double()).abs() <= 2 * b_dx).all()


@requires_gpu
def test_ce_entry_checks():
    """Refused on the host, before any launch, with the offending value."""
    ops = _kernels()
    x = ce_logits(16, 24, F32, 1.0, seed=1).cuda()
    t = ce_targets(16, 24, seed=1).cuda()
    lse = torch.zeros(16, device="cuda")
    gs = torch.ones(1, device="cuda")
    with pytest.raises(RuntimeError, match="target must be int64, got Int"):
        ops.cross_entropy_fwd(x, t.int(), -100)
    with pytest.raises(RuntimeError, match="target is on cpu"):
        ops.cross_entropy_fwd(x, t.cpu(), -100)
    with pytest.raises(RuntimeError, match="16 elements .*got 15"):
        ops.cross_entropy_fwd(x, t[:15], -100)
    with pytest.raises(RuntimeError, match="target must be int64, got Int"):
        ops.cross_entropy_bwd(x, t.int(), lse, gs, -100)
    with pytest.raises(RuntimeError, match="target is on cpu"):
        ops.cross_entropy_bwd(x, t.cpu(), lse, gs, -100)
    with pytest.raises(RuntimeError, match="lse must be contiguous with 16 .*got 15"):
        ops.cross_entropy_bwd(x, t, lse[:15], gs, -100)
    with pytest.raises(RuntimeError, match="lse must be contiguous with 16 .*got 17"):
        ops.cross_entropy_bwd(x, t, torch.zeros(17, device="cuda"), gs, -100)
    with pytest.raises(RuntimeError, match="lse must be fp32, got Double"):
        ops.cross_entropy_bwd(x, t, lse.double(), gs, -100)
    with pytest.raises(RuntimeError, match="lse is on cpu"):
        ops.cross_entropy_bwd(x, t, lse.cpu(), gs, -100)
    torch.cuda.synchronize()


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_nll_loss_autograd(dtype):
    """The shim: a transposed (non-contiguous) logits view, an ignored row,
    and a grad_scale that is not 1. The backward uses the kernel's own lse,
    so `dx` inherits the forward's bound times `|g| * p`."""
    _kernels()
    from unicore_amd.modules.cross_entropy import fused_nll_loss

    N, V = 16, 2056
    x = ce_logits(N, V, dtype, 4.0, seed=9)
    t = ce_targets(N, V, seed=9)
    t[7] = -100
    g = CE_GRAD_SCALE[dtype]
    ref = ce_ref(x, t)
    b_lse, b_loss = ce_fwd_bounds(ref, True)
    b_dx = ce_bwd_bounds(ref, g, dtype) + abs(g) * ref["p"] * b_lse.unsqueeze(1)
    _ce_vacuity(ref, g, b_dx)
    leaf = x.cuda().t().contiguous().requires_grad_()
    view = leaf.t()
    assert not view.is_contiguous() and view.shape == (N, V)
    loss = fused_nll_loss(view, t.cuda())
    (loss * g).backward()
    total = ref["loss"].sum().item()
    # fp32 sum of 16 positive terms: 15 additions
    tol = b_loss.sum().item() + 15 * 2.0**-24 * total
    assert abs(loss.item() - total) <= tol, (loss.item(), total, tol)
    _assert_within("dx", leaf.grad.t(), g * ref["dx"], b_dx)
    assert (leaf.grad.t()[7] == 0).all()


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [31, 2056])
def test_ce_double_run_is_bitwise(dtype, V):
    ops = _kernels()
    x = ce_logits(2051, V, dtype, 2.0, seed=V + 5).cuda()
    t = ce_targets(2051, V, seed=V + 5).cuda()
    gs = torch.tensor([CE_GRAD_SCALE[dtype]], device="cuda")
    a = ops.cross_entropy_fwd(x, t, -100)
    b = ops.cross_entropy_fwd(x, t, -100)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(ops.cross_entropy_bwd(x, t, a[1], gs, -100),
                       ops.cross_entropy_bwd(x, t, a[1], gs, -100))


# ---------------------------------------------------------------------------
# GELU + dropout
# ---------------------------------------------------------------------------


def _pinv(p):
    """`1 / (1 - p)` as the host hands it to the kernel: rounded to fp32."""
    return float(np.float32(1.0 / (1.0 - min(p, 0.999999))))


def _gelu_vacuity(y_ref, b_y, dx_ref, b_d):
    assert (y_ref.abs() > 4 * b_y).double().mean().item() >= 0.9
    assert (dx_ref.abs() > 4 * b_d).double().mean().item() >= 0.9


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["p0", "eval"])
def test_gelu_eval_grid(dtype, mode):
    """`p = 0`, and `is_training = False` with p = 0.5: no dropout, an empty
    dmask that the backward accepts. The grid of `gelu_eval_inputs`."""
    ops = _kernels()
    x = gelu_eval_inputs(dtype)
    g = gelu_random(x.shape, dtype, seed=6, lo=0.5, hi=2.0)
    y_ref, d_ref, xb = gelu_ref(x)
    gd = g.double()
    b_y = gelu_fwd_bound(xb, y_ref, dtype)
    b_d = gelu_bwd_bound(xb, gd, d_ref, dtype)
    _gelu_vacuity(y_ref, b_y, gd * d_ref, b_d)
    p, training = (0.0, True) if mode == "p0" else (0.5, False)
    out, dmask = ops.gelu_dropout_fwd(x.cuda(), p, training)
    assert dmask.numel() == 0 and dmask.dtype == torch.uint8
    assert out.dtype == dtype and out.shape == x.shape
    _assert_within("out", out, y_ref, b_y)
    dx, db = ops.gelu_dropout_bwd(g.cuda(), x.cuda(), dmask, p)
    assert db.numel() == 0
    _assert_within("dx", dx, gd * d_ref, b_d)
    zero = x == 0
    assert zero.sum().item() >= 2 and (out.cpu()[zero] == 0).all()
    torch.cuda.synchronize()


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_gelu_dropout_through_the_bitfield(dtype, p):
    """|x| >= 0.1, so gelu(x) != 0 and `out == 0` means dropped: exactly where
    the returned bit is 0. Kept elements are `gelu * 1/(1-p)` within the
    bound; backward is `g * bit * 1/(1-p) * gelu'`, exactly 0 where dropped.
    8 * 4099 elements: the last block is ragged."""
    ops = _kernels()
    n = 8 * 4099
    x = gelu_random((n,), dtype, seed=7)
    g = gelu_random((n,), dtype, seed=8, lo=0.5, hi=2.0)
    y_ref, d_ref, xb = gelu_ref(x)
    gd, s = g.double(), _pinv(p)
    b_y = gelu_fwd_bound(xb, y_ref, dtype, s)
    b_d = gelu_bwd_bound(xb, gd, d_ref, dtype, s)
    _gelu_vacuity(y_ref * s, b_y, gd * s * d_ref, b_d)
    torch.manual_seed(17)
    out, dmask = ops.gelu_dropout_fwd(x.cuda(), p, True)
    assert dmask.shape == (n // 8,) and dmask.dtype == torch.uint8
    keep = unpack_keep(dmask, n)
    assert torch.equal(out.cpu() != 0, keep)
    lo, hi = binomial_interval(n, keep_probability(p))
    assert lo <= int(keep.sum()) <= hi
    zero = torch.zeros_like(y_ref)
    _assert_within("out", out, torch.where(keep, y_ref * s, zero),
                   torch.where(keep, b_y, zero))
    dx, _ = ops.gelu_dropout_bwd(g.cuda(), x.cuda(), dmask, p)
    assert (dx.cpu()[~keep] == 0).all()
    _assert_within("dx", dx, torch.where(keep, gd * s * d_ref, zero),
                   torch.where(keep, b_d, zero))
    torch.cuda.synchronize()


@requires_gpu
def test_gelu_keep_rate_per_bit_position():
    """2**16 units: each of the eight bit positions keeps with probability
    `1 - floor(p * 65536) / 65536` (6 sigma). Below 2**-16 the threshold is
    0 and nothing is dropped."""
    ops = _kernels()
    n8 = 2**16
    x = gelu_random((n8 * 8,), BF16, seed=10).cuda()
    torch.manual_seed(23)
    for p in (0.3, 1e-6):
        out, dmask = ops.gelu_dropout_fwd(x, p, True)
        keep = unpack_keep(dmask, n8 * 8).reshape(n8, 8)
        lo, hi = binomial_interval(n8, keep_probability(p))
        for j in range(8):
            k = int(keep[:, j].sum())
            assert lo <= k <= hi, (p, j, k, lo, hi)
        if p < 2.0**-16:
            assert keep.all() and (out != 0).all()
        else:
            assert hi < n8


@requires_gpu
def test_gelu_masks_are_independent_and_seeded():
    """`2048 * 256 + 4096` units: the first 4096 threads make a second
    grid-stride trip. Their second byte against their first, and one call
    against the next, agree bit by bit at the rate of independent draws,
    `q**2 + (1 - q)**2`; the same seed repeats bytes and output bitwise. The
    second trip's values are checked against the reference as well."""
    ops = _kernels()
    p, dtype = 0.3, BF16
    n8 = GRID_UNITS + 4096
    x = gelu_random((n8 * 8,), dtype, seed=11)
    xd = x.cuda()
    torch.manual_seed(29)
    out1, m1 = ops.gelu_dropout_fwd(xd, p, True)
    out2, m2 = ops.gelu_dropout_fwd(xd, p, True)  # the offset has moved on
    torch.manual_seed(29)
    out3, m3 = ops.gelu_dropout_fwd(xd, p, True)
    assert torch.equal(m1, m3) and torch.equal(out1, out3)
    torch.manual_seed(30)
    assert not torch.equal(ops.gelu_dropout_fwd(xd, p, True)[1], m1)

    q = keep_probability(p)
    k1 = unpack_keep(m1, n8 * 8).reshape(n8, 8)
    k2 = unpack_keep(m2, n8 * 8).reshape(n8, 8)

    def agree(a, b, what):
        lo, hi = bit_agreement_interval(a.numel(), q)
        k = int((a == b).sum())
        assert lo <= k <= hi, (what, k, a.numel(), lo, hi)

    agree(k1[:4096], k1[GRID_UNITS:], "second trip")
    agree(k1, k2, "second call")
    agree(k1[:-1], k1[1:], "neighbouring units")
    for j in range(1, 8):
        agree(k1[:, 0], k1[:, j], f"bit 0 against bit {j}")

    tail = slice(GRID_UNITS * 8, n8 * 8)
    y_ref, _, xb = gelu_ref(x[tail])
    s = _pinv(p)
    keep = k1.reshape(-1)[tail]
    zero = torch.zeros_like(y_ref)
    assert torch.equal(out1.cpu()[tail] != 0, keep)
    _assert_within("second trip out", out1[tail],
                   torch.where(keep, y_ref * s, zero),
                   torch.where(keep, gelu_fwd_bound(xb, y_ref, dtype, s), zero))


def _bias_rows(C, second_trip):
    """Fewer units than one grid, or the fewest rows with
    `n8 > colsum_grid(n8, C) * 256` (a second grid-stride trip)."""
    if not second_trip:
        return 40
    rows = {8: 524289, 24: 174593, 2040: 2060, 3072: 1365, 4096: 1025}[C]
    n8 = rows * C // 8
    assert n8 > colsum_grid(n8, C) * 256
    if C != 2040:  # as small as the condition allows
        assert (rows - 1) * C // 8 <= colsum_grid((rows - 1) * C // 8, C) * 256
    return rows


@functools.lru_cache(maxsize=1)
def _bias_case(C, rows, dtype):
    x = gelu_random((rows, C), dtype, seed=C)
    bias = gelu_random((C,), dtype, seed=C + 1, lo=0.05, hi=1.0)
    g = gelu_random((rows, C), dtype, seed=C + 2, lo=0.5, hi=2.0)
    return x, bias, g, gelu_ref(x, bias)


@requires_gpu
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("second_trip", [False, True], ids=["one_trip", "two_trips"])
@pytest.mark.parametrize("C", [8, 24, 2040, 3072, 4096])
def test_gelu_folded_bias(C, second_trip, dtype, p):
    """`colsum_grid` multiples 1, 3, 255, 3, 2; C = 2040 has the most
    contributor bands that do not divide the block. `out`, `dx` and the fp32
    `dbias` against float64; `dbias` bitwise equal on a second run. On the
    second trip a thread must add the bias of the columns it latched on the
    first."""
    ops = _kernels()
    rows = _bias_rows(C, second_trip)
    x, bias, g, (y_ref, d_ref, xb) = _bias_case(C, rows, dtype)
    gd, s = g.double(), (_pinv(p) if p else 1.0)
    n = rows * C
    xd, bd, gdv = x.cuda(), bias.cuda(), g.cuda()
    torch.manual_seed(31)
    out, dmask = ops.gelu_dropout_fwd(xd, p, True, bias=bd)
    if p:
        keep = unpack_keep(dmask, n).reshape(rows, C)
        assert (out.cpu()[~keep] == 0).all()  # x + bias may be 0 where kept
    else:
        assert dmask.numel() == 0
        keep = torch.ones(rows, C, dtype=torch.bool)
    zero = torch.zeros_like(y_ref)
    b_y = torch.where(keep, gelu_fwd_bound(xb, y_ref, dtype, s, True), zero)
    terms = torch.where(keep, gd * s * d_ref, zero)
    b32 = torch.where(keep, gelu_bwd_bound32(xb, gd, d_ref, s, True), zero)
    b_d = torch.where(keep, gelu_bwd_bound(xb, gd, d_ref, dtype, s, True), zero)
    if not p:
        _gelu_vacuity(y_ref, b_y, terms, b_d)
    _assert_within("out", out, torch.where(keep, y_ref * s, zero), b_y)
    dx, db = ops.gelu_dropout_bwd(gdv, xd, dmask, p, bias=bd)
    assert db.dtype == F32 and db.shape == (C,)
    _assert_within("dx", dx, terms, b_d)
    b_db = dbias_bound(terms, b32, n // 8, C)
    _assert_within("dbias", db, terms.sum(0), b_db)
    dx2, db2 = ops.gelu_dropout_bwd(gdv, xd, dmask, p, bias=bd)
    assert torch.equal(db, db2) and torch.equal(dx, dx2)
    torch.cuda.synchronize()


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_bias", [False, True])
def test_gelu_module_autograd_and_alignment(dtype, with_bias):
    """The entries refuse a view one element into a buffer (and a ragged
    size, a grad of another shape, a mask of the wrong length); the module
    function gives the aligned call's result on the same view, forward and
    backward."""
    ops = _kernels()
    from unicore_amd.modules.gelu_dropout import gelu_dropout

    rows, C = 40, 24
    x = gelu_random((rows, C), dtype, seed=12)
    g = gelu_random((rows, C), dtype, seed=13, lo=0.5, hi=2.0)
    bias = gelu_random((C,), dtype, seed=14, lo=0.05, hi=1.0) if with_bias else None
    y_ref, d_ref, xb = gelu_ref(x, bias)
    gd = g.double()
    xv, gv = _view(x, 1), _view(g, 1)
    bd = bias.cuda() if with_bias else None
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="x must be 16-byte aligned"):
        ops.gelu_dropout_fwd(xv, 0.0, True, bias=bd)
    with pytest.raises(RuntimeError, match="x must be 16-byte aligned"):
        ops.gelu_dropout_bwd(g.cuda(), xv, empty, 0.0, bias=bd)
    with pytest.raises(RuntimeError, match="grad must be 16-byte aligned"):
        ops.gelu_dropout_bwd(gv, x.cuda(), empty, 0.0, bias=bd)
    if with_bias:
        with pytest.raises(RuntimeError, match="bias must be 16-byte aligned"):
            ops.gelu_dropout_fwd(x.cuda(), 0.0, True, bias=_view(bias, 1))
    with pytest.raises(RuntimeError, match="numel % 8 == 0, got 12"):
        ops.gelu_dropout_bwd(g.cuda()[0, :12], x.cuda()[0, :12], empty, 0.0)
    with pytest.raises(RuntimeError, match="grad must match x"):
        ops.gelu_dropout_bwd(g.cuda()[:39], x.cuda(), empty, 0.0, bias=bd)
    with pytest.raises(RuntimeError, match="grad must match x"):
        ops.gelu_dropout_bwd(g.cuda().float() if dtype != F32 else g.cuda().half(),
                             x.cuda(), empty, 0.0, bias=bd)
    with pytest.raises(RuntimeError, match="dmask must be empty or hold 120"):
        ops.gelu_dropout_bwd(g.cuda(), x.cuda(),
                             torch.zeros(119, dtype=torch.uint8, device="cuda"),
                             0.5, bias=bd)

    leaf = xv.detach().requires_grad_()
    bleaf = bd.clone().requires_grad_() if with_bias else None
    out = gelu_dropout(leaf, 0.0, True, bias=bleaf)
    out.backward(gv)
    _assert_within("out", out, y_ref, gelu_fwd_bound(xb, y_ref, dtype, 1.0, with_bias))
    _assert_within("dx", leaf.grad, gd * d_ref,
                   gelu_bwd_bound(xb, gd, d_ref, dtype, 1.0, with_bias))
    if with_bias:
        terms = gd * d_ref
        b32 = gelu_bwd_bound32(xb, gd, d_ref, 1.0, True)
        b_db = dbias_bound(terms, b32, rows * C // 8, C)
        if dtype != F32:  # the module rounds the fp32 sum to the bias dtype
            from _ce_gelu_reference import round_half_ulp

            b_db = b_db + round_half_ulp(terms.sum(0), b_db, dtype)
        _assert_within("dbias", bleaf.grad, terms.sum(0), b_db)
    torch.cuda.synchronize()
