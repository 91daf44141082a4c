"""float64 references and error bounds for the cross-entropy and GELU-dropout
kernels (`csrc/cross_entropy.hip`, `csrc/gelu_dropout.hip`).

Shared by `test_ce_gelu_kernels.py` (CPU: validates what is in here) and
`test_ce_gelu_kernels_gpu.py` (the HIP kernels against it). Plain helpers, no
fixtures. The bounds are derived in the docstring of the GPU test file; the
functions here are that derivation written out.
"""

import math

import torch

from _optim_reference import U32, agreement_interval, ulp  # noqa: F401

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16

# Accuracy of the device intrinsics on gfx950. ASSUMED, not measured and not
# found in the ROCm documentation installed with the toolchain: `v_exp_f32`
# (2**x) and `v_log_f32` (log2 x) good to 1 ulp of their result, `erff` to 4.
# The ulp of a log2 result is taken at no less than 1.0: the assumption read
# conservatively for sums close to 1, where log2 is close to 0.
EXP2_ULPS = 1.0
LOG2_ULPS = 1.0
ERF_ULPS = 4.0
# Not assumed: fp32(log2 e) and fp32(1/sqrt 2) are 0.23u and 0.29u (relative)
# off their real values, and the product with them rounds once.
EXP_ARG = 1.25  # __expf(x) = v_exp_f32(x * log2e): argument error, units of u*|x|
ERF_ARG = 1.3  # erff(x * 0.70710678f): argument error, units of u*|z|
# A subnormal intermediate or result may be flushed to zero.
TINY = 2.0**-126

GELU_D1_MAX = 1.13  # max |gelu'|  (at x = sqrt 2)
GELU_D2_MAX = 0.80  # max |gelu''| (= 2 phi(0))


def min_spacing(dtype):
    """Spacing of the subnormals of `dtype`."""
    return {F32: 2.0**-149, F16: 2.0**-24, BF16: 2.0**-133}[dtype]


def round_half_ulp(ref, arith, dtype):
    """Bound on the rounding of a result within `arith` of `ref`: the last
    fp32 operation rounds it to fp32, a 2-byte output once more. Half a
    spacing each, at the largest magnitude the value can have.

    Every bound below is the sum of an arithmetic part and this rounding
    part, and returns the two apart with `parts=True`. A correct result uses
    up the rounding part entirely now and then; the margin of a factor 2
    that the CPU tests ask of plain fp32 arithmetic is asked of the
    arithmetic part."""
    mag = ref.abs() + arith
    r = 0.5 * torch.maximum(ulp(mag, F32), torch.full_like(ref, min_spacing(F32)))
    if dtype != F32:
        r = r + 0.5 * torch.maximum(ulp(mag + r, dtype),
                                    torch.full_like(ref, min_spacing(dtype)))
    return r


def _out(arith, rounding, parts):
    return (arith, rounding) if parts else arith + rounding


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------


def ce_per_thread(V, vec8):
    """Most elements one of the 256 threads of a row's block folds into its
    online state: whole 8-vectors every 2048 columns plus the ragged tail
    (vector kernel), every 256th column (scalar kernel)."""
    if vec8:
        return 8 * -(-(V // 8) // 256) + (1 if V % 8 else 0)
    return -(-V // 256)


def ce_ref(logits, target, ignore_index=-100):
    """Per-row `loss`, `lse` and `dx` per unit `grad_scale`, float64, from
    the values the kernel reads. Rows whose target is `ignore_index` or
    outside `[0, V)` have loss 0 and a zero `dx` row; their `lse` is the
    row's all the same. Also returns `live`, the mask of the other rows."""
    x = logits.detach().double().cpu()
    t = target.detach().cpu()
    N, V = x.shape
    live = (t != ignore_index) & (t >= 0) & (t < V)
    tc = torch.where(live, t, torch.zeros_like(t))
    lse = torch.logsumexp(x, dim=1)
    x_t = x.gather(1, tc.unsqueeze(1)).squeeze(1)
    loss = torch.where(live, lse - x_t, torch.zeros_like(lse))
    p = torch.exp(x - lse.unsqueeze(1))
    # exp(-inf - lse) is 0 whatever lse is, also where the row's lse is +inf
    # and torch gives nan for -inf - -inf only
    p = torch.where(x == -math.inf, torch.zeros_like(p), p)
    dx = p.clone()
    rows = torch.arange(N)
    dx[rows, tc] -= 1.0
    dx = torch.where(live.unsqueeze(1), dx, torch.zeros_like(dx))
    return dict(loss=loss, lse=lse, dx=dx, live=live, p=p, x=x, x_t=x_t)


def ce_fwd_bounds(ref, vec8, parts=False):
    """(bound on lse, bound on loss), per row, for finite rows.

    The online sum: every term reaches the result as a product of
    `exp(a_k)`, all `a_k <= 0`, telescoping to `x_i - max`; there are at most
    `T + 9` of them (`T` = `ce_per_thread`, six shuffle steps, three block
    combines), each with a rounded difference, a product and an addition on
    top of `__expf`'s own error. Relative error of the sum `s`:
    `u * (sum_i p_i * (1 + EXP_ARG) * |x_i - max| + (2 * EXP2_ULPS + 3) * (T + 9))`.
    `lse = max + __logf(s)`: the error of `s` passes through the logarithm
    unchanged in absolute terms; `__logf` is `v_log_f32(s) * ln 2` (the
    instruction's ulps at `max(|log2 s|, 1)`, the constant and the product:
    `2u * |log s|`), and the sum rounds once more: half an fp32 ulp of lse.
    `loss = lse - x_t` rounds once more: the rounding part of the loss is
    half an ulp of lse plus half an ulp of the loss."""
    x, p, lse = ref["x"], ref["p"], ref["lse"]
    V = x.shape[1]
    T = ce_per_thread(V, vec8)
    mx = x.max(dim=1).values
    d = torch.where(p > 0, (x - mx.unsqueeze(1)).abs(), torch.zeros_like(x))
    spread = (p * d).sum(dim=1)
    e_s = U32 * ((1 + EXP_ARG) * spread + (2 * EXP2_ULPS + 3) * (T + 9))
    log_s = lse - mx
    e_log = U32 * (2 * LOG2_ULPS * math.log(2.0)
                   * torch.clamp(log_s / math.log(2.0), min=1.0)
                   + 2 * log_s)
    arith = e_s + e_log
    r_lse = round_half_ulp(lse, arith, F32)
    live = ref["live"]
    zero = torch.zeros_like(arith)
    r_loss = r_lse + round_half_ulp(ref["loss"], arith + r_lse, F32)
    return (_out(arith, r_lse, parts),
            _out(torch.where(live, arith, zero), torch.where(live, r_loss, zero),
                 parts))


def ce_bwd_bounds(ref, g, dtype, parts=False):
    """Elementwise bound on `dx = g * (exp(x_i - l) - [i == t])`, where `l`
    is the float64 lse rounded to fp32 (half an fp32 ulp of lse, at most
    `u * |lse|`, relative in `p_i`).
    The difference rounds (`u * |d_i|`), `__expf` adds
    `(EXP_ARG * |d_i| + 2 * EXP2_ULPS) * u`, the product with `g` one `u`
    (arithmetic in the target column, which then subtracts `g`; elsewhere it
    is the last fp32 rounding, counted in the rounding part: `u` to spare).
    Zero rows (ignored targets) are exact."""
    x, p, lse = ref["x"], ref["p"], ref["lse"].unsqueeze(1)
    d = torch.where(p > 0, (x - lse).abs(), torch.zeros_like(x))
    rel = ((1 + EXP_ARG) * d + 2 * EXP2_ULPS + 1) * U32
    dx_ref = g * ref["dx"]
    arith = abs(g) * (p * rel + TINY)
    # the rounding of lse to fp32 is one rounding of a handed-over value:
    # with the output's, the part of the bound that carries no margin
    r_lse = abs(g) * p * 0.5 * ulp(lse.abs(), F32)
    live = ref["live"].unsqueeze(1)
    zero = torch.zeros_like(arith)
    return _out(torch.where(live, arith, zero),
                torch.where(live, r_lse + round_half_ulp(dx_ref, arith + r_lse, dtype),
                            zero),
                parts)


# ---------------------------------------------------------------------------
# GELU + dropout
# ---------------------------------------------------------------------------

_SQRT1_2 = 0.70710678118654752440
_INV_SQRT_2PI = 0.39894228040143267794


def _erf_phi(xb):
    return torch.special.erf(xb * _SQRT1_2), _INV_SQRT_2PI * torch.exp(-0.5 * xb * xb)


def gelu_ref(x, bias=None):
    """(gelu(x + bias), gelu'(x + bias), x + bias), float64, erf form:
    `0.5 * x * (1 + erf(x / sqrt 2))` and `Phi(x) + x * phi(x)`. `bias`
    broadcasts over the last dimension."""
    xb = x.detach().double().cpu()
    if bias is not None:
        xb = xb + bias.detach().double().cpu()
    erf, phi = _erf_phi(xb)
    return 0.5 * xb * (1.0 + erf), 0.5 * (1.0 + erf) + xb * phi, xb


def _one_plus_erf_err(xb):
    """Absolute error of the fp32 `1 + erff(x * 0.70710678f)`: `ERF_ULPS`
    ulps of erf (an ulp is at most `2u * |erf|`), the argument's error
    `ERF_ARG * u * |z|` through `erf' = 2/sqrt(pi) * exp(-z**2)`, the sum's
    rounding. Where `1 + erf` cancels (x << 0) this stays about
    `2 * ERF_ULPS * u`, absolute."""
    erf, _ = _erf_phi(xb)
    z = xb * _SQRT1_2
    return U32 * (2 * ERF_ULPS * erf.abs()
                  + ERF_ARG * z.abs() * 2 / math.sqrt(math.pi) * torch.exp(-z * z)
                  + (1.0 + erf).abs())


def gelu_fwd_bound(xb, y_ref, dtype, scale=1.0, has_bias=False, parts=False):
    """Bound on `out = gelu(x + bias) * scale` (`scale` = 1 / (1 - p) on kept
    elements): `0.5 * |x|` times the error of `1 + erf`; `2u` relative for the
    products of the GELU and, with dropout, `2u` for the rounded `scale` and
    its product; with a bias the rounded sum `x + bias` moves the result by
    at most `max|gelu'| * u * |x + bias|`; half an ulp of the output."""
    b32 = 0.5 * xb.abs() * _one_plus_erf_err(xb) + 2 * U32 * y_ref.abs() + TINY
    if has_bias:
        b32 = b32 + GELU_D1_MAX * U32 * xb.abs()
    ref = y_ref * scale
    b32 = b32 * scale + (2 * U32 * ref.abs() if scale != 1.0 else 0.0)
    return _out(b32, round_half_ulp(ref, b32, dtype), parts)


def gelu_bwd_bound32(xb, g, d_ref, scale=1.0, has_bias=False):
    """Bound on the fp32 `dx = (g * scale) * gelu'(x + bias)` before it is
    rounded to the output dtype (the value the bias-gradient sum takes).
    `gelu' = 0.5 * (1 + erf) + x * pdf`, `pdf = 0.3989..f * __expf(-0.5*x*x)`:
    the argument `a = -x*x/2` is off by `u * |a|`, `__expf` by
    `(EXP_ARG * |a| + 2 * EXP2_ULPS) * u`, the constant and two products by
    `2.3u`; the sum rounds once. `4u` relative for `scale`, `g * scale` and
    the final product."""
    a = 0.5 * xb * xb
    _, phi = _erf_phi(xb)
    e = (0.5 * _one_plus_erf_err(xb)
         + xb.abs() * phi * ((1 + EXP_ARG) * a + 2 * EXP2_ULPS + 2.3) * U32
         + U32 * d_ref.abs() + TINY)
    if has_bias:
        e = e + GELU_D2_MAX * U32 * xb.abs()
    gs = g.abs() * scale
    return gs * e + 4 * U32 * gs * d_ref.abs()  # the last product included


def gelu_bwd_bound(xb, g, d_ref, dtype, scale=1.0, has_bias=False, parts=False):
    b32 = gelu_bwd_bound32(xb, g, d_ref, scale, has_bias)
    return _out(b32, round_half_ulp(g * scale * d_ref, b32, dtype), parts)


def colsum_grid(n8, C):
    """`colsum_grid` of `csrc/common.h`."""
    mult = C // math.gcd(2048, C)
    want = -(-n8 // 256)
    blocks = -(-want // mult) * mult
    cap = max((2048 // mult) * mult, mult)
    return min(blocks, cap)


def dbias_depth(n8, C):
    """Longest chain of fp32 additions between a term and its column's sum:
    a thread's grid-stride trips, the serialized LDS bands of the block fold
    (`ceil(2048 / C)`), then in `unicore_col_fold_kernel` a thread's partial
    rows, six shuffle steps and the four wave sums."""
    grid = colsum_grid(n8, C)
    trips = -(-n8 // (grid * 256))
    return trips + -(-2048 // C) + -(-grid // 256) + 6 + 4


def dbias_bound(terms_ref, terms_b32, n8, C):
    """Per column: the terms' own fp32 bounds (`gelu_bwd_bound32`, which
    counts their last rounding), plus `depth * u * sum |terms|` for the
    summation. `terms_*` are (rows, C)."""
    return terms_b32.sum(0) + dbias_depth(n8, C) * U32 * (
        terms_ref.abs() + terms_b32).sum(0)


# ---------------------------------------------------------------------------
# the dropout bitfield
# ---------------------------------------------------------------------------


def unpack_keep(dmask, n):
    """Bool (n,): bit `j` of byte `i` is element `8 * i + j`."""
    b = dmask.detach().cpu().reshape(-1).to(torch.int64)
    bits = (b.unsqueeze(1) >> torch.arange(8)) & 1
    assert bits.numel() == n, (bits.numel(), n)
    return bits.reshape(-1).bool()


def keep_probability(p):
    """Exact keep probability of `keep16_threshold`: a uniform 16-bit draw is
    kept when it is >= floor(p * 65536) (capped at 65535)."""
    return 1.0 - min(int(min(p, 0.999999) * 65536.0), 65535) / 65536.0


def binomial_interval(n, q, sigmas=6.0):
    """[lo, hi] for K ~ Binomial(n, q) at `sigmas` standard deviations
    (normal approximation: meant for n*q*(1-q) in the thousands or more; for
    q in {0, 1} the interval is the one possible value)."""
    half = sigmas * math.sqrt(n * q * (1 - q))
    return math.ceil(n * q - half), math.floor(n * q + half)


def bit_agreement_interval(n_pairs, q):
    """Interval for the number of equal pairs among `n_pairs` pairs of
    independent bits that are each 1 with probability `q`; for q = 1/2 this
    is `agreement_interval`."""
    if q == 0.5:
        return agreement_interval(n_pairs)
    return binomial_interval(n_pairs, q * q + (1 - q) * (1 - q))


# ---------------------------------------------------------------------------
# inputs of the GPU tests (built on the CPU, so the CPU tests can check the
# bounds against plain fp32 arithmetic at the very same values)
# ---------------------------------------------------------------------------

# the backward's grad_scale: a loss scale for fp16, whose smallest spacing
# (2**-24) is above most softmax entries of a 30k vocabulary; three
# significant bits so the product with it is not trivially exact
CE_GRAD_SCALE = {F32: 0.75, BF16: 0.75, F16: 12288.0}

CE_WIDTHS = (1, 7, 8, 24, 2047, 2048, 2049, 2056, 4096, 30523, 30528)


def ce_logits(N, V, dtype, scale, seed):
    """Uniform in [-scale, scale], rounded to `dtype`. Uniform, not normal:
    at scale 8 the softmax of normal logits spans 40 nats, twice what fp16
    holds, and most of an fp16 `dx` would be zero and untestable."""
    gen = torch.Generator().manual_seed(seed)
    x = (2 * torch.rand(N, V, generator=gen, dtype=torch.float64) - 1) * scale
    return x.to(dtype)


def ce_targets(N, V, seed):
    """Random targets, the first rows pinned to the columns where an index
    slip shows: 0, V - 1, a thread's last lane element (8 * tid + 7), the
    last vector's first and middle element."""
    gen = torch.Generator().manual_seed(seed + 1000)
    t = torch.randint(0, V, (N,), generator=gen, dtype=torch.int64)
    pinned = [0, V - 1, 7, 8 * 5 + 7, (V - 1) // 8 * 8, (V - 1) // 8 * 8 + 3]
    for r, c in enumerate(pinned[:N]):
        t[r] = min(max(c, 0), V - 1)
    return t


def gelu_eval_inputs(dtype):
    """A grid over [-12, 12], three quarters of it on [-4, 4] where the
    function bends (below -4.7 the reference is smaller than four times the
    bound, which there is absolute), plus 0.0, -0.0, the smallest normal and
    the largest magnitudes; padded with ones to a multiple of 8."""
    special = [0.0, -0.0, torch.finfo(dtype).tiny, -torch.finfo(dtype).tiny]
    if dtype == F32:
        special += [1e4, -1e4]
    if dtype == F16:
        special += [65504.0, -65504.0]
    x = torch.cat([
        torch.linspace(-12, 12, 1021, dtype=torch.float64),
        torch.linspace(-4, 4, 3067, dtype=torch.float64),
        torch.tensor(special, dtype=torch.float64),
    ])
    pad = -x.numel() % 8
    return torch.cat([x, torch.ones(pad, dtype=torch.float64)]).to(dtype)


def gelu_random(shape, dtype, seed, lo=0.1, hi=4.0):
    """Random sign, |x| uniform in [lo, hi] after rounding to `dtype`:
    gelu(x) != 0, so `out == 0` means dropped."""
    gen = torch.Generator().manual_seed(seed)
    mag = lo + (hi - lo) * torch.rand(shape, generator=gen, dtype=torch.float64)
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    x = (sign * mag).to(dtype)
    return torch.where(x.abs() < lo, torch.full_like(x, lo), x)


# ---------------------------------------------------------------------------
# plain fp32 evaluations of the kernels' formulas (torch, CPU): what the CPU
# tests hold against the bounds. Not references.
# ---------------------------------------------------------------------------


def ce_plain_fp32(logits, target, g, l32, dtype):
    x = logits.float()
    N, V = x.shape
    lse = torch.logsumexp(x, dim=1)
    live = (target >= 0) & (target < V)
    tc = torch.where(live, target, torch.zeros_like(target))
    loss = torch.where(live, lse - x.gather(1, tc.unsqueeze(1)).squeeze(1),
                       torch.zeros_like(lse))
    gr = torch.where(live, torch.tensor(g, dtype=F32), torch.tensor(0.0))
    dx = torch.exp(x - l32.unsqueeze(1)) * gr.unsqueeze(1)
    dx[torch.arange(N), tc] -= gr
    return loss, lse, dx.to(dtype)


def gelu_plain_fp32(x, bias, g, scale, dtype):
    """(out, dx, fp32 dx before the output rounding)."""
    xb = x.float() if bias is None else x.float() + bias.float()
    cdf = 0.5 * (1.0 + torch.erf(xb * torch.tensor(_SQRT1_2, dtype=F32)))
    out = xb * cdf * torch.tensor(scale, dtype=F32)
    pdf = torch.tensor(_INV_SQRT_2PI, dtype=F32) * torch.exp(-0.5 * xb * xb)
    dx = (g.float() * torch.tensor(scale, dtype=F32)) * (cdf + xb * pdf)
    return out.to(dtype), dx.to(dtype), dx
