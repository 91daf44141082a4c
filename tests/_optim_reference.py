"""float64 references and checkers for the optimizer-step kernels.

Shared by `test_optim_kernels.py` (CPU: validates what is in here) and
`test_optim_kernels_gpu.py` (the HIP kernels against it). Plain helpers, no
fixtures.
"""

import math

import numpy as np
import torch

U32 = 2.0**-24  # unit roundoff of fp32

# grid-stride geometry of `adam.hip` / `rounding.hip`: unicore_grid caps the
# grid at 2048 blocks of 256 threads, 4 elements per thread and trip
TRIP = 2048 * 256 * 4


# ---------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------


def _f32(x):
    """A Python float rounded through fp32, as a kernel argument is."""
    return float(np.float32(x))


def adam_hparams(lr, betas, eps, scale, step, bias_correction, wd):
    """The six numbers `fused_adam` hands its kernel, rounded as it rounds
    them: formed in double on the host, then cast to fp32."""
    step_size = lr
    if bias_correction:
        bc1 = 1.0 - betas[0] ** step
        bc2 = 1.0 - betas[1] ** step
        step_size = lr * math.sqrt(bc2) / bc1
    return dict(
        b1=_f32(betas[0]),
        b2=_f32(betas[1]),
        eps=_f32(eps),
        inv_scale=_f32(1.0 / scale),
        step_size=_f32(step_size),
        wdf=_f32(1.0 - lr * wd),
    )


def adam_ref(p, m, v, g, lr, betas, eps, scale, step, bias_correction, wd):
    """One AdamW step in float64 from the values the kernel reads.

    Returns `(p', m', v', mags)`. `mags` holds the magnitude sums the error
    bounds are relative to (all float64, same shape as `p`):
    `m_mag = |m*b1| + |grad*(1-b1)|`, `v_mag` likewise, `p_decay = |p*wdf|`,
    `p_step = |step_size*m'/(sqrt(v')+eps)|`.
    """
    h = adam_hparams(lr, betas, eps, scale, step, bias_correction, wd)
    p, m, v, g = (t.detach().double().cpu() for t in (p, m, v, g))
    grad = g * h["inv_scale"]
    m_a, m_b = m * h["b1"], grad * (1.0 - h["b1"])
    v_a, v_b = v * h["b2"], grad * grad * (1.0 - h["b2"])
    m1, v1 = m_a + m_b, v_a + v_b
    decay = p * h["wdf"]
    upd = h["step_size"] * m1 / (v1.sqrt() + h["eps"])
    mags = dict(
        m_mag=m_a.abs() + m_b.abs(),
        v_mag=v_a.abs() + v_b.abs(),
        p_decay=decay.abs(),
        p_step=upd.abs(),
    )
    return decay - upd, m1, v1, mags


def ulp(x, dtype):
    """Spacing of `dtype` at |x| (float64 tensor in the normal range)."""
    mant = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}[dtype]
    _, e = torch.frexp(x.abs())  # |x| = f * 2**e, f in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e - 1 - mant)


# ---------------------------------------------------------------------------
# L2 norm
# ---------------------------------------------------------------------------


def l2norm_ref(tensors):
    """sqrt(sum x^2) over a tensor list, float64, as a Python float."""
    total = 0.0
    for t in tensors:
        total += t.detach().double().pow(2).sum().item()
    return math.sqrt(total)


# ---------------------------------------------------------------------------
# Stochastic rounding
# ---------------------------------------------------------------------------

# low 16 bits (the part bf16 discards), one constant per class
SR_CLASSES = (0x0000, 0x0001, 0x4000, 0x8000, 0xC000, 0xFFFF)


def sr_classes(n_per_class, generator):
    """(6, n_per_class) fp32: row k has low 16 bits `SR_CLASSES[k]`, random
    sign, random 7-bit bf16 mantissa and a biased exponent in [64, 190]:
    normal, and far enough from 255 that a carry out of the mantissa stays
    finite."""
    shape = (len(SR_CLASSES), n_per_class)

    def r(hi):
        return torch.randint(0, hi, shape, generator=generator, dtype=torch.int64)

    sign, expo, mant = r(2), 64 + r(127), r(128)
    low = torch.tensor(SR_CLASSES, dtype=torch.int64).unsqueeze(1)
    bits = (sign << 31) | (expo << 23) | (mant << 16) | low
    bits = torch.where(bits >= 2**31, bits - 2**32, bits)  # as signed int32
    return bits.to(torch.int32).view(torch.float32)


def sr_interleave(x):
    """Flatten a (C, N) class-major tensor so that element `4*q + j` comes
    from class `(j - q) % C`: a thread of the kernel owns elements
    `4*q .. 4*q + 3` and spends word `j` of its Philox draw on the j-th, so
    every word position sees every class (`i % C` alone would pair a class
    with one parity of `j` when C is even). N must be a multiple of 4."""
    n_cls, n = x.shape
    assert n % 4 == 0
    i = torch.arange(n_cls * n)
    q, j = i // 4, i % 4
    cls = (j - q) % n_cls
    # each block of 4*C consecutive elements holds every class 4 times
    rank = (i // (4 * n_cls)) * 4 + j
    return x[cls, rank].contiguous()


def _binom_logpmf(n, p, k):
    return (
        math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)
        + k * math.log(p) + (n - k) * math.log1p(-p)
    )


def _small_p_interval(n, p, miss):
    """[lo, hi] for K ~ Binomial(n, p) with a small mean, from the exact
    tails: P(K < lo) <= miss/2 and P(K > hi) <= miss/2."""
    kmax = int(n * p + 40 * math.sqrt(n * p) + 60)  # pmf beyond is < 1e-100
    pmf = [math.exp(_binom_logpmf(n, p, k)) for k in range(min(kmax, n) + 1)]
    lo, acc = 0, 0.0
    while acc + pmf[lo] <= miss / 2:
        acc += pmf[lo]
        lo += 1
    hi, acc = len(pmf) - 1, 0.0
    while acc + pmf[hi] <= miss / 2:
        acc += pmf[hi]
        hi -= 1
    return lo, hi


def sr_interval(n, c):
    """Two-sided interval for the number of `n` elements with discarded bits
    `c` that round away from zero, K ~ Binomial(n, c / 65536).

    The middle classes use the normal interval `n*p +- 6*sigma` (two-sided
    normal tail 2e-9; at n*p*(1-p) >= 4.9e4 the binomial is that close to it).
    The two edge classes have mean 4 (resp. n - 4), where the normal interval
    is meaningless, and use exact binomial tails with total miss 1e-9."""
    p = c / 65536.0
    if c == 0:
        return 0, 0
    if n * min(p, 1 - p) < 1000:
        if p < 0.5:
            return _small_p_interval(n, p, 1e-9)
        lo, hi = _small_p_interval(n, 1 - p, 1e-9)
        return n - hi, n - lo
    half = 6.0 * math.sqrt(n * p * (1 - p))
    return math.ceil(n * p - half), math.floor(n * p + half)


def agreement_interval(n_pairs):
    """6-sigma interval for the number of agreeing pairs among `n_pairs`
    pairs of independent fair bits, Binomial(n_pairs, 1/2)."""
    half = 6.0 * math.sqrt(n_pairs) / 2
    return math.ceil(n_pairs / 2 - half), math.floor(n_pairs / 2 + half)


def _bits16(dst):
    return dst.detach().cpu().contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def sr_round_up(src, dst):
    """Bool tensor: `dst` is the truncation of `src` plus one."""
    bits = src.detach().cpu().contiguous().view(torch.int32).to(torch.int64)
    return _bits16(dst) == (((bits & 0xFFFFFFFF) >> 16) + 1)


def sr_check(src, dst):
    """Assert that bf16 `dst` is a stochastic rounding of fp32 `src`.

    - every `dst` is bitwise `bits >> 16` (truncation: toward zero, the
      format being sign-magnitude) or that plus one (away from zero);
    - Inf and NaN, and every finite value with discarded bits 0, come back as
      `bits >> 16` exactly;
    - for every other value `c` of the discarded bits that `src` holds, the
      number rounded away lies in `sr_interval(count, c)`. Meant for sources
      built by `sr_classes`: few distinct `c`, many elements each.
    """
    bits = src.detach().cpu().contiguous().view(torch.int32).to(torch.int64)
    bits = (bits & 0xFFFFFFFF).reshape(-1)
    got = _bits16(dst).reshape(-1)
    assert got.shape == bits.shape
    trunc = bits >> 16
    up = got == trunc + 1
    same = got == trunc
    bad = ~(up | same)
    assert not bad.any(), (
        f"{int(bad.sum())} outputs are neither the truncation nor one above"
    )
    finite = (bits & 0x7F800000) != 0x7F800000
    low = bits & 0xFFFF
    exact = ~finite | (low == 0)
    assert not (up & exact).any(), (
        f"{int((up & exact).sum())} non-finite or exactly representable "
        "values changed"
    )
    for c in torch.unique(low[finite]).tolist():
        if c == 0:
            continue
        sel = finite & (low == c)
        n, k = int(sel.sum()), int((up & sel).sum())
        lo, hi = sr_interval(n, c)
        assert lo <= k <= hi, (
            f"discarded bits {c:#06x}: {k} of {n} rounded away from zero, "
            f"expected {n * c / 65536:.1f}, allowed [{lo}, {hi}]"
        )
