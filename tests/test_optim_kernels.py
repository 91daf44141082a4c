"""CPU checks of `tests/_optim_reference.py`, so that the GPU tests of the
optimizer-step kernels (`test_optim_kernels_gpu.py`) rest on something
checked: the float64 AdamW reference against the eager oracle, and the
stochastic-rounding checker against one rounding it must accept and two it
must reject."""

import math

import numpy as np
import pytest
import torch

from _optim_reference import (
    SR_CLASSES,
    adam_ref,
    agreement_interval,
    l2norm_ref,
    sr_check,
    sr_classes,
    sr_interleave,
    sr_interval,
    ulp,
)


def test_adam_ref_reproduces_the_eager_oracle():
    """Five steps of `optim.adam.Adam` on float64 parameters (the eager
    oracle: `denom = sqrt(v) + eps`, where `torch.optim.AdamW` has
    `sqrt(v) / sqrt(bc2) + eps`) against five chained `adam_ref` calls, to
    1e-12 relative.

    `adam_ref` rounds six numbers through fp32. betas, eps and the scale are
    fp32 numbers here. `step_size` and `1 - lr*wd` are made fp32 numbers by
    choosing them first and solving for `lr` and `wd`, which change every
    step: the double expression then lands within 1e-15 of an fp32 number
    and the rounding is the identity to that precision."""
    from unicore_amd.optim.adam import Adam

    betas, eps, scale = (0.5, 0.75), 2.0**-20, 2.0
    gen = torch.Generator().manual_seed(3)
    n = 257
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    param = torch.nn.Parameter(p0.clone())
    opt = Adam([param], lr=1.0, betas=betas, eps=eps, weight_decay=1.0)

    p = p0.clone()
    m = torch.zeros(n, dtype=torch.float64)
    v = torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        step_size = (2 + step) * 2.0**-9  # an fp32 number
        bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
        lr = step_size * bc1 / math.sqrt(bc2)
        wd = step * 2.0**-8 / lr  # 1 - lr*wd = 1 - step/256
        g = torch.randn(n, generator=gen, dtype=torch.float64)

        for group in opt.param_groups:
            group["lr"], group["weight_decay"] = lr, wd
        param.grad = g / scale  # the oracle has no fused unscale; exact
        opt.step()

        p, m, v, _ = adam_ref(p, m, v, g, lr, betas, eps, scale, step, True, wd)
        state = opt.state[param]
        for got, ref in ((p, param.data), (m, state["exp_avg"]),
                         (v, state["exp_avg_sq"])):
            rel = ((got - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
            assert rel < 1e-12, (step, rel)
    assert (param.data - p0).abs().mean().item() > 1e-2  # it did move


def test_adam_ref_rounds_hyperparameters_like_the_kernel():
    one = torch.ones(1, dtype=torch.float64)
    zero = torch.zeros(1, dtype=torch.float64)
    p, m, v, mags = adam_ref(one, zero, zero, one, 1e-2, (0.9, 0.999), 1e-8,
                             3.0, 1, False, 0.1)
    inv = float(np.float32(1.0 / 3.0))
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    assert m.item() == inv * (1.0 - b1)
    assert v.item() == inv * inv * (1.0 - b2)
    assert abs((1.0 - b2) / 1e-3 - 1) > 1e-5  # the 3e-5 the contract is about
    upd = float(np.float32(1e-2)) * m.item() / (
        math.sqrt(v.item()) + float(np.float32(1e-8)))
    assert p.item() == float(np.float32(1.0 - 1e-3)) - upd
    assert mags["p_step"].item() == upd
    assert mags["p_decay"].item() == float(np.float32(1.0 - 1e-3))
    assert mags["m_mag"].item() == m.item() and mags["v_mag"].item() == v.item()


def test_ulp_and_l2norm_ref():
    x = torch.tensor([1.0, 1.5, 2.0, 2.0**-6, 0.03], dtype=torch.float64)
    assert ulp(x, torch.bfloat16).tolist() == [
        2.0**-7, 2.0**-7, 2.0**-6, 2.0**-13, 2.0**-13]
    assert ulp(x, torch.float16)[0].item() == 2.0**-10
    assert ulp(x, torch.float32)[0].item() == 2.0**-23
    ts = [torch.tensor([3.0]), torch.empty(0), torch.tensor([4.0, 12.0]).half()]
    assert l2norm_ref(ts) == 13.0


def _sr_source(n_per_class=2**18):
    gen = torch.Generator().manual_seed(11)
    cls = sr_classes(n_per_class, gen)
    special = torch.tensor([float("inf"), float("-inf"), float("nan")])
    return cls, torch.cat([sr_interleave(cls), special])


def test_sr_classes_layout():
    cls, src = _sr_source(1024)
    bits = cls.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    for k, c in enumerate(SR_CLASSES):
        assert ((bits[k] & 0xFFFF) == c).all()
    expo = (bits >> 23) & 0xFF
    assert expo.min().item() >= 64 and expo.max().item() <= 190
    assert torch.isfinite(cls).all()
    assert len(torch.unique(bits >> 31)) == 2 and len(torch.unique(expo)) > 100
    assert len(torch.unique((bits >> 16) & 0x7F)) == 128
    # interleaving keeps every element and shows every class to every word
    # position j = i % 4 of the kernel's draw, equally often
    flat = src[:-3]
    assert torch.equal(flat.view(torch.int32).sort().values,
                       cls.view(torch.int32).reshape(-1).sort().values)
    low = flat.view(torch.int32).to(torch.int64) & 0xFFFF
    for j in range(4):
        for c in SR_CLASSES:
            assert int((low[j::4] == c).sum()) == 1024 // 4


def test_sr_interval_is_computed_not_tabulated():
    n = 2**18
    assert sr_interval(n, 0x0000) == (0, 0)
    # middle classes: n*p +- 6 sqrt(n p (1-p))
    lo, hi = sr_interval(n, 0x8000)
    assert (lo, hi) == (n // 2 - 1536, n // 2 + 1536)
    lo, hi = sr_interval(n, 0x4000)
    half = 6 * math.sqrt(n * 0.25 * 0.75)
    assert lo == math.ceil(n / 4 - half) and hi == math.floor(n / 4 + half)
    # edge classes: mean 4; P(K = 0) = e^-4 cannot be excluded, and the
    # upper end is where the exact tail drops under 5e-10
    lo, hi = sr_interval(n, 0x0001)
    assert lo == 0 and 20 <= hi <= 30
    tail = 1.0 - sum(
        math.comb(n, k) * (1 / 65536) ** k * (1 - 1 / 65536) ** (n - k)
        for k in range(hi + 1)
    )
    assert tail <= 5e-10 + 1e-15
    assert sr_interval(n, 0xFFFF) == (n - hi, n)
    assert agreement_interval(2**20) == (2**19 - 3072, 2**19 + 3072)


def test_sr_check_accepts_the_torch_fallback():
    from unicore_amd import utils

    _, src = _sr_source()
    dst = torch.empty_like(src, dtype=torch.bfloat16)
    utils.fp32_to_bf16_sr(src, dst)
    sr_check(src, dst)
    tail = dst[-3:].view(torch.int16).to(torch.int64) & 0xFFFF
    assert tail.tolist() == [0x7F80, 0xFF80, 0x7FC0]


def test_sr_check_rejects_round_to_nearest():
    src = _sr_source()[1][:-3]  # finite part: a cast may rewrite a NaN
    with pytest.raises(AssertionError, match="rounded away from zero"):
        sr_check(src, src.bfloat16())


def test_sr_check_rejects_a_coin_flip():
    """Rounds up with probability 1/2 whatever the discarded bits are."""
    src = _sr_source()[1][:-3]  # finite part: a cast may rewrite a NaN
    gen = torch.Generator().manual_seed(5)
    coin = torch.randint(0, 2, src.shape, generator=gen, dtype=torch.int32)
    bits = src.view(torch.int32)
    finite = torch.isfinite(src)
    out = torch.where(finite, bits + (coin << 16), bits) & ~0xFFFF
    dst = out.view(torch.float32).bfloat16()  # low bits are 0: exact
    with pytest.raises(AssertionError):
        sr_check(src, dst)
    # also when it leaves representable values alone, as a kernel that
    # tested `low16 != 0` first would
    keep = (bits & 0xFFFF) == 0
    out = torch.where(finite & ~keep, bits + (coin << 16), bits) & ~0xFFFF
    with pytest.raises(AssertionError, match="rounded away from zero"):
        sr_check(src, out.view(torch.float32).bfloat16())


def test_sr_check_rejects_a_wrong_neighbour():
    src = sr_classes(8, torch.Generator().manual_seed(2)).reshape(-1)
    bits = src.view(torch.int32)
    two_up = ((bits + (2 << 16)) & ~0xFFFF).view(torch.float32).bfloat16()
    with pytest.raises(AssertionError, match="neither"):
        sr_check(src, two_up)
