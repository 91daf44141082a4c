"""The three kernels that end every training step, against float64 (MI355X):
`fused_adam` (`csrc/adam.hip`), `multi_tensor_l2norm` (`csrc/multi_tensor.hip`)
and `fp32_to_bf16_sr` (`csrc/rounding.hip`). References and checkers come from
`_optim_reference.py`, which `test_optim_kernels.py` validates on the CPU.

Every tolerance is a rounding-error bound, `u = 2**-24`:

Adam, one step. The kernel rounds after each fp32 operation (or fewer times,
where the compiler fuses a multiply-add); `1 - beta` is exact in fp32 for
`beta` in [0.5, 1], and the unscale `g * inv_scale` is exact because every
scale used here is a power of two.
- `m' = m*b1 + grad*(1-b1)`: at most two roundings per term, bounded by
  `4u * (|m*b1| + |grad*(1-b1)|)` with room to spare. `v'` has three on its
  second term (`grad*grad`, `*(1-b2)`, the sum): the same `4u` form.
- `p' = p*wdf - T`, `T = step_size*m'/(sqrt(v')+eps)`. The decay term is
  rounded twice (product, final sum): `2u*|p*wdf|`. `T` carries the relative
  error of `m'`, half that of `v'` (<= 1.5u) plus the roundings of sqrt, the
  sum with eps, `step_size*m'`, the quotient and the final sum: `e_m + 6.5u`.
  With inputs that keep `|m'| >= 0.5 * (|m*b1| + |grad*(1-b1)|)` (no
  cancellation: `e_m <= 6u`) and `|T| <= |p*wdf|`, the total
  `2u*|p*wdf| + 12.5u*|T|` is below the bound `8u * (|p*wdf| + |T|)`. The
  tests assert both premises on their inputs.
- A 2-byte parameter is the fp32 result rounded to nearest: half an ulp of
  the dtype at `|p_ref|` more.
Several steps: the sum of the one-step bounds along the float64 trajectory.

L2 norm: every term is non-negative, so a sum formed by any tree of fp32
additions of depth `k` has relative error at most `k*u`; one more `u` for the
square and one to spare give `(k + 2) * u` on the sum of squares. The square
root halves a relative error and rounds once, and the result is an fp32
number: half of that plus one fp32 ulp on the norm. `k` is counted from the
kernel's geometry in `_l2_chain`.

Stochastic rounding: binomial intervals, see `_optim_reference.sr_interval`.
"""

import math

import numpy as np
import pytest
import torch

from _optim_reference import (
    TRIP,
    U32,
    adam_hparams,
    adam_ref,
    agreement_interval,
    l2norm_ref,
    sr_check,
    sr_classes,
    sr_interleave,
    sr_round_up,
    ulp,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]


def _kernels():
    from unicore_amd import ops

    assert ops.has_kernels(), "HIP extension must be built/loaded on a GPU box"
    return ops


def _view(t, off):
    """`t` as the slice `flat[off : off + n]` of a larger device buffer: `off`
    elements past an allocation, the layout `flat_ddp` gives a gradient."""
    flat = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
    out = flat[off : off + t.numel()]
    out.copy_(t)
    assert out.data_ptr() == flat.data_ptr() + off * t.element_size()
    return out


# ---------------------------------------------------------------------------
# fused_adam
# ---------------------------------------------------------------------------

ADAM = dict(lr=1e-2, betas=(0.9, 0.98), eps=1e-6, scale=2.0, step=3,
            bias_correction=True, wd=0.01)


def _rand(gen, n, lo, hi):
    return lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64)


def _sign(gen, n):
    return torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1


def _adam_inputs(n, dtype, scale, seed=0):
    """CPU tensors as the kernel will read them (p, g in `dtype`; m, v fp32).
    `|p|` in [2**-6, 2**-4] against an update of `lr * |m'|/sqrt(v')` with the
    ratio in about [0.4, 1.4]: hundreds of bf16 ulps. `|grad|` within a
    factor 2 of `|m|`, so `|m'| >= (0.9 - 0.2)/(0.9 + 0.2)` of its magnitude
    sum even with opposite signs. From n = 1024 on, every 128th element has
    g = m = v = 0: only the weight decay acts on it."""
    gen = torch.Generator().manual_seed(seed)
    p = (_sign(gen, n) * _rand(gen, n, 2.0**-6, 2.0**-4)).to(dtype)
    am = _rand(gen, n, 2.0**-7, 2.0**-6)
    m = (_sign(gen, n) * am).float()
    g = (_sign(gen, n) * am * _rand(gen, n, 0.5, 2.0) * scale).to(dtype)
    v = ((am * _rand(gen, n, 0.8, 1.6)) ** 2).float()
    idle = torch.zeros(n, dtype=torch.bool)
    if n >= 1024:
        idle[5::128] = True
        m[idle], v[idle], g[idle] = 0, 0, 0
    return p, m, v, g, idle


def _adam_bounds(mags, p_ref, dtype):
    bm = 4 * U32 * mags["m_mag"]
    bv = 4 * U32 * mags["v_mag"]
    bp = 8 * U32 * (mags["p_decay"] + mags["p_step"])
    if dtype != F32:
        bp = bp + 0.5 * ulp(p_ref, dtype)
    return bp, bm, bv


def _assert_premises(mags, m_ref, idle):
    """What the derivation of the p bound assumes (module docstring)."""
    assert (m_ref.abs() >= 0.5 * mags["m_mag"]).all()
    assert (mags["p_step"] <= mags["p_decay"]).all()
    assert (mags["p_step"][~idle] > 0).all()


def _assert_within(name, got, ref, bound):
    err = (got.detach().double().cpu() - ref).abs()
    worst = (err - bound).argmax().item()
    assert (err <= bound).all(), (
        f"{name}: |err| {err[worst].item():.3e} > bound {bound[worst].item():.3e} "
        f"at element {worst} (ref {ref[worst].item():.6e}); "
        f"{int((err > bound).sum())} of {err.numel()} outside"
    )


def _adam_case(n, dtype, offsets=None, **overrides):
    ops = _kernels()
    hp = dict(ADAM, **overrides)
    p, m, v, g, idle = _adam_inputs(n, dtype, hp["scale"])
    p_ref, m_ref, v_ref, mags = adam_ref(p, m, v, g, **hp)
    bp, bm, bv = _adam_bounds(mags, p_ref, dtype)
    _assert_premises(mags, m_ref, idle)

    # Self-check, on the CPU: the reference moves the parameter by more than
    # the bound, so a kernel that left it alone (or moved it by a fraction)
    # cannot pass. Only the weight-decay-only elements are allowed not to.
    moved = (p_ref - p.double()).abs() > bp
    assert moved.double().mean().item() >= 0.99
    assert moved[~idle].all()

    dev = {}
    for name, t in (("p", p), ("m", m), ("v", v), ("g", g)):
        off = (offsets or {}).get(name, 0)
        dev[name] = _view(t, off) if off else t.cuda()
    g_before = dev["g"].clone()
    ops.fused_adam(dev["p"], dev["m"], dev["v"], dev["g"], hp["lr"],
                   hp["betas"][0], hp["betas"][1], hp["eps"], hp["scale"],
                   hp["step"], hp["bias_correction"], hp["wd"])
    torch.cuda.synchronize()

    _assert_within("m", dev["m"], m_ref, bm)
    _assert_within("v", dev["v"], v_ref, bv)
    _assert_within("p", dev["p"], p_ref, bp)
    assert torch.equal(dev["g"], g_before)
    if idle.any():
        # nothing but the decay: moments stay 0, p is the rounded product
        wdf = torch.tensor(adam_hparams(**hp)["wdf"], dtype=F32)
        assert (dev["m"].cpu()[idle] == 0).all() and (dev["v"].cpu()[idle] == 0).all()
        assert torch.equal(dev["p"].cpu()[idle], (p.float() * wdf).to(dtype)[idle])


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 3, 4, 1024, 4099, TRIP + 8, TRIP + 5])
def test_adam_one_step(dtype, n):
    """n = 1, 3: fewer elements than one thread's four (`n / 4 == 0`);
    4, 1024: the vector kernel; 4099: the scalar kernel; `TRIP + 8` /
    `TRIP + 5`: a second grid-stride trip of the vector / scalar kernel."""
    _adam_case(n, dtype)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1024, 4099])
@pytest.mark.parametrize(
    "override",
    [dict(bias_correction=False), dict(wd=0.0), dict(scale=1.0)],
    ids=["no_bias_correction", "no_weight_decay", "unit_scale"],
)
def test_adam_variants(dtype, n, override):
    _adam_case(n, dtype, **override)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("which", ["p", "g", "m", "v"])
def test_adam_unaligned_views(dtype, which, off):
    """One operand starts `off` elements past an allocation, n % 4 == 0: no
    16-byte (fp32) or 8-byte (2-byte p / g) vector may touch it, so the host
    entry has to pick the scalar kernel; the bounds are the same."""
    _adam_case(1024, dtype, offsets={which: off})


@requires_gpu
@pytest.mark.parametrize("n", [1024, 4099])
def test_adam_ten_steps(n):
    """Ten steps, fp32, the state carried by the kernel, against the float64
    trajectory; bound = sum of the ten one-step bounds. The gradients keep the
    sign of m, so no step cancels, and `|p| >= 2**-5` against ten updates of
    about 1e-3 keeps `|T| <= |p*wdf|` all the way."""
    ops = _kernels()
    hp = dict(ADAM, lr=1e-3)
    gen = torch.Generator().manual_seed(n)
    s = _sign(gen, n)
    am = _rand(gen, n, 2.0**-7, 2.0**-6)
    p0 = (_sign(gen, n) * _rand(gen, n, 2.0**-5, 2.0**-4)).float()
    m0 = (s * am).float()
    v0 = ((am * _rand(gen, n, 0.8, 1.6)) ** 2).float()
    grads = [(s * am * _rand(gen, n, 0.5, 2.0) * hp["scale"]).float()
             for _ in range(10)]
    none_idle = torch.zeros(n, dtype=torch.bool)

    p, m, v = p0, m0, v0
    bp = bm = bv = 0.0
    for t, g in enumerate(grads, start=1):
        p, m, v, mags = adam_ref(p, m, v, g, **dict(hp, step=t))
        _assert_premises(mags, m, none_idle)
        dp, dm, dv = _adam_bounds(mags, p, F32)
        bp, bm, bv = bp + dp, bm + dm, bv + dv
    assert ((p - p0.double()).abs() > bp).all()

    pk, mk, vk = p0.cuda(), m0.cuda(), v0.cuda()
    for t, g in enumerate(grads, start=1):
        ops.fused_adam(pk, mk, vk, g.cuda(), hp["lr"], *hp["betas"], hp["eps"],
                       hp["scale"], t, True, hp["wd"])
    _assert_within("m", mk, m, bm)
    _assert_within("v", vk, v, bv)
    _assert_within("p", pk, p, bp)


@requires_gpu
def test_fused_adam_optimizer_against_the_eager_oracle():
    """`FusedAdam` (fp32, GPU) against `optim.adam.Adam` (float64, CPU): two
    groups with their own lr and weight decay, `step(scale=4.0)`, three steps.

    betas, eps, lr and `1 - lr*wd` are fp32 numbers, so the oracle and the
    kernel use the same hyperparameters except `step_size`, which the kernel
    rounds to fp32: `u * |T|` per step on top of the one-step bound. The
    magnitudes come from `adam_ref` run next to the oracle."""
    _kernels()
    from unicore_amd.optim.adam import Adam
    from unicore_amd.optim.fused_adam import FusedAdam

    betas, eps, scale = (0.5, 0.75), 2.0**-20, 4.0
    groups = [dict(n=1024, lr=2.0**-8, wd=0.5), dict(n=4099, lr=2.0**-9, wd=0.25)]
    gen = torch.Generator().manual_seed(9)
    for grp in groups:
        n = grp["n"]
        grp["sign"] = _sign(gen, n)
        grp["p0"] = (_sign(gen, n) * _rand(gen, n, 2.0**-5, 2.0**-4)).float()
        grp["cpu"] = torch.nn.Parameter(grp["p0"].double())
        grp["gpu"] = torch.nn.Parameter(grp["p0"].cuda())
        grp["ref"] = (grp["p0"].double(), torch.zeros(n, dtype=torch.float64),
                      torch.zeros(n, dtype=torch.float64))
        grp["bounds"] = [0.0, 0.0, 0.0]

    def make(cls, key):
        return cls(
            [dict(params=[grp[key]], lr=grp["lr"], weight_decay=grp["wd"])
             for grp in groups],
            betas=betas, eps=eps,
        )

    oracle, fused = make(Adam, "cpu"), make(FusedAdam, "gpu")
    none_idle = {grp["n"]: torch.zeros(grp["n"], dtype=torch.bool) for grp in groups}
    for step in range(1, 4):
        for grp in groups:
            n = grp["n"]
            g = (grp["sign"] * _rand(gen, n, 2.0**-7, 2.0**-6) * scale).float()
            grp["cpu"].grad = g.double() / scale  # exact: the oracle has no scale
            grp["gpu"].grad = g.cuda()
            p, m, v, mags = adam_ref(*grp["ref"], g, grp["lr"], betas, eps, scale,
                                     step, True, grp["wd"])
            _assert_premises(mags, m, none_idle[n])
            grp["ref"] = (p, m, v)
            dp, dm, dv = _adam_bounds(mags, p, F32)
            grp["bounds"][0] = grp["bounds"][0] + dp + U32 * mags["p_step"]
            grp["bounds"][1] = grp["bounds"][1] + dm
            grp["bounds"][2] = grp["bounds"][2] + dv
        oracle.step()
        fused.step(scale=scale)

    for grp in groups:
        bp, bm, bv = grp["bounds"]
        want, got = oracle.state[grp["cpu"]], fused.state[grp["gpu"]]
        assert got["step"] == want["step"] == 3
        assert ((grp["cpu"].data - grp["p0"].double()).abs() > bp).all()
        _assert_within("m", got["exp_avg"], want["exp_avg"], bm)
        _assert_within("v", got["exp_avg_sq"], want["exp_avg_sq"], bv)
        _assert_within("p", grp["gpu"].data, grp["cpu"].data, bp)


# ---------------------------------------------------------------------------
# multi_tensor_l2norm
# ---------------------------------------------------------------------------

L2_MAX_TENSORS = 48  # kMaxTensors: (pointer, numel) pairs per launch
L2_GRID = 1024
CHUNK = 1024


def _l2_chain(sizes, chunk_size):
    """Longest chain of fp32 additions between a square and the result.

    Per launch (48 non-empty tensors): a block visits
    `ceil(n_chunks / grid)` chunks, and in each a thread adds at most one
    head element, `4 * ceil(chunk_size / 1024)` vector elements and three
    tail elements; 6 shuffle steps and 3 adds fold the block; the cleanup
    kernel adds `ceil(grid / 256)` partials per thread and folds again
    (6 + 3). Every launch after the first adds once more into the output."""
    sizes = [n for n in sizes if n > 0]
    launches = [sizes[i : i + L2_MAX_TENSORS]
                for i in range(0, len(sizes), L2_MAX_TENSORS)]
    longest = 0
    for launch in launches:
        n_chunks = sum(-(-n // chunk_size) for n in launch)
        grid = min(n_chunks, L2_GRID)
        per_thread = -(-n_chunks // grid) * (4 * -(-chunk_size // 1024) + 4)
        longest = max(longest, per_thread + 9 + -(-grid // 256) + 9)
    return longest + max(len(launches) - 1, 0)


def _l2_tolerance(ref, sizes, chunk_size):
    k = _l2_chain(sizes, chunk_size)
    return ref * (k + 2) * U32 / 2 + float(np.spacing(np.float32(ref)))


def _l2_case(tensors, chunk_size=CHUNK):
    ops = _kernels()
    ref = l2norm_ref(tensors)
    out = ops.fused_l2norm(tensors, chunk_size)
    assert out.dtype == F32 and out.dim() == 0
    got = out.item()
    tol = _l2_tolerance(ref, [t.numel() for t in tensors], chunk_size)
    assert abs(got - ref) <= tol, (
        f"norm {got!r} vs {ref!r}: |err| {abs(got - ref):.3e} > {tol:.3e}"
    )
    return out


def _randn(n, dtype, gen, scale=1.0):
    return (torch.randn(n, generator=gen, dtype=torch.float64) * scale).to(dtype).cuda()


def test_l2_chain_counts():
    # one chunk of 1024: 8 per thread, two folds of 9, one cleanup partial
    assert _l2_chain([1024], 1024) == 8 + 9 + 1 + 9
    # 1031 chunks on 1024 blocks: two visits; four partials per cleanup thread
    assert _l2_chain([1030 * 1024 + 7], 1024) == 16 + 9 + 4 + 9
    # 97 one-chunk tensors: launches of 48, 48 and 1, two accumulations
    assert _l2_chain([0, 5] + [3] * 96, 1024) == (8 + 9 + 1 + 9) + 2
    assert _l2_chain([0, 0], 1024) == 0


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_l2norm_tensor_spanning_chunks(dtype, r):
    gen = torch.Generator().manual_seed(r)
    _l2_case([_randn(5 * CHUNK + r, dtype, gen)])


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_l2norm_grid_strides(dtype):
    """1031 chunks on a grid capped at 1024: the first seven blocks visit two
    chunks. Run twice: a reducing kernel must repeat bitwise."""
    gen = torch.Generator().manual_seed(4)
    tensors = [_randn(1030 * CHUNK + 7, dtype, gen)]
    assert torch.equal(_l2_case(tensors), _l2_case(tensors))


def _mixed_list(count, dtype, gen):
    """`count` non-empty tensors of mixed small sizes with empty ones among
    them (also in front: entry 0 supplies the dtype and device)."""
    sizes = [1, 2, 3, 17, CHUNK, CHUNK + 5, 255, 2 * CHUNK + 1, 1000, 4]
    tensors = [torch.empty(0, dtype=dtype, device="cuda")]
    for i in range(count):
        tensors.append(_randn(sizes[i % len(sizes)], dtype, gen))
        if i % 20 == 7 or i == count - 1:
            tensors.append(torch.empty(0, dtype=dtype, device="cuda"))
    return tensors


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", [49, 96, 97])
def test_l2norm_more_tensors_than_one_launch(dtype, count):
    """49: a second launch with one tensor; 96: two full launches; 97: a
    third. Each launch after the first must add to the running sum."""
    gen = torch.Generator().manual_seed(count)
    tensors = _mixed_list(count, dtype, gen)
    assert sum(t.numel() == 0 for t in tensors) >= 3
    assert torch.equal(_l2_case(tensors), _l2_case(tensors))
    # every launch carries weight: without the last one, and with the last
    # one alone (a sum that is overwritten), the norm is far outside the bound
    live = [t for t in tensors if t.numel()]
    last = (count - 1) // L2_MAX_TENSORS * L2_MAX_TENSORS
    full = l2norm_ref(tensors)
    tol = _l2_tolerance(full, [t.numel() for t in tensors], CHUNK)
    assert full - l2norm_ref(live[:last]) > 10 * tol
    assert full - l2norm_ref(live[last:]) > 10 * tol


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_l2norm_all_empty(dtype):
    ops = _kernels()
    tensors = [torch.empty(0, dtype=dtype, device="cuda") for _ in range(3)]
    assert ops.fused_l2norm(tensors, CHUNK).item() == 0.0


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("off", [1, 2, 3])
def test_l2norm_views_into_a_flat_buffer(dtype, off):
    """Gradients as `flat_ddp` lays them out: consecutive slices of one flat
    buffer, the first `off` elements in. With sizes 3, 768, 5, 2304 the four
    start 1..3, 0..2, ... elements past a vector boundary; 2304 spans three
    chunks, each with a head and a tail."""
    gen = torch.Generator().manual_seed(off)
    sizes = (3, 768, 5, 2304)
    flat = _randn(off + sum(sizes) + 8, dtype, gen)
    views, at = [], off
    for n in sizes:
        views.append(flat[at : at + n])
        at += n
    vec = 4 * flat.element_size()
    assert {v.data_ptr() % vec for v in views} - {0}, "no unaligned view"
    assert torch.equal(_l2_case(views), _l2_case(views))


@requires_gpu
def test_l2norm_fp16_near_the_top_of_the_range():
    """|x| around 6e4: x*x overflows fp16 but not the fp32 accumulator."""
    gen = torch.Generator().manual_seed(6)
    n = 5 * CHUNK + 3
    x = _sign(gen, n) * _rand(gen, n, 4.0e4, 6.4e4)
    out = _l2_case([x.to(F16).cuda()])
    assert math.isfinite(out.item()) and out.item() > 4.0e4 * math.sqrt(n)


@requires_gpu
def test_l2norm_rejects_a_chunk_size_that_breaks_vector_alignment():
    ops = _kernels()
    t = [torch.ones(64, device="cuda")]
    for bad in (0, -4, 1022, 1023):
        with pytest.raises(RuntimeError, match="chunk_size"):
            ops.fused_l2norm(t, bad)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_l2norm_propagates_non_finite_values(dtype):
    """One inf, then one nan, in a vector-body element, a ragged-tail element,
    a tensor of the second launch, and the head and the body of an unaligned
    view: the norm is non-finite each time and the loss scaler sees the
    overflow. Nothing else tells `DynamicLossScaler` about a bad gradient."""
    from unicore_amd.optim.dynamic_loss_scaler import DynamicLossScaler

    ops = _kernels()
    gen = torch.Generator().manual_seed(8)
    big = _randn(5 * CHUNK + 3, dtype, gen)
    flat = _randn(2304 + 8, dtype, gen)
    view = flat[1 : 1 + 2304]
    tensors = [big, view] + [_randn(7, dtype, gen) for _ in range(48)]
    places = {
        "vector body": (big, 2 * CHUNK + 40),
        "ragged tail": (big, big.numel() - 1),
        "second launch": (tensors[-1], 3),
        "view head": (view, 0),
        "view body": (view, CHUNK + 600),
    }
    scaler = DynamicLossScaler(init_scale=2.0**15)
    scaler.check_overflow(ops.fused_l2norm(tensors, CHUNK))  # finite: no raise
    for where, (t, i) in places.items():
        for bad in (float("inf"), float("nan")):
            keep = t[i].clone()
            t[i] = bad
            norm = ops.fused_l2norm(tensors, CHUNK)
            t[i] = keep
            assert not math.isfinite(norm.item()), (where, bad, norm.item())
            before = scaler.loss_scale
            with pytest.raises(OverflowError):
                scaler.check_overflow(norm)
            assert scaler.loss_scale == before / 2
    assert math.isfinite(ops.fused_l2norm(tensors, CHUNK).item())


# ---------------------------------------------------------------------------
# fp32_to_bf16_sr
# ---------------------------------------------------------------------------


def _sr(ops, src, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    dst = torch.empty_like(src, dtype=BF16)
    ops.fused_fp32_to_bf16_sr(src, dst)
    return dst


@requires_gpu
def test_sr_rounds_up_with_probability_low16_over_65536():
    """2**18 elements per class of discarded bits, interleaved so that each of
    the four words of a thread's draw meets every class, then Inf, -Inf and
    NaN: n = 6 * 2**18 + 3, no multiple of 4."""
    ops = _kernels()
    gen = torch.Generator().manual_seed(11)
    cls = sr_interleave(sr_classes(2**18, gen))
    special = torch.tensor([float("inf"), float("-inf"), float("nan")])
    src = torch.cat([cls, special]).cuda()
    assert src.numel() % 4 == 3
    dst = _sr(ops, src, seed=21)
    sr_check(src, dst)
    tail = dst[-3:].cpu().view(torch.int16).to(torch.int64) & 0xFFFF
    assert tail.tolist() == [0x7F80, 0xFF80, 0x7FC0]
    # per word of the draw as well: a word that is never used, or used for
    # two elements, shows up in its own quarter
    for j in range(4):
        sr_check(src[:-3][j::4], dst[:-3][j::4])


@requires_gpu
def test_sr_draws_are_independent():
    """All elements have discarded bits 0x8000: each rounds up with
    probability 1/2, and two decisions made from different random numbers
    agree with probability 1/2 (6 sigma of Binomial(pairs, 1/2)).
    `n = 2 * TRIP + 3`: every thread makes a second grid-stride trip."""
    ops = _kernels()
    gen = torch.Generator().manual_seed(12)
    n = 2 * TRIP + 3
    row = sr_classes(2**16, gen)[3]
    src = row.repeat(-(-n // row.numel()))[:n].contiguous().cuda()
    dst = _sr(ops, src, seed=31)
    again = _sr(ops, src)  # no reseeding: the generator's offset has moved on
    sr_check(src, dst)
    sr_check(src, again)
    up = sr_round_up(src, dst)
    idx = torch.arange(n)

    def agree(a, b):
        lo, hi = agreement_interval(a.numel())
        k = int((a == b).sum())
        return lo <= k <= hi, (k, a.numel(), lo, hi)

    for d in (1, 2, 3):  # same thread, same draw, another word of it
        same_thread = (idx[:-d] % 4) + d < 4
        ok, info = agree(up[:-d][same_thread], up[d:][same_thread])
        assert ok, (d, info)
    for d in (4, TRIP):  # the neighbouring thread; the same thread's next trip
        ok, info = agree(up[:-d], up[d:])
        assert ok, (d, info)
    ok, info = agree(up, sr_round_up(src, again))
    assert ok, ("second call", info)


@requires_gpu
def test_sr_same_seed_same_bits_also_for_a_view():
    """Same seed, same result; and a source that is a slice of a larger fp32
    buffer at an odd offset, as the bf16 optimizer's write-back passes it,
    gives the result of a contiguous copy."""
    ops = _kernels()
    gen = torch.Generator().manual_seed(13)
    n = 4099
    flat = torch.randn(n + 16, generator=gen).cuda()
    a = _sr(ops, flat[:n].clone(), seed=7)
    assert torch.equal(a, _sr(ops, flat[:n].clone(), seed=7))
    assert not torch.equal(a, _sr(ops, flat[:n].clone(), seed=8))
    for off in (1, 5):
        view = flat[off : off + n]
        assert view.data_ptr() % 8 == 4
        got = _sr(ops, view, seed=7)
        assert torch.equal(got, _sr(ops, view.clone(), seed=7))
