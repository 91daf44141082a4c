"""Shared-axis dropout of the fused residual joins on the GPU (the join
kernels of csrc/dropout_add.hip and csrc/dropout_add_ln.hip with the shared
mask map of csrc/dropout_mask.h): mask sharing and storage, keep rate,
values, backward, determinism, the keying shared with the flat map,
fallbacks, host checks, the Evoformer joins and the trainer.

Shapes are the smallest that reach every branch: odd R and T with C below
one wave's span, and one shape per LN register tile (NV = 1, 2, 4)."""

import math

import pytest
import torch
import torch.nn.functional as F

from unicore_amd.modules import LayerNorm, dropout_add
from unicore_amd.modules.dropout_add_ln import dropout_add_ln, dropout_add_ln_pre

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

SHAPES = [(2, 5, 7, 24), (1, 3, 4, 520), (1, 2, 3, 1032)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# one rounding of the output dtype; fp32 must match exactly
ONE_ROUNDING = {torch.float32: 0.0, torch.float16: 2.0 ** -11,
                torch.bfloat16: 2.0 ** -8}
P = 0.3


def _inputs(shape, dtype, bias, seed=0, positive=False):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rnd(*s):
        t = torch.rand(*s, device="cuda", generator=g)
        # positive: x in [1, 2), bias in [0.5, 1.5): x + bias has no zeros
        return (t + 1.0 if positive else t * 2.0 - 1.0).to(dtype)

    x = rnd(*shape)
    res = torch.zeros(shape, device="cuda", dtype=dtype) if positive \
        else rnd(*shape)
    b = (rnd(shape[-1]) - (0.5 if positive else 0.0)).to(dtype) if bias else None
    return x, res, b


def _unpack(dmask, shape, shared_dim):
    """Small bitfield -> bool keep of the full shape (bit j of byte m is
    element 8m + j of the (B, T, C) or (B, R, C) mask tensor)."""
    B, R, T, C = shape
    bits = (dmask.view(-1, 1) >> torch.arange(8, device=dmask.device,
                                              dtype=torch.uint8)) & 1
    small = bits.bool().view(B, T if shared_dim == 1 else R, C)
    return small.unsqueeze(shared_dim).expand(shape)


def _rel_close(got, want, tol, what):
    got, want = got.float(), want.float()
    if tol == 0.0:
        assert torch.equal(got, want), what
        return
    err = (got - want).abs()
    bound = tol * want.abs()
    worst = (err - bound).max().item()
    print(f"{what}: max abs err {err.max().item():.3e}, "
          f"max err/|want| {(err / want.abs().clamp_min(1e-30)).max().item():.3e}"
          f" (bound {tol:.3e})")
    assert worst <= 0, what


def _reference(x, res, bias, keep, p, dtype):
    """fp32 reference from the recovered mask, rounded once."""
    xb = x.float() + bias.float() if bias is not None else x.float()
    pinv = 1.0 / (1.0 - p)
    s = res.float() + torch.where(keep, xb * pinv, torch.zeros_like(xb))
    return s.to(dtype)


# ---------------------------------------------------------------------------
# mask sharing and storage
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shared_dim", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("entry", ["add", "ln"])
def test_mask_is_shared_and_stored_small(entry, shape, shared_dim, dtype,
                                         with_bias):
    from unicore_amd import ops

    B, R, T, C = shape
    x, res, bias = _inputs(shape, dtype, with_bias, positive=True)
    torch.manual_seed(21)
    if entry == "add":
        out, dmask = ops.shared_dropout_add_fwd(x, res, P, shared_dim, bias)
    else:
        gamma = torch.ones(C, device="cuda", dtype=dtype)
        beta = torch.zeros(C, device="cuda", dtype=dtype)
        _, out, dmask, _, _ = ops.shared_dropout_add_ln_fwd(
            x, res, bias, gamma, beta, P, shared_dim, 1e-5)
    keep = out != 0
    first = keep.select(shared_dim, 0).unsqueeze(shared_dim)
    assert torch.equal(keep, first.expand_as(keep)), "not shared"
    other = 3 - shared_dim
    ref = keep.select(other, 0).unsqueeze(other)
    assert not torch.equal(keep, ref.expand_as(keep)), "constant along other"
    if B > 1:
        assert not torch.equal(keep[0], keep[1]), "constant along batch"
    assert 0.4 < keep.float().mean().item() < 0.95
    n_small = B * (T if shared_dim == 1 else R) * C // 8
    assert dmask.dtype == torch.uint8 and dmask.numel() == n_small
    assert torch.equal(_unpack(dmask, shape, shared_dim), keep)


@pytest.mark.parametrize("p", [0.15, 0.25])
def test_keep_rate(p):
    """N = 2*64*256 independent decisions; five standard errors plus the
    16-bit threshold's quantisation."""
    from unicore_amd import ops

    shape = (2, 3, 64, 256)
    x, res, _ = _inputs(shape, torch.bfloat16, False, positive=True)
    torch.manual_seed(33)
    _, dmask = ops.shared_dropout_add_fwd(x, res, p, 1)
    n = 2 * 64 * 256
    assert dmask.numel() * 8 == n
    bits = (dmask.view(-1, 1) >> torch.arange(8, device="cuda",
                                              dtype=torch.uint8)) & 1
    rate = bits.float().mean().item()
    bound = 5 * math.sqrt(p * (1 - p) / n) + 2.0 ** -16
    print(f"p={p}: keep rate {rate:.6f}, want {1 - p:.6f}, bound {bound:.6f}")
    assert abs(rate - (1 - p)) <= bound


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shared_dim", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_dropout_add_forward_values(shape, shared_dim, dtype, with_bias):
    from unicore_amd import ops

    x, res, bias = _inputs(shape, dtype, with_bias, seed=1)
    torch.manual_seed(22)
    out, dmask = ops.shared_dropout_add_fwd(x, res, P, shared_dim, bias)
    keep = _unpack(dmask, shape, shared_dim)
    want = _reference(x, res, bias, keep, P, dtype)
    _rel_close(out, want, ONE_ROUNDING[dtype], f"out {shape} {dtype}")


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shared_dim", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_dropout_add_ln_forward_values(shape, shared_dim, dtype, with_bias):
    from unicore_amd import ops

    C = shape[-1]
    x, res, bias = _inputs(shape, dtype, with_bias, seed=2)
    g = torch.Generator(device="cuda").manual_seed(3)
    gamma = (torch.rand(C, device="cuda", generator=g) + 0.5).to(dtype)
    beta = (torch.rand(C, device="cuda", generator=g) - 0.5).to(dtype)
    torch.manual_seed(23)
    normed, summed, dmask, mean, invvar = ops.shared_dropout_add_ln_fwd(
        x, res, bias, gamma, beta, P, shared_dim, 1e-5)
    keep = _unpack(dmask, shape, shared_dim)
    want = _reference(x, res, bias, keep, P, dtype)
    _rel_close(summed, want, ONE_ROUNDING[dtype], f"summed {shape} {dtype}")
    # normed against F.layer_norm of summed in fp32, with the bounds of
    # test_dropout_add_ln_fused_parity
    s32 = summed.float()
    ref = F.layer_norm(s32, (C,), gamma.float(), beta.float(), 1e-5)
    # fp16 is not in that test: four roundings of its format (summed is
    # rounded once, the kernel norms the unrounded sum and rounds once)
    tol = {torch.float32: 2e-5, torch.bfloat16: 2e-2,
           torch.float16: 4 * 2.0 ** -11}[dtype]
    d = (normed.float() - ref).abs().max().item()
    s = ref.abs().max().item() + 1e-6
    print(f"normed {shape} {dtype}: {d:.3e} / {s:.3e} = {d / s:.3e} (< {tol})")
    assert d / s < tol


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------


def _check_grads(x, res, bias, g_total, dmask, shared_dim, dtype):
    """dx = g * keep / (1 - p) within one rounding and d_res = g exactly.
    The bias grad is the kernel's fp32 column sum (rounded once to the bias
    dtype by the autograd Function): the sum is held against the float64
    column sum of the fp32 dx, bound rows * 2**-23 * sum|dx| per column."""
    from unicore_amd import ops

    keep = _unpack(dmask, tuple(x.shape), shared_dim)
    pinv = 1.0 / (1.0 - P)
    g32 = g_total.float()
    dx32 = torch.where(keep, g32 * pinv, torch.zeros_like(g32))
    _rel_close(x.grad, dx32.to(dtype), ONE_ROUNDING[dtype], f"dx {dtype}")
    assert torch.equal(res.grad, g_total)
    if bias is not None:
        C = x.shape[-1]
        rows = x.numel() // C
        dx_k, db = ops.shared_dropout_add_bwd(g_total.contiguous(), dmask, P,
                                              shared_dim, C)
        assert db.dtype == torch.float32 and torch.equal(dx_k, x.grad)
        want = dx32.double().view(rows, C).sum(0)
        bound = rows * 2.0 ** -23 * dx32.abs().double().view(rows, C).sum(0)
        err = (db.double() - want).abs()
        print(f"dbias {dtype} rows={rows}: max err {err.max().item():.3e}, "
              f"min (bound - err) {(bound - err).min().item():.3e}")
        assert (err <= bound).all()
        assert torch.equal(bias.grad, db.to(dtype))


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shared_dim", [1, 2])
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_dropout_add_backward(shape, shared_dim, dtype, with_bias):
    from unicore_amd import ops

    x, res, bias = _inputs(shape, dtype, with_bias, seed=4)
    for t in (x, res, bias):
        if t is not None:
            t.requires_grad_(True)
    torch.manual_seed(24)
    out = dropout_add(x, res, P, True, bias=bias, shared_dim=shared_dim)
    # the same seed through the raw entry gives the mask
    torch.manual_seed(24)
    out_raw, dmask = ops.shared_dropout_add_fwd(
        x.detach(), res.detach(), P, shared_dim,
        bias.detach() if with_bias else None)
    assert torch.equal(out_raw, out)
    g = _inputs(shape, dtype, False, seed=5)[0]
    out.backward(g)
    _check_grads(x, res, bias, g, dmask, shared_dim, dtype)


@pytest.mark.parametrize("use_normed", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shared_dim", [1, 2])
def test_dropout_add_ln_pre_backward(shared_dim, dtype, use_normed):
    """Both outputs used, and only the summed stream used."""
    from unicore_amd import ops

    shape = SHAPES[0]
    C = shape[-1]
    x, res, bias = _inputs(shape, dtype, True, seed=6)
    ln = LayerNorm(C).cuda().to(dtype)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.uniform_(-0.5, 0.5)
    for t in (x, res, bias):
        t.requires_grad_(True)
    torch.manual_seed(25)
    s, n = dropout_add_ln_pre(x, res, ln, P, True, bias=bias,
                              shared_dim=shared_dim)
    # the same seed through the raw entry gives the mask
    torch.manual_seed(25)
    _, s_raw, dmask, mean, invvar = ops.shared_dropout_add_ln_fwd(
        x.detach(), res.detach(), bias.detach(), ln.weight.detach(),
        ln.bias.detach(), P, shared_dim, ln.eps)
    assert torch.equal(s_raw, s)
    gs = _inputs(shape, dtype, False, seed=7)[0]
    gn = _inputs(shape, dtype, False, seed=8)[0]
    if use_normed:
        torch.autograd.backward([s, n], [gs, gn])
        d_ln, dgamma, dbeta = ops.layernorm_bwd(gn, s.detach(), mean, invvar,
                                                ln.weight.detach())
        g_total = d_ln + gs
        assert torch.equal(ln.weight.grad, dgamma.to(dtype))
        assert torch.equal(ln.bias.grad, dbeta.to(dtype))
    else:
        s.backward(gs)
        g_total = gs
        assert ln.weight.grad is None or not ln.weight.grad.any()
    _check_grads(x, res, bias, g_total, dmask, shared_dim, dtype)


def test_dropout_add_ln_backward():
    """Post-LN join: gradients flow through layernorm_bwd and the mask."""
    from unicore_amd import ops

    shape, dtype, shared_dim = SHAPES[1], torch.bfloat16, 2
    C = shape[-1]
    x, res, bias = _inputs(shape, dtype, True, seed=9)
    ln = LayerNorm(C).cuda().to(dtype)
    for t in (x, res, bias):
        t.requires_grad_(True)
    torch.manual_seed(26)
    out = dropout_add_ln(x, res, ln, P, True, bias=bias, shared_dim=shared_dim)
    torch.manual_seed(26)
    n_raw, s, dmask, mean, invvar = ops.shared_dropout_add_ln_fwd(
        x.detach(), res.detach(), bias.detach(), ln.weight.detach(),
        ln.bias.detach(), P, shared_dim, ln.eps)
    assert torch.equal(n_raw, out)
    gn = _inputs(shape, dtype, False, seed=10)[0]
    out.backward(gn)
    d_ln, _, _ = ops.layernorm_bwd(gn, s, mean, invvar, ln.weight.detach())
    _check_grads(x, res, bias, d_ln, dmask, shared_dim, dtype)


# ---------------------------------------------------------------------------
# determinism and generator use
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shared_dim", [1, 2])
def test_determinism_and_generator_use(shared_dim):
    from unicore_amd import ops

    shape, dtype = SHAPES[0], torch.bfloat16
    ln = LayerNorm(shape[-1]).cuda().to(dtype)
    g = _inputs(shape, dtype, False, seed=12)[0]

    def run(seed):
        x, res, bias = _inputs(shape, dtype, True, seed=11)
        for t in (x, res, bias):
            t.requires_grad_(True)
        torch.manual_seed(seed)
        s, n = dropout_add_ln_pre(x, res, ln, P, True, bias=bias,
                                  shared_dim=shared_dim)
        o = dropout_add(n, s, P, True, shared_dim=shared_dim)
        o.backward(g)
        return [s.detach(), n.detach(), o.detach(), x.grad, res.grad,
                bias.grad]

    a, b, c = run(40), run(40), run(41)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not torch.equal(a[0], c[0])

    x, res, _ = _inputs(shape, dtype, False, positive=True)
    torch.manual_seed(42)
    _, m1 = ops.shared_dropout_add_fwd(x, res, P, shared_dim)
    _, m2 = ops.shared_dropout_add_fwd(x, res, P, shared_dim)
    torch.manual_seed(42)
    _, m3 = ops.shared_dropout_add_fwd(x, res, P, shared_dim)
    torch.manual_seed(43)
    _, m4 = ops.shared_dropout_add_fwd(x, res, P, shared_dim)
    assert torch.equal(m1, m3)
    assert not torch.equal(m1, m2), "consecutive calls drew one mask"
    assert not torch.equal(m1, m4), "the seed does not reach the mask"


# ---------------------------------------------------------------------------
# the two mask maps share one keying
# ---------------------------------------------------------------------------

# shared extent 1: the shared map is the identity, as the flat map is; the
# last two reach the LN register tiles NV = 2 and NV = 4
UNIT_EXTENT = [((2, 1, 7, 24), 1), ((2, 5, 1, 24), 2), ((1, 1, 4, 520), 1),
               ((1, 1, 3, 1032), 1)]


def _generator_offset():
    return torch.cuda.default_generators[torch.cuda.current_device()] \
        .get_offset()


def _scale_add_close(flat, shared, x, res, bias, dtype, what):
    """The flat kernels may contract the scale into the add, the shared ones
    round the product on its own: two roundings of at most 2**-24 each,
    relative to terms no larger than |res| + |x + b| * pinv, hence
    |flat - shared| <= 2**-23 * (|res| + |x + b| * pinv) in fp32; the
    2-byte dtypes add one rounding of the output on top."""
    xb = x.float() + bias.float() if bias is not None else x.float()
    pinv = 1.0 / (1.0 - P)
    bound = 2.0 ** -23 * (res.float().abs() + xb.abs() * pinv) \
        + ONE_ROUNDING[dtype] * shared.float().abs()
    err = (flat.float() - shared.float()).abs()
    print(f"{what}: max err {err.max().item():.3e}, "
          f"max (err - bound) {(err - bound).max().item():.3e}, "
          f"{(err > 0).sum().item()} of {err.numel()} differ")
    assert (err <= bound).all(), what


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,shared_dim", UNIT_EXTENT)
def test_unit_shared_extent_is_the_flat_map(shape, shared_dim, dtype,
                                            with_bias):
    """With a shared extent of 1 the shared entries draw the mask of the
    unshared entries from the same seed and reserve the same generator
    range; backward, which has no add to contract, agrees bitwise. (normed
    is a function of summed and is held to its own reference in
    test_dropout_add_ln_forward_values.)"""
    from unicore_amd import ops

    C = shape[-1]
    x, res, bias = _inputs(shape, dtype, with_bias, seed=13)
    g = torch.Generator(device="cuda").manual_seed(14)
    gamma = (torch.rand(C, device="cuda", generator=g) + 0.5).to(dtype)
    beta = (torch.rand(C, device="cuda", generator=g) - 0.5).to(dtype)

    torch.manual_seed(27)
    out_f, mask_f = ops.dropout_add_fwd(x, res, P, True, bias)
    off_f = _generator_offset()
    torch.manual_seed(27)
    out_s, mask_s = ops.shared_dropout_add_fwd(x, res, P, shared_dim, bias)
    off_s = _generator_offset()
    assert torch.equal(mask_f, mask_s), "add: masks differ"
    assert off_f == off_s, (off_f, off_s)
    _scale_add_close(out_f, out_s, x, res, bias, dtype, f"out {shape} {dtype}")

    torch.manual_seed(28)
    _, sum_f, lmask_f, _, _ = ops.dropout_add_ln_fwd(
        x, res, bias, gamma, beta, P, True, 1e-5)
    off_f = _generator_offset()
    torch.manual_seed(28)
    _, sum_s, lmask_s, _, _ = ops.shared_dropout_add_ln_fwd(
        x, res, bias, gamma, beta, P, shared_dim, 1e-5)
    off_s = _generator_offset()
    assert torch.equal(lmask_f, lmask_s), "ln: masks differ"
    assert off_f == off_s, (off_f, off_s)
    _scale_add_close(sum_f, sum_s, x, res, bias, dtype,
                     f"summed {shape} {dtype}")

    grad = _inputs(shape, dtype, False, seed=15)[0]
    bias_dim = C if with_bias else 0
    dx_f, db_f = ops.dropout_add_bwd(grad, mask_f, P, bias_dim)
    dx_s, db_s = ops.shared_dropout_add_bwd(grad, mask_f, P, shared_dim,
                                            bias_dim)
    assert torch.equal(dx_f, dx_s), "dx differs"
    assert db_f.shape == db_s.shape and torch.equal(db_f, db_s), "dbias differs"


# ---------------------------------------------------------------------------
# fallbacks and checks
# ---------------------------------------------------------------------------


def _assert_shared(out, shared_dim):
    keep = out != 0
    first = keep.select(shared_dim, 0).unsqueeze(shared_dim)
    assert torch.equal(keep, first.expand_as(keep))
    other = 3 - shared_dim
    ref = keep.select(other, 0).unsqueeze(other)
    assert not torch.equal(keep, ref.expand_as(keep))
    assert 0 < keep.float().mean().item() < 1


@pytest.mark.parametrize("shared_dim", [1, 2])
def test_odd_width_takes_the_eager_path(shared_dim, monkeypatch):
    from unicore_amd import ops

    def boom(*a, **k):
        raise AssertionError("fused entry reached with C % 8 != 0")

    monkeypatch.setattr(ops, "shared_dropout_add_fwd", boom)
    monkeypatch.setattr(ops, "shared_dropout_add_ln_fwd", boom)
    shape = (2, 5, 7, 20)
    x = torch.ones(shape, device="cuda", dtype=torch.bfloat16)
    res = torch.zeros_like(x)
    ln = LayerNorm(20).cuda().bfloat16()
    _assert_shared(dropout_add(x, res, 0.4, True, shared_dim=shared_dim),
                   shared_dim)
    s, n = dropout_add_ln_pre(x, res, ln, 0.4, True, shared_dim=shared_dim)
    _assert_shared(s, shared_dim)
    assert torch.isfinite(dropout_add_ln(x, res, ln, 0.4, True,
                                         shared_dim=shared_dim)).all()


@pytest.mark.parametrize("shared_dim", [1, 2])
def test_gate_off_falls_back_with_a_shared_mask(shared_dim, monkeypatch):
    from unicore_amd import ops

    def boom(*a, **k):
        raise AssertionError("fused entry reached with the gate off")

    monkeypatch.setenv("UNICORE_SHARED_DROPOUT_FUSED", "0")
    monkeypatch.setattr(ops, "shared_dropout_add_fwd", boom)
    monkeypatch.setattr(ops, "shared_dropout_add_ln_fwd", boom)
    shape = SHAPES[0]
    x = torch.ones(shape, device="cuda", dtype=torch.bfloat16)
    res = torch.zeros_like(x)
    bias = torch.ones(shape[-1], device="cuda", dtype=torch.bfloat16)
    ln = LayerNorm(shape[-1]).cuda().bfloat16()
    p = 0.5
    out = dropout_add(x, res, p, True, bias=bias, shared_dim=shared_dim)
    _assert_shared(out, shared_dim)
    assert torch.equal(out[out != 0], torch.full_like(out[out != 0], 4.0))
    s, n = dropout_add_ln_pre(x, res, ln, p, True, bias=bias,
                              shared_dim=shared_dim)
    _assert_shared(s, shared_dim)
    assert torch.equal(n, ln(s))


def test_gate_on_reaches_the_fused_entry(monkeypatch):
    from unicore_amd import ops

    calls = []
    real = ops.shared_dropout_add_fwd

    def spy(*a, **k):
        calls.append(a[3])
        return real(*a, **k)

    monkeypatch.setattr(ops, "shared_dropout_add_fwd", spy)
    x, res, _ = _inputs(SHAPES[0], torch.bfloat16, False)
    dropout_add(x, res, P, True, shared_dim=2)
    assert calls == [2]


def test_host_checks_name_the_value():
    from unicore_amd import ops

    dt = torch.bfloat16
    x = torch.ones(2, 5, 7, 24, device="cuda", dtype=dt)
    gamma = torch.ones(24, device="cuda", dtype=dt)

    def fwd(x_, res_, sd=1, bias=None, p=P):
        return ops.shared_dropout_add_fwd(x_, res_, p, sd, bias)

    with pytest.raises(RuntimeError, match="on the GPU, got device cpu"):
        fwd(x.cpu(), x.cpu())
    xt = x.transpose(1, 2)
    with pytest.raises(RuntimeError, match=r"contiguous, got sizes \[2, 7, 5, 24\]"):
        fwd(xt, xt)
    with pytest.raises(RuntimeError, match=r"residual sizes \[2, 5, 7, 16\]"):
        fwd(x, x[..., :16].contiguous())
    with pytest.raises(RuntimeError, match="residual dtype Half"):
        fwd(x, x.half())
    with pytest.raises(RuntimeError, match=r"4-D.*got 3-D with sizes \[10, 7, 24\]"):
        fwd(x.view(10, 7, 24), x.view(10, 7, 24))
    with pytest.raises(RuntimeError, match="shared_dim must be 1 or 2, got 3"):
        fwd(x, x, sd=3)
    x20 = torch.ones(2, 5, 7, 20, device="cuda", dtype=dt)
    with pytest.raises(RuntimeError, match="multiple of 8, got 20"):
        fwd(x20, x20)
    with pytest.raises(RuntimeError, match="bias has 16 elements.*width is 24"):
        fwd(x, x, bias=gamma[:16].contiguous())
    with pytest.raises(RuntimeError, match=r"p must be in \(0, 1\).*got 0"):
        fwd(x, x, p=0.0)
    wide = torch.ones(1, 1, 2, 2056, device="cuda", dtype=dt)
    gw = torch.ones(2056, device="cuda", dtype=dt)
    with pytest.raises(RuntimeError, match="at most 2048, got 2056"):
        ops.shared_dropout_add_ln_fwd(wide, wide, None, gw, gw, P, 1, 1e-5)
    with pytest.raises(RuntimeError, match="gamma/beta have 16/24 elements"):
        ops.shared_dropout_add_ln_fwd(x, x, None, gamma[:16].contiguous(),
                                      gamma, P, 1, 1e-5)
    _, dmask = fwd(x, x, sd=1)          # B*T*C/8 = 42 bytes
    with pytest.raises(RuntimeError, match="mask has 42 bytes.*needs 30"):
        ops.shared_dropout_add_bwd(x, dmask, P, 2)
    with pytest.raises(RuntimeError, match="bias_dim must be 0 or.*24.*got 16"):
        ops.shared_dropout_add_bwd(x, dmask, P, 1, 16)


# ---------------------------------------------------------------------------
# model and trainer
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("triangle_attention", [False, True])
def test_evoformer_block_joins_get_the_table(triangle_attention, monkeypatch):
    from unicore_amd.models import evoformer
    from unicore_amd.models.evoformer import EvoformerBlock

    torch.manual_seed(5)
    blk = EvoformerBlock(d_msa=64, d_pair=32, heads=4, dropout=0.0,
                         triangle_attention=triangle_attention,
                         msa_dropout=0.15, pair_dropout=0.25)
    blk = blk.cuda().bfloat16().train()
    seen = []
    real_pre, real_add = evoformer.dropout_add_ln_pre, evoformer.dropout_add

    def spy_pre(x, residual, ln, p, is_training, bias=None, shared_dim=None):
        seen.append((ln, p, shared_dim))
        return real_pre(x, residual, ln, p, is_training, bias=bias,
                        shared_dim=shared_dim)

    def spy_add(x, residual, p, is_training, bias=None, shared_dim=None):
        seen.append((None, p, shared_dim))
        return real_add(x, residual, p, is_training, bias=bias,
                        shared_dim=shared_dim)

    monkeypatch.setattr(evoformer, "dropout_add_ln_pre", spy_pre)
    monkeypatch.setattr(evoformer, "dropout_add", spy_add)
    fused = []
    from unicore_amd import ops
    real_fused = ops.shared_dropout_add_ln_fwd

    def spy_fused(*a, **k):
        fused.append((a[5], a[6]))
        return real_fused(*a, **k)

    monkeypatch.setattr(ops, "shared_dropout_add_ln_fwd", spy_fused)
    msa = torch.randn(1, 8, 16, 64, device="cuda", dtype=torch.bfloat16)
    pair = torch.randn(1, 16, 16, 32, device="cuda", dtype=torch.bfloat16)
    blk(msa, pair)
    # a join is named by the norm it feeds: the one AFTER the module listed
    want = [
        (blk.col_attn.norm, 0.15, 1),            # after row_attn
        (blk.msa_transition.norm, 0.0, None),    # after col_attn
        (blk.opm.norm, 0.0, None),               # after msa_transition
        (blk.tri_out.norm, 0.0, None),           # after opm
        (blk.tri_in.norm, 0.25, 1),              # after tri_out
    ]
    if triangle_attention:
        want += [
            (blk.tri_att_start.norm, 0.25, 1),   # after tri_in
            (blk.tri_att_end.norm, 0.25, 1),     # after tri_att_start
            (blk.pair_transition.norm, 0.25, 2),  # after tri_att_end
        ]
    else:
        want += [(blk.pair_transition.norm, 0.25, 1)]  # after tri_in
    want += [(None, 0.0, None)]                  # after pair_transition
    assert len(seen) == len(want)
    for got, exp in zip(seen, want):
        assert got[0] is exp[0] and got[1:] == exp[1:], (got, exp)
    # and every shared join ran the fused kernel
    assert fused == [(w[1], w[2]) for w in want if w[2] is not None]


@pytest.mark.parametrize("triangle_attention", [False, True])
def test_evoformer_block_checkpoint_redraws_the_masks(triangle_attention):
    from unicore_amd import utils
    from unicore_amd.models.evoformer import EvoformerBlock

    def run(checkpoint, seed):
        torch.manual_seed(5)
        blk = EvoformerBlock(d_msa=64, d_pair=32, heads=4, dropout=0.0,
                             triangle_attention=triangle_attention,
                             msa_dropout=0.15, pair_dropout=0.25)
        blk = blk.cuda().bfloat16().train()
        torch.manual_seed(9)
        msa = torch.randn(1, 8, 16, 64, device="cuda", dtype=torch.bfloat16)
        pair = torch.randn(1, 16, 16, 32, device="cuda", dtype=torch.bfloat16)
        msa.requires_grad_(True)
        pair.requires_grad_(True)
        torch.manual_seed(seed)
        if checkpoint:
            m, p = utils.checkpoint_sequential(
                [lambda a, b: blk(a, b)], (msa, pair))
        else:
            m, p = blk(msa, pair)
        # a sum, not a mean: gradients well above the absolute tolerance,
        # so that it can tell two sets of masks apart
        ((m.float().square().sum() + p.float().square().sum()) / 16).backward()
        return {k: v.grad.float().clone() for k, v in blk.named_parameters()
                if v.grad is not None}

    plain = run(False, 70)
    ckpt = run(True, 70)
    other = run(False, 71)
    assert set(plain) == set(ckpt) == set(other)

    def close(a, b):
        return all(torch.allclose(a[k], b[k], rtol=1e-2, atol=1e-2) for k in a)

    assert close(plain, ckpt), max(
        (plain[k] - ckpt[k]).abs().max().item() for k in plain)
    # another seed draws other masks: the tolerance tells them apart
    assert not close(plain, other)


def test_trainer_three_steps_are_finite_and_repeatable():
    from unicore_amd import options, tasks
    from unicore_amd.trainer import Trainer

    def run():
        argv = [
            "--task", "evoformer_synthetic",
            "--arch", "evoformer",
            "--loss", "masked_msa",
            "--optimizer", "adam",
            "--lr-scheduler", "fixed",
            "--lr", "1e-3",
            "--batch-size", "1",
            "--dataset-size", "8",
            "--msa-depth", "8",
            "--residues", "24",
            "--evo-layers", "2",
            "--msa-dim", "64",
            "--pair-dim", "32",
            "--evo-heads", "4",
            "--msa-dropout", "0.15",
            "--pair-dropout", "0.25",
            "--triangle-attention",
            "--seed", "5",
            "--bf16",
            "--log-format", "none",
            "--num-workers", "0",
        ]
        parser = options.get_training_parser()
        args = options.parse_args_and_arch(parser, input_args=argv)
        args.distributed_world_size = 1
        args.distributed_rank = 0
        args.device_id = 0
        args.distributed_no_spawn = True
        torch.manual_seed(args.seed)
        task = tasks.setup_task(args)
        task.load_dataset("train")
        model = task.build_model(args)
        loss = task.build_loss(args)
        trainer = Trainer(args, task, model, loss)
        epoch_itr = trainer.get_train_iterator(epoch=1)
        trainer.init_total_train_steps(epoch_itr)
        itr = epoch_itr.next_epoch_itr(shuffle=False)
        return [float(trainer.train_step([next(itr)])["loss"])
                for _ in range(3)]

    a, b = run(), run()
    assert all(math.isfinite(v) for v in a), a
    assert a == b, (a, b)
