"""Softmax-dropout kernels on the paths training actually runs (MI355X).

Every test compares `csrc/softmax_dropout.hip` with plain torch in float64 on
the device, computed from the same rounded inputs the kernel sees: the kernel
forms `x + mask`, then `+ bias`, in fp32 before the max, so the reference
does that fp32 sum in that order and only then goes to float64 for the
softmax and its backward (otherwise a `-1e9` row disagrees for a reason that
is no bug). Dropout is checked through the bitfield the kernel returns:
`keep[row, e] = (dmask[row, e // 8] >> (e % 8)) & 1`.

Tolerances are the project's (`TOL` of `tests/test_kernels_gpu.py`): forward
`|err| < TOL`, dx `|err| < 4 * TOL` for a unit-normal upstream gradient, bias
gradient `max|err| / (max|ref| + 1e-3) < 10 * TOL`.
"""

import math
import os
import subprocess
import sys

import pytest
import torch

from test_kernels_gpu import TOL

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def _kernels():
    from unicore_amd import ops

    assert ops.has_kernels(), "HIP extension must be built/loaded on a GPU box"
    return ops


def _neg(dtype):
    return -3e4 if dtype == F16 else -1e9


def _unpack(dmask, k):
    """(n, q, k/8) uint8 bitfield -> (n, q, k) bool."""
    bits = torch.arange(8, device=dmask.device, dtype=torch.int32)
    keep = (dmask.to(torch.int32).unsqueeze(-1) >> bits) & 1
    return keep.bool().reshape(*dmask.shape[:-1], k)


def _ref_fwd(x, mask, bias):
    """float64 softmax of the fp32 sum (x + mask) + bias."""
    v = x.float()
    if mask is not None:
        v = v + mask.float()
    if bias is not None:
        v = v + bias.float()
    return torch.softmax(v.double().reshape(x.shape), dim=-1)


def _ref_bwd(y, gout, keep, p):
    t = gout.double()
    if keep is not None:
        t = t * keep / (1.0 - p)
    return y * (t - (t * y).sum(-1, keepdim=True))


def _ref_out(y, keep, p):
    return y if keep is None else y * keep / (1.0 - p)


def _err(got, ref):
    return (got.double() - ref).abs().max().item()


def _bias_err(got, ref):
    return _err(got, ref) / (ref.abs().max().item() + 1e-3)


def _pad_mask(shape, dtype, frac=0.3):
    """Additive key mask shaped like `additive_key_mask` output: 0 for a live
    key, -1e9 (-3e4 in fp16) for a padded one; key 0 stays live."""
    pad = torch.rand(shape, device="cuda") < frac
    pad[..., 0] = False
    return torch.where(pad, _neg(dtype), 0.0).to(dtype)


@pytest.fixture
def spy(monkeypatch):
    """Count the three kernel entry points and keep the last forward's
    (dropout bitfield, softmax result)."""
    ops = _kernels()
    rec = {"fwd": 0, "bwd": 0, "bwd_bias": 0, "dmask": None, "y": None}

    real_fwd = ops.softmax_dropout_fwd
    real_bwd = ops.softmax_dropout_bwd
    real_bwd_bias = ops.softmax_dropout_bwd_bias

    def fwd(*args):
        rec["fwd"] += 1
        r = real_fwd(*args)
        rec["dmask"], rec["y"] = r[1], r[2]
        return r

    def bwd(*args):
        rec["bwd"] += 1
        return real_bwd(*args)

    def bwd_bias(*args):
        rec["bwd_bias"] += 1
        return real_bwd_bias(*args)

    monkeypatch.setattr(ops, "softmax_dropout_fwd", fwd)
    monkeypatch.setattr(ops, "softmax_dropout_bwd", bwd)
    monkeypatch.setattr(ops, "softmax_dropout_bwd_bias", bwd_bias)
    return rec


def _run_module(spy, x, mask, bias, p, gout, seed=77):
    """softmax_dropout(inplace=False) forward and backward.

    Returns (out, dx, dbias or None, keep or None). `bias` may be a
    non-contiguous view; its gradient comes back in the view's shape."""
    from unicore_amd.modules import softmax_dropout

    xk = x.clone().requires_grad_(True)
    bk = None if bias is None else bias.detach().requires_grad_(True)
    torch.manual_seed(seed)
    out = softmax_dropout(xk, p, is_training=True, mask=mask, bias=bk,
                          inplace=False)
    keep = None
    if p > 0 and x.shape[-1] % 8 == 0:
        q, k = x.shape[-2:]
        assert spy["dmask"].shape == (x.numel() // (q * k), q, k // 8)
        keep = _unpack(spy["dmask"], k).view(x.shape)
    elif p > 0:
        # no fused dropout at this width: torch's dropout ran on the kernel's
        # softmax, and a softmax of finite logits has no zero of its own
        # (a padded key is zero either way)
        assert spy["dmask"].numel() == 0
        keep = out.detach() != 0
    ins = [xk] if bk is None else [xk, bk]
    grads = torch.autograd.grad(out, ins, gout.clone())
    return out.detach(), grads[0], (grads[1] if bk is not None else None), keep


def _check_against_ref(x, mask, bias, p, gout, out, dx, dbias, keep):
    dtype = x.dtype
    y = _ref_fwd(x, mask, bias)
    dx_ref = _ref_bwd(y, gout, keep, p)
    errs = {"fwd": _err(out, _ref_out(y, keep, p)), "dx": _err(dx, dx_ref)}
    if bias is not None:
        errs["dbias"] = _bias_err(dbias, dx_ref.sum_to_size(bias.shape))
    print(f"  {tuple(x.shape)} {dtype} p={p}: {errs}")
    assert torch.isfinite(out).all() and torch.isfinite(dx).all()
    assert errs["fwd"] < TOL[dtype], errs
    assert errs["dx"] < 4 * TOL[dtype], errs
    if bias is not None:
        assert errs["dbias"] < 10 * TOL[dtype], errs
    return errs


# ---------------------------------------------------------------------------
# 1. broadcast contract at the real call sites
# ---------------------------------------------------------------------------

L, S = 24, 5  # L = T (keys), S = R (rows of the outer axis): rows get a tail


def _site(name, dtype):
    """(x, mask, bias, expected backward route) shaped like a call site."""
    dev = "cuda"
    if name in ("row_b1", "row_b2"):
        B, H = (1, 4) if name == "row_b1" else (2, 4)
        x = torch.randn(B, H, S, L, L, device=dev, dtype=dtype)
        # the pair bias comes out of a Linear as (B, L, L, H)
        bias = torch.randn(B, L, L, H, device=dev, dtype=dtype)
        bias = bias.permute(0, 3, 1, 2).unsqueeze(2)
        assert not bias.is_contiguous()
        mask = _pad_mask((B, 1, S, 1, L), dtype)
        return x, mask, bias, "fallback"      # bb*bq = H*L = 96 < 512
    if name == "col":
        B, H = 2, 4
        x = torch.randn(B, L, H, S, S, device=dev, dtype=dtype)
        return x, _pad_mask((B, L, 1, 1, S), dtype), None, "plain"
    if name == "tri":
        B, H, R, T = 1, 4, S, L
        x = torch.randn(B, H, R, T, T, device=dev, dtype=dtype)
        bias = torch.randn(B, H, 1, T, T, device=dev, dtype=dtype)
        return x, _pad_mask((B, 1, R, 1, T), dtype), bias, "fallback"
    if name == "bert":
        B, H, q, k = 3, 8, 64, L
        x = torch.randn(B, H, q, k, device=dev, dtype=dtype)
        bias = torch.randn(1, H, q, k, device=dev, dtype=dtype)
        return x, _pad_mask((B, 1, 1, k), dtype), bias, "fused"  # 8*64 = 512
    raise AssertionError(name)


@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("site", ["row_b1", "row_b2", "col", "tri", "bert"])
def test_call_site_broadcasts(spy, site, p, dtype):
    from unicore_amd.modules.softmax_dropout import _broadcast_descr

    torch.manual_seed(20)
    x, mask, bias, route = _site(site, dtype)
    # B = 2 row attention keeps (B, 1, S): two separated dims, eager merge
    merged = _broadcast_descr(tuple(mask.shape[:-2]), x.shape[:-2]) is None
    assert merged == (site == "row_b2")
    gout = torch.randn_like(x)
    out, dx, dbias, keep = _run_module(spy, x, mask, bias, p, gout)
    want = {"fused": (0, 1), "fallback": (1, 0), "plain": (1, 0)}[route]
    assert (spy["bwd"], spy["bwd_bias"]) == want, (route, spy)
    assert spy["fwd"] == 1
    _check_against_ref(x, mask, bias, p, gout, out, dx, dbias, keep)
    # padded keys carry exactly nothing, forward and backward
    dead = (mask.float() < 0).expand_as(x)
    assert (out[dead] == 0).all() and (dx[dead] == 0).all()


# ---------------------------------------------------------------------------
# 2. fused bias-gradient kernel
# ---------------------------------------------------------------------------

# (batch dims, q, k, bias shape, (a, bb, bq, od))
FUSED_CASES = {
    "od3_a1": ((2, 4, 3), 64, 64, (2, 4, 1, 64, 64), (1, 8, 64, 3)),
    "od3_a2_k72": ((2, 8, 3), 64, 72, (1, 8, 1, 64, 72), (2, 8, 64, 3)),
    "bq1": ((2, 512), 4, 24, (1, 512, 1, 24), (2, 512, 1, 1)),
    "bq1_od3": ((2, 512, 3), 4, 24, (1, 512, 1, 1, 24), (2, 512, 1, 3)),
    "nv2_k520": ((2, 8), 64, 520, (1, 8, 64, 520), (2, 8, 64, 1)),
    "nv4_k1032": ((2, 8), 64, 1032, (1, 8, 64, 1032), (2, 8, 64, 1)),
    "nv4_k2048": ((2, 8), 64, 2048, (1, 8, 64, 2048), (2, 8, 64, 1)),
    "rows2100": ((3, 2100), 1, 8, (1, 2100, 1, 8), (3, 2100, 1, 1)),
}

UNSUPPORTED_CASES = {
    "k2056": ((2, 8), 64, 2056, (1, 8, 64, 2056), (2, 8, 64, 1)),
    "rows96_od3_a2": ((2, 4, 3), 24, 24, (1, 4, 1, 24, 24), (2, 4, 24, 3)),
    "bq1_small": ((2, 16), 4, 24, (1, 16, 1, 24), (2, 16, 1, 1)),
}


def _unfused(ops, gout, y, dmask, p, a, bb, bq, od):
    """The shim's fallback on the same inputs: plain backward kernel and the
    eager reduction onto the bias."""
    n, q, k = y.shape
    dx = ops.softmax_dropout_bwd(gout.clone().view(n, q, k), y, dmask, p)
    g = dx.view(a, bb, od, q, k).sum(dim=(0, 2))
    if bq == 1 and q != 1:
        g = g.sum(dim=1, keepdim=True)
    return dx, g


@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("case", list(FUSED_CASES))
def test_fused_bias_grad_kernel(spy, case, p, dtype):
    ops = _kernels()
    batch, q, k, bias_shape, (a, bb, bq, od) = FUSED_CASES[case]
    n = math.prod(batch)
    assert n == a * bb * od
    assert ops.softmax_dropout_bwd_bias_supported(n, q, k, bb, bq, od)
    torch.manual_seed(21)
    x = torch.randn(*batch, q, k, device="cuda", dtype=dtype)
    bias = torch.randn(*bias_shape, device="cuda", dtype=dtype)
    gout = torch.randn_like(x)
    out, dx, dbias, keep = _run_module(spy, x, None, bias, p, gout)
    assert (spy["bwd"], spy["bwd_bias"]) == (0, 1), spy
    _check_against_ref(x, None, bias, p, gout, out, dx, dbias, keep)

    # the unfused route on the same inputs: both kernels do the same per-row
    # math in the same order, so dx is bitwise equal
    dx_u, db_u = _unfused(ops, gout, spy["y"], spy["dmask"], p, a, bb, bq, od)
    assert torch.equal(dx_u.view_as(dx), dx)
    e = _bias_err(db_u.reshape(bias_shape), dbias.double())
    assert e < 10 * TOL[dtype], e


@requires_gpu
@pytest.mark.parametrize("case", ["od3_a1", "bq1"])
def test_fused_bias_grad_kernel_double_run(case):
    ops = _kernels()
    batch, q, k, _, (a, bb, bq, od) = FUSED_CASES[case]
    n = math.prod(batch)
    torch.manual_seed(22)
    g = torch.randn(n, q, k, device="cuda", dtype=BF16)
    x = torch.randn(n, q, k, device="cuda", dtype=BF16)
    torch.manual_seed(23)
    _, dmask, y = ops.softmax_dropout_fwd(True, x, None, 1, None, 1, 0.3)
    r1 = ops.softmax_dropout_bwd_bias(g.clone(), y, dmask, 0.3, bb, bq, od)
    r2 = ops.softmax_dropout_bwd_bias(g.clone(), y, dmask, 0.3, bb, bq, od)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    assert r1[1].shape == (bb * bq, k) and r1[1].dtype == F32


@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("case", list(UNSUPPORTED_CASES))
def test_unsupported_bias_grad_takes_fallback(spy, case, p, dtype):
    ops = _kernels()
    batch, q, k, bias_shape, (a, bb, bq, od) = UNSUPPORTED_CASES[case]
    n = math.prod(batch)
    assert not ops.softmax_dropout_bwd_bias_supported(n, q, k, bb, bq, od)
    torch.manual_seed(24)
    x = torch.randn(*batch, q, k, device="cuda", dtype=dtype)
    bias = torch.randn(*bias_shape, device="cuda", dtype=dtype)
    gout = torch.randn_like(x)
    out, dx, dbias, keep = _run_module(spy, x, None, bias, p, gout)
    assert (spy["bwd"], spy["bwd_bias"]) == (1, 0), spy
    _check_against_ref(x, None, bias, p, gout, out, dx, dbias, keep)


# ---------------------------------------------------------------------------
# 3. tails and grid stride
# ---------------------------------------------------------------------------

# (rows, k): the grid is capped at 2048 blocks of 16 / 8 / 4 rows
# (k <= 512 / <= 1024 / wider) or of one row (block kernel), so the large
# row counts take a second trip, and none is a multiple of the block's rows
TAIL_CASES = [
    (1, 8), (5, 8), (17, 8), (65541, 8),
    (16387, 520), (8195, 1032), (8195, 2056),
    (2051, 13), (7, 770), (2051, 4100),
]
TAIL_PARAMS = [(r, k, BF16) for r, k in TAIL_CASES] + [
    (1, 8, F32), (5, 8, F32), (17, 8, F32), (7, 770, F32)]


@requires_gpu
@pytest.mark.parametrize(
    "rows,k,dtype", TAIL_PARAMS,
    ids=[f"{r}x{k}-{'bf16' if d == BF16 else 'fp32'}" for r, k, d in TAIL_PARAMS])
def test_row_tails_and_grid_stride(rows, k, dtype):
    ops = _kernels()
    torch.manual_seed(30)
    # rows viewed as (n, q = 5) where 5 divides them, with a mask per n and a
    # bias per q, so the broadcast addressing strides along with the rows
    q = 5 if rows % 5 == 0 and rows > 5 else 1
    n = rows // q
    x = torch.randn(n, q, k, device="cuda", dtype=dtype)
    gout = torch.randn_like(x)
    mask = bias = None
    if q == 5:
        mask = torch.randn(n, 1, k, device="cuda", dtype=dtype)
        bias = torch.randn(1, q, k, device="cuda", dtype=dtype)
    y_ref = _ref_fwd(x, mask, bias)
    vec = k % 8 == 0 and k <= 4096
    tail = slice(max(0, n - (32 + q - 1) // q), n)  # covers the last 32 rows

    for p in ([0.0, 0.25] if vec else [0.0]):
        torch.manual_seed(31)
        out, dmask, y = ops.softmax_dropout_fwd(
            True, x.clone(), mask, 1, bias, 1, p)
        keep = None
        if p > 0:
            assert dmask.shape == (n, q, k // 8)
            keep = _unpack(dmask, k)
            if dtype == F32:
                pinv = torch.tensor(1.0 / (1.0 - p), dtype=F32, device="cuda")
                assert torch.equal(out, torch.where(keep, y * pinv, 0.0))
        dx = ops.softmax_dropout_bwd(gout.clone(), y, dmask, p)
        out_ref = _ref_out(y_ref, keep, p)
        dx_ref = _ref_bwd(y_ref, gout, keep, p)
        assert torch.isfinite(out).all() and torch.isfinite(y).all()
        assert torch.isfinite(dx).all()
        e = (_err(y, y_ref), _err(out, out_ref), _err(dx, dx_ref))
        et = (_err(out[tail], out_ref[tail]), _err(dx[tail], dx_ref[tail]))
        print(f"  {rows}x{k} {dtype} p={p}: y/out/dx {e} tail {et}")
        assert e[0] < TOL[dtype] and e[1] < TOL[dtype], e
        assert e[2] < 4 * TOL[dtype], e
        assert et[0] < TOL[dtype] and et[1] < 4 * TOL[dtype], et


@requires_gpu
def test_odd_width_with_dropout_routes_through_torch_dropout():
    """k % 8 != 0 with p > 0: the kernel's dropout needs whole 8-key vectors,
    so the shim runs the block kernel with p = 0 and torch's dropout."""
    _kernels()
    from unicore_amd.modules import softmax_dropout

    torch.manual_seed(32)
    p = 0.25
    x = torch.randn(7, 3, 13, device="cuda", dtype=F32, requires_grad=True)
    out = softmax_dropout(x, p, is_training=True, inplace=False)
    gout = torch.randn_like(out)
    (dx,) = torch.autograd.grad(out, [x], gout.clone())
    keep = out.detach() != 0
    assert 0.5 < keep.float().mean().item() < 0.95
    y = _ref_fwd(x.detach(), None, None)
    assert _err(out.detach(), _ref_out(y, keep, p)) < TOL[F32]
    assert _err(dx, _ref_bwd(y, gout, keep, p)) < 4 * TOL[F32]


# ---------------------------------------------------------------------------
# 4. dropout at NV > 1
# ---------------------------------------------------------------------------

P_DROP = 0.3
P_EFF = math.floor(P_DROP * 65536) / 65536  # the kernel's 16-bit threshold


def _near(frac, expect, nbits, what):
    bound = 5.0 * math.sqrt(expect * (1.0 - expect) / nbits)
    assert abs(frac - expect) <= bound, (what, frac, expect, bound, nbits)


def _agree(a, b, what):
    c = P_EFF ** 2 + (1.0 - P_EFF) ** 2
    _near((a == b).double().mean().item(), c, a.numel(), what)


@requires_gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("rows,k", [(256, 4096), (512, 1032)])
def test_dropout_mask_beyond_first_band(rows, k, dtype):
    ops = _kernels()
    q = 4
    n = rows // q
    torch.manual_seed(40)
    x = torch.randn(n, q, k, device="cuda", dtype=dtype)
    gout = torch.randn_like(x)

    def fwd():
        out, dmask, y = ops.softmax_dropout_fwd(
            True, x.clone(), None, 1, None, 1, P_DROP)
        assert dmask.shape == (n, q, k // 8)
        return out, dmask, y

    torch.manual_seed(41)
    out, dmask, y = fwd()
    out_next, dmask_next, _ = fwd()          # second call under one seed
    torch.manual_seed(41)
    out_again, dmask_again, _ = fwd()
    assert torch.equal(out, out_again) and torch.equal(dmask, dmask_again)

    keep = _unpack(dmask, k).view(rows, k)
    if dtype == F32:
        pinv = torch.tensor(1.0 / (1.0 - P_DROP), dtype=F32, device="cuda")
        assert torch.equal(out, torch.where(keep.view_as(y), y * pinv, 0.0))

    # keep fraction: overall, per 512-column band, per bit position
    _near(keep.double().mean().item(), 1 - P_EFF, keep.numel(), "overall")
    bands = [keep[:, c:c + 512] for c in range(0, k, 512)]
    for i, b in enumerate(bands):
        _near(b.double().mean().item(), 1 - P_EFF, b.numel(), f"band {i}")
    for j in range(8):
        b = keep[:, j::8]
        _near(b.double().mean().item(), 1 - P_EFF, b.numel(), f"bit {j}")

    # independence: bands of one row (compared over their common width),
    # neighbouring rows, consecutive calls
    for i in range(len(bands)):
        for j in range(i + 1, len(bands)):
            w = min(bands[i].shape[1], bands[j].shape[1])
            _agree(bands[i][:, :w], bands[j][:, :w], f"bands {i},{j}")
    _agree(keep[:-1], keep[1:], "rows r, r+1")
    _agree(keep, _unpack(dmask_next, k).view(rows, k), "consecutive calls")
    assert not torch.equal(out, out_next)

    # backward reads the stored mask
    dx = ops.softmax_dropout_bwd(gout.clone(), y, dmask, P_DROP)
    y_ref = _ref_fwd(x, None, None)
    kq = keep.view_as(y)
    assert _err(y, y_ref) < TOL[dtype]
    assert _err(out, _ref_out(y_ref, kq, P_DROP)) < TOL[dtype]
    e = _err(dx, _ref_bwd(y_ref, gout, kq, P_DROP))
    print(f"  {rows}x{k} {dtype}: dx err {e}")
    assert e < 4 * TOL[dtype], e


# ---------------------------------------------------------------------------
# 5. numerical edges
# ---------------------------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("k", [24, 520])
def test_masked_rows(spy, k, dtype):
    torch.manual_seed(50)
    neg = _neg(dtype)
    x = torch.randn(4, 3, k, device="cuda", dtype=dtype)
    mask = torch.zeros(4, 1, k, device="cuda", dtype=dtype)
    mask[0] = neg                     # batch 0: every key padded
    mask[1] = neg
    mask[1, 0, k // 3] = 0            # batch 1: one live key
    mask[2, 0, 1::3] = float("-inf")  # batch 2: some keys at -inf
    mask[2, 0, k - 1] = float("-inf")
    gout = torch.randn_like(x)        # batch 3: no mask at all
    out, dx, _, _ = _run_module(spy, x, mask, None, 0.0, gout)
    _check_against_ref(x, mask, None, 0.0, gout, out, dx, None, None)

    tol = TOL[dtype]
    assert torch.isfinite(out[0]).all()
    assert (out[0].double().sum(-1) - 1).abs().max().item() < tol * k
    assert (out[1, :, k // 3] >= 1 - tol).all()
    dead = torch.isinf(mask[2, 0])
    assert (out[2][:, dead] == 0).all() and (dx[2][:, dead] == 0).all()
    assert (out[2][:, ~dead] > 0).all()


@requires_gpu
@pytest.mark.parametrize("k", [24, 520])
def test_large_logits_fp32(spy, k):
    torch.manual_seed(51)
    x = 30 * torch.randn(4, 3, k, device="cuda", dtype=F32)
    gout = torch.randn_like(x)
    out, dx, _, _ = _run_module(spy, x, None, None, 0.0, gout)
    _check_against_ref(x, None, None, 0.0, gout, out, dx, None, None)


# ---------------------------------------------------------------------------
# 6. aliasing contract
# ---------------------------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_not_inplace_leaves_input_untouched(p):
    _kernels()
    from unicore_amd.modules import softmax_dropout

    torch.manual_seed(60)
    x = torch.randn(3, 5, 72, device="cuda", dtype=BF16)
    mask = _pad_mask((3, 1, 72), BF16)
    before = x.clone()
    out = softmax_dropout(x, p, is_training=True, mask=mask, inplace=False)
    assert torch.equal(x, before)
    assert out.data_ptr() != x.data_ptr()


@requires_gpu
def test_inplace_shares_storage_without_dropout():
    _kernels()
    from unicore_amd.modules import softmax_dropout

    torch.manual_seed(61)
    x = torch.randn(3, 5, 72, device="cuda", dtype=F32)
    y_ref = _ref_fwd(x, None, None)
    out = softmax_dropout(x, 0.0, is_training=True, inplace=True)
    assert out.data_ptr() == x.data_ptr()
    assert _err(out, y_ref) < TOL[F32] and torch.equal(out, x)


@requires_gpu
def test_non_contiguous_input():
    _kernels()
    from unicore_amd.modules import softmax_dropout

    torch.manual_seed(62)
    base = torch.randn(5, 3, 7, 72, device="cuda", dtype=F32)
    x = base.transpose(0, 1)
    assert not x.is_contiguous()
    before = base.clone()
    for inplace in (False, True):
        out = softmax_dropout(x, 0.0, is_training=True, inplace=inplace)
        assert out.shape == x.shape
        assert _err(out, _ref_fwd(before.transpose(0, 1), None, None)) < TOL[F32]
    assert torch.equal(base, before)  # the kernel worked on a contiguous copy


# ---------------------------------------------------------------------------
# 7. bias-major gate (read once per process: checked in a child interpreter)
# ---------------------------------------------------------------------------

_BIASMAJOR_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
from unicore_amd import ops
from unicore_amd.modules import softmax_dropout

assert ops.has_kernels()
dmasks = []
real = ops.softmax_dropout_fwd
def fwd(*a):
    r = real(*a)
    dmasks.append(r[1])
    return r
ops.softmax_dropout_fwd = fwd

def unpack(dmask, k):
    bits = torch.arange(8, device=dmask.device, dtype=torch.int32)
    return ((dmask.to(torch.int32).unsqueeze(-1) >> bits) & 1).bool().reshape(
        *dmask.shape[:-1], k)

for dtype, tol in ((torch.float32, 1e-5), (torch.bfloat16, 8e-3)):
    torch.manual_seed(70)
    x = torch.randn(3, 4, 5, 72, device="cuda", dtype=dtype)
    bias = torch.randn(1, 4, 5, 72, device="cuda", dtype=dtype)
    mask = torch.randn(3, 1, 1, 72, device="cuda", dtype=dtype)
    ref = torch.softmax(
        ((x.float() + mask.float()) + bias.float()).double(), -1)
    out = softmax_dropout(x, 0.0, True, mask=mask, bias=bias, inplace=False)
    err = (out.double() - ref).abs().max().item()
    assert err < tol, ("forward", dtype, err)
    outs = []
    for _ in range(2):
        torch.manual_seed(71)
        outs.append(softmax_dropout(x, 0.3, True, mask=mask, bias=bias,
                                    inplace=False))
    assert torch.equal(outs[0], outs[1]), "same seed, different dropout"
    assert torch.equal(dmasks[-1], dmasks[-2])
    assert dmasks[-1].shape == (12, 5, 9)
    keep = unpack(dmasks[-1], 72).view(x.shape)
    frac = keep.double().mean().item()
    assert 0.6 < frac < 0.8, frac
    err = (outs[0].double() - ref * keep / 0.7).abs().max().item()
    assert err < tol, ("dropout", dtype, err)
print("BIASMAJOR_OK")
"""


@requires_gpu
def test_bias_major_gate_in_child_process():
    """(3,4) x q=5 x k=72 with bias (1,4,5,72), mask (3,1,1,72): 60 rows, no
    multiple of the 16 a block takes, permuted inside the forward kernel."""
    _kernels()
    env = dict(os.environ, UNICORE_SM_BIASMAJOR="1")
    r = subprocess.run(
        [sys.executable, "-c", _BIASMAJOR_CHILD, REPO], env=env, timeout=120,
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "BIASMAJOR_OK" in r.stdout, r.stdout[-2000:]
