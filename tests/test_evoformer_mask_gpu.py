"""GPU tests of the padding-mask kernels and of the masked Evoformer (bf16).

Weighted outer-product-mean entries (csrc/outer_product.hip, ``*_w``).  R is
the float64 contraction weighted in float64, Rabs the same on |operands|,
K the contraction length (S, J*32 or I*32).  Forward, as in test_opm_gpu.py:

    |got - R| <= 2**-8 |R| + K 2**-23 Rabs

The gradient entries multiply every d_o tile by its weight and round the
product to bf16 once more before the MFMA, so every product carries a
relative error of at most 2**-8 on top:

    |got - R| <= 2**-8 |R| + (K 2**-23 + 2**-8) Rabs

Row-masked gated multiply (csrc/gated.hip).  The kernels evaluate in fp32
with the fast exponential; the reference is the float64 expression.  One
rounding to the dtype (relative u = 2**-8 bf16, 2**-11 fp16, 2**-24 fp32,
or, in the subnormal range, half the subnormal spacing: 2**-25 for fp16)
plus the fp32 evaluation: two bias additions, the exponential (argument
error |g| 2**-24 with |g| < 8 here, result error 2 ulp), 1 + e, the
reciprocal and three multiplies, under 32 half-ulps in all; 2**-18 = 64
half-ulps is taken, relative to the product before the (1 - s) factor of dg
(that factor cancels, so its error is absolute in s).  The bias gradients are
fp32 sums of K = rows such values and get the K 2**-23 Rabs summation term
of the contractions above as well.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)

T = 4  # (i, j) pairs a forward block owns per side (OT in the kernel)
EPS = 1e-3

# (B, S, I, J): the shape logic of tests/test_opm_gpu.py
SHAPES = [
    (2, 32, T, T),
    (1, 40, T + 1, 2 * T - 1),
    (1, 13, 3, 5),
    (2, 1, 1, 1),
    (1, 8, 40, 40),
    (1, 100, T + 1, 3),
    (1, 150, 3, T + 1),
]
# random masks everywhere, plus trailing padding as a collater produces it
# and one case with pairs whose normaliser is 0
CASES = [(s, "random") for s in SHAPES] + [
    ((1, 40, T + 1, 2 * T - 1), "trailing"),
    ((1, 13, 3, 5), "zero_norm"),
]
ENTRIES = ["fwd", "bwd_a", "bwd_b"]


def _kernels():
    from unicore_amd import ops

    assert ops.has_kernels(), "HIP extension must be built/loaded on a GPU box"
    return ops


def _randn(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g).to(torch.bfloat16)


def _rand01(*shape, seed=0, keep=0.7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(*shape, device="cuda", generator=g) < keep).float()


def _weight(shape, kind):
    """fp32 (B, I, J) reciprocal normaliser of 0/1 masks: one mask when
    I == J, two independent ones otherwise."""
    B, S, I, J = shape
    if kind == "trailing":
        ma, mb = torch.zeros(B, S, I, device="cuda"), torch.zeros(B, S, J, device="cuda")
        ma[:, : S - 7, : I - 2] = 1
        mb[:, : S - 7, : J - 3] = 1
    else:
        ma = _rand01(B, S, I, seed=21)
        mb = ma if I == J else _rand01(B, S, J, seed=22)
        if kind == "zero_norm":
            ma = ma.clone()
            ma[:, :, 0] = 0
    norm = torch.einsum("bsi,bsj->bij", ma, mb)
    if kind != "random":
        assert bool((norm == 0).any())
    return (1.0 / (EPS + norm)).contiguous()


def _contract(entry, a, b, d_o, w):
    if entry == "fwd":
        return torch.einsum("bsic,bsjd->bijcd", a, b) * w[..., None, None]
    dw = d_o * w[..., None, None]
    if entry == "bwd_a":
        return torch.einsum("bijcd,bsjd->bsic", dw, b)
    return torch.einsum("bijcd,bsic->bsjd", dw, a)


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """Operands, weight and the float64 references of all three entries;
    computed once per case and never modified."""
    B, S, I, J = shape
    a, b = _randn(B, S, I, 32, seed=1), _randn(B, S, J, 32, seed=2)
    d_o = _randn(B, I, J, 32, 32, seed=3)
    w = _weight(shape, kind)
    a64, b64, d64, w64 = a.double(), b.double(), d_o.double(), w.double()
    ref = {e: (_contract(e, a64, b64, d64, w64),
               _contract(e, a64.abs(), b64.abs(), d64.abs(), w64)) for e in ENTRIES}
    return a, b, d_o, w, ref


def _klen(entry, shape):
    B, S, I, J = shape
    return {"fwd": S, "bwd_a": J * 32, "bwd_b": I * 32}[entry]


def _check_bound(got, R, Rabs, K, backward, what=""):
    err = (got.double() - R).abs()
    extra = 2.0 ** -8 if backward else 0.0
    bound = 2.0 ** -8 * R.abs() + (K * 2.0 ** -23 + extra) * Rabs
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.4e}, max(err - bound) {worst:.4e}")
    assert bool((err <= bound).all()), (what, worst)


@requires_gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_opm_weighted_entry_parity(case, entry):
    ops = _kernels()
    shape, kind = case
    B, S, I, J = shape
    a, b, d_o, w, ref = _case(shape, kind)

    def call():
        if entry == "fwd":
            return ops.opm_fwd_w(a, b, w), (B, I, J, 32, 32)
        if entry == "bwd_a":
            return ops.opm_bwd_a_w(d_o, b, w), (B, S, I, 32)
        return ops.opm_bwd_b_w(d_o, a, w), (B, S, J, 32)

    got, want_shape = call()
    assert got.shape == want_shape and got.dtype == torch.bfloat16
    assert got.is_contiguous()
    R, Rabs = ref[entry]
    _check_bound(got, R, Rabs, _klen(entry, shape), entry != "fwd",
                 f"{entry}_w {shape} {kind}")
    assert torch.equal(call()[0], got)  # bitwise reproducible


@requires_gpu
def test_opm_weighted_constant_weight_is_the_scaled_entry():
    """w == scale everywhere: the forward is bitwise the unweighted entry
    (same accumulation, same fp32 multiply)."""
    ops = _kernels()
    a, b, d_o, _, _ = _case((1, 40, T + 1, 2 * T - 1), "random")
    w = torch.full((1, T + 1, 2 * T - 1), 1.0 / 40, device="cuda")
    assert torch.equal(ops.opm_fwd_w(a, b, w), ops.opm_fwd(a, b, 1.0 / 40))
    # a power of two survives the extra bf16 rounding of the gradients
    w = torch.full_like(w, 0.25)
    assert torch.equal(ops.opm_bwd_a_w(d_o, b, w), ops.opm_bwd_a(d_o, b, 0.25))
    assert torch.equal(ops.opm_bwd_b_w(d_o, a, w), ops.opm_bwd_b(d_o, a, 0.25))


@requires_gpu
def test_opm_weighted_host_checks():
    ops = _kernels()
    a, b, d_o, w, _ = _case((1, 13, 3, 5), "random")
    calls = [lambda w: ops.opm_fwd_w(a, b, w),
             lambda w: ops.opm_bwd_a_w(d_o, b, w),
             lambda w: ops.opm_bwd_b_w(d_o, a, w)]
    for call in calls:
        call(w)
        with pytest.raises(RuntimeError, match=r"must be \(B, I, J\)"):
            call(w.transpose(1, 2).contiguous())
        with pytest.raises(RuntimeError, match=r"must be \(B, I, J\)"):
            call(w[0])
        with pytest.raises(RuntimeError, match="must be fp32"):
            call(w.to(torch.bfloat16))
        with pytest.raises(RuntimeError, match="must be contiguous"):
            call(torch.empty(1, 5, 3, device="cuda").transpose(1, 2))
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call(w.cpu())
    with pytest.raises(RuntimeError, match="must agree in B and S"):
        ops.opm_fwd_w(a, _randn(1, 12, 5, 32), w)
    with pytest.raises(RuntimeError, match="must be bf16"):
        ops.opm_fwd_w(a.float(), b.float(), w)


AG_SHAPE = (1, 40, 9, 9)


@functools.lru_cache(maxsize=None)
def _autograd_case():
    from unicore_amd.modules.outer_product import _eager_masked, opm_mask_inv_norm

    B, S, I, J = AG_SHAPE
    a, b = _randn(B, S, I, 32, seed=4), _randn(B, S, J, 32, seed=5)
    d_out = _randn(B, I, J, 1024, seed=6)
    mask = torch.zeros(B, S, I, device="cuda")
    mask[:, :31, :7] = 1  # trailing padding
    mask[:, 3, 2] = 0
    # the masked eager expression in float64, under autograd
    a64, b64 = a.double().requires_grad_(), b.double().requires_grad_()
    m64 = mask.double()
    o64 = _eager_masked(a64, b64, m64, opm_mask_inv_norm(m64))
    assert o64.dtype == torch.float64
    o64.backward(d_out.double())
    w64 = opm_mask_inv_norm(m64)
    am, bm = a.double().abs() * m64[..., None], b.double().abs() * m64[..., None]
    d5 = d_out.double().abs().view(B, I, J, 32, 32)
    absr = {e: _contract(e, am, bm, d5, w64) for e in ENTRIES}
    absr["fwd"] = absr["fwd"].reshape(B, I, J, 1024)
    absr["bwd_a"] = absr["bwd_a"] * m64[..., None]
    absr["bwd_b"] = absr["bwd_b"] * m64[..., None]
    return a, b, d_out, mask.to(torch.bfloat16), o64.detach(), a64.grad, b64.grad, absr


@requires_gpu
@pytest.mark.parametrize("fused", ["1", "0"])
def test_outer_product_mean_masked_autograd(monkeypatch, fused):
    """outer_product_mean(mask=) against the masked eager expression on the
    same bf16 inputs; with the gate off the fallback is taken and agrees."""
    from unicore_amd import ops
    from unicore_amd.modules import outer_product_mean

    _kernels()
    monkeypatch.setenv("UNICORE_OPM_FUSED", fused)
    calls = {"opm_fwd_w": 0, "opm_bwd_a_w": 0, "opm_bwd_b_w": 0}

    def spy(name):
        real = getattr(ops, name)

        def wrapped(*args):
            calls[name] += 1
            return real(*args)

        monkeypatch.setattr(ops, name, wrapped)

    for name in calls:
        spy(name)
    a, b, d_out, mask, o64, da64, db64, absr = _autograd_case()
    B, S, I, J = AG_SHAPE
    a1 = a.detach().clone().requires_grad_()
    b1 = b.detach().clone().requires_grad_()
    o = outer_product_mean(a1, b1, mask=mask)
    o.backward(d_out)
    n = 1 if fused == "1" else 0
    assert calls == {"opm_fwd_w": n, "opm_bwd_a_w": n, "opm_bwd_b_w": n}, calls
    assert o.shape == (B, I, J, 1024) and o.dtype == torch.bfloat16
    assert a1.grad.shape == a.shape and b1.grad.shape == b.shape
    back = fused == "1"  # the fallback computes in fp32 and rounds once
    _check_bound(o.detach(), o64, absr["fwd"], S, False, "masked out")
    _check_bound(a1.grad, da64, absr["bwd_a"], J * 32, back, "masked da")
    _check_bound(b1.grad, db64, absr["bwd_b"], I * 32, back, "masked db")
    # padded rows and residues get no gradient and give no output
    assert bool((a1.grad[mask == 0] == 0).all())
    assert bool((b1.grad[mask == 0] == 0).all())
    assert bool((o.detach()[:, 7:] == 0).all()) and bool((o.detach()[:, :, 7:] == 0).all())


# ---------------------------------------------------------------------------
# row-masked gated multiply
# ---------------------------------------------------------------------------
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
# half the spacing of the dtype's subnormals: the floor of one rounding
TINY = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25,
        torch.float32: 2.0 ** -150}
EVAL = 2.0 ** -18  # fp32 evaluation, see the module docstring

# (leading shape, C, biases)
GATED_CASES = [((3, 5), 64, True), ((1,), 8, True), ((130,), 128, True),
               ((3, 5), 64, False)]


@functools.lru_cache(maxsize=None)
def _gated_case(lead, C, dtype):
    g = torch.Generator(device="cuda").manual_seed(31)

    def rn(*s):
        return torch.randn(*s, device="cuda", generator=g).to(dtype)

    x, gt, G = rn(*lead, C), rn(*lead, C), rn(*lead, C)
    bx, bg = rn(C), rn(C)
    m = (torch.rand(*lead, device="cuda", generator=g) < 0.6).to(dtype)
    if m.numel() > 1:
        m.view(-1)[0], m.view(-1)[-1] = 1, 0
    return x, gt, G, bx, bg, m


def _run_gated(x, gt, G, bx, bg, m):
    from unicore_amd.modules import gated_mul

    leaves = [t.detach().clone().requires_grad_() if t is not None else None
              for t in (x, gt, bx, bg)]
    out = gated_mul(*leaves, row_mask=m)
    out.backward(G)
    return [out.detach()] + [t.grad if t is not None else None for t in leaves]


def _within(got, R, scale, u, K=0, what=""):
    err = (got.double() - R).abs()
    bound = (u * R.abs()).clamp_min(TINY[got.dtype]) + (EVAL + K * 2.0 ** -23) * scale
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.4e}, max(err - bound) {worst:.4e}")
    assert bool((err <= bound).all()), (what, worst)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32],
                         ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("case", GATED_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_gated_mul_row_mask(monkeypatch, case, dtype):
    from unicore_amd import ops

    _kernels()
    lead, C, biased = case
    x, gt, G, bx, bg, m = _gated_case(lead, C, dtype)
    if not biased:
        bx = bg = None
    hit = {"fwd": 0, "bwd": 0}
    real_f, real_b = ops.gated_mul_masked_fwd, ops.gated_mul_masked_bwd
    monkeypatch.setattr(ops, "gated_mul_masked_fwd",
                        lambda *a: (hit.__setitem__("fwd", hit["fwd"] + 1), real_f(*a))[1])
    monkeypatch.setattr(ops, "gated_mul_masked_bwd",
                        lambda *a: (hit.__setitem__("bwd", hit["bwd"] + 1), real_b(*a))[1])
    out, dx, dg, dbx, dbg = _run_gated(x, gt, G, bx, bg, m)
    assert hit == {"fwd": 1, "bwd": 1}, hit
    assert out.dtype == dx.dtype == dg.dtype == dtype
    assert out.shape == dx.shape == dg.shape == x.shape

    u = U[dtype]
    m64 = m.double()[..., None]
    xb = x.double() + (bx.double() if biased else 0)
    s = torch.sigmoid(gt.double() + (bg.double() if biased else 0))
    R_out, R_dx = xb * s * m64, G.double() * s * m64
    pre_dg = G.double() * xb * s * m64  # dg before the cancelling (1 - s)
    R_dg = pre_dg * (1 - s)
    tag = f"{lead}x{C} {dtype}"
    _within(out, R_out, R_out.abs(), u, what=f"out {tag}")
    _within(dx, R_dx, R_dx.abs(), u, what=f"dx {tag}")
    _within(dg, R_dg, pre_dg.abs(), u, what=f"dg {tag}")
    rows = m.numel()
    if biased:
        flat = lambda t: t.reshape(rows, C)  # noqa: E731
        assert dbx.shape == dbg.shape == (C,) and dbx.dtype == dtype
        _within(dbx, flat(R_dx).sum(0), flat(R_dx).abs().sum(0), u, K=rows,
                what=f"dbx {tag}")
        _within(dbg, flat(R_dg).sum(0), flat(pre_dg).abs().sum(0), u, K=rows,
                what=f"dbg {tag}")
    # masked rows are exactly 0
    dead = m == 0
    for t in (out, dx, dg):
        assert bool((t[dead] == 0).all())
    # bitwise reproducible
    for p, q in zip(_run_gated(x, gt, G, bx, bg, m), (out, dx, dg, dbx, dbg)):
        assert (p is None and q is None) or torch.equal(p, q)
    # m == 1 is the existing gated_mul, bitwise
    ones = torch.ones_like(m)
    for p, q in zip(_run_gated(x, gt, G, bx, bg, ones),
                    _run_gated(x, gt, G, bx, bg, None)):
        assert (p is None and q is None) or torch.equal(p, q)


@requires_gpu
def test_gated_mul_row_mask_host_checks_and_fallback():
    from unicore_amd.modules import gated_mul

    ops = _kernels()
    x, gt, G, bx, bg, m = _gated_case((3, 5), 64, torch.bfloat16)
    with pytest.raises(RuntimeError, match="row_mask"):
        ops.gated_mul_masked_fwd(x, gt, bx, bg, m.float())
    with pytest.raises(RuntimeError, match="row_mask"):
        ops.gated_mul_masked_fwd(x, gt, bx, bg, m.reshape(-1)[:-1])
    with pytest.raises(RuntimeError, match="row_mask"):
        ops.gated_mul_masked_bwd(G, x, gt, bx, bg, m.reshape(-1)[:-1])
    # a channel dim that is no multiple of 8 takes the eager expression
    x4, g4 = x[..., :4].contiguous(), gt[..., :4].contiguous()
    assert x4.numel() % 8 != 0 or x4.shape[-1] % 8 != 0
    want = x4 * torch.sigmoid(g4) * m[..., None]
    assert torch.equal(gated_mul(x4, g4, row_mask=m), want)


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
EVO_ARGV = [
    "--task", "evoformer_synthetic",
    "--arch", "evoformer",
    "--loss", "masked_msa",
    "--optimizer", "adam",
    "--lr-scheduler", "fixed",
    "--lr", "1e-3",
    "--batch-size", "2",
    "--dataset-size", "8",
    "--msa-depth", "6",
    "--residues", "16",
    "--evo-layers", "2",
    "--msa-dim", "64",
    "--pair-dim", "64",
    "--evo-heads", "4",
    "--tri-attn-heads", "4",
    "--triangle-attention",
    "--bf16",
    "--log-format", "none",
    "--num-workers", "0",
]


def _parse(extra):
    from unicore_amd import options

    parser = options.get_training_parser()
    args = options.parse_args_and_arch(parser, input_args=EVO_ARGV + list(extra))
    args.distributed_world_size = 1
    args.distributed_rank = 0
    args.device_id = 0
    args.distributed_no_spawn = True
    return args


def _model(extra):
    from unicore_amd import tasks

    args = _parse(["--dropout", "0.0"] + list(extra))
    task = tasks.setup_task(args)
    torch.manual_seed(11)
    return task.build_model(args).cuda().to(torch.bfloat16).eval()


@requires_gpu
def test_padding_invariance_gpu(monkeypatch):
    """Folded chain, bf16, fused gates on: the valid logits of the padded
    (2, 6, 16) batch against the (6, 16) and (4, 9) samples run alone.

    Different shapes take different tilings, so the yardstick is this
    model's own bf16 noise: the spread of the unmasked model between
    UNICORE_FOLD_BIAS=1 and 0, on the two samples run alone, i.e. over
    exactly the elements that are compared.  Allowed: twice that spread.

    Two statistics over the 8448 compared logits.  The maximum is an
    extreme value of the output's bf16 quantisation (the spread below is one
    ulp of a logit in [2, 4)); the root mean square is the size of the
    typical element.  The masked model must be inside the allowance in both.
    The flag-off leak is systematic, not a tail, and lives in the padded
    sample alone (nothing can leak into the full-size one), so it is taken
    as the rms over the (4, 9) sample and must be at least 10x the rms
    allowance.

    Measured on an MI355X: spread max 1.5625e-02 / rms 2.9227e-03; masked
    difference max 7.8125e-03 / rms 1.3367e-03 (0.25x / 0.23x the
    allowance); flag-off leak rms 8.4609e-02, 14.5x the allowance (its
    maximum, 2.9492e-01, is 9.4x the maximum allowance)."""
    _kernels()
    monkeypatch.setenv("UNICORE_OPM_FUSED", "1")
    monkeypatch.setenv("UNICORE_TRIATTN_FUSED", "1")
    shapes = ((6, 16), (4, 9))
    g = torch.Generator().manual_seed(3)
    alone = [torch.randint(5, 20, (1, s, l), generator=g).cuda() for s, l in shapes]
    masked, plain = _model(["--msa-padding-mask"]), _model([])
    batch = torch.full((2, 6, 16), masked.padding_idx, dtype=torch.long, device="cuda")
    for i, t in enumerate(alone):
        batch[i, : t.shape[1], : t.shape[2]] = t[0]

    def run_alone(model):
        with torch.no_grad():
            return [model(t)[0].float() for t in alone]

    def diffs(model):
        """Per sample: alone minus the same positions of the padded batch."""
        with torch.no_grad():
            padded = model(batch).float()
        return [a - padded[i, : a.shape[0], : a.shape[1]]
                for i, a in enumerate(run_alone(model))]

    def stat(ds):
        d = torch.cat([x.reshape(-1) for x in ds])
        return d.abs().max().item(), d.pow(2).mean().sqrt().item()

    monkeypatch.setenv("UNICORE_FOLD_BIAS", "1")
    folded = run_alone(plain)
    m_max, m_rms = stat(diffs(masked))
    leak = diffs(plain)
    l_max, l_rms = stat(leak[1:])  # the padded sample
    monkeypatch.setenv("UNICORE_FOLD_BIAS", "0")
    s_max, s_rms = stat([a - b for a, b in zip(run_alone(plain), folded)])
    print(f"spread max {s_max:.4e} rms {s_rms:.4e} | masked max {m_max:.4e} "
          f"rms {m_rms:.4e} | leak max {l_max:.4e} rms {l_rms:.4e}")
    assert s_max > 0 and s_rms > 0
    assert m_max <= 2 * s_max, (m_max, s_max)
    assert m_rms <= 2 * s_rms, (m_rms, s_rms)
    assert l_rms >= 10 * 2 * s_rms, (l_rms, s_rms)


@requires_gpu
def test_training_step_with_ragged_batches():
    """One repeated padded batch, shared dropout on: the loss is finite and
    lower after 5 steps.  Attention dropout is off: its fused kernel takes
    key lengths that are multiples of 8 only, which ragged batches are not."""
    from unicore_amd import tasks
    from unicore_amd.trainer import Trainer

    args = _parse(["--msa-padding-mask", "--min-residues", "8",
                   "--min-msa-depth", "3", "--msa-dropout", "0.15",
                   "--pair-dropout", "0.25", "--dropout", "0.0",
                   "--seed", "5"])
    torch.manual_seed(args.seed)
    task = tasks.setup_task(args)
    task.load_dataset("train")
    model = task.build_model(args)
    loss = task.build_loss(args)
    trainer = Trainer(args, task, model, loss)
    epoch_itr = trainer.get_train_iterator(epoch=1)
    trainer.init_total_train_steps(epoch_itr)
    pad = task.dictionary.pad()
    # the first batch in which the two samples drew different shapes
    sample = next(s for s in epoch_itr.next_epoch_itr(shuffle=False)
                  if bool(s["net_input"]["src_tokens"].eq(pad).any()))
    losses = [float(trainer.train_step([sample])["loss"]) for _ in range(5)]
    print("losses", losses)
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
