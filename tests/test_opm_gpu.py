"""GPU tests of the outer-product-mean contractions (csrc/outer_product.hip)
and modules.outer_product_mean.

Tolerance (derived, not measured).  R is the float64 contraction, Rabs the
same contraction on |operands|, K the contraction length of the entry
(S, J*32 or I*32).  Every element must satisfy

    |got - R| <= 2**-8 * |R| + K * 2**-23 * Rabs

The first term is one bf16 rounding.  Products of two bf16 values are exact
in fp32, so the only other error is fp32 summation: first order
(K - 1) * 2**-24 * Rabs in any order; the second term is twice that and
also covers the fp32 scale multiply.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)

T = 4  # (i, j) pairs a forward block owns per side (OT in the kernel)

# (B, S, I, J)
SHAPES = [
    (2, 32, T, T),              # exactly one tile and one k-step
    (1, 40, T + 1, 2 * T - 1),  # ragged in every direction
    (1, 13, 3, 5),              # odd S, smaller than a tile
    (2, 1, 1, 1),               # degenerate
    (1, 8, 40, 40),             # long K = 1280 for the gradients
    # the forward steps s by 64, a gradient block owns 128 s:
    (1, 100, T + 1, 3),         # two forward steps, the second ragged
    (1, 150, 3, T + 1),         # three forward steps; two gradient s chunks
]
# scale = 1/S everywhere, plus one case with scale = 1.0
CASES = [(s, None) for s in SHAPES] + [((1, 40, T + 1, 2 * T - 1), 1.0)]
ENTRIES = ["fwd", "bwd_a", "bwd_b"]


def _kernels():
    from unicore_amd import ops

    assert ops.has_kernels(), "HIP extension must be built/loaded on a GPU box"
    return ops


def _randn(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g).to(torch.bfloat16)


def _contract(entry, a, b, d_o):
    if entry == "fwd":
        return torch.einsum("bsic,bsjd->bijcd", a, b)
    if entry == "bwd_a":
        return torch.einsum("bijcd,bsjd->bsic", d_o, b)
    return torch.einsum("bijcd,bsic->bsjd", d_o, a)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Operands and the unscaled float64 references of all three entries;
    computed once per shape and never modified."""
    B, S, I, J = shape
    a, b = _randn(B, S, I, 32, seed=1), _randn(B, S, J, 32, seed=2)
    d_o = _randn(B, I, J, 32, 32, seed=3)
    a64, b64, d64 = a.double(), b.double(), d_o.double()
    ref = {e: (_contract(e, a64, b64, d64),
               _contract(e, a64.abs(), b64.abs(), d64.abs())) for e in ENTRIES}
    return a, b, d_o, ref


def _klen(entry, shape):
    B, S, I, J = shape
    return {"fwd": S, "bwd_a": J * 32, "bwd_b": I * 32}[entry]


def _check_bound(got, R, Rabs, K, what=""):
    err = (got.double() - R).abs()
    bound = 2.0 ** -8 * R.abs() + K * 2.0 ** -23 * Rabs
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.4e}, max(err - bound) {worst:.4e}")
    assert bool((err <= bound).all()), (what, worst)


@requires_gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_opm_entry_parity(case, entry):
    ops = _kernels()
    shape, scale = case
    B, S, I, J = shape
    if scale is None:
        scale = 1.0 / S
    a, b, d_o, ref = _case(shape)
    if entry == "fwd":
        got, want_shape = ops.opm_fwd(a, b, scale), (B, I, J, 32, 32)
    elif entry == "bwd_a":
        got, want_shape = ops.opm_bwd_a(d_o, b, scale), (B, S, I, 32)
    else:
        got, want_shape = ops.opm_bwd_b(d_o, a, scale), (B, S, J, 32)
    assert got.shape == want_shape and got.dtype == torch.bfloat16
    assert got.is_contiguous()
    R, Rabs = ref[entry]
    _check_bound(got, R * scale, Rabs * scale, _klen(entry, shape),
                 f"{entry} {shape}")


def _fused_on(monkeypatch):
    monkeypatch.setenv("UNICORE_OPM_FUSED", "1")


def _eager(a, b):
    o = torch.einsum("bsic,bsjd->bijcd", a.float(), b.float()) / a.shape[1]
    return o.reshape(*o.shape[:3], a.shape[-1] * b.shape[-1]).to(a.dtype)


def _run_opm(a, b, d_out):
    from unicore_amd.modules import outer_product_mean

    a = a.detach().clone().requires_grad_()
    b = b.detach().clone().requires_grad_()
    o = outer_product_mean(a, b)
    o.backward(d_out)
    return o.detach(), a.grad, b.grad


AG_SHAPE = (2, 24, 20, 20)


@functools.lru_cache(maxsize=None)
def _autograd_case():
    B, S, I, J = AG_SHAPE
    a, b = _randn(B, S, I, 32, seed=4), _randn(B, S, J, 32, seed=5)
    d_out = _randn(B, I, J, 1024, seed=6)
    # the fp32 eager expression under autograd
    af, bf = a.float().requires_grad_(), b.float().requires_grad_()
    of = torch.einsum("bsic,bsjd->bijcd", af, bf) / S
    of = of.reshape(*of.shape[:3], 1024)
    of.backward(d_out.float())
    d5 = d_out.double().abs().view(B, I, J, 32, 32)
    absr = {e: _contract(e, a.double().abs(), b.double().abs(), d5) / S
            for e in ENTRIES}
    absr["fwd"] = absr["fwd"].reshape(B, I, J, 1024)
    return a, b, d_out, of.detach(), af.grad, bf.grad, absr


@requires_gpu
@pytest.mark.parametrize("dout_view", [False, True])
def test_outer_product_mean_autograd(monkeypatch, dout_view):
    _kernels()
    _fused_on(monkeypatch)
    a, b, d_out, of, daf, dbf, absr = _autograd_case()
    if dout_view:
        d_in = d_out.transpose(1, 2).contiguous().transpose(1, 2)
        assert not d_in.is_contiguous() and torch.equal(d_in, d_out)
    else:
        d_in = d_out
    o, da, db = _run_opm(a, b, d_in)
    B, S, I, J = AG_SHAPE
    assert o.shape == (B, I, J, 1024) and o.dtype == torch.bfloat16
    assert da.is_contiguous() and db.is_contiguous()
    assert da.shape == a.shape and db.shape == b.shape
    _check_bound(o, of.double(), absr["fwd"], S, "autograd out")
    _check_bound(da, daf.double(), absr["bwd_a"], J * 32, "autograd da")
    _check_bound(db, dbf.double(), absr["bwd_b"], I * 32, "autograd db")


@requires_gpu
def test_outer_product_mean_needs_input_grad(monkeypatch):
    from unicore_amd.modules import outer_product_mean

    _kernels()
    _fused_on(monkeypatch)
    a, b, d_out, _, _, _, _ = _autograd_case()
    full = _run_opm(a, b, d_out)
    a1 = a.detach().clone().requires_grad_()
    outer_product_mean(a1, b).backward(d_out)
    assert torch.equal(a1.grad, full[1])
    b1 = b.detach().clone().requires_grad_()
    outer_product_mean(a, b1).backward(d_out)
    assert torch.equal(b1.grad, full[2])


@requires_gpu
def test_outer_product_mean_deterministic(monkeypatch):
    _kernels()
    _fused_on(monkeypatch)
    a, b, d_out, _, _, _, _ = _autograd_case()
    r1 = _run_opm(a, b, d_out)
    r2 = _run_opm(a, b, d_out)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)


@requires_gpu
def test_outer_product_mean_no_activation_sized_temporaries(monkeypatch):
    from unicore_amd.modules import outer_product_mean

    _kernels()
    _fused_on(monkeypatch)
    a, b = _randn(1, 32, 48, 32, seed=7), _randn(1, 32, 48, 32, seed=8)
    with torch.no_grad():
        outer_product_mean(a, b)  # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        o = outer_product_mean(a, b)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    out_bytes = o.numel() * o.element_size()
    # the eager path needs >= 6x (fp32 GEMM result, permuted copy, division)
    assert rise < 1.5 * out_bytes, (rise, out_bytes)


@requires_gpu
def test_outer_product_mean_fallback_and_host_checks(monkeypatch):
    from unicore_amd.modules import outer_product_mean

    ops = _kernels()
    _fused_on(monkeypatch)
    # fp32 inputs
    a32, b32 = _randn(1, 6, 5, 32, seed=9).float(), _randn(1, 6, 5, 32, seed=10).float()
    assert torch.equal(outer_product_mean(a32, b32), _eager(a32, b32))
    # c = 16
    a16, b16 = _randn(1, 6, 5, 16, seed=11), _randn(1, 6, 5, 16, seed=12)
    o16 = outer_product_mean(a16, b16)
    assert o16.shape == (1, 5, 5, 256) and torch.equal(o16, _eager(a16, b16))
    # non-contiguous operands (channel slices of a wider projection)
    wide = _randn(1, 6, 5, 64, seed=13)
    an, bn = wide[..., :32], wide[..., 32:]
    assert not an.is_contiguous() and not bn.is_contiguous()
    assert torch.equal(outer_product_mean(an, bn), _eager(an, bn))
    assert torch.equal(outer_product_mean(an, bn.contiguous()),
                       _eager(an, bn.contiguous()))
    # host checks of the raw entry
    with pytest.raises(RuntimeError, match="must agree in B and S"):
        ops.opm_fwd(_randn(1, 6, 5, 32), _randn(1, 7, 5, 32), 1.0)
    with pytest.raises(RuntimeError, match="only width 32 is supported"):
        ops.opm_fwd(a16, b16, 1.0)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        ops.opm_fwd(an, bn, 1.0)
    with pytest.raises(RuntimeError, match="must be bf16"):
        ops.opm_fwd(a32, b32, 1.0)
    d_o = _randn(1, 5, 5, 32, 32, seed=14)
    with pytest.raises(RuntimeError, match="must agree in B and J"):
        ops.opm_bwd_a(d_o, _randn(1, 6, 4, 32), 1.0)
    with pytest.raises(RuntimeError, match="must agree in B and I"):
        ops.opm_bwd_b(d_o, _randn(1, 6, 4, 32), 1.0)
    with pytest.raises(RuntimeError, match="only width 32 is supported"):
        ops.opm_bwd_a(_randn(1, 5, 5, 32, 16), _randn(1, 6, 5, 32), 1.0)
    mis = _randn(6 * 5 * 32 + 4)[4:].view(1, 6, 5, 32)
    assert mis.is_contiguous() and mis.data_ptr() % 16 == 8
    with pytest.raises(RuntimeError, match="not 16-byte aligned"):
        ops.opm_fwd(mis, mis, 1.0)
    # the wrapper takes the eager expression for a misaligned operand
    assert torch.equal(outer_product_mean(mis, mis), _eager(mis, mis))


@requires_gpu
def test_outer_product_mean_misaligned_d_out(monkeypatch):
    """A contiguous d_out that is not 16 B aligned is copied, not rejected."""
    _kernels()
    _fused_on(monkeypatch)
    a, b, d_out, _, _, _, _ = _autograd_case()
    want = _run_opm(a, b, d_out)
    buf = torch.empty(d_out.numel() + 4, device="cuda", dtype=d_out.dtype)
    d_mis = buf[4:].view(d_out.shape)
    d_mis.copy_(d_out)
    assert d_mis.is_contiguous() and d_mis.data_ptr() % 16 == 8
    got = _run_opm(a, b, d_mis)
    for x, y in zip(got, want):
        assert torch.equal(x, y)


@requires_gpu
def test_outer_product_mean_module_vs_fp32(monkeypatch):
    """max|F-R| <= 2 max|E-R| + 1e-6 for output and every gradient: F fused
    bf16, E eager bf16, R fp32 eager copy. Both bf16 runs differ from fp32
    by rounding noise of the same size; 2 covers two independent one-ulp
    noises adding."""
    import copy

    from unicore_amd.models.evoformer import OuterProductMean

    _kernels()
    torch.manual_seed(16)
    ref = OuterProductMean(d_msa=64, d_pair=64).cuda()
    mod = copy.deepcopy(ref).to(torch.bfloat16)
    x = _randn(1, 16, 24, 64, seed=17)
    d_out = _randn(1, 24, 24, 64, seed=18)

    def run(m, inp, dout):
        m.zero_grad(set_to_none=True)
        inp = inp.detach().clone().requires_grad_()
        out = m(inp)
        out.backward(dout)
        res = {"out": out.detach().float(), "d_in": inp.grad.float()}
        for n, p in m.named_parameters():
            res["d_" + n] = p.grad.detach().float()
        return res

    # count the kernel entries: F must take them, E must not
    from unicore_amd import ops

    calls = {"opm_fwd": 0, "opm_bwd_a": 0, "opm_bwd_b": 0}

    def spy(name):
        real = getattr(ops, name)

        def wrapped(*args):
            calls[name] += 1
            return real(*args)

        monkeypatch.setattr(ops, name, wrapped)

    for name in calls:
        spy(name)
    monkeypatch.setenv("UNICORE_OPM_FUSED", "1")
    Fr = run(mod, x, d_out)
    assert calls == {"opm_fwd": 1, "opm_bwd_a": 1, "opm_bwd_b": 1}, calls
    monkeypatch.setenv("UNICORE_OPM_FUSED", "0")
    Er = run(mod, x, d_out)
    assert calls == {"opm_fwd": 1, "opm_bwd_a": 1, "opm_bwd_b": 1}, calls
    Rr = run(ref, x.float(), d_out.float())
    assert set(Fr) == set(Er) == set(Rr)
    for k in Rr:
        f = (Fr[k] - Rr[k]).abs().max().item()
        e = (Er[k] - Rr[k]).abs().max().item()
        print(f"{k}: max|F-R|={f:.4e} max|E-R|={e:.4e}")
        assert f <= 2 * e + 1e-6, (k, f, e)
