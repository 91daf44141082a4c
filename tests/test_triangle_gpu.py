"""GPU tests of the channel-last triangle contraction (csrc/triangle.hip)
and modules.triangle_multiply.

Tolerance (derived, not measured): one correct bf16 rounding of an fp32 sum
is within 2**-8 relative; the fp32 reorder error at Z <= 72 is orders of
magnitude below atol. The fp32 reference rounded to bf16 passes by
construction.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)

RTOL, ATOL = 2.0 ** -7, 1e-3

# (Bt, X, Y, Z, C)
CONFIGS = [
    (2, 16, 16, 32, 64),    # exactly one tile and one z-step
    (1, 24, 40, 72, 64),    # ragged x, y, z; three z-steps
    (2, 1, 1, 1, 32),       # degenerate
    (1, 33, 17, 8, 128),    # tile boundary + 1, several channel chunks
]

EQ = {True: "bikc,bjkc->bijc", False: "bkic,bkjc->bijc"}


def _kernels():
    from unicore_amd import ops

    assert ops.has_kernels(), "HIP extension must be built/loaded on a GPU box"
    return ops


def _randn(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g).to(torch.bfloat16)


def _ref(a, b):
    return torch.einsum("bxzc,byzc->bxyc", a.float(), b.float())


def _close(got, ref):
    torch.testing.assert_close(got.float(), ref.float(), rtol=RTOL, atol=ATOL)


@requires_gpu
@pytest.mark.parametrize("cfg", CONFIGS)
def test_tri_contract_parity(cfg):
    ops = _kernels()
    Bt, X, Y, Z, C = cfg
    a, b = _randn(Bt, X, Z, C, seed=1), _randn(Bt, Y, Z, C, seed=2)
    o = ops.tri_contract(a, b)
    assert o.shape == (Bt, X, Y, C) and o.dtype == torch.bfloat16
    assert o.is_contiguous()
    _close(o, _ref(a, b))


@requires_gpu
@pytest.mark.parametrize("cfg", CONFIGS)
def test_tri_contract_strided_operands(cfg):
    ops = _kernels()
    Bt, X, Y, Z, C = cfg
    # stored the other way round: (Bt, Z, X, C) / (Bt, Z, Y, C)
    at = _randn(Bt, Z, X, C, seed=3).transpose(1, 2)
    bt = _randn(Bt, Z, Y, C, seed=4).transpose(1, 2)
    ac, bc = at.contiguous(), bt.contiguous()
    want = ops.tri_contract(ac, bc)
    _close(want, _ref(ac, bc))
    assert torch.equal(ops.tri_contract(at, bc), want)
    assert torch.equal(ops.tri_contract(ac, bt), want)
    assert torch.equal(ops.tri_contract(at, bt), want)
    # slices of wider buffers: batch stride larger than X*Z*C
    wa = _randn(Bt, X + 3, Z, C, seed=5)
    wb = _randn(Bt, Y + 2, Z, C, seed=6)
    wa[:, 1:X + 1].copy_(ac)
    wb[:, 2:Y + 2].copy_(bc)
    sa, sb = wa[:, 1:X + 1], wb[:, 2:Y + 2]
    assert sa.stride(0) > X * Z * C and sb.stride(0) > Y * Z * C
    assert torch.equal(ops.tri_contract(sa, sb), want)


def _fused_on(monkeypatch):
    monkeypatch.setenv("UNICORE_TRI_FUSED", "1")


def _run_tm(a, b, outgoing, d_out):
    from unicore_amd.modules import triangle_multiply

    a = a.detach().clone().requires_grad_()
    b = b.detach().clone().requires_grad_()
    o = triangle_multiply(a, b, outgoing)
    o.backward(d_out)
    return o.detach(), a.grad, b.grad


@requires_gpu
@pytest.mark.parametrize("outgoing", [True, False])
@pytest.mark.parametrize("dout_transposed", [False, True])
def test_triangle_multiply_direction_and_grads(monkeypatch, outgoing,
                                               dout_transposed):
    _kernels()
    _fused_on(monkeypatch)
    B, L, C = 2, 40, 64
    a, b = _randn(B, L, L, C, seed=7), _randn(B, L, L, C, seed=8)
    d_out = _randn(B, L, L, C, seed=9)
    if dout_transposed:
        d_out = d_out.transpose(1, 2)
        assert not d_out.is_contiguous()
    o, da, db = _run_tm(a, b, outgoing, d_out)
    assert da.is_contiguous() and db.is_contiguous()

    af = a.float().requires_grad_()
    bf = b.float().requires_grad_()
    of = torch.einsum(EQ[outgoing], af, bf)
    of.backward(d_out.float())
    _close(o, of.detach())
    _close(da, af.grad)
    _close(db, bf.grad)


@requires_gpu
@pytest.mark.parametrize("outgoing", [True, False])
def test_triangle_multiply_deterministic(monkeypatch, outgoing):
    _kernels()
    _fused_on(monkeypatch)
    B, L, C = 2, 40, 64
    a, b = _randn(B, L, L, C, seed=10), _randn(B, L, L, C, seed=11)
    d_out = _randn(B, L, L, C, seed=12)
    r1 = _run_tm(a, b, outgoing, d_out)
    r2 = _run_tm(a, b, outgoing, d_out)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)


@requires_gpu
@pytest.mark.parametrize("outgoing", [True, False])
def test_triangle_multiply_no_activation_sized_temporaries(monkeypatch,
                                                           outgoing):
    from unicore_amd.modules import triangle_multiply

    _kernels()
    _fused_on(monkeypatch)
    B, L, C = 1, 64, 64
    a, b = _randn(B, L, L, C, seed=13), _randn(B, L, L, C, seed=14)
    with torch.no_grad():
        triangle_multiply(a, b, outgoing)  # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        o = triangle_multiply(a, b, outgoing)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    out_bytes = o.numel() * o.element_size()
    # einsum needs >= 4x (two operand copies, permuted result, copy back)
    assert rise < 1.5 * out_bytes, (rise, out_bytes)


@requires_gpu
def test_triangle_multiply_fallback_and_host_check(monkeypatch):
    from unicore_amd.modules import triangle_multiply

    ops = _kernels()
    _fused_on(monkeypatch)
    g = torch.Generator(device="cuda").manual_seed(15)
    a = torch.randn(1, 6, 6, 12, device="cuda", generator=g)
    b = torch.randn(1, 6, 6, 12, device="cuda", generator=g)
    assert not ops.tri_contract_supported(12, torch.float32)
    for outgoing in (True, False):
        o = triangle_multiply(a, b, outgoing)
        assert torch.equal(o, torch.einsum(EQ[outgoing], a, b))
    for C in (32, 64, 128):
        assert ops.tri_contract_supported(C, torch.bfloat16)
    with pytest.raises(Exception):
        ops.tri_contract(_randn(1, 16, 32, 64), _randn(1, 16, 24, 64))


@requires_gpu
@pytest.mark.parametrize("outgoing", [True, False])
def test_triangle_multiplication_module_vs_fp32(monkeypatch, outgoing):
    """max|F-R| <= 2 max|E-R| + 1e-6 for output and every gradient: F fused
    bf16, E einsum bf16, R fp32 eager copy. Both bf16 runs differ from fp32
    by rounding noise of the same size; 2 covers two independent one-ulp
    noises adding."""
    import copy

    from unicore_amd.models.evoformer import TriangleMultiplication

    _kernels()
    torch.manual_seed(16)
    ref = TriangleMultiplication(d_pair=64, c=64, outgoing=outgoing).cuda()
    mod = copy.deepcopy(ref).to(torch.bfloat16)
    x = _randn(1, 24, 24, 64, seed=17)
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

    monkeypatch.setenv("UNICORE_TRI_FUSED", "1")
    Fr = run(mod, x, d_out)
    monkeypatch.setenv("UNICORE_TRI_FUSED", "0")
    Er = run(mod, x, d_out)
    Rr = run(ref, x.float(), d_out.float())
    assert set(Fr) == set(Er) == set(Rr)
    for k in Rr:
        f = (Fr[k] - Rr[k]).abs().max().item()
        e = (Er[k] - Rr[k]).abs().max().item()
        print(f"{k}: max|F-R|={f:.4e} max|E-R|={e:.4e}")
        assert f <= 2 * e + 1e-6, (k, f, e)
