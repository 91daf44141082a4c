"""Head-dim-32 fused attention (csrc/evo_attn.hip) against the plain
expression in float64.

Reference: softmax(q k^T + bias + mask) (keep / (1 - p) applied to it under
dropout) times v, and its autograd gradients, in float64 on the bf16-rounded
inputs.  `chain` is the same expression in bf16 torch ops on the same inputs
and keep mask.  With err(x) = max|x - ref| / max|ref|, every quantity obeys

    err(kernel) <= 2 * err(chain) + 1e-6

(2: another summation order around the same single bf16 rounding of P).
Both evaluate the kernels' documented score floor, max(score, -8192) with
the gradient passed straight through: it is what -1e9 turns into.
"""

import math

import pytest
import torch

from unicore_amd import ops

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

BF16 = torch.bfloat16
QUANTITIES = ["o", "lse", "dq", "dk", "dv", "dbias"]


def _inputs(dims, T, with_bias, mask_kind, seed=0):
    """q, k, v, d_o (*dims, T, 32); bias (b0, b1, 1, T, T); mask row style
    (1, 1, b2, 1, T) with batch row 1 fully masked, or column style
    (b0, b1, 1, 1, T).  Also the kernel-form (tensor, outer_div) of both."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    b0, b1, b2 = dims

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, device="cuda", generator=g) * scale).to(BF16)

    q, k, v, d_o = (rnd(*dims, T, 32, scale=s) for s in (0.4, 1.0, 1.0, 0.3))
    bias = rnd(b0, b1, 1, T, T) if with_bias else None
    mask = None
    if mask_kind is not None:
        shape = (1, 1, b2, 1, T) if mask_kind == "row" else (b0, b1, 1, 1, T)
        dead = torch.rand(shape, device="cuda", generator=g) < 0.25
        dead[..., 0] = False
        if mask_kind == "row":
            dead[0, 0, 1] = True
        mask = torch.zeros(shape, device="cuda", dtype=BF16).masked_fill_(dead, -1e9)
    bias_k = (bias.reshape(b0 * b1, T, T), b2) if with_bias else (None, 1)
    mask_k = (None, 1)
    if mask_kind is not None:
        mask_k = (mask.reshape(-1, 1, T), 1 if mask_kind == "row" else b2)
    return q, k, v, d_o, bias, mask, bias_k, mask_k


def _expr(ct, q, k, v, d_o, bias, mask, keep=None, p=0.0):
    q, k, v = (t.to(ct).requires_grad_() for t in (q, k, v))
    z = q @ k.transpose(-1, -2)
    if bias is not None:
        bias = bias.to(ct).requires_grad_()
        z = z + bias
    if mask is not None:
        z = z + mask.to(ct)
    z = z + (z.clamp_min(-8192.0) - z).detach()
    prob = torch.softmax(z, dim=-1)
    if keep is not None:
        prob = prob * (keep.to(ct) / (1.0 - p))
    o = prob @ v
    o.backward(d_o.to(ct))
    res = {"o": o, "lse": torch.logsumexp(z, dim=-1), "dq": q.grad, "dk": k.grad,
           "dv": v.grad}
    if bias is not None:
        res["dbias"] = bias.grad
    return {name: t.detach().double() for name, t in res.items()}


def _kernel(q, k, v, d_o, bias_k, mask_k, p=0.0, training=False):
    T = q.shape[-2]
    q, k, v, d_o = (t.reshape(-1, T, 32) for t in (q, k, v, d_o))
    (b, b_od), (m, m_od) = bias_k, mask_k
    o, lse, seed = ops.evo_attn_fwd(q, k, v, b, b_od, m, m_od, p, training)
    grads = ops.evo_attn_bwd(d_o, q, k, v, o, lse, b, b_od, b is not None, m,
                             m_od, p, training and p > 0, int(seed))
    res = dict(zip(QUANTITIES, [o, lse, *grads]))
    return res, int(seed)


def _check(kern, ref, chain):
    for name, r in ref.items():
        scale = r.abs().max().item()
        e_k = (kern[name].double().reshape(r.shape) - r).abs().max().item() / scale
        e_c = (chain[name] - r).abs().max().item() / scale
        print(f"{name}: kernel {e_k:.3e} chain {e_c:.3e}")
        assert math.isfinite(e_k) and e_k <= 2 * e_c + 1e-6, (name, e_k, e_c)


@pytest.mark.parametrize("mask_kind", [None, "row", "col"])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dims", [(1, 2, 3), (2, 2, 2)])
@pytest.mark.parametrize("T", [64, 128, 192])
def test_evo_attn_parity(T, dims, with_bias, mask_kind):
    q, k, v, d_o, bias, mask, bias_k, mask_k = _inputs(dims, T, with_bias, mask_kind)
    kern, _ = _kernel(q, k, v, d_o, bias_k, mask_k)
    _check(kern, _expr(torch.float64, q, k, v, d_o, bias, mask),
           _expr(BF16, q, k, v, d_o, bias, mask))
    if mask_kind == "row" and not with_bias:
        # every key of batch row 1 is masked: uniform and finite
        o = kern["o"].view(*dims, T, 32)[:, :, 1].float()
        mean_v = v[:, :, 1].float().mean(dim=-2, keepdim=True)
        assert torch.isfinite(o).all()
        torch.testing.assert_close(o, mean_v.expand_as(o), atol=2e-2, rtol=0)
        lse = kern["lse"].view(*dims, T)[:, :, 1]
        torch.testing.assert_close(lse, torch.full_like(lse, -8192 + math.log(T)))


@pytest.mark.parametrize("with_bias", [False, True])
def test_evo_attn_dropout_explicit_mask(with_bias):
    """T / 32 forwards from one generator state, each with one 32-row
    identity block in V, read out the keep mask; forward and backward with a
    random V and that seed then face the explicit-mask reference."""
    dims, T, p = (1, 2, 3), 128, 0.3
    q, k, v, d_o, bias, _, bias_k, mask_k = _inputs(dims, T, with_bias, None, seed=1)
    N = dims[0] * dims[1] * dims[2]
    cols, seeds = [], set()
    for c in range(T // 32):
        v_id = torch.zeros(N, T, 32, device="cuda", dtype=BF16)
        v_id[:, 32 * c:32 * (c + 1)] = torch.eye(32, device="cuda", dtype=BF16)
        torch.manual_seed(13)
        o_c, _, seed_c = ops.evo_attn_fwd(q.view(N, T, 32), k.view(N, T, 32), v_id,
                                          *bias_k, *mask_k, p, True)
        cols.append(o_c != 0)
        seeds.add(int(seed_c))
    keep = torch.cat(cols, dim=-1).view(*dims, T, T)
    assert len(seeds) == 1, seeds
    rate = keep.float().mean().item()
    sigma = math.sqrt(p * (1.0 - p) / keep.numel())
    assert abs(rate - (1.0 - p)) < 5.0 * sigma + 2.0 ** -16, (rate, sigma)

    torch.manual_seed(13)
    kern, seed = _kernel(q, k, v, d_o, bias_k, mask_k, p, True)
    assert seed in seeds
    _check(kern, _expr(torch.float64, q, k, v, d_o, bias, None, keep, p),
           _expr(BF16, q, k, v, d_o, bias, None, keep, p))


def test_evo_attn_double_run_bitwise():
    q, k, v, d_o, _, _, bias_k, mask_k = _inputs((1, 2, 3), 192, True, "row", seed=2)
    runs = []
    for _ in range(2):
        torch.manual_seed(7)
        runs.append(_kernel(q, k, v, d_o, bias_k, mask_k, 0.2, True)[0])
    for name in QUANTITIES:
        assert torch.equal(runs[0][name], runs[1][name]), name


def _bad_cases():
    def base(N=4, T=64, D=32, dtype=BF16):
        return [torch.randn(N, T, D, device="cuda").to(dtype) for _ in range(3)]

    q, k, v = base()
    bias = torch.zeros(2, 64, 64, device="cuda", dtype=BF16)
    mask = torch.zeros(2, 1, 64, device="cuda", dtype=BF16)
    yield "D = 64", base(D=64), {}
    yield "T = 96", base(T=96), {}
    yield "T = 576", base(T=576), {}
    yield "fp16", base(dtype=torch.float16), {}
    yield "strided q", [torch.randn(4, 64, 64, device="cuda").to(BF16)[..., :32], k, v], {}
    yield "misaligned q", [torch.randn(4 * 64 * 32 + 4, device="cuda").to(BF16)[4:]
                           .view(4, 64, 32), k, v], {}
    yield "k shape", [q, base(N=2)[0], v], {}
    yield "bias T", [q, k, v], {"bias": bias[:, :, :32].contiguous()}
    yield "bias rows", [q, k, v], {"bias": bias[:, :32].contiguous()}
    yield "bias fp32", [q, k, v], {"bias": bias.float()}
    yield "N % (nb * od)", [q, k, v], {"bias": bias, "bias_od": 4}
    yield "mask rows", [q, k, v], {"mask": bias}
    yield "N % mask nb", [q, k, v], {"mask": mask.repeat(3, 1, 1)[:3].contiguous()}
    yield "p = 1", [q, k, v], {"p": 1.0}


@pytest.mark.parametrize("name", [
    "D = 64", "T = 96", "T = 576", "fp16", "strided q", "misaligned q", "k shape",
    "bias T", "bias rows", "bias fp32", "N % (nb * od)", "mask rows",
    "N % mask nb", "p = 1"])
def test_evo_attn_rejects(name):
    (q, k, v), kw = {c[0]: c[1:] for c in _bad_cases()}[name]
    args = (kw.get("bias"), kw.get("bias_od", 1), kw.get("mask"), 1)
    with pytest.raises(RuntimeError, match="evo_attn"):
        ops.evo_attn_fwd(q, k, v, *args, kw.get("p", 0.0), True)
    if q.shape == k.shape and not kw:
        lse = torch.zeros(q.shape[:2], device="cuda")
        with pytest.raises(RuntimeError, match="evo_attn"):
            ops.evo_attn_bwd(v, q, k, v, v, lse, None, 1, False, None, 1, 0.0,
                             False, 0)
        if q.is_contiguous() and q.data_ptr() % 16 == 0:
            assert not ops.evo_attn_supported(*q.shape, q.dtype)


def test_evo_attn_supported_and_dbias_needs_full_bias():
    assert ops.evo_attn_supported(4, 64, 32, BF16)
    assert ops.evo_attn_supported(4, 512, 32, BF16)
    q, k, v, d_o, *_ = _inputs((1, 2, 2), 64, False, None)
    q, k, v, d_o = (t.view(4, 64, 32) for t in (q, k, v, d_o))
    bias = torch.zeros(2, 1, 64, device="cuda", dtype=BF16)
    o, lse, _ = ops.evo_attn_fwd(q, k, v, bias, 2, None, 1, 0.0, False)
    with pytest.raises(RuntimeError, match="bias gradient"):
        ops.evo_attn_bwd(d_o, q, k, v, o, lse, bias, 2, True, None, 1, 0.0, False, 0)


def _module_case(kind):
    from unicore_amd.models.evoformer import MSARowAttentionWithPairBias
    from unicore_amd.modules import TriangleAttention

    torch.manual_seed(3)
    L = 64
    pair = torch.randn(1, L, L, 64, device="cuda")
    if kind == "msa_row":
        mod = MSARowAttentionWithPairBias(64, 64, 2, 0.0)
        args = (torch.randn(1, 3, L, 64, device="cuda"), pair)
        weights = [mod.pair_bias.weight, mod.qkv.weight]
    else:
        mod = TriangleAttention(64, 2, 0.0, starting=(kind == "tri_start"))
        args = (pair,)
        weights = [mod.bias_proj.weight, mod.qkv.weight]
    return mod.cuda(), args, weights


def _module_run(mod, args, weights, dtype, d_out):
    mod.to(dtype).zero_grad(set_to_none=True)
    xs = [a.detach().to(dtype).requires_grad_() for a in args]
    out = mod(*xs)
    out.backward(d_out.to(dtype))
    got = [out, *(x.grad for x in xs), *(w.grad for w in weights)]
    return [t.detach().double() for t in got]


@pytest.mark.parametrize("kind", ["tri_start", "tri_end", "msa_row"])
def test_modules_gate_on_vs_off(kind, monkeypatch):
    """Output, input gradients and the bias / qkv weight gradients with the
    gate on: within twice the gate-off path's own error against an fp32 run
    of the module on the same (bf16-representable) weights."""
    mod, args, weights = _module_case(kind)
    with torch.no_grad():
        for prm in mod.parameters():
            prm.copy_(prm.to(BF16))
    args = tuple(a.to(BF16).float() for a in args)
    d_out = torch.randn_like(args[0]).to(BF16)
    monkeypatch.setenv("UNICORE_EVO_ATTN", "0")
    ref = _module_run(mod, args, weights, torch.float32, d_out)
    off = _module_run(mod, args, weights, BF16, d_out)
    monkeypatch.setenv("UNICORE_EVO_ATTN", "1")
    on = _module_run(mod, args, weights, BF16, d_out)
    for i, r in enumerate(ref):
        scale = r.abs().max().item()
        e_on = (on[i] - r).abs().max().item() / scale
        e_off = (off[i] - r).abs().max().item() / scale
        print(f"{kind}[{i}]: on {e_on:.3e} off {e_off:.3e}")
        assert e_on <= 2 * e_off + 1e-6, (kind, i, e_on, e_off)
