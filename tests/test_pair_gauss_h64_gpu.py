"""bf16-MFMA kernels of the Uni-Mol pair embedding at K = 128, H = 64
(csrc/pair_gauss_h64.hip) against the eager definition run in float64.

Method of test_pair_attn_d8_gpu.py. Reference: pair_gauss_eager_ab in fp64 on
the same bf16-representable values. chain: the same function with the Linear
tensors in bf16, which is what a bf16 module runs eager. With
err(q) = max|q - ref| / max|ref|, every quantity obeys
err(kernel) <= 2 * err(chain) + 1e-6; out is compared over real keys, padded
keys equal finfo.min exactly.

The definition masks keys only: a padded atom's row i still holds o_ij at real
keys j. The pads test therefore compares the real (i, j) block of out, and
gives d_out zeros in the rows of padded atoms, as a loss that never reads
those rows does.
"""

import pytest
import torch

from unicore_amd import ops
from unicore_amd.modules import PairGaussianEmbed
from unicore_amd.modules.pair_gauss import pair_gauss_eager_ab

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

BF = torch.bfloat16
NAMES = ["out", "d_a", "d_b", "d_means", "d_stds", "dW1", "db1", "dW2", "db2"]
# less than one 16-j tile, exactly one, a ragged second, more than 64, more
# than 128; (33, 64) is 2112 rows: the forward's 512 blocks of 4 rows make a
# second trip, the backward's 256 blocks nine, and 256 partials rows are folded
SHAPES = [(1, 8), (2, 16), (1, 24), (2, 72), (1, 136), (33, 64)]


@pytest.fixture(autouse=True)
def _gate_on(monkeypatch):
    monkeypatch.setenv("UNICORE_PAIR_GAUSS_H64", "1")
    monkeypatch.delenv("UNICORE_GAUSSIAN_EAGER", raising=False)


def _inputs(B, L, padded, seed=0, K=128, H=64, n_types=8):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, device="cuda", generator=g)

    def ru(*s):
        return torch.rand(*s, device="cuda", generator=g)

    coords = 2 * rn(B, L, 3)
    tokens = torch.randint(0, n_types, (B, L), device="cuda", generator=g)
    mask = None
    if padded:
        mask = torch.zeros(B, L, dtype=torch.bool, device="cuda")
        mask[0, L - 3:] = True
        mask[-1, L - (5 if L <= 16 else 17):] = True
    sign = torch.where(torch.arange(K, device="cuda") % 2 == 0, 1.0, -1.0)
    p = dict(
        mul=1 + 0.1 * rn(n_types * n_types, 1), bias=0.1 * rn(n_types * n_types, 1),
        means=3 * ru(K), stds=(0.3 + 2.7 * ru(K)) * sign,
        w1=rn(K, K) / K ** 0.5, b1=rn(K) / K ** 0.5,
        w2=rn(H, K) / K ** 0.5, b2=rn(H) / K ** 0.5,
    )
    p = {k: v.to(BF) for k, v in p.items()}  # bf16-representable everywhere
    t = tokens.unsqueeze(2) * n_types + tokens.unsqueeze(1)
    a = p["mul"][t].view(B, L, L).float()
    b = p["bias"][t].view(B, L, L).float()
    d_out = rn(B, H, L, L).to(BF)
    return dict(coords=coords, tokens=tokens, mask=mask, a=a, b=b, p=p,
                d_out=d_out, n_types=n_types)


def _eager(x, dtype):
    """pair_gauss_eager_ab with the Linear tensors in dtype, fp64 or bf16"""
    ct = torch.float64 if dtype == torch.float64 else torch.float32
    p = x["p"]
    leaves = [x["a"].to(ct), x["b"].to(ct), p["means"].to(ct), p["stds"].to(ct),
              p["w1"].to(dtype), p["b1"].to(dtype), p["w2"].to(dtype),
              p["b2"].to(dtype)]
    leaves = [t.detach().requires_grad_(True) for t in leaves]
    out = pair_gauss_eager_ab(x["coords"].to(ct), *leaves, x["mask"])
    out.backward(x["d_out"].to(dtype))
    return dict(zip(NAMES, [out.detach()] + [t.grad for t in leaves]))


def _kernel(x):
    p = x["p"]
    w = (p["means"].float(), p["stds"].float(), p["w1"], p["b1"], p["w2"])
    out = ops.pair_gauss_fwd(x["coords"], x["a"], x["b"], x["mask"], *w,
                             p["b2"], torch.finfo(BF).min)
    grads = ops.pair_gauss_bwd(x["d_out"], x["coords"], x["a"], x["b"],
                               x["mask"], *w)
    return dict(zip(NAMES, [out] + list(grads)))


def _check(tag, got, chain, ref, mask, real=None):
    """the bound on every quantity; out over the keys (or the block) real"""
    B, H, L, _ = ref["out"].shape
    if real is None:
        real = torch.ones(B, 1, 1, L, dtype=torch.bool, device="cuda")
        if mask is not None:
            real = ~mask.view(B, 1, 1, L)
    real = real.expand(B, H, L, L)
    failures = []
    for name in NAMES:
        k, c, r = got[name].double(), chain[name].double(), ref[name].double()
        assert torch.isfinite(k).all(), name
        if name == "out":
            k, c, r = k[real], c[real], r[real]
        scale = r.abs().max()
        assert scale > 0, name
        ek = ((k - r).abs().max() / scale).item()
        ec = ((c - r).abs().max() / scale).item()
        print(f"pair_gauss_h64 {tag} {name}: err(kernel)={ek:.3e} "
              f"err(chain)={ec:.3e}")
        if not ek <= 2 * ec + 1e-6:
            failures.append((name, ek, ec))
    assert not failures, failures


@pytest.mark.parametrize("padded", [False, True], ids=["nopad", "pad"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity(shape, padded):
    x = _inputs(*shape, padded)
    got = _kernel(x)
    assert got["out"].dtype == BF
    assert all(got[n].dtype == torch.float32 for n in NAMES[1:])
    _check(f"{shape[0]}x{shape[1]} {'pad' if padded else 'nopad'}", got,
           _eager(x, BF), _eager(x, torch.float64), x["mask"])
    if padded:
        dead = x["mask"].view(shape[0], 1, 1, shape[1]).expand_as(got["out"])
        assert dead.any()
        assert (got["out"][dead] == torch.finfo(BF).min).all()


def test_padded_atoms_never_enter():
    x = _inputs(2, 72, True, seed=5)
    B, L = x["mask"].shape
    realq = ~x["mask"]
    x["d_out"] = x["d_out"] * realq.view(B, 1, L, 1)
    block = (realq.view(B, 1, L, 1) & realq.view(B, 1, 1, L))
    ref = _kernel(x)
    y = dict(x)
    g = torch.Generator(device="cuda").manual_seed(9)
    junk = 50 * torch.randn(B, L, 3, device="cuda", generator=g)
    y["coords"] = torch.where(x["mask"].unsqueeze(-1), junk, x["coords"])
    pm = x["mask"].view(B, L, 1) | x["mask"].view(B, 1, L)
    y["a"] = torch.where(pm, torch.full_like(x["a"], -3.0), x["a"])
    y["b"] = torch.where(pm, torch.full_like(x["b"], 7.0), x["b"])
    got = _kernel(y)
    dead = x["mask"].view(B, 1, 1, L).expand_as(got["out"])
    assert (got["out"][dead] == torch.finfo(BF).min).all()
    assert torch.equal(got["out"][block.expand_as(dead)],
                       ref["out"][block.expand_as(dead)])
    # every gradient against the clean inputs' references
    for name in ("d_a", "d_b"):
        assert torch.equal(got[name][pm], torch.zeros_like(got[name][pm]))
    _check("garbage", got, _eager(x, BF), _eager(x, torch.float64), x["mask"],
           real=block)


def test_deterministic():
    x = _inputs(2, 72, True, seed=3)
    a, b = _kernel(x), _kernel(x)
    for name in NAMES:
        assert torch.equal(a[name], b[name]), name


def _spy(monkeypatch):
    calls = []
    real = ops.pair_gauss_fwd

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "pair_gauss_fwd", spy)
    return calls


def test_dispatch(monkeypatch):
    calls = _spy(monkeypatch)

    def run(L=72, H=64, dtype=BF, coord_grad=False):
        x = _inputs(2, L, True, H=H)
        m = PairGaussianEmbed(128, H, x["n_types"]).cuda().to(dtype)
        out = m(x["coords"].requires_grad_(coord_grad), x["tokens"], x["mask"])
        out.backward(x["d_out"].to(dtype))
        assert out.shape == (2, H, L, L) and out.dtype == dtype
        for p in m.parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all()
            assert p.grad.abs().max() > 0
        return len(calls)

    assert run() == 1
    monkeypatch.setenv("UNICORE_PAIR_GAUSS_H64", "0")
    assert run() == 1
    monkeypatch.setenv("UNICORE_PAIR_GAUSS_H64", "1")
    monkeypatch.setenv("UNICORE_GAUSSIAN_EAGER", "1")
    assert run() == 1
    monkeypatch.delenv("UNICORE_GAUSSIAN_EAGER")
    assert run(L=20) == 1
    assert run(H=8) == 1
    assert run(dtype=torch.float32) == 1
    assert run(coord_grad=True) == 1
    assert run() == 2

    assert ops.pair_gauss_supported(128, 64, BF, 72)
    for K, H, dt, L in ((128, 64, BF, 20), (64, 64, BF, 72), (128, 8, BF, 72),
                        (128, 64, torch.float16, 72), (128, 64, torch.float32, 72)):
        assert not ops.pair_gauss_supported(K, H, dt, L)
    # the C++ entries refuse by name
    for kw in (dict(L=20), dict(K=64), dict(H=8), dict(dtype=torch.float16)):
        dt = kw.pop("dtype", BF)
        x = _inputs(1, kw.pop("L", 16), True, **kw)
        p = {k: v.to(dt) for k, v in x["p"].items()}
        w = (p["means"].float(), p["stds"].float(), p["w1"], p["b1"], p["w2"])
        with pytest.raises(RuntimeError, match="pair_gauss_forward"):
            ops.pair_gauss_fwd(x["coords"], x["a"], x["b"], x["mask"], *w,
                               p["b2"], -1.0)
        with pytest.raises(RuntimeError, match="pair_gauss_backward"):
            ops.pair_gauss_bwd(x["d_out"].to(dt), x["coords"], x["a"], x["b"],
                               x["mask"], *w)
