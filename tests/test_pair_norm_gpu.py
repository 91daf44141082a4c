"""Norm regulariser kernels (csrc/pair_norm.hip) against the eager
definitions run in float64.

Method of test_pair_dist_h64_gpu.py. Oracle: the eager definition in fp64 on
the same, already rounded, inputs. Baseline: the eager definition in fp32.
With err(q) = max|q - oracle| / (max|oracle| + 1e-12):

  loss, coef, and gradients for fp32 inputs:
      err(kernel) <= 4 * err(baseline) + 1e-6
  gradients for bf16 inputs: err <= 2^-8, one bf16 rounding.

The error has kinks at n = sqrt(C) +- 1, so the inputs put every reduced
vector at a norm of sqrt(C) - 3 (0.3 if sqrt(C) <= 3), sqrt(C) or
sqrt(C) + 3.5, the three classes dealt out evenly over (b, i, j), and every
parity test first asserts on the oracle that each class holds >= 20% of the
valid positions (where there are at least 5 of them: a 3-row case cannot)
and that none is within 0.25 of a kink.
"""

import functools
import math

import pytest
import torch

from unicore_amd import ops
from unicore_amd.modules import norm_loss
from unicore_amd.modules.norm_loss import pair_norm_eager, x_norm_eager

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

# (B, H, L): less than a block; one sample left with a single atom; a partial
# block; blocks straddle rows and samples; two heads per wave; one per wave
SHAPES = [(1, 64, 8), (2, 64, 16), (1, 64, 24), (2, 64, 72), (1, 8, 136),
          (3, 4, 64)]
# second trips of the grid-stride loops: (17,4,256) is 2176 blocks of the
# forward (cap 2048), (5,64,120) 2250 blocks of the backward
STRIDE = [(17, 4, 256), (5, 64, 120)]
ROWS = [(3, 8), (5, 512), (70, 520)]  # (N, E); 520: a second trip of the wave
DTYPES = [torch.float32, torch.bfloat16]
GRAD = 1.7  # upstream gradient of the scalar


@pytest.fixture(autouse=True)
def _gate_on(monkeypatch):
    monkeypatch.setenv("UNICORE_PAIR_NORM", "1")


def _mask(B, L, padded):
    if not padded:
        return None
    mask = torch.zeros(B, L, dtype=torch.bool, device="cuda")
    mask[0, L - min(3, L - 1):] = True  # a key run of 3
    if B > 1:
        mask[1, 1:] = True  # a single real atom
    return mask


def _vectors(shape, dim, seed):
    """fp32 vectors along ``dim`` with the three norms of the docstring"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.randn(shape, device="cuda", generator=g)
    u = u / u.norm(dim=dim, keepdim=True)
    root = math.sqrt(shape[dim])
    t = torch.tensor([root - 3 if root > 3 else 0.3, root, root + 3.5],
                     device="cuda")
    rest = [s for d, s in enumerate(shape) if d != dim]
    idx = sum((1, 1, 2)[k] * torch.arange(s, device="cuda").view(
        [-1 if d == k else 1 for d in range(len(rest))])
        for k, s in enumerate(rest))
    return u * t[idx % 3].unsqueeze(dim), g


def _pair_inputs(B, H, L, dtype, padded, seed=0):
    delta, g = _vectors((B, H, L, L), 1, seed)
    bias = (1.5 * torch.randn(B, H, L, L, device="cuda", generator=g)).to(dtype)
    pair = (bias.float() + delta).to(dtype)
    mask = _mask(B, L, padded)
    if padded:  # what the pair embedding leaves at padded keys
        fill = mask.view(B, 1, 1, L)
        pair = pair.masked_fill(fill, torch.finfo(dtype).min)
        bias = bias.masked_fill(fill, torch.finfo(dtype).min)
    return pair.contiguous(), bias.contiguous(), mask


def _coef(ss, C, valid):
    n = torch.sqrt(ss + 1e-10)
    d = n - math.sqrt(C)
    return torch.where(valid & (d.abs() > 1), torch.sign(d) / n,
                       torch.zeros_like(n)), d


def _run_pair(pair, bias, mask, ct=None):
    """the public function (ct None), or the eager definition in ct"""
    B, H, L, _ = pair.shape
    real = torch.ones(B, L, dtype=torch.bool, device="cuda") if mask is None else ~mask
    valid = real.unsqueeze(2) & real.unsqueeze(1)
    if ct is None:
        p, q = (t.detach().clone().requires_grad_(True) for t in (pair, bias))
        loss = norm_loss.pair_norm(p, q, mask)
        coef = ops.pair_norm_fwd(pair, bias, mask)[0]
    else:
        p, q = (t.detach().to(ct).requires_grad_(True) for t in (pair, bias))
        loss = pair_norm_eager(p, q, mask)
        ss = torch.where(valid.unsqueeze(1), (p - q).detach(), 0.0).pow(2).sum(1)
        coef, d = _coef(ss, H, valid)
    loss.backward(torch.tensor(GRAD, device="cuda", dtype=loss.dtype))
    res = dict(loss=loss.detach(), coef=coef, d_pair=p.grad, d_bias=q.grad)
    if ct is not None:
        res.update(d=d, valid=valid)
    return res


def _run_rows(x, mask, ct=None):
    B, L, E = x.shape
    valid = torch.ones(B, L, dtype=torch.bool, device="cuda") if mask is None else ~mask
    if ct is None:
        v = x.detach().clone().requires_grad_(True)
        loss = norm_loss.x_norm(v, mask)
        coef = ops.row_norm_fwd(x.view(B * L, E), None if mask is None
                                else mask.view(-1))[0].view(B, L)
    else:
        v = x.detach().to(ct).requires_grad_(True)
        loss = x_norm_eager(v, mask)
        ss = torch.where(valid.unsqueeze(-1), v.detach(), 0.0).pow(2).sum(-1)
        coef, d = _coef(ss, E, valid)
    loss.backward(torch.tensor(GRAD, device="cuda", dtype=loss.dtype))
    res = dict(loss=loss.detach(), coef=coef, dx=v.grad)
    if ct is not None:
        res.update(d=d, valid=valid)
    return res


@functools.lru_cache(maxsize=None)
def _pair_case(shape, dtype, padded):
    """inputs, kernel, fp32 baseline, fp64 oracle: computed once, read after"""
    args = _pair_inputs(*shape, dtype, padded)
    return (args, _run_pair(*args), _run_pair(*args, torch.float32),
            _run_pair(*args, torch.float64))


def _err(q, oracle):
    q, oracle = q.double(), oracle.double()
    return ((q - oracle).abs().max() / (oracle.abs().max() + 1e-12)).item()


def _check(tag, names, dtype, kernel, base, oracle):
    d = oracle["d"][oracle["valid"]]
    assert ((d.abs() - 1).abs() >= 0.25).all()
    if d.numel() >= 5:
        for cls in (d < -1, d.abs() <= 1, d > 1):
            assert cls.double().mean() >= 0.2
    failures = []
    for name in names:
        grad = name.startswith("d")
        assert kernel[name].dtype == (dtype if grad else torch.float32)
        assert kernel[name].shape == oracle[name].shape
        ek, eb = _err(kernel[name], oracle[name]), _err(base[name], oracle[name])
        print(f"{tag} {name}: err(kernel)={ek:.3e} err(eager fp32)={eb:.3e}")
        if grad and dtype != torch.float32:
            ok = ek <= 2.0 ** -8
        else:
            ok = ek <= 4 * eb + 1e-6
        if not ok:
            failures.append((name, ek, eb))
    assert not failures, failures


def _id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    return "pad" if v else "nopad"


@pytest.mark.parametrize(
    "shape,dtype,padded",
    [(s, d, p) for s in SHAPES for d in DTYPES for p in (False, True)]
    + [(s, torch.bfloat16, True) for s in STRIDE],
    ids=_id,
)
def test_pair_parity(shape, dtype, padded):
    _, kernel, base, oracle = _pair_case(shape, dtype, padded)
    _check(f"pair_norm {_id(shape)} {_id(dtype)} {_id(padded)}",
           ["loss", "coef", "d_pair", "d_bias"], dtype, kernel, base, oracle)
    assert kernel["loss"] > 0 and kernel["d_pair"].abs().max() > 0


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_pair_exact_properties(dtype):
    (pair, bias, mask), kernel, _, oracle = _pair_case((2, 64, 72), dtype, True)
    d_pair, d_bias = kernel["d_pair"], kernel["d_bias"]
    assert torch.equal(_bits(d_bias), _bits(-d_pair))
    # exactly 0 inside the band and at every padded row and column
    still = ~oracle["valid"] | (oracle["d"].abs() <= 1)
    assert (~oracle["valid"]).any() and (oracle["d"].abs() <= 1).any()
    assert (d_pair != 0).any(1)[~still].all()
    still = still.unsqueeze(1).expand_as(d_pair)
    assert torch.equal(d_pair[still], torch.zeros_like(d_pair[still]))
    # what padded rows and columns hold never enters
    dead = (~oracle["valid"]).unsqueeze(1)
    again = _run_pair(pair.masked_fill(dead, float("nan")),
                      bias.masked_fill(dead, float("inf")), mask)
    rerun = _run_pair(pair, bias, mask)
    for name in ("loss", "coef", "d_pair", "d_bias"):
        assert torch.equal(_bits(kernel[name]), _bits(again[name])), name
        assert torch.equal(_bits(kernel[name]), _bits(rerun[name])), name


def _row_inputs(N, E, dtype):
    B = 2 if N % 2 == 0 else 1
    x = _vectors((B, N // B, E), 2, seed=1)[0].to(dtype)
    mask = torch.zeros(B, N // B, dtype=torch.bool, device="cuda")
    mask[0, 1] = True
    if B > 1:
        mask[1, 1:] = True
    return x.masked_fill(mask.unsqueeze(-1), float("inf")).contiguous(), mask


@pytest.mark.parametrize("shape", ROWS, ids=_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_row_parity_and_exactness(shape, dtype):
    x, mask = _row_inputs(*shape, dtype)
    kernel = _run_rows(x, mask)
    _check(f"row_norm {_id(shape)} {_id(dtype)}", ["loss", "coef", "dx"], dtype,
           kernel, _run_rows(x, mask, torch.float32),
           _run_rows(x, mask, torch.float64))
    dx = kernel["dx"]
    assert torch.equal(dx[mask], torch.zeros_like(dx[mask]))
    assert dx.abs().max() > 0
    rerun = _run_rows(x, mask)
    for name in ("loss", "coef", "dx"):
        assert torch.equal(_bits(kernel[name]), _bits(rerun[name])), name


def test_dispatch(monkeypatch):
    calls = []
    for name in ("pair_norm_fwd", "pair_norm_bwd"):
        real = getattr(ops, name)
        monkeypatch.setattr(
            ops, name,
            lambda *a, _n=name, _r=real: (calls.append(_n), _r(*a))[1])
    pair, bias, mask = _pair_inputs(1, 64, 16, torch.bfloat16, True)
    small = _pair_inputs(1, 64, 20, torch.float32, True)

    def run(p, q, m):
        p, q = (t.detach().clone().requires_grad_(True) for t in (p, q))
        norm_loss.pair_norm(p, q, m).backward()

    run(pair, bias, mask)
    assert calls == ["pair_norm_fwd", "pair_norm_bwd"]
    monkeypatch.setenv("UNICORE_PAIR_NORM", "0")
    run(pair, bias, mask)
    monkeypatch.setenv("UNICORE_PAIR_NORM", "1")
    run(*small)  # L = 20
    run(*_pair_inputs(1, 6, 16, torch.float32, True))  # H = 6
    assert len(calls) == 2
    # the C++ refusals, by name
    with pytest.raises(RuntimeError, match="one shape.*16, 16.*8, 8"):
        ops.pair_norm_fwd(pair, bias[:, :, :8, :8].contiguous(), None)
    with pytest.raises(RuntimeError, match="fp32 or bf16, got Half"):
        ops.pair_norm_fwd(pair.half(), bias.half(), mask)
    with pytest.raises(RuntimeError, match="multiple of 8.*L = 20"):
        ops.pair_norm_fwd(*small)
