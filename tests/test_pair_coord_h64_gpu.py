"""fp32-MFMA kernels of the coordinate head at H = 64
(csrc/pair_coord_h64.hip) against the eager definition run in float64.

Method of test_pair_coord_gpu.py. Oracle: pair_coord_eager in fp64 on the
same, already rounded, inputs. Baseline: pair_coord_eager in fp32. With
err(q) = max|q - oracle| / (max|oracle| + 1e-12):

  update, dW1, db1, dW2, db2, and dpair for fp32 inputs:
      err(kernel) <= 4 * err(baseline) + 1e-6
  dpair for bf16 inputs: err <= 2^-8, one bf16 rounding.
"""

import functools

import pytest
import torch

from unicore_amd import ops
from unicore_amd.modules import PairCoordHead
from unicore_amd.modules.pair_coord import pair_coord_eager

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

H = 64
# (B, L): one tile, one sample left with a single atom; less than a tile; a
# half-tile tail; several tiles, a tail and more than one staging step;
# beyond 128
SHAPES = [(2, 16), (1, 8), (1, 24), (2, 72), (1, 136)]
DTYPES = [torch.float32, torch.bfloat16]
QUANTITIES = ["update", "dW1", "db1", "dW2", "db2"]
GRADS = ["dpair", "dW1", "db1", "dW2", "db2"]


@pytest.fixture(autouse=True)
def _gate_on(monkeypatch):
    monkeypatch.setenv("UNICORE_PAIR_COORD_H64", "1")
    monkeypatch.delenv("UNICORE_PAIR_COORD_EAGER", raising=False)


def _inputs(B, L, dtype, padded, seed=0):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(seed)
    mask = None
    coords = 2.0 * torch.randn(B, L, 3, device=dev, generator=g)
    pair0 = torch.randn(B, H, L, L, device=dev, generator=g).to(dtype)
    pair = pair0 + torch.randn(B, H, L, L, device=dev, generator=g).to(dtype)
    if padded:
        mask = torch.zeros(B, L, dtype=torch.bool, device=dev)
        for b, n in enumerate(((3, L - 1) if L == 16 else (3, 0))[:B]):
            if n:
                mask[b, L - n:] = True
        # what the gaussian pair bias leaves at padded keys
        pair0 = pair0.masked_fill(mask.view(B, 1, 1, L), torch.finfo(dtype).min)
        pair = torch.where(mask.view(B, 1, 1, L), pair0, pair)
    head = PairCoordHead(H).to(dev)
    with torch.no_grad():
        for p in head.parameters():
            # fc1 rows of 64 terms: keep the hidden units O(1)
            p.copy_(0.2 * torch.randn(p.shape, device=dev, generator=g))
    grad = torch.randn(B, L, 3, device=dev, generator=g)
    return head, pair.contiguous(), pair0.contiguous(), coords, mask, grad


def _params(head):
    return [head.fc1.weight, head.fc1.bias, head.fc2.weight, head.fc2.bias]


def _run_head(head, pair, pair0, coords, mask, grad):
    pair = pair.detach().clone().requires_grad_(True)
    pair0 = pair0.detach().clone().requires_grad_(True)
    head.zero_grad(set_to_none=True)
    out = head(pair, pair0, coords, mask)
    out.backward(grad)
    w1, b1, w2, b2 = (p.grad.clone() for p in _params(head))
    return {"update": out.detach(), "dpair": pair.grad, "dpair0": pair0.grad,
            "dW1": w1, "db1": b1, "dW2": w2.view(-1), "db2": b2}


def _run_eager(head, pair, pair0, coords, mask, grad, ct):
    pair = pair.detach().to(ct).requires_grad_(True)
    params = [p.detach().to(ct).requires_grad_(True) for p in _params(head)]
    out = pair_coord_eager(pair, pair0.detach().to(ct), coords.to(ct), *params,
                           mask)
    out.backward(grad.to(ct))
    return {"update": out.detach(), "dpair": pair.grad,
            "dW1": params[0].grad, "db1": params[1].grad,
            "dW2": params[2].grad.view(-1), "db2": params[3].grad}


def _spy(monkeypatch):
    calls = []
    real = ops.pair_coord_fwd

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "pair_coord_fwd", spy)
    return calls


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, padded):
    """kernel (and whether ops.pair_coord_fwd was reached), fp32 eager
    baseline and fp64 oracle of one case, computed once, only read after"""
    args = _inputs(*shape, dtype, padded)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("UNICORE_PAIR_COORD_H64", "1")
        calls = _spy(mp)
        kernel = _run_head(*args)
    base = _run_eager(*args, torch.float32)
    oracle = _run_eager(*args, torch.float64)
    return args, kernel, len(calls), base, oracle


def _err(q, oracle):
    q, oracle = q.double(), oracle.double()
    return ((q - oracle).abs().max() / (oracle.abs().max() + 1e-12)).item()


def _id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    return "pad" if v else "nopad"


cases = pytest.mark.parametrize(
    "shape,dtype,padded",
    [(s, d, p) for s in SHAPES for d in DTYPES for p in (False, True)],
    ids=_id,
)


@cases
def test_fp32_results(shape, dtype, padded):
    _, kernel, calls, base, oracle = _case(shape, dtype, padded)
    assert calls == 1
    failures = []
    for name in QUANTITIES:
        assert kernel[name].dtype == torch.float32
        ek, eb = _err(kernel[name], oracle[name]), _err(base[name], oracle[name])
        print(f"pair_coord_h64 {_id(shape)} {_id(dtype)} {_id(padded)} {name}: "
              f"err(kernel)={ek:.3e} err(eager fp32)={eb:.3e}")
        if not ek <= 4 * eb + 1e-6:
            failures.append((name, ek, eb))
    assert not failures, failures


@cases
def test_dpair(shape, dtype, padded):
    (head, pair, pair0, coords, mask, grad), kernel, calls, base, oracle = _case(
        shape, dtype, padded)
    assert calls == 1
    dpair = kernel["dpair"]
    assert dpair.dtype == dtype and dpair.shape == pair.shape
    ek = _err(dpair, oracle["dpair"])
    eb = _err(base["dpair"], oracle["dpair"])
    print(f"pair_coord_h64 {_id(shape)} {_id(dtype)} {_id(padded)} dpair: "
          f"err(kernel)={ek:.3e} err(eager fp32)={eb:.3e}")
    if dtype == torch.float32:
        assert ek <= 4 * eb + 1e-6
    else:
        assert ek <= 2.0 ** -8
    if padded:
        B, L = mask.shape
        dead = (mask.view(B, 1, L, 1) | mask.view(B, 1, 1, L)).expand_as(dpair)
        assert dead.any()
        assert torch.equal(dpair[dead], torch.zeros_like(dpair[dead]))
    assert dpair.abs().max() > 0
    assert torch.equal(kernel["dpair0"], -dpair)


def test_deterministic():
    args = _inputs(2, 72, torch.bfloat16, True, seed=3)
    a = _run_head(*args)
    b = _run_head(*args)
    for name in ["update"] + GRADS:
        assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_padded_entries_never_enter(dtype):
    head, pair, pair0, coords, mask, grad = _inputs(2, 16, dtype, True)
    ref = _run_head(head, pair, pair0, coords, mask, grad)
    fill = torch.finfo(dtype).min
    g = torch.Generator(device="cuda").manual_seed(9)

    def garbage(t):
        r = torch.rand(t.shape, device="cuda", generator=g) * 2 - 1
        out = torch.where(t == fill, (t.float() * r).to(dtype), t)
        assert torch.isfinite(out).all() and (out != t).any()
        return out.contiguous()

    got = _run_head(head, garbage(pair), garbage(pair0), coords, mask, grad)
    for name in ["update", "dpair0"] + GRADS:
        assert torch.equal(ref[name], got[name]), name


def test_dispatch(monkeypatch):
    bf16 = torch.bfloat16
    assert ops.pair_coord_supported(64, bf16, 16)
    assert not ops.pair_coord_supported(64, bf16, 20)
    # L = 20: the C++ entry refuses it by name
    args = _inputs(1, 20, torch.float32, True)
    head, pair, pair0, coords, mask, _ = args
    inv_n = torch.ones(1, device="cuda")
    w1, b1, w2, b2 = (p.detach() for p in _params(head))
    with pytest.raises(RuntimeError, match="multiple of 8.*L = 20"):
        ops.pair_coord_fwd(pair, pair0, coords, inv_n, mask, w1, b1,
                           w2.view(-1), b2)
    # and the module runs eager, silently, and right
    calls = _spy(monkeypatch)
    got = _run_head(*args)
    assert not calls
    oracle = _run_eager(*args, torch.float64)
    for name in QUANTITIES + ["dpair"]:
        assert _err(got[name], oracle[name]) <= 1e-5, name
    args = _inputs(1, 16, bf16, True)
    _run_head(*args)
    assert len(calls) == 1
    monkeypatch.setenv("UNICORE_PAIR_COORD_H64", "0")
    _run_head(*args)
    assert len(calls) == 1
    monkeypatch.setenv("UNICORE_PAIR_COORD_H64", "1")
    monkeypatch.setenv("UNICORE_PAIR_COORD_EAGER", "1")
    _run_head(*args)
    assert len(calls) == 1


def test_mfma_f32_probe():
    from unicore_amd.ops import _kernels as K

    g = torch.Generator(device="cuda").manual_seed(1)
    A = torch.randn(16, 4, device="cuda", generator=g)
    B = torch.randn(4, 16, device="cuda", generator=g)
    D = K.mfma_gemm_16x16x4_f32(A, B)
    ref = A.double() @ B.double()
    assert (D.double() - ref).abs().max().item() <= 1e-5
