"""fp32-MFMA kernels of the pair distance head at H = 64
(csrc/pair_dist_h64.hip) against the eager definition run in float64.

Method of test_pair_coord_h64_gpu.py. Oracle: pair_dist_eager in fp64 on the
same, already rounded, inputs. Baseline: pair_dist_eager in fp32. With
err(q) = max|q - oracle| / (max|oracle| + 1e-12):

  dist, dW1, db1, dgamma, dbeta, dw2, db2, and dpair for fp32 inputs:
      err(kernel) <= 4 * err(baseline) + 1e-6
  dpair for bf16 inputs: err <= 2^-8, one bf16 rounding.
"""

import functools

import pytest
import torch

from unicore_amd import ops
from unicore_amd.modules import PairDistHead
from unicore_amd.modules.pair_dist import pair_dist_eager

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

# (B, L): one tile, one sample left with a single atom; less than a tile; a
# half-tile tail; several tiles, a tail and more than one staging step;
# beyond 128
SHAPES = [(2, 16), (1, 8), (1, 24), (2, 72), (1, 136)]
DTYPES = [torch.float32, torch.bfloat16]
PARAMS = ["dW1", "db1", "dgamma", "dbeta", "dw2", "db2"]
ALL = ["dist", "dpair"] + PARAMS


@pytest.fixture(autouse=True)
def _gate_on(monkeypatch):
    monkeypatch.setenv("UNICORE_PAIR_DIST_H64", "1")
    monkeypatch.delenv("UNICORE_PAIR_COORD_EAGER", raising=False)


def _inputs(B, L, dtype, padded, seed=0, H=64):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(seed)
    mask = None
    pair = (1.5 * torch.randn(B, H, L, L, device=dev, generator=g)).to(dtype)
    if padded:
        mask = torch.zeros(B, L, dtype=torch.bool, device=dev)
        for b, n in enumerate(((3, L - 1) if L == 16 else (3, 0))[:B]):
            if n:
                mask[b, L - n:] = True
        # what the gaussian pair bias leaves at padded keys
        pair = pair.masked_fill(mask.view(B, 1, 1, L), torch.finfo(dtype).min)
    head = PairDistHead(H).to(dev)
    with torch.no_grad():
        for p in head.parameters():
            # dense rows of 64 terms: keep the hidden units O(1)
            p.copy_(0.2 * torch.randn(p.shape, device=dev, generator=g))
        head.layer_norm.weight.add_(1.0)  # gamma around 1, beta around 0
    grad = torch.randn(B, L, L, device=dev, generator=g)
    return head, pair.contiguous(), mask, grad


def _params(head):
    return [head.dense.weight, head.dense.bias, head.layer_norm.weight,
            head.layer_norm.bias, head.out_proj.weight, head.out_proj.bias]


def _run(head, pair, mask, grad, ct=None):
    """the module (ct None), or the eager definition in ct"""
    pair = pair.detach().clone().requires_grad_(True)
    if ct is None:
        head.zero_grad(set_to_none=True)
        out = head(pair, mask)
        out.backward(grad)
        grads = [p.grad.clone() for p in _params(head)]
    else:
        pair = pair.detach().to(ct).requires_grad_(True)
        params = [p.detach().to(ct).requires_grad_(True) for p in _params(head)]
        out = pair_dist_eager(pair, *params, mask, head.layer_norm.eps)
        out.backward(grad.to(ct))
        grads = [p.grad for p in params]
    res = dict(zip(PARAMS, grads))
    res["dw2"] = res["dw2"].view(-1)
    res.update(dist=out.detach(), dpair=pair.grad)
    return res


def _spy(monkeypatch):
    calls = []
    real = ops.pair_dist_fwd

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "pair_dist_fwd", spy)
    return calls


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, padded):
    """kernel (and how often ops.pair_dist_fwd was reached), fp32 eager
    baseline and fp64 oracle of one case, computed once, only read after"""
    args = _inputs(*shape, dtype, padded)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("UNICORE_PAIR_DIST_H64", "1")
        calls = _spy(mp)
        kernel = _run(*args)
    return (args, kernel, len(calls), _run(*args, torch.float32),
            _run(*args, torch.float64))


def _err(q, oracle):
    q, oracle = q.double(), oracle.double()
    return ((q - oracle).abs().max() / (oracle.abs().max() + 1e-12)).item()


def _id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    return "pad" if v else "nopad"


@pytest.mark.parametrize(
    "shape,dtype,padded",
    [(s, d, p) for s in SHAPES for d in DTYPES for p in (False, True)],
    ids=_id,
)
def test_parity_and_structure(shape, dtype, padded):
    (head, pair, mask, grad), kernel, calls, base, oracle = _case(
        shape, dtype, padded)
    assert calls == 1
    failures = []
    for name in ALL:
        want = dtype if name == "dpair" else torch.float32
        assert kernel[name].dtype == want
        assert kernel[name].shape == oracle[name].shape
        ek, eb = _err(kernel[name], oracle[name]), _err(base[name], oracle[name])
        print(f"pair_dist_h64 {_id(shape)} {_id(dtype)} {_id(padded)} {name}: "
              f"err(kernel)={ek:.3e} err(eager fp32)={eb:.3e}")
        if name == "dpair" and dtype != torch.float32:
            ok = ek <= 2.0 ** -8
        else:
            ok = ek <= 4 * eb + 1e-6
        if not ok:
            failures.append((name, ek, eb))
    assert not failures, failures
    dist, dpair = kernel["dist"], kernel["dpair"]
    assert torch.equal(dist, dist.transpose(1, 2))
    assert dpair.abs().max() > 0
    if padded:
        B, L = mask.shape
        dead = mask.view(B, L, 1) | mask.view(B, 1, L)
        assert dead.any()
        assert torch.equal(dist[dead], torch.zeros_like(dist[dead]))
        dead = dead.unsqueeze(1).expand_as(dpair)
        assert torch.equal(dpair[dead], torch.zeros_like(dpair[dead]))


def test_deterministic():
    args = _inputs(2, 72, torch.bfloat16, True, seed=3)
    a, b = _run(*args), _run(*args)
    for name in ALL:
        assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_padded_entries_never_enter(dtype):
    head, pair, mask, grad = _inputs(2, 16, dtype, True)
    ref = _run(head, pair, mask, grad)
    fill = torch.finfo(dtype).min
    g = torch.Generator(device="cuda").manual_seed(9)
    r = torch.rand(pair.shape, device="cuda", generator=g) * 2 - 1
    garbage = torch.where(pair == fill, (pair.float() * r).to(dtype), pair)
    assert torch.isfinite(garbage).all() and (garbage != pair).any()
    got = _run(head, garbage.contiguous(), mask, grad)
    for name in ALL:
        assert torch.equal(ref[name], got[name]), name


def test_dispatch(monkeypatch):
    bf16 = torch.bfloat16
    assert ops.pair_dist_supported(64, bf16, 16)
    assert not ops.pair_dist_supported(64, bf16, 20)
    assert not ops.pair_dist_supported(8, bf16, 16)
    # L = 20: the C++ entry refuses it by name
    args = _inputs(1, 20, torch.float32, True)
    head, pair, mask, _ = args
    w = [p.detach() for p in _params(head)]
    w[4] = w[4].view(-1)
    with pytest.raises(RuntimeError, match="multiple of 8.*L = 20"):
        ops.pair_dist_fwd(pair, mask, *w, 1e-5)
    # and the module runs eager there and at H = 8, silently, and right
    calls = _spy(monkeypatch)
    for eager_args in (args, _inputs(2, 16, torch.float32, True, H=8)):
        got = _run(*eager_args)
        oracle = _run(*eager_args, torch.float64)
        for name in ALL:
            assert _err(got[name], oracle[name]) <= 1e-5, name
    assert not calls
    args = _inputs(1, 16, bf16, True)
    _run(*args)
    assert len(calls) == 1
    monkeypatch.setenv("UNICORE_PAIR_DIST_H64", "0")
    _run(*args)
    assert len(calls) == 1
    monkeypatch.setenv("UNICORE_PAIR_DIST_H64", "1")
    monkeypatch.setenv("UNICORE_PAIR_COORD_EAGER", "1")
    _run(*args)
    assert len(calls) == 1
