"""Head-dim-8 pair-track attention (csrc/pair_attn_d8.hip) against the plain
expression in float64, with the method of test_pair_attn_gpu.py.

Reference: logits = q k^T + bias, o = (keep / (1 - p) * softmax(logits)) v,
and the autograd gradients of sum(o * d_o) + sum(logits * d_logits), in
float64 on the bf16-rounded inputs.  `chain` is the same expression in bf16
torch ops on the same inputs and keep mask.  With err(x) = max|x - ref| /
max|ref|, every quantity obeys

    err(kernel) <= 2 * err(chain) + 1e-6

logits are compared over real keys only; padded keys (finfo.min in the bias)
must come out <= -1e30.
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
FMIN = torch.finfo(BF16).min
QUANTITIES = ["o", "logits", "lse", "dq", "dk", "dv", "dbias"]


def _inputs(B, H, L, pad, seed=0, D=8, dtype=BF16):
    """q, k, v, d_o (B*H, L, D); bias, d_logits (B, H, L, L).  pad: the last
    3 keys of sample 0 and the last 17 of the last sample carry finfo.min."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dtype)

    q, k, v, d_o = (rnd(B * H, L, D, scale=s) for s in (0.4, 1.0, 1.0, 0.3))
    bias, d_logits = rnd(B, H, L, L), rnd(B, H, L, L, scale=0.05)
    if pad:
        bias[0, :, :, L - 3:] = FMIN
        bias[-1, :, :, L - 17:] = FMIN
    return q, k, v, bias, d_o, d_logits


def _expr(ct, q, k, v, bias, d_o, d_logits, keep=None, p=0.0):
    q, k, v, bias = (t.detach().to(ct).requires_grad_() for t in (q, k, v, bias))
    logits = (q @ k.transpose(-1, -2)).view(bias.shape) + bias
    prob = torch.softmax(logits, dim=-1)
    if keep is not None:
        prob = prob * (keep.to(ct) / (1.0 - p))
    o = prob.view(-1, *prob.shape[2:]) @ v
    loss = (o * d_o.to(ct)).sum()
    if d_logits is not None:
        loss = loss + (logits * d_logits.to(ct)).sum()
    loss.backward()
    res = [o, logits, torch.logsumexp(logits, dim=-1), q.grad, k.grad, v.grad,
           bias.grad]
    return {n: t.detach().double() for n, t in zip(QUANTITIES, res)}


def _kernel(q, k, v, bias, d_o, d_logits, p=0.0, training=False):
    o, logits, lse, seed = ops.pair_attn_fwd(q, k, v, bias, p, training)
    grads = ops.pair_attn_bwd(d_o, d_logits, q, k, v, o, lse, logits, p,
                              training and p > 0, int(seed))
    return dict(zip(QUANTITIES, [o, logits, lse, *grads])), int(seed)


def _check(kern, ref, chain, bias):
    real = bias > -1e30
    assert (kern["logits"][~real] <= -1e30).all()
    for name, r in ref.items():
        got, ch = kern[name].double().reshape(r.shape), chain[name]
        if name == "logits":
            got, ch, r = (t.masked_fill(~real, 0.0) for t in (got, ch, r))
        scale = r.abs().max().item()
        e_k = (got - r).abs().max().item() / scale
        e_c = (ch - r).abs().max().item() / scale
        print(f"{name}: kernel {e_k:.3e} chain {e_c:.3e}")
        assert math.isfinite(e_k) and e_k <= 2 * e_c + 1e-6, (name, e_k, e_c)


CASES = [(L, dims, pad, with_dl) for L in (64, 128, 192)
         for dims in ((1, 2), (2, 3)) for pad in (False, True)
         for with_dl in (False, True)]
# all eight dq accumulators and the largest LDS residency
CASES.append((512, (1, 2), True, True))


@pytest.mark.parametrize("L,dims,pad,with_dl", CASES)
def test_pair_attn_d8_parity(L, dims, pad, with_dl):
    q, k, v, bias, d_o, d_logits = _inputs(*dims, L, pad)
    if not with_dl:
        d_logits = None
    kern, _ = _kernel(q, k, v, bias, d_o, d_logits)
    _check(kern, _expr(torch.float64, q, k, v, bias, d_o, d_logits),
           _expr(BF16, q, k, v, bias, d_o, d_logits), bias)


@pytest.fixture(scope="module")
def keep_case():
    """L / 8 = 8 forwards from one generator state, each with one 8-row
    identity block in V, read out the keep mask of that state."""
    B, H, L, p = 2, 3, 64, 0.3
    inputs = _inputs(B, H, L, True, seed=1)
    q, k, _, bias = inputs[:4]
    cols, seeds = [], set()
    for c in range(L // 8):
        v_id = torch.zeros(B * H, L, 8, device="cuda", dtype=BF16)
        v_id[:, 8 * c:8 * (c + 1)] = torch.eye(8, device="cuda", dtype=BF16)
        torch.manual_seed(13)
        o_c, _, _, seed_c = ops.pair_attn_fwd(q, k, v_id, bias, p, True)
        cols.append(o_c != 0)
        seeds.add(int(seed_c))
    assert len(seeds) == 1, seeds
    return inputs, torch.cat(cols, dim=-1).view(B, H, L, L), p, seeds.pop()


def test_pair_attn_d8_dropout_rate(keep_case):
    (_, _, _, bias, _, _), keep, p, _ = keep_case
    real = bias > -1e30   # P is exactly 0 at padded keys: nothing to read there
    assert not keep[~real].any()
    n = int(real.sum())
    rate = keep[real].float().mean().item()
    sigma = math.sqrt(p * (1.0 - p) / n)
    assert abs(rate - (1.0 - p)) < 5.0 * sigma + 2.0 ** -16, (rate, sigma)


@pytest.mark.parametrize("with_dl", [False, True])
def test_pair_attn_d8_dropout_explicit_mask(keep_case, with_dl):
    (q, k, v, bias, d_o, d_logits), keep, p, seed0 = keep_case
    if not with_dl:
        d_logits = None
    torch.manual_seed(13)
    kern, seed = _kernel(q, k, v, bias, d_o, d_logits, p, True)
    assert seed == seed0
    _check(kern, _expr(torch.float64, q, k, v, bias, d_o, d_logits, keep, p),
           _expr(BF16, q, k, v, bias, d_o, d_logits, keep, p), bias)


def test_pair_attn_d8_double_run_bitwise():
    inputs = _inputs(2, 3, 192, True, seed=2)
    runs = []
    for _ in range(2):
        torch.manual_seed(7)
        runs.append(_kernel(*inputs, 0.2, True)[0])
    for name in QUANTITIES:
        assert torch.equal(runs[0][name], runs[1][name]), name


def test_pair_attn_d8_supported():
    assert ops.pair_attn_supported(64, 8, BF16)
    assert ops.pair_attn_supported(512, 8, BF16)


@pytest.mark.parametrize("L,D,dtype", [(96, 8, BF16), (576, 8, BF16),
                                       (64, 16, BF16), (64, 8, torch.float16)])
def test_pair_attn_d8_host_refusals(L, D, dtype):
    assert not ops.pair_attn_supported(L, D, dtype)
    q, k, v, bias = _inputs(2, 2, L, False, D=D, dtype=dtype)[:4]
    with pytest.raises(RuntimeError, match="pair_attn_forward"):
        ops.pair_attn_fwd(q, k, v, bias, 0.0, False)
    lse = torch.zeros(q.shape[:2], device="cuda")
    with pytest.raises(RuntimeError, match="pair_attn_backward"):
        ops.pair_attn_bwd(v, None, q, k, v, v, lse, bias, 0.0, False, 0)


def _module_run(mod, x, bias, dtype, d_out, d_logits):
    mod.to(dtype).zero_grad(set_to_none=True)
    x, bias = (t.detach().to(dtype).requires_grad_() for t in (x, bias))
    out, logits = mod(x, attn_bias=bias, return_logits=True)
    ((out * d_out.to(dtype)).sum() + (logits * d_logits.to(dtype)).sum()).backward()
    got = [out, logits, x.grad, bias.grad, *(p.grad for p in mod.parameters())]
    return [t.detach().double() for t in got]


def test_module_64_heads_gates(monkeypatch):
    """SelfMultiheadAttention(512, 64) at L 128: outputs and input / bias /
    parameter gradients with both gates on are within twice the chain's own
    error against an fp32 run on the same (bf16-representable) weights.  The
    fused entry runs once with the gates on and not at all with either off."""
    from unicore_amd.modules import SelfMultiheadAttention

    L, H = 128, 64
    torch.manual_seed(3)
    mod = SelfMultiheadAttention(512, H, dropout=0.0).cuda()
    with torch.no_grad():
        for prm in mod.parameters():
            prm.copy_(prm.to(BF16))
    x, d_out = (torch.randn(2, L, 512, device="cuda").to(BF16).float() for _ in range(2))
    bias, d_logits = (torch.randn(2, H, L, L, device="cuda").to(BF16).float() * s
                      for s in (1.0, 0.05))
    calls = []
    fwd = ops.pair_attn_fwd
    monkeypatch.setattr(ops, "pair_attn_fwd",
                        lambda *a: calls.append(1) or fwd(*a))
    monkeypatch.setenv("UNICORE_PAIR_ATTN", "0")
    monkeypatch.setenv("UNICORE_PAIR_ATTN_D8", "1")
    ref = _module_run(mod, x, bias, torch.float32, d_out, d_logits)
    off = _module_run(mod, x, bias, BF16, d_out, d_logits)
    monkeypatch.setenv("UNICORE_PAIR_ATTN", "1")
    monkeypatch.setenv("UNICORE_PAIR_ATTN_D8", "0")
    _module_run(mod, x, bias, BF16, d_out, d_logits)
    assert not calls
    monkeypatch.setenv("UNICORE_PAIR_ATTN_D8", "1")
    on = _module_run(mod, x, bias, BF16, d_out, d_logits)
    assert len(calls) == 1
    for i, r in enumerate(ref):
        scale = r.abs().max().item()
        e_on = (on[i] - r).abs().max().item() / scale
        e_off = (off[i] - r).abs().max().item() / scale
        print(f"[{i}]: on {e_on:.3e} off {e_off:.3e}")
        assert e_on <= 2 * e_off + 1e-6, (i, e_on, e_off)
