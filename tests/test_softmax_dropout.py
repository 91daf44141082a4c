"""CPU tests of the softmax-dropout shim (`SoftmaxDropoutFast`,
`_prep_additive`, the kernel route of `softmax_dropout`) against a pure-torch
stand-in for the four `ops.softmax_dropout_*` entry points.

The stand-in implements the documented kernel contract and nothing else:
source row ``((b // od) % nb) * sq + qi % sq``, softmax written in place over
the input, the keep mask as a bitfield (one byte per 8 keys, bit j = key
8*byte + j), and the fused backward's ``(bb*bq, k)`` fp32 bias gradient. With
it in place of `ops`, the shim runs on CPU float64 tensors, so its
`view(a, bb, od, q, k)` fallback reduction, the `bq == 1` sum and the
broadcast description are checked against autograd through the eager
expression without a GPU.
"""

import importlib
import itertools

import pytest
import torch

# the package re-exports the function under the module's own name
sd = importlib.import_module("unicore_amd.modules.softmax_dropout")


def _src_index(nb, sq, od, n, q):
    b = torch.arange(n)
    qi = torch.arange(q)
    return ((b // od) % nb)[:, None] * sq + (qi % sq)[None, :]  # (n, q)


def _unpack(dmask, k):
    bits = torch.arange(8, dtype=torch.uint8)
    keep = (dmask.unsqueeze(-1) >> bits) & 1
    return keep.reshape(*dmask.shape[:-1], k).bool()


def _pack(keep):
    n, q, k = keep.shape
    w = (1 << torch.arange(8)).to(torch.int64)
    return (keep.view(n, q, k // 8, 8).to(torch.int64) * w).sum(-1).to(torch.uint8)


class StandIn:
    """Pure-torch `ops.softmax_dropout_*`; `fused` decides what
    `softmax_dropout_bwd_bias_supported` answers."""

    def __init__(self, fused):
        self.fused = fused
        self.calls = {"fwd": 0, "bwd": 0, "bwd_bias": 0}
        self.last_dmask = None

    def softmax_dropout_fwd(self, is_training, inputs, mask, mask_od, bias,
                            bias_od, p):
        self.calls["fwd"] += 1
        assert inputs.dim() == 3 and inputs.is_contiguous()
        n, q, k = inputs.shape
        x = inputs
        for src, od in ((mask, mask_od), (bias, bias_od)):
            if src is None:
                continue
            assert src.dim() == 3 and src.is_contiguous() and src.shape[2] == k
            nb, sq, _ = src.shape
            x = x + src.reshape(nb * sq, k)[_src_index(nb, sq, od, n, q)]
        inputs.copy_(torch.softmax(x, dim=-1))
        if is_training and p > 0:
            assert k % 8 == 0
            keep = torch.rand(n, q, k) >= p
            dmask = _pack(keep)
            out = torch.where(keep, inputs / (1.0 - p), torch.zeros_like(inputs))
        else:
            dmask = torch.empty(0, dtype=torch.uint8)
            out = inputs
        self.last_dmask = dmask
        return out, dmask, inputs

    @staticmethod
    def _dx(g, y, dmask, p):
        t = g
        if dmask.numel() > 0:
            t = torch.where(_unpack(dmask, g.shape[-1]), g / (1.0 - p),
                            torch.zeros_like(g))
        return y * (t - (t * y).sum(-1, keepdim=True))

    def softmax_dropout_bwd(self, g, y, dmask, p):
        self.calls["bwd"] += 1
        g.copy_(self._dx(g, y, dmask, p))
        return g

    def softmax_dropout_bwd_bias_supported(self, n, q, k, bb, bq, od):
        return self.fused

    def softmax_dropout_bwd_bias(self, g, y, dmask, p, bb, bq, od):
        self.calls["bwd_bias"] += 1
        n, q, k = g.shape
        a = n // (bb * od)
        g.copy_(self._dx(g, y, dmask, p))
        # row = ((t*bb + jb)*od + e)*q + m*bq + qb reduces onto (jb, qb)
        dbias = g.view(a, bb, od, q // bq, bq, k).sum(dim=(0, 2, 3))
        return g, dbias.reshape(bb * bq, k).float()


@pytest.fixture(params=[False, True], ids=["fallback", "fused"])
def standin(request, monkeypatch):
    from unicore_amd import ops

    s = StandIn(request.param)
    for name in ("softmax_dropout_fwd", "softmax_dropout_bwd",
                 "softmax_dropout_bwd_bias_supported",
                 "softmax_dropout_bwd_bias"):
        monkeypatch.setattr(ops, name, getattr(s, name))
    return s


def _check(standin, x, mask, bias, p=0.0, tol=1e-12):
    """Run the kernel route and the eager expression on the same float64
    inputs; compare output and the gradients of x and (if given) bias."""
    torch.manual_seed(5)
    xk = x.clone().requires_grad_(True)
    bk = None if bias is None else bias.clone().requires_grad_(True)
    out = sd._kernel_softmax_dropout(xk, p, True, mask, bk, False)
    gout = torch.randn_like(out)
    out.backward(gout.clone())

    xr = x.clone().requires_grad_(True)
    br = None if bias is None else bias.clone().requires_grad_(True)
    # (a source with extra leading 1-dims makes the eager result grow them)
    ref = sd._eager_softmax_dropout(xr, 0.0, True, mask, br).view(x.shape)
    if p > 0:
        keep = _unpack(standin.last_dmask, x.shape[-1]).view(x.shape)
        ref = ref * keep / (1.0 - p)
    ref.backward(gout)

    assert torch.equal(xk.detach(), x), "inplace=False must not touch x"
    assert (out - ref).abs().max().item() < tol
    assert (xk.grad - xr.grad).abs().max().item() < tol
    if bias is not None:
        assert bk.grad.shape == bias.shape
        # the fused stand-in hands the bias gradient back in fp32, as the
        # kernel does; the fallback reduction stays in float64
        btol = 1e-5 if standin.fused and standin.calls["bwd_bias"] else tol
        assert (bk.grad - br.grad).abs().max().item() < btol, (
            (bk.grad - br.grad).abs().max().item())


def test_bias_and_mask_gradients_over_broadcast_patterns(standin):
    """Every 0/1 pattern of kept batch dims, for the shapes of
    `test_broadcast_descr_matches_torch_semantics`, with sq in {1, q}: the
    describable ones go to the stand-in kernel, the others to the eager
    merge, and all of them match autograd through the eager expression."""
    torch.manual_seed(9)
    q, k = 2, 8
    described = merged = 0
    for batch_dims in [(2,), (2, 3), (2, 3, 4)]:
        m = len(batch_dims)
        x = torch.randn(*batch_dims, q, k, dtype=torch.float64)
        for keep in itertools.product([False, True], repeat=m):
            sb = tuple(b if kp else 1 for b, kp in zip(batch_dims, keep))
            # the mask keeps the complementary dims, so both descriptors
            # are exercised with different (nb, od) in one call
            mb = tuple(1 if kp else b for b, kp in zip(batch_dims, keep))
            for sq in (1, q):
                bias = torch.randn(*sb, sq, k, dtype=torch.float64)
                mask = torch.randn(*mb, q + 1 - sq, k, dtype=torch.float64)
                before = dict(standin.calls)
                _check(standin, x, mask, bias)
                descr = sd._broadcast_descr(sb, batch_dims)
                took_bias = (standin.calls["bwd_bias"] - before["bwd_bias"]
                             + standin.calls["bwd"] - before["bwd"])
                assert took_bias == 1
                if descr is None:
                    merged += 1
                    # autograd does the bias gradient of a merged source
                    assert standin.calls["bwd_bias"] == before["bwd_bias"]
                else:
                    described += 1
                    fused = standin.calls["bwd_bias"] - before["bwd_bias"]
                    assert fused == (1 if standin.fused else 0)
    assert described >= 20 and merged >= 2, (described, merged)


@pytest.mark.parametrize("batch,q,k,bias_shape", [
    ((2, 4, 3), 4, 8, (2, 4, 1, 4, 8)),      # od = 3, a = 1
    ((2, 4, 3), 4, 8, (1, 4, 1, 4, 8)),      # a = 2 and od = 3
    ((2, 4, 3), 4, 8, (1, 4, 1, 1, 8)),      # bq = 1 with od = 3
    ((2, 4), 4, 8, (1, 4, 1, 8)),            # bq = 1, od = 1
    ((5, 2), 3, 8, (2, 3, 8)),               # bias shorter than the batch
])
def test_call_site_reductions(standin, batch, q, k, bias_shape):
    torch.manual_seed(10)
    x = torch.randn(*batch, q, k, dtype=torch.float64)
    bias = torch.randn(*bias_shape, dtype=torch.float64)
    _check(standin, x, None, bias)
    _check(standin, x, None, bias, p=0.4)


def test_one_dim_mask_leading_ones_and_eager_merge(standin):
    torch.manual_seed(11)
    B, H, S, q, k = 2, 3, 4, 2, 8
    x = torch.randn(B, H, S, q, k, dtype=torch.float64)
    # 1-D mask (k,)
    _check(standin, x, torch.randn(k, dtype=torch.float64), None)
    # a source with more dims than the input, all extra ones of size 1
    bias = torch.randn(1, 1, 1, H, 1, q, k, dtype=torch.float64)
    _check(standin, x, None, bias)
    # (B, 1, S) keeps two separated dims: not one block, merged eagerly
    mask = torch.randn(B, 1, S, 1, k, dtype=torch.float64)
    assert sd._broadcast_descr((B, 1, S), (B, H, S)) is None
    bias = torch.randn(B, H, 1, q, k, dtype=torch.float64)
    before = standin.calls["fwd"]
    _check(standin, x, mask, bias)
    assert standin.calls["fwd"] == before + 1
    # a source whose q is neither 1 nor q cannot be described either
    x1 = torch.randn(B, 4, k, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        sd._kernel_softmax_dropout(
            x1, 0.0, True, torch.randn(B, 2, k, dtype=torch.float64), None,
            False)


def test_width_not_multiple_of_8_with_dropout_uses_torch_dropout(standin):
    """The kernel's dropout needs k % 8 == 0; other widths take the fused
    softmax with p = 0 and torch's dropout, like rows wider than 4096."""
    torch.manual_seed(12)
    x = torch.randn(3, 2, 13, dtype=torch.float64)
    out = sd._kernel_softmax_dropout(x, 0.5, True, None, None, False)
    assert standin.last_dmask.numel() == 0
    y = torch.softmax(x, -1)
    kept = out != 0
    assert 0 < kept.sum().item() < kept.numel()
    assert (out[kept] - 2.0 * y[kept]).abs().max().item() < 1e-12
    # not training: no dropout at all, on either route
    out = sd._kernel_softmax_dropout(x, 0.5, False, None, None, False)
    assert (out - y).abs().max().item() < 1e-12


def test_standin_bitfield_layout():
    keep = torch.zeros(1, 1, 16, dtype=torch.bool)
    keep[0, 0, 1] = keep[0, 0, 15] = True
    dmask = _pack(keep)
    assert dmask.tolist() == [[[2, 128]]]
    assert torch.equal(_unpack(dmask, 16), keep)
