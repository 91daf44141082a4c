"""CPU contract of modules.outer_product_mean: the eager branch IS the two
lines OuterProductMean used inline, bit for bit, whatever the gate says."""

import copy

import pytest
import torch
import torch.nn.functional as F

from unicore_amd import ops
from unicore_amd.models import evoformer
from unicore_amd.modules import outer_product_mean


def _inline(a, b, S, c, dtype):
    o = torch.einsum("bsic,bsjd->bijcd", a.float(), b.float()) / S
    return o.reshape(*o.shape[:3], c * c).to(dtype)


@pytest.mark.parametrize("gate", ["0", "1"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_outer_product_mean_cpu_equals_inline(monkeypatch, gate, dtype):
    monkeypatch.setenv("UNICORE_OPM_FUSED", gate)
    g = torch.Generator().manual_seed(0)
    a = torch.randn(2, 5, 3, 32, generator=g).to(dtype)
    b = torch.randn(2, 5, 4, 32, generator=g).to(dtype)
    o = outer_product_mean(a, b)
    assert o.shape == (2, 3, 4, 1024) and o.dtype == dtype
    assert torch.equal(o, _inline(a, b, 5, 32, dtype))


@pytest.mark.parametrize("gate", ["0", "1"])
def test_outer_product_mean_cpu_autograd_matches_inline(monkeypatch, gate):
    monkeypatch.setenv("UNICORE_OPM_FUSED", gate)
    g = torch.Generator().manual_seed(1)
    a = torch.randn(1, 6, 4, 8, generator=g)
    b = torch.randn(1, 6, 4, 8, generator=g)
    d_out = torch.randn(1, 4, 4, 64, generator=g)
    a1, b1 = a.clone().requires_grad_(), b.clone().requires_grad_()
    a2, b2 = a.clone().requires_grad_(), b.clone().requires_grad_()
    outer_product_mean(a1, b1).backward(d_out)
    _inline(a2, b2, 6, 8, torch.float32).backward(d_out)
    assert torch.equal(a1.grad, a2.grad)
    assert torch.equal(b1.grad, b2.grad)


def _inline_opm_forward(self, msa, skip_out_bias=False, x_normed=None):
    # OuterProductMean.forward as it stood before outer_product_mean
    x = self.norm(msa) if x_normed is None else x_normed
    a = self.a(x)
    b = self.b(x)
    o = torch.einsum("bsic,bsjd->bijcd", a.float(), b.float()) / msa.shape[1]
    o = o.reshape(*o.shape[:3], self.c * self.c).to(msa.dtype)
    if skip_out_bias:
        return F.linear(o, self.out.weight)
    return self.out(o)


def test_evoformer_block_cpu_bit_identical_to_inline_opm(monkeypatch):
    torch.manual_seed(0)
    block = evoformer.EvoformerBlock(d_msa=32, d_pair=16, heads=4, dropout=0.0)
    block2 = copy.deepcopy(block)
    msa = torch.randn(1, 3, 6, 32)
    pair = torch.randn(1, 6, 6, 16)
    g = torch.Generator().manual_seed(1)
    d_m = torch.randn(1, 3, 6, 32, generator=g)
    d_p = torch.randn(1, 6, 6, 16, generator=g)

    def run(blk):
        m_in = msa.clone().requires_grad_()
        p_in = pair.clone().requires_grad_()
        m, p = blk(m_in, p_in)
        torch.autograd.backward([m, p], [d_m, d_p])
        grads = {n: q.grad for n, q in blk.named_parameters()}
        return m.detach(), p.detach(), m_in.grad, p_in.grad, grads

    m1, p1, dm1, dp1, g1 = run(block)
    monkeypatch.setattr(evoformer.OuterProductMean, "forward", _inline_opm_forward)
    m2, p2, dm2, dp2, g2 = run(block2)
    assert torch.equal(m1, m2) and torch.equal(p1, p2)
    assert torch.equal(dm1, dm2) and torch.equal(dp1, dp2)
    assert set(g1) == set(g2)
    for n in g1:
        assert (g1[n] is None) == (g2[n] is None), n
        if g1[n] is not None:
            assert torch.equal(g1[n], g2[n]), n


def test_opm_supported_is_width_32_bf16_only():
    assert ops.opm_supported(32, 32, torch.bfloat16)
    for c, d in ((16, 16), (64, 64), (32, 16), (16, 32), (0, 0), (33, 33)):
        assert not ops.opm_supported(c, d, torch.bfloat16)
    for dtype in (torch.float32, torch.float16, torch.float64):
        assert not ops.opm_supported(32, 32, dtype)
