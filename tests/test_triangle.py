"""CPU contract of modules.triangle_multiply: the eager branch IS the two
einsum lines TriangleMultiplication used inline, bit for bit."""

import torch
import torch.nn.functional as F

from unicore_amd.models import evoformer
from unicore_amd.modules import triangle_multiply

EQ = {True: "bikc,bjkc->bijc", False: "bkic,bkjc->bijc"}


def _inputs(seed=0, B=2, L=5, C=8):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, L, L, C, generator=g),
            torch.randn(B, L, L, C, generator=g))


def test_triangle_multiply_cpu_equals_einsum():
    a, b = _inputs()
    for outgoing in (True, False):
        o = triangle_multiply(a, b, outgoing)
        assert o.shape == (2, 5, 5, 8)
        assert torch.equal(o, torch.einsum(EQ[outgoing], a, b))


def test_triangle_multiply_cpu_autograd_matches_einsum():
    a, b = _inputs(1)
    d_out = torch.randn(2, 5, 5, 8, generator=torch.Generator().manual_seed(2))
    for outgoing in (True, False):
        a1, b1 = a.clone().requires_grad_(), b.clone().requires_grad_()
        a2, b2 = a.clone().requires_grad_(), b.clone().requires_grad_()
        triangle_multiply(a1, b1, outgoing).backward(d_out)
        torch.einsum(EQ[outgoing], a2, b2).backward(d_out)
        assert torch.equal(a1.grad, a2.grad)
        assert torch.equal(b1.grad, b2.grad)


def _inline_einsum_forward(self, pair, p_normed=None):
    # TriangleMultiplication.forward as it stood before triangle_multiply
    p = self.norm(pair) if p_normed is None else p_normed
    _fold_ok, gated_mul = evoformer._fold_ok, evoformer.gated_mul
    if _fold_ok(self.a_proj.bias, self.a_gate.bias, self.b_proj.bias,
                self.b_gate.bias, self.out.bias, self.gate.bias):
        a = gated_mul(F.linear(p, self.a_proj.weight),
                      F.linear(p, self.a_gate.weight),
                      self.a_proj.bias, self.a_gate.bias)
        b = gated_mul(F.linear(p, self.b_proj.weight),
                      F.linear(p, self.b_gate.weight),
                      self.b_proj.bias, self.b_gate.bias)
    else:
        a = self.a_proj(p) * torch.sigmoid(self.a_gate(p))
        b = self.b_proj(p) * torch.sigmoid(self.b_gate(p))
    if self.outgoing:
        o = torch.einsum("bikc,bjkc->bijc", a, b)
    else:
        o = torch.einsum("bkic,bkjc->bijc", a, b)
    if _fold_ok(self.out.bias, self.gate.bias):
        return gated_mul(F.linear(self.out_norm(o), self.out.weight),
                         F.linear(p, self.gate.weight),
                         self.out.bias, self.gate.bias)
    o = self.out(self.out_norm(o))
    return o * torch.sigmoid(self.gate(p))


def test_evoformer_block_cpu_bit_identical_to_inline_einsum(monkeypatch):
    torch.manual_seed(0)
    block = evoformer.EvoformerBlock(d_msa=32, d_pair=16, heads=4, dropout=0.0)
    block.eval()
    msa = torch.randn(1, 3, 6, 32)
    pair = torch.randn(1, 6, 6, 16)
    with torch.no_grad():
        m1, p1 = block(msa, pair)
        monkeypatch.setattr(evoformer.TriangleMultiplication, "forward",
                            _inline_einsum_forward)
        m2, p2 = block(msa, pair)
    assert torch.equal(m1, m2)
    assert torch.equal(p1, p2)
