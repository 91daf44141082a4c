"""CPU tests of triangle self-attention (modules/triangle_attention.py) and
its place in the Evoformer model (--triangle-attention)."""

import argparse
import math
import sys

import pytest
import torch

from unicore_amd.modules import (
    TriangleAttention,
    pair_arrange,
    pair_arrange_qkv,
    pair_bias_arrange,
    pair_merge,
)


def _reference(m, pair):
    """Algorithms 13 / 14 of the AlphaFold 2 supplement, written index by
    index with einsum; shares only the parameters with the module."""
    B, I, J, C = pair.shape
    H = m.heads
    c = C // H
    x = torch.nn.functional.layer_norm(pair, (C,), m.norm.weight, m.norm.bias,
                                       m.norm.eps)
    wq, wk, wv = m.qkv.weight.view(3, H, c, C)
    q = torch.einsum("bijx,hcx->bijhc", x, wq)
    k = torch.einsum("bijx,hcx->bijhc", x, wk)
    v = torch.einsum("bijx,hcx->bijhc", x, wv)
    b = torch.einsum("bijx,hx->bijh", x, m.bias_proj.weight)
    g = torch.sigmoid(torch.einsum("bijx,yx->bijy", x, m.gate.weight)
                      + m.gate.bias).view(B, I, J, H, c)
    if m.starting:
        # a_ijk = softmax_k(q_ij . k_ik / sqrt(c) + b_jk); o_ij = sum_k a v_ik
        s = torch.einsum("bijhc,bikhc->bhijk", q, k) / math.sqrt(c)
        s = s + torch.einsum("bjkh->bhjk", b)[:, :, None, :, :]
        a = torch.softmax(s, dim=-1)
        o = torch.einsum("bhijk,bikhc->bijhc", a, v)
    else:
        # a_ijk = softmax_k(q_ij . k_kj / sqrt(c) + b_ki); o_ij = sum_k a v_kj
        s = torch.einsum("bijhc,bkjhc->bhijk", q, k) / math.sqrt(c)
        s = s + torch.einsum("bkih->bhik", b)[:, :, :, None, :]
        a = torch.softmax(s, dim=-1)
        o = torch.einsum("bhijk,bkjhc->bijhc", a, v)
    o = (g * o).reshape(B, I, J, C)
    return torch.einsum("bijx,yx->bijy", o, m.out.weight) + m.out.bias


@pytest.mark.parametrize("starting", [True, False])
def test_matches_einsum_reference_float64(starting):
    torch.manual_seed(0)
    m = TriangleAttention(16, 4, 0.0, starting=starting).double().eval()
    # LayerNorm / bias parameters away from their 1 / 0 initial values
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.3 * torch.randn_like(p))
    pair = torch.randn(2, 6, 6, 16, dtype=torch.float64)  # not symmetric
    assert not torch.allclose(pair, pair.transpose(1, 2))
    got = m(pair)
    want = _reference(m, pair)
    err = (got - want).abs().max().item()
    print(f"starting={starting}: max abs err {err:.3e}")
    assert err <= 1e-10
    # the two bias indexings really differ on this input
    other = TriangleAttention(16, 4, 0.0, starting=not starting).double().eval()
    other.load_state_dict(m.state_dict())
    assert (other(pair) - want).abs().max().item() > 1e-4


def test_ending_is_starting_on_the_transposed_pair():
    torch.manual_seed(1)
    end = TriangleAttention(16, 4, 0.0, starting=False).eval()
    start = TriangleAttention(16, 4, 0.0, starting=True).eval()
    start.load_state_dict(end.state_dict())
    pair = torch.randn(2, 6, 6, 16)
    with torch.no_grad():
        a = end(pair)
        b = start(pair.transpose(1, 2)).transpose(1, 2)
    assert torch.equal(a, b)


@pytest.mark.parametrize("transpose", [False, True])
def test_functional_fallbacks_equal_permutes(transpose):
    torch.manual_seed(2)
    B, I, J, H, D = 2, 5, 7, 4, 8
    R, T = (J, I) if transpose else (I, J)
    perm = (0, 3, 2, 1, 4) if transpose else (0, 3, 1, 2, 4)
    inv = (0, 3, 2, 1, 4) if transpose else (0, 2, 3, 1, 4)

    x = torch.randn(B, I, J, 3 * H * D).chunk(3, -1)[1].requires_grad_()
    out = pair_arrange(x, H, transpose)
    assert out.shape == (B, H, R, T, D) and out.is_contiguous()
    assert torch.equal(out, x.view(B, I, J, H, D).permute(*perm))
    g = torch.randn(B, H, R, T, D)
    (gx,) = torch.autograd.grad(out, x, g)
    assert torch.equal(gx, g.permute(*inv).reshape(B, I, J, H * D))

    qkv = torch.randn(B, I, J, 3 * H * D, requires_grad=True)
    parts = pair_arrange_qkv(qkv, H, transpose)
    gs = [torch.randn(B, H, R, T, D) for _ in range(3)]
    (gq,) = torch.autograd.grad(parts, qkv, gs)
    for n, t in enumerate(qkv.chunk(3, -1)):
        assert torch.equal(parts[n], t.reshape(B, I, J, H, D).permute(*perm))
    assert torch.equal(gq, torch.cat(
        [g.permute(*inv).reshape(B, I, J, H * D) for g in gs], -1))

    o = torch.randn(B * H * R, T, D, requires_grad=True)
    merged = pair_merge(o, B, I, J, H, transpose)
    assert merged.shape == (B, I, J, H * D)
    assert torch.equal(
        merged, o.view(B, H, R, T, D).permute(*inv).reshape(B, I, J, H * D))
    g = torch.randn(B, I, J, H * D)
    (go,) = torch.autograd.grad(merged, o, g)
    assert torch.equal(
        go, g.view(B, I, J, H, D).permute(*perm).reshape(B * H * R, T, D))
    # merge inverts arrange
    assert torch.equal(
        pair_merge(out.reshape(B * H * R, T, D), B, I, J, H, transpose), x)

    L = 6
    lin = torch.randn(B, L, L, H, requires_grad=True)
    bperm = (0, 3, 2, 1) if transpose else (0, 3, 1, 2)
    binv = (0, 3, 2, 1) if transpose else (0, 2, 3, 1)
    bias = pair_bias_arrange(lin, transpose)
    assert bias.shape == (B, H, L, L) and bias.is_contiguous()
    assert torch.equal(bias, lin.permute(*bperm))
    g = torch.randn(B, H, L, L)
    (gl,) = torch.autograd.grad(bias, lin, g)
    assert torch.equal(gl, g.permute(*binv))


def _model_args(**kw):
    args = argparse.Namespace(
        evo_layers=2, msa_dim=32, pair_dim=16, evo_heads=4, dropout=0.0,
        max_rel_pos=8,
    )
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def _build(seed=5, **kw):
    from unicore_amd.data import Dictionary
    from unicore_amd.models.evoformer import EvoformerModel

    d = Dictionary()
    for sym in ("[CLS]", "[PAD]", "[SEP]", "[UNK]"):
        d.add_symbol(sym, is_special=True)
    for i in range(20):
        d.add_symbol(f"res{i}")
    torch.manual_seed(seed)
    return EvoformerModel(_model_args(**kw), d), d


def test_model_without_the_flag_is_unchanged():
    m0, d = _build()
    m1, _ = _build(triangle_attention=False)
    assert not any("tri_att" in k for k in m0.state_dict())
    assert list(m0.state_dict()) == list(m1.state_dict())
    for (k, a), b in zip(m0.state_dict().items(), m1.state_dict().values()):
        assert torch.equal(a, b), k
    tokens = torch.randint(4, len(d), (2, 4, 8))
    m0.eval(), m1.eval()
    with torch.no_grad():
        assert torch.equal(m0(tokens), m1(tokens))


def test_model_with_the_flag_adds_two_modules_per_block():
    m0, d = _build()
    m, _ = _build(triangle_attention=True, tri_attn_heads=2)
    for blk in m.blocks:
        assert isinstance(blk.tri_att_start, TriangleAttention)
        assert isinstance(blk.tri_att_end, TriangleAttention)
        assert blk.tri_att_start.starting and not blk.tri_att_end.starting
        assert blk.tri_att_start.heads == 2
        new = [n for n, _ in blk.named_children() if n.startswith("tri_att")]
        assert new == ["tri_att_start", "tri_att_end"]
    extra = set(m.state_dict()) - set(m0.state_dict())
    assert extra and all(".tri_att_" in k for k in extra)
    assert set(m0.state_dict()) <= set(m.state_dict())
    # default head count
    m4, _ = _build(triangle_attention=True)
    assert m4.blocks[0].tri_att_end.heads == 4
    tokens = torch.randint(4, len(d), (2, 4, 8))
    out = m(tokens)
    assert out.shape == (2, 4, 8, len(d))
    out.float().pow(2).mean().backward()
    # the last block's pair stack does not reach the logits
    for n, p in m.named_parameters():
        if n.startswith("blocks.0.tri_att"):
            assert p.grad is not None and torch.isfinite(p.grad).all(), n


@pytest.mark.parametrize("extra", [[], ["--activation-checkpoint"]],
                         ids=["plain", "activation-checkpoint"])
def test_cli_training_with_triangle_attention(tmp_path, monkeypatch, extra):
    from unicore_amd.trainer import Trainer
    from unicore_cli import train as train_cli

    argv = [
        "train.py", "--task", "evoformer_synthetic", "--arch", "evoformer",
        "--loss", "masked_msa", "--optimizer", "adam",
        "--lr-scheduler", "fixed", "--lr", "1e-4",
        "--max-update", "3", "--dataset-size", "8", "--batch-size", "2",
        "--msa-depth", "8", "--residues", "16", "--evo-layers", "2",
        "--msa-dim", "32", "--pair-dim", "16", "--evo-heads", "4",
        "--triangle-attention", "--tri-attn-heads", "2",
        "--cpu", "--log-interval", "1", "--log-format", "simple",
        "--no-save", "--save-dir", str(tmp_path), "--num-workers", "0",
    ] + extra
    logs, models = [], []
    real_step = Trainer.train_step

    def spy(self, samples, **kw):
        out = real_step(self, samples, **kw)
        logs.append(out)
        models.append(self.model)
        return out

    monkeypatch.setattr(Trainer, "train_step", spy)
    monkeypatch.setattr(sys, "argv", argv)
    train_cli.cli_main()
    assert len(logs) == 3
    for out in logs:
        assert math.isfinite(float(out["loss"])), out
    model = models[-1]
    assert all(hasattr(b, "tri_att_start") for b in model.blocks)
    assert all(torch.isfinite(p).all() for p in model.parameters())
