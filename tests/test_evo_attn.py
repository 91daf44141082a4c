"""CPU side of the head-dim-32 fused attention: what the module helper
accepts, and that the UNICORE_EVO_ATTN gate changes nothing off the GPU."""

import pytest
import torch

from unicore_amd.models.evoformer import (
    MSAColumnAttention,
    MSARowAttentionWithPairBias,
)
from unicore_amd.modules import TriangleAttention
from unicore_amd.modules.evo_attention import _evo_plan, evo_attention

BF16 = torch.bfloat16


def _qkv(dims=(1, 2, 3), T=64, D=32, dtype=BF16):
    return [torch.zeros(*dims, T, D, dtype=dtype) for _ in range(3)]


def test_plan_accepts_the_three_sites():
    bias = torch.zeros(1, 2, 1, 64, 64, dtype=BF16)
    row_mask = torch.zeros(1, 1, 3, 1, 64, dtype=BF16)
    b, b_od, m, m_od = _evo_plan(*_qkv(), bias, row_mask)
    assert (tuple(b.shape), b_od, tuple(m.shape), m_od) == ((2, 64, 64), 3, (3, 1, 64), 1)
    # column attention: batches (B, L, H), mask (B, L, 1, 1, S)
    col_mask = torch.zeros(2, 5, 1, 1, 64, dtype=BF16)
    _, _, m, m_od = _evo_plan(*_qkv(dims=(2, 5, 4)), None, col_mask)
    assert (tuple(m.shape), m_od) == ((10, 1, 64), 4)


@pytest.mark.parametrize("case", ["fp16", "fp32", "head dim 64", "T = 96", "T = 576",
                                  "B > 1 row mask", "bias q = 1", "fp32 bias"])
def test_plan_refuses(case):
    dims = (2, 2, 3) if case == "B > 1 row mask" else (1, 2, 3)
    T = {"T = 96": 96, "T = 576": 576}.get(case, 64)
    D = 64 if case == "head dim 64" else 32
    dtype = {"fp16": torch.float16, "fp32": torch.float32}.get(case, BF16)
    bias = mask = None
    if case == "B > 1 row mask":
        mask = torch.zeros(2, 1, 3, 1, T, dtype=BF16)
    if case == "bias q = 1":
        bias = torch.zeros(1, 2, 1, 1, T, dtype=BF16)
    if case == "fp32 bias":
        bias = torch.zeros(1, 2, 1, T, T)
    assert _evo_plan(*_qkv(dims, T, D, dtype), bias, mask) is None


def test_helper_returns_none_on_cpu(monkeypatch):
    monkeypatch.setenv("UNICORE_EVO_ATTN", "1")
    assert _evo_plan(*_qkv(), None, None) is not None
    assert evo_attention(*_qkv(), None, None, 0.0, False) is None


@pytest.mark.parametrize("kind", ["tri_start", "tri_end", "msa_row", "msa_col"])
def test_modules_ignore_the_gate_on_cpu(kind, monkeypatch):
    torch.manual_seed(0)
    pair = torch.randn(1, 64, 64, 64)
    msa = torch.randn(1, 3, 64, 64)
    if kind == "msa_row":
        mod, args = MSARowAttentionWithPairBias(64, 64, 2, 0.0), (msa, pair)
    elif kind == "msa_col":
        mod, args = MSAColumnAttention(64, 2, 0.0), (msa.transpose(1, 2),)
    else:
        mod, args = TriangleAttention(64, 2, 0.0, starting=kind == "tri_start"), (pair,)
    mod = mod.to(BF16)
    args = tuple(a.to(BF16) for a in args)
    monkeypatch.delenv("UNICORE_EVO_ATTN", raising=False)
    want = mod(*args)
    monkeypatch.setenv("UNICORE_EVO_ATTN", "1")
    assert torch.equal(mod(*args), want)
