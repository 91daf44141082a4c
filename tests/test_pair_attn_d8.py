"""Head dim 8 (64 heads at embed 512) on the CPU: the pair_attention helper
declines, and the 64-head layer's return_pair shapes."""

import torch

from unicore_amd.models.mol_pairbias import PairBiasEncoderLayer
from unicore_amd.modules.pair_attention import pair_attention


def test_d8_cpu_declines_and_layer_shapes(monkeypatch):
    monkeypatch.setenv("UNICORE_PAIR_ATTN", "1")
    monkeypatch.setenv("UNICORE_PAIR_ATTN_D8", "1")
    B, H, L = 2, 64, 64
    q, k, v = (torch.zeros(B * H, L, 8, dtype=torch.bfloat16) for _ in range(3))
    bias = torch.zeros(B, H, L, L, dtype=torch.bfloat16)
    assert pair_attention(q, k, v, bias, B, H, 0.1, True) is None

    layer = PairBiasEncoderLayer(512, 256, H, 0.0, 0.0, 0.0)
    x, pair = layer(torch.randn(B, 24, 512), torch.randn(B, H, 24, 24), None,
                    return_pair=True)
    assert x.shape == (B, 24, 512) and pair.shape == (B, H, 24, 24)
