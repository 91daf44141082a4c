"""return_logits of SelfMultiheadAttention and the pair_attention helper, on
the CPU: what the keyword returns and what the helper declines."""

import pytest
import torch

from unicore_amd.models.mol_pairbias import PairBiasEncoderLayer
from unicore_amd.modules import SelfMultiheadAttention
from unicore_amd.modules.pair_attention import pair_attention


def test_return_logits_matches_return_attn():
    torch.manual_seed(0)
    mod = SelfMultiheadAttention(128, 2, dropout=0.0)
    x, bias = torch.randn(2, 24, 128), torch.randn(2, 2, 24, 24)
    out_a, weights, probs = mod(x, attn_bias=bias, return_attn=True)
    out_l, logits = mod(x, attn_bias=bias, return_logits=True)
    assert probs.shape == (4, 24, 24)
    assert torch.equal(out_l, out_a) and torch.equal(logits, weights)


@pytest.mark.parametrize("case", ["cpu", "gate off", "L = 96", "D = 32", "fp32",
                                  "no bias", "broadcast bias", "key mask",
                                  "tgt != src"])
def test_pair_attention_declines(case, monkeypatch):
    monkeypatch.setenv("UNICORE_PAIR_ATTN", "0" if case == "gate off" else "1")
    B, H = 2, 2
    L = 96 if case == "L = 96" else 64
    D = 32 if case == "D = 32" else 64
    dtype = torch.float32 if case == "fp32" else torch.bfloat16
    q, k, v = (torch.zeros(B * H, L, D, dtype=dtype) for _ in range(3))
    bias = torch.zeros(B, 1 if case == "broadcast bias" else H, L, L, dtype=dtype)
    if case == "tgt != src":
        k = v = torch.zeros(B * H, 2 * L, D, dtype=dtype)
    mask = torch.zeros(B, 1, 1, L, dtype=dtype) if case == "key mask" else None
    got = pair_attention(q, k, v, None if case == "no bias" else bias, B, H, 0.1,
                         True, key_padding_mask=mask)
    assert got is None


def test_layer_return_pair_shapes():
    layer = PairBiasEncoderLayer(128, 256, 2, 0.0, 0.0, 0.0)
    x, pair = layer(torch.randn(2, 24, 128), torch.randn(2, 2, 24, 24), None,
                    return_pair=True)
    assert x.shape == (2, 24, 128) and pair.shape == (2, 2, 24, 24)
