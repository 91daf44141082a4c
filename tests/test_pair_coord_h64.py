"""CPU side of the H = 64 coordinate head: the dispatch predicate, and the
module on the CPU (the eager definition). The kernels are tested in
test_pair_coord_h64_gpu.py."""

import pytest
import torch

from unicore_amd import ops
from unicore_amd.modules import PairCoordHead
from unicore_amd.modules.pair_coord import pair_coord_eager

bf16 = torch.bfloat16


@pytest.mark.parametrize("H,L,want", [
    (64, 16, True), (64, 8, True), (64, 136, True),
    (64, 20, False), (64, 4, False), (64, 0, False), (64, None, False),
    (8, 20, True), (16, 33, True), (32, 16, False),
])
def test_predicate_with_L(H, L, want):
    assert ops.pair_coord_supported(H, bf16, L) is want


@pytest.mark.parametrize("H,want", [(8, True), (16, True), (32, False),
                                    (64, False)])
def test_predicate_two_arguments(H, want):
    assert ops.pair_coord_supported(H, torch.float32) is want
    assert not ops.pair_coord_supported(H, torch.float64)


def test_module_on_cpu_is_the_eager_function(monkeypatch):
    monkeypatch.setenv("UNICORE_PAIR_COORD_H64", "1")
    torch.manual_seed(0)
    B, L = 2, 16
    head = PairCoordHead(64)
    pair0 = torch.randn(B, 64, L, L)
    pair = pair0 + torch.randn(B, 64, L, L)
    coords = torch.randn(B, L, 3)
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[0, -3:] = True
    want = pair_coord_eager(pair, pair0, coords, head.fc1.weight,
                            head.fc1.bias, head.fc2.weight, head.fc2.bias, mask)
    assert torch.equal(head(pair, pair0, coords, mask), want)
