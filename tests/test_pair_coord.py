"""Pair track + SE(3)-equivariant coordinate head of mol_pairbias (CPU):
the --coord-head flag and the model contract, the unchanged default, and the
eager definition of PairCoordHead (equivariance, gradients, degenerate atom
counts). The HIP kernels are tested in test_pair_coord_gpu.py."""

import pytest
import torch
import torch.nn as nn

from unicore_amd import options, tasks
from unicore_amd.modules import PairCoordHead
from unicore_amd.modules.pair_coord import pair_coord_eager

ARGV = [
    "--task", "unimol_synthetic",
    "--arch", "mol_pairbias",
    "--loss", "mol_pretrain",
    "--optimizer", "adam",
    "--lr-scheduler", "fixed",
    "--lr", "1e-4",
    "--batch-size", "2",
    "--dataset-size", "4",
    "--atoms-per-mol", "12",
    "--encoder-layers", "2",
    "--encoder-embed-dim", "32",
    "--encoder-ffn-embed-dim", "64",
    "--encoder-attention-heads", "8",
    "--gaussian-kernels", "16",
    "--dropout", "0.0",
    "--attention-dropout", "0.0",
    "--log-format", "none",
    "--num-workers", "0",
    "--no-save",
    "--cpu",
]

DEFAULT_KEYS = [
    "embed_tokens.weight",
    "pair_bias.means",
    "pair_bias.stds",
    "pair_bias.out.weight",
    "pair_bias.out.bias",
    "layers.0.attn.in_proj.weight",
    "layers.0.attn.in_proj.bias",
    "layers.0.attn.out_proj.weight",
    "layers.0.attn.out_proj.bias",
    "layers.0.attn_norm.weight",
    "layers.0.fc1.weight",
    "layers.0.fc1.bias",
    "layers.0.fc2.weight",
    "layers.0.fc2.bias",
    "layers.0.ffn_norm.weight",
    "layers.1.attn.in_proj.weight",
    "layers.1.attn.in_proj.bias",
    "layers.1.attn.out_proj.weight",
    "layers.1.attn.out_proj.bias",
    "layers.1.attn_norm.weight",
    "layers.1.fc1.weight",
    "layers.1.fc1.bias",
    "layers.1.fc2.weight",
    "layers.1.fc2.bias",
    "layers.1.ffn_norm.weight",
    "final_norm.weight",
    "lm_head.weight",
    "coord_head.weight",
    "coord_head.bias",
]


def _build(extra):
    parser = options.get_training_parser()
    args = options.parse_args_and_arch(parser, input_args=ARGV + extra)
    torch.manual_seed(3)
    task = tasks.setup_task(args)
    return args, task, task.build_model(args)


def _sample(task, B=2, L=12, n_pad=3):
    g = torch.Generator().manual_seed(11)
    pad = task.dictionary.pad()
    toks = torch.randint(5, 20, (B, L), generator=g)
    toks[0, L - n_pad:] = pad
    target = torch.full((B, L), pad)
    target[:, 1] = toks[:, 1]
    target[:, 4] = toks[:, 4]
    return {
        "net_input": {
            "src_tokens": toks,
            "src_coord": torch.randn(B, L, 3, generator=g),
        },
        "target": target,
        "coord_target": 0.1 * torch.randn(B, L, 3, generator=g),
    }


def test_flag_and_contract():
    args, task, model = _build(["--coord-head", "equivariant"])
    assert isinstance(model.coord_head, PairCoordHead)
    sample = _sample(task)
    logits, coord_delta = model(**sample["net_input"])
    assert logits.shape == (2, 12, len(task.dictionary))
    assert coord_delta.shape == (2, 12, 3)
    assert coord_delta.dtype == torch.float32
    pads = sample["net_input"]["src_tokens"].eq(task.dictionary.pad())
    assert pads.sum() == 3
    assert torch.equal(coord_delta[pads], torch.zeros(3, 3))
    assert coord_delta[~pads].abs().max() > 0

    loss_fn = task.build_loss(args)
    loss, _, _ = loss_fn(model, sample)
    loss.backward()
    for p in (model.coord_head.fc1.weight, model.coord_head.fc1.bias,
              model.coord_head.fc2.weight, model.coord_head.fc2.bias):
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert model.coord_head.fc2.weight.grad.abs().max() > 0

    # coord_loss alone: the only path from it to the first layer's attention
    # runs through the pair track (layer 0 logits -> layer 1 bias -> head)
    model.zero_grad(set_to_none=True)
    _, coord_delta = model(**sample["net_input"])
    atom = (~pads).unsqueeze(-1)
    ((coord_delta - sample["coord_target"]) * atom).pow(2).sum().backward()
    g0 = model.layers[0].attn.in_proj.weight.grad
    assert g0 is not None and torch.isfinite(g0).all() and g0.abs().max() > 0


@pytest.mark.parametrize("extra", [[], ["--coord-head", "linear"]])
def test_default_unchanged(extra):
    _, _, model = _build(extra)
    assert list(model.state_dict().keys()) == DEFAULT_KEYS
    assert isinstance(model.coord_head, nn.Linear)
    assert model.coord_head.out_features == 3


def _head_inputs(B, L, H, n_pad, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros(B, L, dtype=torch.bool)
    for b, n in enumerate(n_pad):
        if n:
            mask[b, L - n:] = True
    fill = torch.finfo(dtype).min
    key_pad = mask.view(B, 1, 1, L)
    pair0 = torch.randn(B, H, L, L, generator=g, dtype=dtype)
    pair0 = pair0.masked_fill(key_pad, fill)
    pair = pair0 + torch.randn(B, H, L, L, generator=g, dtype=dtype)
    pair = torch.where(key_pad, pair0, pair)
    coords = torch.randn(B, L, 3, generator=g, dtype=dtype)
    head = PairCoordHead(H).to(dtype)
    with torch.no_grad():
        for p in head.parameters():
            p.copy_(0.5 * torch.randn(p.shape, generator=g, dtype=dtype))
    return head, pair, pair0, coords, mask


def test_head_equivariance_fp64():
    head, pair, pair0, x, mask = _head_inputs(2, 9, 8, (2, 0))
    g = torch.Generator().manual_seed(5)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    assert torch.det(q) == pytest.approx(1.0, abs=1e-12)
    t = torch.randn(3, generator=g, dtype=torch.float64)
    with torch.no_grad():
        base = head(pair, pair0, x, mask)
        moved = head(pair, pair0, x @ q.T + t, mask)
    assert base.dtype == torch.float64
    scale = base.abs().max()
    assert scale > 0
    assert (moved - base @ q.T).abs().max() <= 1e-10 * scale


def test_eager_gradcheck_fp64():
    head, pair, pair0, x, mask = _head_inputs(1, 5, 8, (2,))
    # finite pads: gradcheck perturbs every entry, pads must simply not matter
    pair0 = torch.where(pair0 == torch.finfo(torch.float64).min,
                        torch.zeros_like(pair0), pair0)
    pair = torch.where(mask.view(1, 1, 1, 5), pair0, pair)
    params = [p.detach().clone().requires_grad_(True)
              for p in (head.fc1.weight, head.fc1.bias, head.fc2.weight,
                        head.fc2.bias)]
    pair = pair.clone().requires_grad_(True)
    pair0 = pair0.clone().requires_grad_(True)

    def fn(pair, pair0, w1, b1, w2, b2):
        return pair_coord_eager(pair, pair0, x, w1, b1, w2, b2, mask)

    assert torch.autograd.gradcheck(fn, (pair, pair0, *params))


def test_coords_take_no_gradient():
    head, pair, pair0, x, mask = _head_inputs(1, 5, 8, (0,))
    with pytest.raises(RuntimeError, match="coords"):
        head(pair, pair0, x.requires_grad_(True), mask)


def test_degenerate_counts():
    # sample 0: one real atom (n clamps to 1, update 0); sample 1: all pads
    head, pair, pair0, x, mask = _head_inputs(3, 6, 8, (5, 6, 0),
                                              dtype=torch.float32)
    assert (pair[1] == torch.finfo(torch.float32).min).all()
    pair = pair.requires_grad_(True)
    out = head(pair, pair0, x, mask)
    assert torch.isfinite(out).all()
    assert torch.equal(out[0], torch.zeros(6, 3))
    assert torch.equal(out[1], torch.zeros(6, 3))
    assert out[2].abs().max() > 0
    out.pow(2).sum().backward()
    assert torch.isfinite(pair.grad).all()
    assert torch.equal(pair.grad[:2], torch.zeros_like(pair.grad[:2]))
    for p in head.parameters():
        assert torch.isfinite(p.grad).all()
