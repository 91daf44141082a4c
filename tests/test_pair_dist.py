"""Pair distance head (CPU): the eager definition of PairDistHead, the
--dist-head flag of mol_pairbias and the masked distance loss of
mol_pretrain. The HIP kernels are tested in test_pair_dist_h64_gpu.py."""

import pytest
import torch

from unicore_amd import options, tasks
from unicore_amd.modules import PairDistHead

ARGV = [
    "--task", "unimol_synthetic", "--arch", "mol_pairbias",
    "--loss", "mol_pretrain", "--optimizer", "adam", "--lr-scheduler", "fixed",
    "--lr", "1e-4", "--batch-size", "2", "--dataset-size", "4",
    "--atoms-per-mol", "12", "--encoder-layers", "2",
    "--encoder-embed-dim", "32", "--encoder-ffn-embed-dim", "64",
    "--encoder-attention-heads", "8", "--gaussian-kernels", "16",
    "--dropout", "0.0", "--attention-dropout", "0.0", "--log-format", "none",
    "--num-workers", "0", "--no-save", "--cpu",
]
EQUIVARIANT = ["--coord-head", "equivariant"]

LAYER_KEYS = [
    "attn.in_proj.weight", "attn.in_proj.bias", "attn.out_proj.weight",
    "attn.out_proj.bias", "attn_norm.weight", "fc1.weight", "fc1.bias",
    "fc2.weight", "fc2.bias", "ffn_norm.weight",
]
# the equivariant model as it stands without --dist-head
KEYS = (
    ["embed_tokens.weight", "pair_bias.means", "pair_bias.stds",
     "pair_bias.out.weight", "pair_bias.out.bias"]
    + [f"layers.{n}.{k}" for n in (0, 1) for k in LAYER_KEYS]
    + ["final_norm.weight", "lm_head.weight", "coord_head.fc1.weight",
       "coord_head.fc1.bias", "coord_head.fc2.weight", "coord_head.fc2.bias"]
)
DIST_KEYS = [
    "dist_head.dense.weight", "dist_head.dense.bias",
    "dist_head.layer_norm.weight", "dist_head.layer_norm.bias",
    "dist_head.out_proj.weight", "dist_head.out_proj.bias",
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
        "net_input": {"src_tokens": toks,
                      "src_coord": torch.randn(B, L, 3, generator=g)},
        "target": target,
        "coord_target": 0.1 * torch.randn(B, L, 3, generator=g),
    }


def _head_inputs(B=2, L=10, H=8, n_pad=(3, 0)):
    g = torch.Generator().manual_seed(0)
    mask = torch.zeros(B, L, dtype=torch.bool)
    for b, n in enumerate(n_pad):
        if n:
            mask[b, L - n:] = True
    pair = torch.randn(B, H, L, L, generator=g, dtype=torch.float64)
    pair = pair.masked_fill(mask.view(B, 1, 1, L), torch.finfo(torch.float64).min)
    head = PairDistHead(H).double()
    with torch.no_grad():
        for p in head.parameters():
            p.copy_(0.5 * torch.randn(p.shape, generator=g, dtype=torch.float64))
    return head, pair, mask


def test_eager_symmetric_and_zero_at_pads():
    head, pair, mask = _head_inputs()
    dist = head(pair, mask)
    assert dist.shape == (2, 10, 10)
    assert torch.equal(dist, dist.transpose(1, 2))
    dead = mask.unsqueeze(2) | mask.unsqueeze(1)
    assert torch.equal(dist[dead], torch.zeros_like(dist[dead]))
    assert dist[~dead].abs().min() > 0


def test_sample_alone_equals_sample_in_padded_batch():
    head, pair, mask = _head_inputs()
    alone = head(pair[:1, :, :7, :7].contiguous())
    assert torch.allclose(head(pair, mask)[0, :7, :7], alone[0], rtol=0,
                          atol=1e-12)


def test_permuting_atoms_permutes_rows_and_columns():
    head, pair, _ = _head_inputs(n_pad=(0, 0))
    perm = torch.randperm(10, generator=torch.Generator().manual_seed(1))
    got = head(pair[:, :, perm][:, :, :, perm])
    want = head(pair)[:, perm][:, :, perm]
    assert torch.allclose(got, want, rtol=0, atol=1e-12)


def test_flag_trains_one_step():
    args, task, model = _build(
        EQUIVARIANT + ["--dist-head", "--dist-loss-weight", "1"])
    assert list(model.state_dict().keys()) == KEYS + DIST_KEYS
    sample = _sample(task)
    logits, coord_delta, dist = model(**sample["net_input"])
    assert coord_delta.shape == (2, 12, 3)
    assert dist.shape == (2, 12, 12) and dist.dtype == torch.float32
    loss, _, log = task.build_loss(args)(model, sample)
    assert torch.isfinite(log["dist_loss"]) and log["dist_loss"] > 0
    assert torch.equal(
        loss.data, log["token_loss"] + log["coord_loss"] + log["dist_loss"])
    loss.backward()
    for p in model.dist_head.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
        assert p.grad.abs().max() > 0
    before = model.dist_head.dense.weight.detach().clone()
    torch.optim.SGD(model.parameters(), lr=0.1).step()
    assert not torch.equal(model.dist_head.dense.weight, before)


def test_flag_needs_the_equivariant_head():
    with pytest.raises(ValueError, match="--coord-head equivariant"):
        _build(["--dist-head"])


def test_positive_weight_needs_distances():
    args, task, model = _build(EQUIVARIANT + ["--dist-loss-weight", "1"])
    with pytest.raises(ValueError, match="--dist-head"):
        task.build_loss(args)(model, _sample(task))


@pytest.mark.parametrize("w", [1.0, 0.25])
def test_without_the_flag_nothing_changes(w):
    args, task, model = _build(EQUIVARIANT + ["--coord-loss-weight", str(w)])
    assert list(model.state_dict().keys()) == KEYS
    sample = _sample(task)
    assert len(model(**sample["net_input"])) == 2
    loss, _, log = task.build_loss(args)(model, sample)
    assert "dist_loss" not in log
    assert torch.equal(loss.data, log["token_loss"] + w * log["coord_loss"])
