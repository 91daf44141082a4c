"""Uni-Mol pair embedding (CPU): the eager definition of PairGaussianEmbed and
the --pair-embed flag of mol_pairbias. The HIP kernels are tested in
test_pair_gauss_h64_gpu.py."""

import math

import torch

from unicore_amd import options, tasks
from unicore_amd.modules import PairGaussianEmbed
from unicore_amd.modules.pair_gauss import pair_gauss_fused_ok

from test_pair_dist import ARGV, EQUIVARIANT, KEYS, _sample


def test_eager_is_the_written_definition():
    B, L, K, H, T = 2, 8, 16, 4, 5
    g = torch.Generator().manual_seed(0)
    m = PairGaussianEmbed(K, H, T).double()
    with torch.no_grad():
        m.mul.weight.copy_(1 + 0.1 * torch.randn(T * T, 1, generator=g))
        m.bias.weight.copy_(0.1 * torch.randn(T * T, 1, generator=g))
        m.stds.mul_(torch.where(torch.arange(K) % 2 == 0, 1.0, -1.0))
    coords = 2 * torch.randn(B, L, 3, generator=g, dtype=torch.float64)
    tokens = torch.randint(0, T, (B, L), generator=g)
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[0, L - 3:] = True
    assert not pair_gauss_fused_ok(coords, K, H, torch.float64)
    out = m(coords, tokens, mask)
    assert out.shape == (B, H, L, L)
    w1, b1 = m.linear1.weight, m.linear1.bias
    w2, b2 = m.linear2.weight, m.linear2.bias
    want = torch.empty(B, H, L, L, dtype=torch.float64)
    for b in range(B):
        for i in range(L):
            for j in range(L):
                d = 0.0 if i == j else math.dist(coords[b, i], coords[b, j])
                t = int(tokens[b, i]) * T + int(tokens[b, j])
                x = float(m.mul.weight.data[t]) * d + float(m.bias.weight.data[t])
                gk = torch.empty(K, dtype=torch.float64)
                for k in range(K):
                    s = abs(float(m.stds.data[k])) + 1e-5
                    z = (x - float(m.means.data[k])) / s
                    gk[k] = math.exp(-0.5 * z * z) / (math.sqrt(2 * 3.14159) * s)
                pre = w1 @ gk + b1
                h = 0.5 * pre * (1 + torch.erf(pre / math.sqrt(2)))
                want[b, :, i, j] = w2 @ h + b2
    want[0, :, :, L - 3:] = torch.finfo(torch.float64).min
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    out.masked_fill(mask.view(B, 1, 1, L), 0.0).square().sum().backward()
    for p in m.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
        assert p.grad.abs().max() > 0
    assert len(list(m.parameters())) == 8


def test_flag_builds_the_embedding_and_default_is_unchanged():
    def build(extra):
        parser = options.get_training_parser()
        args = options.parse_args_and_arch(parser, input_args=ARGV + extra)
        torch.manual_seed(3)
        task = tasks.setup_task(args)
        return task, task.build_model(args)

    task, model = build(EQUIVARIANT)
    assert list(model.state_dict().keys()) == KEYS
    task, model = build(EQUIVARIANT + ["--pair-embed", "unimol"])
    assert isinstance(model.pair_bias, PairGaussianEmbed)
    assert torch.equal(model.pair_bias.mul.weight,
                       torch.ones_like(model.pair_bias.mul.weight))
    sample = _sample(task)
    toks = sample["net_input"]["src_tokens"]
    pad = toks.eq(task.dictionary.pad())
    bias = model.pair_bias(sample["net_input"]["src_coord"], toks, pad)
    B, L = toks.shape
    assert bias.shape == (B, 8, L, L)
    dead = pad.view(B, 1, 1, L).expand_as(bias)
    assert dead.any() and (bias[dead] == torch.finfo(bias.dtype).min).all()
    assert torch.isfinite(bias[~dead]).all()
    logits, coord_delta = model(**sample["net_input"])
    assert coord_delta.shape == (B, L, 3) and torch.isfinite(coord_delta).all()
