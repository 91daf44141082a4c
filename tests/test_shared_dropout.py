"""Shared-axis (row-/column-wise) dropout of the residual joins, CPU side:
the eager fallback of the three module functions, argument validation and
the Evoformer flags (--msa-dropout / --pair-dropout)."""

import pytest
import torch

from unicore_amd.modules import LayerNorm, dropout_add
from unicore_amd.modules.dropout_add_ln import dropout_add_ln, dropout_add_ln_pre

SHAPE = (2, 5, 7, 24)


def _summed(fn, x, res, p, training, shared_dim, bias=None):
    """residual + dropout(x + bias): dropout_add's result, or the summed
    stream of dropout_add_ln_pre."""
    if fn is dropout_add:
        return dropout_add(x, res, p, training, bias=bias, shared_dim=shared_dim)
    s, _ = dropout_add_ln_pre(x, res, LayerNorm(x.shape[-1]), p, training,
                              bias=bias, shared_dim=shared_dim)
    return s


@pytest.mark.parametrize("fn", [dropout_add, dropout_add_ln_pre])
@pytest.mark.parametrize("shared_dim", [1, 2])
def test_fallback_pattern_is_shared(fn, shared_dim):
    p = 0.4
    x = torch.ones(SHAPE)
    res = torch.zeros(SHAPE)
    out = _summed(fn, x, res, p, True, shared_dim)
    keep = out != 0
    # constant along the shared axis
    first = keep.select(shared_dim, 0).unsqueeze(shared_dim)
    assert torch.equal(keep, first.expand_as(keep))
    # not constant along batch, the other spatial axis, channels
    for d in (0, 3 - shared_dim, 3):
        ref = keep.select(d, 0).unsqueeze(d)
        assert not torch.equal(keep, ref.expand_as(keep)), d
    assert 0 < keep.float().mean() < 1
    assert torch.equal(out[keep], torch.full_like(out[keep], 1 / (1 - p)))


@pytest.mark.parametrize("shared_dim", [1, 2])
def test_fallback_post_ln_and_normed_stream(shared_dim):
    """dropout_add_ln returns only ln(sum), dropout_add_ln_pre's second
    output is the same: both must be the LayerNorm of the shared-mask sum
    that dropout_add draws under the same seed, and so constant along the
    shared axis and along no other."""
    p = 0.4
    C = SHAPE[-1]
    ln = LayerNorm(C)
    with torch.no_grad():
        ln.bias.copy_(torch.arange(C, dtype=torch.float32))
    x = torch.ones(SHAPE)
    res = torch.zeros(SHAPE)
    torch.manual_seed(7)
    s = dropout_add(x, res, p, True, shared_dim=shared_dim)
    torch.manual_seed(7)
    out = dropout_add_ln(x, res, ln, p, True, shared_dim=shared_dim)
    torch.manual_seed(7)
    s2, n2 = dropout_add_ln_pre(x, res, ln, p, True, shared_dim=shared_dim)
    assert torch.equal(s2, s)
    assert torch.equal(out, ln(s)) and torch.equal(n2, out)
    first = out.select(shared_dim, 0).unsqueeze(shared_dim)
    assert torch.equal(out, first.expand_as(out))
    for d in (0, 3 - shared_dim):
        ref = out.select(d, 0).unsqueeze(d)
        assert not torch.equal(out, ref.expand_as(out)), d


@pytest.mark.parametrize("shared_dim", [1, 2])
@pytest.mark.parametrize("p,training", [(0.0, True), (0.3, False)])
def test_no_dropout_is_bit_identical(shared_dim, p, training):
    torch.manual_seed(3)
    x = torch.randn(SHAPE)
    res = torch.randn(SHAPE)
    bias = torch.randn(SHAPE[-1])
    ln = LayerNorm(SHAPE[-1])
    assert torch.equal(
        dropout_add(x, res, p, training, bias=bias, shared_dim=shared_dim),
        dropout_add(x, res, p, training, bias=bias),
    )
    assert torch.equal(
        dropout_add_ln(x, res, ln, p, training, bias=bias,
                       shared_dim=shared_dim),
        dropout_add_ln(x, res, ln, p, training, bias=bias),
    )
    a = dropout_add_ln_pre(x, res, ln, p, training, bias=bias,
                           shared_dim=shared_dim)
    b = dropout_add_ln_pre(x, res, ln, p, training, bias=bias)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_fallback_folds_bias_before_the_mask():
    torch.manual_seed(4)
    x = torch.randn(SHAPE)
    bias = torch.randn(SHAPE[-1])
    res = torch.zeros(SHAPE)
    p = 0.5
    out = dropout_add(x, res, p, True, bias=bias, shared_dim=1)
    keep = out != 0
    want = torch.where(keep, (x + bias) / (1 - p), torch.zeros(()))
    assert torch.allclose(out, want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("fn", ["add", "ln", "pre"])
def test_argument_validation(fn):
    ln = LayerNorm(8)

    def call(x, shared_dim, p=0.1, training=True):
        if fn == "add":
            return dropout_add(x, x, p, training, shared_dim=shared_dim)
        f = dropout_add_ln if fn == "ln" else dropout_add_ln_pre
        return f(x, x, ln, p, training, shared_dim=shared_dim)

    x4 = torch.randn(2, 3, 4, 8)
    for bad in (0, 3, -1):
        with pytest.raises(ValueError, match=f"shared_dim.*{bad}"):
            call(x4, bad)
    with pytest.raises(ValueError, match="4-D.*3-D"):
        call(torch.randn(3, 4, 8), 1)
    with pytest.raises(ValueError, match="4-D.*5-D"):
        call(torch.randn(1, 2, 3, 4, 8), 2)
    # caller errors even where no mask would be drawn
    with pytest.raises(ValueError):
        call(x4, 3, p=0.0)
    with pytest.raises(ValueError):
        call(torch.randn(4, 8), 1, training=False)


def test_shared_dropout_supported_mirrors_host_checks():
    from unicore_amd import ops

    assert ops.shared_dropout_supported((2, 5, 7, 24), torch.bfloat16)
    assert ops.shared_dropout_supported((1, 1, 1, 8), torch.float32)
    assert not ops.shared_dropout_supported((2, 5, 7, 20), torch.bfloat16)
    assert not ops.shared_dropout_supported((5, 7, 24), torch.bfloat16)
    assert not ops.shared_dropout_supported((2, 5, 7, 24), torch.float64)


# ---------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------

EVO_ARGV = [
    "--task", "evoformer_synthetic",
    "--arch", "evoformer",
    "--loss", "masked_msa",
    "--optimizer", "adam",
    "--lr-scheduler", "fixed",
    "--lr", "1e-4",
    "--batch-size", "2",
    "--dataset-size", "8",
    "--msa-depth", "8",
    "--residues", "24",
    "--evo-layers", "2",
    "--msa-dim", "64",
    "--pair-dim", "32",
    "--evo-heads", "4",
    "--dropout", "0.0",
    "--triangle-attention",
    "--log-format", "none",
    "--num-workers", "0",
    "--no-save",
    "--cpu",
    "--save-dir", "unused",
]


def _build(extra=()):
    from unicore_amd import options, tasks

    parser = options.get_training_parser()
    args = options.parse_args_and_arch(parser, input_args=EVO_ARGV + list(extra))
    task = tasks.setup_task(args)
    torch.manual_seed(11)
    return task.build_model(args), args


def _tokens():
    return torch.randint(5, 20, (2, 4, 12), generator=torch.Generator().manual_seed(2))


def test_model_flags_default_to_zero_and_plumb_through():
    model, args = _build()
    assert args.msa_dropout == 0.0 and args.pair_dropout == 0.0
    model, args = _build(["--msa-dropout", "0.15", "--pair-dropout", "0.25"])
    assert args.msa_dropout == 0.15 and args.pair_dropout == 0.25
    for blk in model.blocks:
        assert blk.msa_dropout == 0.15 and blk.pair_dropout == 0.25


def test_model_flags_absent_is_the_unflagged_model(monkeypatch):
    """Without the flags: same parameters, and the forward never reaches a
    shared-dropout code path (train mode, so an active path would draw)."""
    from unicore_amd.models import evoformer
    from unicore_amd.modules import shared_dropout

    flagged, _ = _build(["--msa-dropout", "0.15", "--pair-dropout", "0.25"])
    model, _ = _build()
    assert list(model.state_dict()) == list(flagged.state_dict())
    for (k, a), b in zip(model.state_dict().items(),
                         flagged.state_dict().values()):
        assert torch.equal(a, b), k

    toks = _tokens()
    model.train()
    want = model(toks)

    def boom(*a, **k):
        raise AssertionError("shared-dropout path reached with flags at 0")

    monkeypatch.setattr(shared_dropout, "apply_shared_mask", boom)
    monkeypatch.setattr(shared_dropout, "check_shared_dim", boom)
    monkeypatch.setattr(evoformer, "dropout_add", boom)  # plain chain: adds
    assert torch.equal(model(toks), want)
    # and it is the model the flags give in eval mode, where they are off
    assert torch.equal(model.eval()(toks), flagged.eval()(toks))


def test_model_flags_train_and_eval():
    base, _ = _build()
    model, _ = _build(["--msa-dropout", "0.15", "--pair-dropout", "0.25"])
    toks = _tokens()
    want = base.eval()(toks)
    assert torch.equal(model.eval()(toks), want)
    model.train()
    torch.manual_seed(5)
    out = model(toks)
    assert torch.isfinite(out).all()
    assert not torch.equal(out, base.train()(toks))
    out.float().pow(2).mean().backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters()
               if p.grad is not None)


def test_model_joins_get_the_table_cpu(monkeypatch):
    """Plain residual chain: exactly the five joins of the table reach
    dropout_add, with their (p, shared_dim)."""
    from unicore_amd.models import evoformer

    model, _ = _build(["--msa-dropout", "0.15", "--pair-dropout", "0.25",
                       "--evo-layers", "1"])
    seen = []
    real = evoformer.dropout_add

    def spy(x, residual, p, is_training, bias=None, shared_dim=None):
        seen.append((tuple(x.shape[1:3]), p, shared_dim))
        return real(x, residual, p, is_training, bias=bias,
                    shared_dim=shared_dim)

    monkeypatch.setattr(evoformer, "dropout_add", spy)
    model.train()(_tokens())
    assert seen == [
        ((4, 12), 0.15, 1),    # row_attn
        ((12, 12), 0.25, 1),   # tri_out
        ((12, 12), 0.25, 1),   # tri_in
        ((12, 12), 0.25, 1),   # tri_att_start
        ((12, 12), 0.25, 2),   # tri_att_end
    ]


def test_hip_graph_blocks_refuses_shared_dropout():
    model, _ = _build(["--msa-dropout", "0.15"])
    with pytest.raises(AssertionError, match="msa-dropout"):
        model._graphed_trunk(torch.zeros(1), torch.zeros(1))
