"""CPU tests of the Evoformer padding masks (``--msa-padding-mask``): fp32,
eval mode, ``--dropout 0``.

A padded batch must compute, at its valid positions, what each sample
computes alone and unpadded.  The only difference left is fp32 summation
order (a reduction over a padded axis adds exact zeros in other places), so
the tolerance is atol = rtol = 1e-5.
"""

import copy
import functools

import pytest
import torch

from unicore_amd.modules import gated_mul, outer_product_mean
from unicore_amd.modules.outer_product import OPM_MASK_EPS, opm_mask_inv_norm
from unicore_amd.modules.padding_mask import (
    additive_key_mask,
    additive_mask_value,
    build_evoformer_masks,
)

EVO_ARGV = [
    "--task", "evoformer_synthetic",
    "--arch", "evoformer",
    "--loss", "masked_msa",
    "--optimizer", "adam",
    "--lr-scheduler", "fixed",
    "--lr", "1e-4",
    "--batch-size", "2",
    "--dataset-size", "8",
    "--msa-depth", "5",
    "--residues", "7",
    "--evo-layers", "2",
    "--msa-dim", "32",
    "--pair-dim", "32",
    "--evo-heads", "4",
    "--tri-attn-heads", "4",
    "--dropout", "0.0",
    "--triangle-attention",
    "--log-format", "none",
    "--num-workers", "0",
    "--no-save",
    "--cpu",
    "--save-dir", "unused",
]

TOL = 1e-5
SHAPES = ((5, 7), (3, 4))  # (S, L) of the two samples


def _setup(extra=()):
    from unicore_amd import options, tasks

    parser = options.get_training_parser()
    args = options.parse_args_and_arch(parser, input_args=EVO_ARGV + list(extra))
    return tasks.setup_task(args), args


def _build(extra=()):
    task, args = _setup(extra)
    torch.manual_seed(11)
    return task.build_model(args).eval(), args


@functools.lru_cache(maxsize=None)
def _samples():
    """The two unpadded samples, (1, S, L) each, and their padded batch."""
    g = torch.Generator().manual_seed(3)
    pad = _build()[0].padding_idx
    alone = tuple(torch.randint(5, 20, (1, s, l), generator=g) for s, l in SHAPES)
    S, L = max(s for s, _ in SHAPES), max(l for _, l in SHAPES)
    batch = torch.full((len(SHAPES), S, L), pad, dtype=torch.long)
    for i, t in enumerate(alone):
        batch[i, : t.shape[1], : t.shape[2]] = t[0]
    return alone, batch


def _valid_logits(model, dtype=torch.float32):
    """Logits of every sample alone and the same positions of the batch."""
    alone, batch = _samples()
    model = copy.deepcopy(model).to(dtype)
    with torch.no_grad():
        padded = model(batch)
        single = [model(t)[0] for t in alone]
    cut = [padded[i, : t.shape[0], : t.shape[1]] for i, t in enumerate(single)]
    return single, cut


@pytest.mark.parametrize("fold", ["1", "0"])
def test_padding_invariance(monkeypatch, fold):
    """Valid logits of the padded (2, 5, 7) batch equal the logits of the
    (5, 7) and (3, 4) samples run alone.  Measured maximum difference: 0.0
    in fp32 and 0.0 in the float64 rerun (at these sizes the padded
    reductions add exact zeros in the same order), so the tolerance stays
    at 1e-5.  Without the flag the same comparison differs by 0.217."""
    monkeypatch.setenv("UNICORE_FOLD_BIAS", fold)
    model, _ = _build(["--msa-padding-mask"])
    single, cut = _valid_logits(model)
    for a, b in zip(single, cut):
        print("masked: max diff", (a - b).abs().max().item())
    for a, b in zip(single, cut):
        torch.testing.assert_close(b, a, atol=TOL, rtol=TOL)
    s64, c64 = _valid_logits(model, torch.float64)
    for a, b in zip(s64, c64):
        print("masked, float64: max diff", (a - b).abs().max().item())
        torch.testing.assert_close(b, a, atol=1e-12, rtol=1e-12)

    # the same model without the flag leaks padding into the small sample
    plain, _ = _build()
    assert list(plain.state_dict()) == list(model.state_dict())
    single, cut = _valid_logits(plain)
    leak = (single[1] - cut[1]).abs().max().item()
    print("unmasked: max diff", leak)
    assert leak > 100 * TOL, leak


def _valid_loss(logits):
    # a fixed smooth scalar of the logits
    return (logits.float() ** 2).sum() + logits.float().sum()


def test_padding_invariance_of_gradients():
    """Parameter gradients of a scalar loss over the valid positions of the
    padded batch equal the sum of the unpadded runs' gradients.  Gradients
    here reach magnitude ~1e2, hence rtol next to atol; measured maximum
    |diff| / (atol + rtol |ref|) is 0.105."""
    model, _ = _build(["--msa-padding-mask"])
    alone, batch = _samples()

    def grads(run):
        model.zero_grad(set_to_none=True)
        run()
        return {n: p.grad.clone() for n, p in model.named_parameters()
                if p.grad is not None}

    def run_alone():
        for t in alone:
            _valid_loss(model(t)).backward()

    def run_padded():
        out = model(batch)
        loss = sum(_valid_loss(out[i, : t.shape[1], : t.shape[2]])
                   for i, t in enumerate(alone))
        loss.backward()

    want, got = grads(run_alone), grads(run_padded)
    assert set(want) == set(got)
    worst = max(((got[n] - want[n]).abs() / (TOL + TOL * want[n].abs())).max().item()
                for n in want)
    print("worst |diff| / allowed", worst)
    for n in want:
        torch.testing.assert_close(got[n], want[n], atol=TOL, rtol=TOL, msg=n)


def test_all_ones_mask_only_rescales_opm():
    """Flag on, no padding: every module computes what it computes without a
    mask, except the OPM, whose mean is over S + 1e-3."""
    from unicore_amd.models import evoformer

    torch.manual_seed(0)
    B, S, L, Dm, Dp = 2, 3, 5, 32, 16
    msa, pair = torch.randn(B, S, L, Dm), torch.randn(B, L, L, Dp)
    masks = build_evoformer_masks(torch.ones(B, S, L), torch.float32)
    assert masks.row_key.shape == (B, 1, S, 1, L)
    assert masks.col_key.shape == (B, L, 1, 1, S)
    assert masks.tri_start_key.shape == masks.tri_end_key.shape == (B, 1, L, 1, L)
    assert masks.opm_inv_norm.shape == (B, L, L)
    assert masks.opm_inv_norm.dtype == torch.float32
    blk = evoformer.EvoformerBlock(Dm, Dp, 4, 0.0, triangle_attention=True).eval()
    with torch.no_grad():
        assert torch.equal(blk.row_attn(msa, pair, key_mask=masks.row_key),
                           blk.row_attn(msa, pair))
        assert torch.equal(blk.col_attn(msa, key_mask=masks.col_key),
                           blk.col_attn(msa))
        assert torch.equal(blk.tri_out(pair, pair_mask=masks.pair),
                           blk.tri_out(pair))
        assert torch.equal(blk.tri_in(pair, pair_mask=masks.pair),
                           blk.tri_in(pair))
        assert torch.equal(blk.tri_att_start(pair, key_mask=masks.tri_start_key),
                           blk.tri_att_start(pair))
        assert torch.equal(blk.tri_att_end(pair, pair_mask=masks.pair),
                           blk.tri_att_end(pair))
        a, b = torch.randn(B, S, L, 32), torch.randn(B, S, L, 32)
        masked = outer_product_mean(a, b, mask=masks.msa,
                                    inv_norm=masks.opm_inv_norm)
        plain = outer_product_mean(a, b)
        torch.testing.assert_close(masked, plain * (S / (S + OPM_MASK_EPS)),
                                   atol=1e-6, rtol=1e-6)

    # whole model: the flag changes the unpadded logits only through that
    # factor, S / (S + 1e-3) = 1 - 2e-4 at S = 5
    alone, _ = _samples()
    on, off = _build(["--msa-padding-mask"])[0], _build()[0]
    with torch.no_grad():
        d = (on(alone[0]) - off(alone[0])).abs().max().item()
    print("flag on vs off, unpadded: max diff", d)
    assert 0 < d < 1e-2


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_fully_padded_row_and_column_stay_finite(dtype):
    assert additive_mask_value(torch.float16) == -3e4
    assert additive_mask_value(torch.bfloat16) == -1e9
    assert additive_mask_value(torch.float32) == -1e9
    keep = torch.tensor([[1.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    am = additive_key_mask(keep, dtype)
    assert am.dtype == dtype and am.shape == keep.shape
    assert bool(torch.isfinite(am).all())
    assert am[0, 0] == 0 and am[0, 1] == additive_mask_value(dtype)
    # scores of the mask's dtype: a fully masked row is uniform, not NaN
    scores = torch.randn(2, 3).to(dtype)
    p = torch.softmax((scores + am).float(), dim=-1)
    assert bool(torch.isfinite(p).all())
    assert p[0, 1] == 0
    torch.testing.assert_close(p[1], torch.full((3,), 1 / 3), atol=1e-3, rtol=0)

    if dtype == torch.float16:
        return  # the fp32 model below covers the modules
    _, batch = _samples()
    model, _ = _build(["--msa-padding-mask"])
    pad = model.padding_idx
    batch = batch.clone()
    batch[0, 2, :] = pad   # an MSA row of sample 0
    batch[0, :, 3] = pad   # a residue column of sample 0
    with torch.no_grad():
        out = model(batch)
    assert bool(torch.isfinite(out).all())


def test_explicit_msa_mask_overrides_the_derived_one():
    _, batch = _samples()
    model, _ = _build(["--msa-padding-mask"])
    with torch.no_grad():
        derived = model(batch)
        same = model(batch, msa_mask=batch.ne(model.padding_idx))
        other = model(batch, msa_mask=torch.ones_like(batch))
    assert torch.equal(derived, same)
    assert not torch.equal(derived, other)


def _opm_ref64(a, b, m):
    am, bm = a.double() * m[..., None].double(), b.double() * m[..., None].double()
    num = torch.einsum("bsic,bsjd->bijcd", am, bm)
    norm = torch.einsum("bsi,bsj->bij", m.double(), m.double())
    o = num / (OPM_MASK_EPS + norm)[..., None, None]
    return o.reshape(*o.shape[:3], -1)


def test_eager_masked_outer_product_mean():
    g = torch.Generator().manual_seed(5)
    B, S, L, c = 2, 6, 5, 4
    a, b = torch.randn(B, S, L, c, generator=g), torch.randn(B, S, L, c, generator=g)
    m = (torch.rand(B, S, L, generator=g) < 0.6).float()
    m[0, :, 2] = 0  # a residue no row has: its normaliser is 0
    got = outer_product_mean(a, b, mask=m)
    assert got.dtype == torch.float32 and got.shape == (B, L, L, c * c)
    torch.testing.assert_close(got.double(), _opm_ref64(a, b, m),
                               atol=1e-5, rtol=1e-5)
    assert bool((got[0, 2] == 0).all()) and bool((got[0, :, 2] == 0).all())
    # a given inv_norm is the one used
    w = opm_mask_inv_norm(m)
    assert w.dtype == torch.float32 and w.shape == (B, L, L)
    assert torch.equal(outer_product_mean(a, b, mask=m, inv_norm=w), got)
    # float64 gradients
    a64 = a[:1, :3, :3].double().requires_grad_()
    b64 = b[:1, :3, :3].double().requires_grad_()
    m64 = m[:1, :3, :3].double()
    assert torch.autograd.gradcheck(
        lambda x, y: outer_product_mean(x, y, mask=m64), (a64, b64))


def test_eager_gated_mul_row_mask():
    g = torch.Generator().manual_seed(6)
    x, gt = torch.randn(2, 3, 5, 8, generator=g), torch.randn(2, 3, 5, 8, generator=g)
    bx, bg = torch.randn(8, generator=g), torch.randn(8, generator=g)
    m = (torch.rand(2, 3, 5, generator=g) < 0.5).float()
    want = ((x.double() + bx.double()) * torch.sigmoid(gt.double() + bg.double())
            * m.double()[..., None])
    got = gated_mul(x, gt, bx, bg, row_mask=m)
    torch.testing.assert_close(got.double(), want, atol=1e-6, rtol=1e-6)
    assert bool((got[m == 0] == 0).all())
    # flat mask, no biases
    got = gated_mul(x, gt, row_mask=m.reshape(-1))
    want = x.double() * torch.sigmoid(gt.double()) * m.double()[..., None]
    torch.testing.assert_close(got.double(), want, atol=1e-6, rtol=1e-6)
    # without a mask nothing changes
    assert torch.equal(gated_mul(x, gt, bx, bg),
                       (x + bx) * torch.sigmoid(gt + bg))
    args = [t.double().requires_grad_() for t in (x[:1, :2, :2], gt[:1, :2, :2], bx, bg)]
    m64 = m[:1, :2, :2].double()
    assert torch.autograd.gradcheck(
        lambda *t: gated_mul(*t, row_mask=m64), args)


def _batches(extra, n=2):
    task, args = _setup(extra)
    task.load_dataset("train")
    ds = task.datasets["train"]
    out = []
    for k in range(n):
        idx = range(k * args.batch_size, (k + 1) * args.batch_size)
        out.append(ds.collater([ds[i] for i in idx]))
    return out, task.dictionary.pad()


def test_task_ragged_batches_are_padded_and_repeatable():
    extra = ["--msa-depth", "6", "--residues", "16", "--min-msa-depth", "3",
             "--min-residues", "8", "--batch-size", "4", "--seed", "3"]
    batches, pad = _batches(extra)
    shapes = set()
    for bt in batches:
        src, tgt = bt["net_input"]["src_tokens"], bt["target"]
        assert src.shape == tgt.shape and src.dtype == tgt.dtype == torch.long
        B, S, L = src.shape
        assert 3 <= S <= 6 and 8 <= L <= 16
        is_pad = src.eq(pad)
        assert bool(tgt[is_pad].eq(pad).all())
        assert bool(tgt.ne(pad).any())
        for i in range(B):
            # real tokens form the leading (depth, length) rectangle
            real = ~is_pad[i]
            d, l = int(real[:, 0].sum()), int(real[0].sum())
            assert 3 <= d <= 6 and 8 <= l <= 16
            assert bool(real[:d, :l].all()) and int(real.sum()) == d * l
            shapes.add((d, l))
        # padded to the batch maximum, no further
        assert bool((~is_pad).any(dim=0).any(dim=1).all())
        assert bool((~is_pad).any(dim=0).any(dim=0).all())
    assert len(shapes) > 1, shapes
    again, _ = _batches(extra)
    for x, y in zip(batches, again):
        assert torch.equal(x["net_input"]["src_tokens"], y["net_input"]["src_tokens"])
        assert torch.equal(x["target"], y["target"])


def test_task_defaults_are_unchanged():
    """Without the new flags (or with them at the fixed sizes) the batches
    are the stacked fixed-shape samples of the original dataset."""
    import numpy as np

    from unicore_amd.data import data_utils

    base, pad = _batches([])
    same, _ = _batches(["--min-msa-depth", "5", "--min-residues", "7"])
    task, args = _setup([])
    for k, (x, y) in enumerate(zip(base, same)):
        assert torch.equal(x["net_input"]["src_tokens"], y["net_input"]["src_tokens"])
        assert torch.equal(x["target"], y["target"])
        assert x["target"].shape == (2, 5, 7)
        for i in range(2):
            # the original draw, spelled out
            with data_utils.numpy_seed(args.seed, 1, 2 * k + i):
                toks = np.random.randint(5, task.mask_idx, size=(5, 7))
                mask = np.random.rand(5, 7) < args.mask_prob
            src = toks.copy()
            src[mask] = task.mask_idx
            assert x["net_input"]["src_tokens"][i].numpy().tobytes() == \
                src.astype(np.int64).tobytes()


def test_hip_graph_blocks_with_the_flag_raises():
    with pytest.raises(AssertionError, match="--msa-padding-mask"):
        _build(["--msa-padding-mask", "--hip-graph-blocks"])
    model, args = _build()
    assert args.msa_padding_mask is False and model.msa_padding_mask is False
