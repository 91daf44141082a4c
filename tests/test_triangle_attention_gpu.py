"""GPU tests of the triangle-attention layout moves (csrc/tri_attn.hip) and
of modules.TriangleAttention on top of them.

The four entries are pure copies, so every comparison with the permute
expression is ``torch.equal``.  The fused module differs from the permute
chain only by exact copies feeding the same kernels, so its forward is
compared bitwise too; gradients are compared with a float64 CPU run.
"""

import argparse
import copy
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)

GATE = "UNICORE_TRIATTN_FUSED"


def _kernels():
    from unicore_amd import ops

    assert ops.has_kernels(), "HIP extension must be built/loaded on a GPU box"
    return ops


def _randn(*shape, seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g).to(dtype)


def _arrange_ref(x, H, transpose):
    B, I, J, C = x.shape
    x5 = x.reshape(B, I, J, H, C // H)
    perm = (0, 3, 2, 1, 4) if transpose else (0, 3, 1, 2, 4)
    return x5.permute(*perm).contiguous()


def _merge_ref(o, B, I, J, H, transpose):
    R, T = (J, I) if transpose else (I, J)
    o5 = o.view(B, H, R, T, o.shape[-1])
    perm = (0, 3, 2, 1, 4) if transpose else (0, 2, 3, 1, 4)
    return o5.permute(*perm).reshape(B, I, J, -1)


def _bias_ref(lin, transpose):
    perm = (0, 3, 2, 1) if transpose else (0, 3, 1, 2)
    return lin.permute(*perm).contiguous()


def _bias_bwd_ref(d, transpose):
    perm = (0, 3, 2, 1) if transpose else (0, 2, 3, 1)
    return d.permute(*perm).contiguous()


PAIR_SHAPES = [(2, 5, 7), (1, 1, 1), (1, 33, 17)]
HEADS = [(4, 8), (8, 16)]


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("transpose", [False, True])
def test_pair_arrange_and_merge_equal_permute(transpose, dtype):
    ops = _kernels()
    for (B, I, J), (H, D) in itertools.product(PAIR_SHAPES, HEADS):
        C = H * D
        R, T = (J, I) if transpose else (I, J)
        wide = _randn(B, I, J, 3 * C, seed=1, dtype=dtype)
        views = list(wide.chunk(3, -1))
        views.append(_randn(B, J, I, C, seed=2, dtype=dtype).transpose(1, 2))
        for n, x in enumerate(views):
            assert x.shape == (B, I, J, C)
            got = ops.pair_arrange(x, H, transpose)
            assert got.shape == (B, H, R, T, D) and got.is_contiguous()
            assert got.dtype == dtype
            assert torch.equal(got, _arrange_ref(x, H, transpose)), (
                B, I, J, H, D, n)
            back = ops.pair_merge(got.view(B * H * R, T, D), B, I, J, H,
                                  transpose)
            assert back.shape == (B, I, J, C) and back.is_contiguous()
            assert torch.equal(back, x), (B, I, J, H, D, n)
        o = _randn(B * H * R, T, D, seed=3, dtype=dtype)
        got = ops.pair_merge(o, B, I, J, H, transpose)
        want = _merge_ref(o, B, I, J, H, transpose)
        assert torch.equal(got, want), (B, I, J, H, D)
        # merged straight into one third of a wider buffer
        for n in range(3):
            buf = torch.zeros(B, I, J, 3 * C, device="cuda", dtype=dtype)
            parts = buf.chunk(3, -1)
            ret = ops.pair_merge(o, B, I, J, H, transpose, parts[n])
            assert ret.data_ptr() == parts[n].data_ptr()
            for m in range(3):
                assert torch.equal(parts[m], want if m == n
                                   else torch.zeros_like(want)), (n, m)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16,
                                   torch.float32],
                         ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("transpose", [False, True])
def test_pair_bias_arrange_equal_permute(transpose, dtype):
    ops = _kernels()
    B = 2
    # one 8-block; a non-power-of-two block count; more than one wave of rows
    for L, H in itertools.product((8, 24, 40), (4, 8)):
        assert ops.pair_bias_arrange_supported(H, L)
        lin = _randn(B, L, L, H, seed=4, dtype=dtype)
        got = ops.pair_bias_arrange(lin, transpose)
        assert got.shape == (B, H, L, L) and got.is_contiguous()
        assert got.dtype == dtype
        assert torch.equal(got, _bias_ref(lin, transpose)), (L, H)
        assert torch.equal(ops.pair_bias_arrange_bwd(got, transpose), lin), (
            L, H)
        d = _randn(B, H, L, L, seed=5, dtype=dtype)
        back = ops.pair_bias_arrange_bwd(d, transpose)
        assert back.shape == (B, L, L, H) and back.is_contiguous()
        assert torch.equal(back, _bias_bwd_ref(d, transpose)), (L, H)


@requires_gpu
def test_host_checks_and_silent_fallbacks(monkeypatch):
    from unicore_amd.modules import (pair_arrange, pair_bias_arrange,
                                     pair_merge)

    ops = _kernels()
    monkeypatch.setenv(GATE, "1")
    assert not ops.pair_bias_arrange_supported(3, 8)
    assert not ops.pair_bias_arrange_supported(4, 12)

    good = _randn(1, 4, 4, 32)
    cpu = good.cpu()
    with pytest.raises(RuntimeError, match="expected a CUDA tensor"):
        ops.pair_arrange(cpu, 4, False)
    with pytest.raises(RuntimeError, match="expected a CUDA tensor"):
        ops.pair_merge(cpu.view(16, 4, 8), 1, 4, 4, 4, False)
    with pytest.raises(RuntimeError, match="expected a CUDA tensor"):
        ops.pair_bias_arrange(torch.zeros(1, 8, 8, 4), False)
    with pytest.raises(RuntimeError, match="expected a CUDA tensor"):
        ops.pair_bias_arrange_bwd(torch.zeros(1, 4, 8, 8), False)
    # D = 4
    with pytest.raises(RuntimeError, match="must be a positive multiple of 8"):
        ops.pair_arrange(good, 8, False)
    with pytest.raises(RuntimeError, match="must be a positive multiple of 8"):
        ops.pair_merge(_randn(32, 4, 4), 1, 4, 4, 8, False)
    # stride(3) != 1
    strided = _randn(1, 4, 4, 64)[..., ::2]
    assert strided.shape == good.shape and strided.stride(3) == 2
    with pytest.raises(RuntimeError, match="channel dim must be contiguous"):
        ops.pair_arrange(strided, 4, False)
    # a row stride that is no multiple of 8
    odd = _randn(1, 4, 4, 36)[..., :32]
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.pair_arrange(odd, 4, False)
    # misaligned storage offset
    mis = _randn(4 * 4 * 32 + 4)[4:].view(1, 4, 4, 32)
    assert mis.is_contiguous() and mis.data_ptr() % 16 == 8
    with pytest.raises(RuntimeError, match="not 16-byte aligned"):
        ops.pair_arrange(mis, 4, False)
    with pytest.raises(RuntimeError, match="not 16-byte aligned"):
        ops.pair_merge(mis.view(16, 4, 8), 1, 4, 4, 4, False)
    o_ok = _randn(16, 4, 8)
    with pytest.raises(RuntimeError, match="is not \\(B, I, J, C\\)"):
        ops.pair_merge(o_ok, 1, 4, 4, 4, False, _randn(1, 4, 5, 32))
    with pytest.raises(RuntimeError, match="not 16-byte aligned"):
        ops.pair_merge(o_ok, 1, 4, 4, 4, False, mis)
    with pytest.raises(RuntimeError, match="positive multiple of 8"):
        ops.pair_merge(o_ok, 1, 4, 4, 4, False, odd)
    with pytest.raises(RuntimeError, match="device and dtype"):
        ops.pair_merge(o_ok, 1, 4, 4, 4, False, good.float())
    mis_b = _randn(8 * 8 * 4 + 4)[4:].view(1, 8, 8, 4)
    with pytest.raises(RuntimeError, match="not 16-byte aligned"):
        ops.pair_bias_arrange(mis_b, False)
    # H = 3, L = 12
    h3, l12 = _randn(1, 8, 8, 3), _randn(1, 12, 12, 4)
    with pytest.raises(RuntimeError, match="H = 3 is not supported"):
        ops.pair_bias_arrange(h3, False)
    with pytest.raises(RuntimeError, match="L = 12 must be a positive multiple"):
        ops.pair_bias_arrange(l12, True)
    with pytest.raises(RuntimeError, match="H = 3 is not supported"):
        ops.pair_bias_arrange_bwd(_randn(1, 3, 8, 8), False)
    with pytest.raises(RuntimeError, match="L = 12 must be a positive multiple"):
        ops.pair_bias_arrange_bwd(_randn(1, 4, 12, 12), False)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        ops.pair_bias_arrange(_randn(1, 8, 8, 8)[..., :4], False)

    # the module-level functions take the permute expression instead
    called = []
    for name in ("pair_arrange", "pair_merge", "pair_bias_arrange"):
        monkeypatch.setattr(
            ops, name, lambda *a, _n=name, **k: called.append(_n))
    for tr in (False, True):
        assert torch.equal(pair_arrange(cpu, 4, tr), _arrange_ref(cpu, 4, tr))
        for x, H in ((good, 8), (strided, 4), (odd, 4), (mis, 4)):
            assert torch.equal(pair_arrange(x, H, tr), _arrange_ref(x, H, tr))
        o4 = _randn(32, 4, 4)
        assert torch.equal(pair_merge(o4, 1, 4, 4, 8, tr),
                           _merge_ref(o4, 1, 4, 4, 8, tr))
        om = mis.view(16, 4, 8)
        assert torch.equal(pair_merge(om, 1, 4, 4, 4, tr),
                           _merge_ref(om, 1, 4, 4, 4, tr))
        for lin in (torch.randn(1, 8, 8, 4), h3, l12, mis_b):
            assert torch.equal(pair_bias_arrange(lin, tr), _bias_ref(lin, tr))
    assert called == []


# --- module ---------------------------------------------------------------

L_MOD, D_PAIR, H_MOD = 24, 32, 4


@functools.lru_cache(maxsize=None)
def _module_case(starting):
    """bf16 module, its input and output gradient, and the float64 CPU
    gradients of the same module (dropout 0); built once, never modified."""
    from unicore_amd.modules import TriangleAttention

    torch.manual_seed(20 + int(starting))
    mod = TriangleAttention(D_PAIR, H_MOD, 0.1, starting=starting)
    with torch.no_grad():
        for p in mod.parameters():
            p.add_(0.1 * torch.randn_like(p))
    mod = mod.cuda().to(torch.bfloat16)
    pair = _randn(1, L_MOD, L_MOD, D_PAIR, seed=21)
    d_out = _randn(1, L_MOD, L_MOD, D_PAIR, seed=22)

    ref = copy.deepcopy(mod).cpu().double()
    ref.dropout = 0.0
    x = pair.detach().cpu().double().requires_grad_()
    ref(x).backward(d_out.cpu().double())
    want = {"pair": x.grad}
    want.update({n: p.grad for n, p in ref.named_parameters()})
    return mod, pair, d_out, want


def _run(mod, pair, d_out=None, train=False, p=None, seed=7):
    from unicore_amd import utils

    mod.train(train)
    old = mod.dropout
    if p is not None:
        mod.dropout = p
    try:
        mod.zero_grad(set_to_none=True)
        x = pair.detach().clone().requires_grad_(d_out is not None)
        with utils.torch_seed(seed):
            out = mod(x)
            if d_out is None:
                return out.detach()
            out.backward(d_out)
        grads = {"pair": x.grad}
        grads.update({n: q.grad.clone() for n, q in mod.named_parameters()})
        return out.detach(), grads
    finally:
        mod.dropout = old
        mod.zero_grad(set_to_none=True)
        mod.eval()


@requires_gpu
@pytest.mark.parametrize("starting", [True, False], ids=["start", "end"])
def test_module_forward_fused_equals_permute_chain(monkeypatch, starting):
    _kernels()
    mod, pair, _, _ = _module_case(starting)
    outs = {}
    for gate in ("1", "0"):
        monkeypatch.setenv(GATE, gate)
        with torch.no_grad():
            outs[gate] = (_run(mod, pair), _run(mod, pair, train=True))
    assert torch.isfinite(outs["1"][0].float()).all()
    assert torch.equal(outs["1"][0], outs["0"][0])
    assert torch.equal(outs["1"][1], outs["0"][1])
    # dropout was really on
    assert not torch.equal(outs["1"][0], outs["1"][1])


@requires_gpu
@pytest.mark.parametrize("starting", [True, False], ids=["start", "end"])
def test_module_gradients_against_float64(monkeypatch, starting):
    """For every tensor, max|gate 1 - R| <= 2 max|gate 0 - R| with R the
    float64 CPU run: the two paths run the same kernels on the same values
    and differ only in which strided GEMM the library picks for the qkv /
    bias_proj gradients."""
    _kernels()
    mod, pair, d_out, want = _module_case(starting)
    errs = {}
    for gate in ("1", "0"):
        monkeypatch.setenv(GATE, gate)
        _, grads = _run(mod, pair, d_out, train=True, p=0.0)
        assert set(grads) == set(want)
        errs[gate] = {
            n: (grads[n].double().cpu() - want[n]).abs().max().item()
            for n in want
        }
    for n in want:
        e1, e0 = errs["1"][n], errs["0"][n]
        print(f"{n}: max|gate1 - f64| = {e1:.4e}  max|gate0 - f64| = {e0:.4e}"
              f"  (max|f64| = {want[n].abs().max().item():.3e})")
    for n in want:
        assert errs["1"][n] <= 2 * errs["0"][n], (n, errs["1"][n], errs["0"][n])


@requires_gpu
@pytest.mark.parametrize("starting", [True, False], ids=["start", "end"])
def test_module_deterministic_with_dropout(monkeypatch, starting):
    _kernels()
    monkeypatch.setenv(GATE, "1")
    mod, pair, d_out, _ = _module_case(starting)
    o1, g1 = _run(mod, pair, d_out, train=True)
    o2, g2 = _run(mod, pair, d_out, train=True)
    assert torch.equal(o1, o2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


@requires_gpu
def test_module_call_counts(monkeypatch):
    from unicore_amd import ops

    _kernels()
    mod, pair, _, _ = _module_case(True)
    calls = {"pair_arrange": 0, "pair_merge": 0, "pair_bias_arrange": 0,
             "pair_bias_arrange_bwd": 0}

    def spy(name):
        real = getattr(ops, name)

        def wrapped(*args):
            calls[name] += 1
            return real(*args)

        monkeypatch.setattr(ops, name, wrapped)

    for name in calls:
        spy(name)
    monkeypatch.setenv(GATE, "1")
    with torch.no_grad():
        _run(mod, pair)
    assert calls == {"pair_arrange": 3, "pair_merge": 1,
                     "pair_bias_arrange": 1, "pair_bias_arrange_bwd": 0}, calls
    monkeypatch.setenv(GATE, "0")
    with torch.no_grad():
        _run(mod, pair)
    assert calls == {"pair_arrange": 3, "pair_merge": 1,
                     "pair_bias_arrange": 1, "pair_bias_arrange_bwd": 0}, calls


# --- model ----------------------------------------------------------------


@requires_gpu
def test_tiny_evoformer_with_triangle_attention(monkeypatch):
    from unicore_amd.data import Dictionary
    from unicore_amd.models.evoformer import EvoformerModel

    _kernels()
    d = Dictionary()
    for sym in ("[CLS]", "[PAD]", "[SEP]", "[UNK]"):
        d.add_symbol(sym, is_special=True)
    for i in range(20):
        d.add_symbol(f"res{i}")
    args = argparse.Namespace(
        evo_layers=2, msa_dim=32, pair_dim=32, evo_heads=4, dropout=0.1,
        max_rel_pos=8, triangle_attention=True,
    )
    torch.manual_seed(30)
    model = EvoformerModel(args, d).cuda().to(torch.bfloat16)
    g = torch.Generator().manual_seed(31)
    tokens = torch.randint(4, len(d), (1, 8, 16), generator=g).cuda()
    target = torch.randint(4, len(d), (1, 8, 16), generator=g).cuda()

    monkeypatch.setenv(GATE, "1")
    model.train()
    logits = model(tokens)
    loss = torch.nn.functional.cross_entropy(
        logits.float().view(-1, len(d)), target.view(-1))
    loss.backward()
    assert torch.isfinite(loss).item()
    seen = 0
    for n, p in model.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad.float()).all(), n
            seen += "tri_att" in n
    assert seen > 0

    model.eval()
    out = {}
    for gate in ("1", "0"):
        monkeypatch.setenv(GATE, gate)
        with torch.no_grad():
            out[gate] = model(tokens)
    assert torch.isfinite(out["1"].float()).all()
    assert torch.equal(out["1"], out["0"])
