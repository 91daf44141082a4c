"""Flash attention kernel parity tests (MI355X, bf16, D=64)."""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)


def _ref_attn(q, k, v, bias=None, mask=None):
    s = q.float() @ k.float().transpose(-1, -2)
    if bias is not None:
        s = s + bias.float()
    if mask is not None:
        s = s + mask.float()
    p = F.softmax(s, dim=-1)
    return p @ v.float(), s


@requires_gpu
@pytest.mark.parametrize("L", [64, 128, 512])
def test_flash_fwd_plain(L):
    from unicore_amd import ops

    torch.manual_seed(0)
    BH = 8
    q = torch.randn(BH, L, 64, device="cuda", dtype=torch.bfloat16) * 0.2
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    o, lse, seed = ops.flash_attn_fwd(q, k, v, None, 1, None, 1, 0.0, True)
    ref, s = _ref_attn(q, k, v)
    assert (o.float() - ref).abs().max().item() < 2e-2, (o.float() - ref).abs().max()
    ref_lse = torch.logsumexp(s, dim=-1)
    assert (lse - ref_lse).abs().max().item() < 1e-3


@requires_gpu
@pytest.mark.parametrize("with_bias_mask", [False, True])
def test_flash_fwd_tiled(with_bias_mask):
    """L = 576 (9 tiles) is the smallest L > 512: the tiled forward, which
    stages V^T per tile, is what every longer no_grad forward runs."""
    from unicore_amd import ops

    torch.manual_seed(12)
    B, H, L = 2, 3, 576
    q = torch.randn(B * H, L, 64, device="cuda", dtype=torch.bfloat16) * 0.2
    k, v = torch.randn_like(q), torch.randn_like(q)
    bias = mask = bias4 = mask4 = None
    if with_bias_mask:
        bias = torch.randn(H, L, L, device="cuda", dtype=torch.bfloat16)
        mask = torch.zeros(B, 1, L, device="cuda", dtype=torch.bfloat16)
        mask[:, :, -17:] = float(torch.finfo(torch.float16).min)
        bias4, mask4 = bias.unsqueeze(0), mask.view(B, 1, 1, L)
    o, lse, seed = ops.flash_attn_fwd(q, k, v, bias, 1, mask, H, 0.0, True)
    ref, s = _ref_attn(q.view(B, H, L, 64), k.view(B, H, L, 64),
                       v.view(B, H, L, 64), bias4, mask4)
    diff = (o.view(B, H, L, 64).float() - ref).abs().max().item()
    assert diff < 2e-2, diff
    ref_lse = torch.logsumexp(s, dim=-1)
    assert (lse.view(B, H, L) - ref_lse).abs().max().item() < 1e-3


@requires_gpu
def test_flash_fwd_bias_mask():
    from unicore_amd import ops

    torch.manual_seed(1)
    B, H, L = 3, 4, 128
    q = torch.randn(B * H, L, 64, device="cuda", dtype=torch.bfloat16) * 0.2
    k, v = torch.randn_like(q), torch.randn_like(q)
    # bias (1, H, L, L) broadcast over batch -> kernel form (H, L, L), od=1
    bias = torch.randn(H, L, L, device="cuda", dtype=torch.bfloat16)
    # mask (B, 1, 1, L) -> kernel form (B, 1, L), od=H
    mask = torch.zeros(B, 1, L, device="cuda", dtype=torch.bfloat16)
    mask[:, :, -17:] = float(torch.finfo(torch.float16).min)
    o, lse, seed = ops.flash_attn_fwd(q, k, v, bias, 1, mask, H, 0.0, True)

    bias4 = bias.unsqueeze(0)
    mask4 = mask.view(B, 1, 1, L)
    q4 = q.view(B, H, L, 64)
    ref, _ = _ref_attn(q4, k.view(B, H, L, 64), v.view(B, H, L, 64), bias4, mask4)
    diff = (o.view(B, H, L, 64).float() - ref).abs().max().item()
    assert diff < 2e-2, diff


@requires_gpu
def test_flash_fwd_dropout_stats_and_determinism():
    from unicore_amd import ops

    torch.manual_seed(2)
    BH, L, p = 8, 256, 0.3
    q = torch.randn(BH, L, 64, device="cuda", dtype=torch.bfloat16) * 0.2
    k, v = torch.randn_like(q), torch.randn_like(q)
    torch.manual_seed(7)
    o1, lse1, seed1 = ops.flash_attn_fwd(q, k, v, None, 1, None, 1, p, True)
    torch.manual_seed(7)
    o2, lse2, seed2 = ops.flash_attn_fwd(q, k, v, None, 1, None, 1, p, True)
    assert torch.equal(o1, o2) and int(seed1) == int(seed2)
    # mean of dropout(P)V stays close to PV (unbiased dropout)
    ref, _ = _ref_attn(q, k, v)
    rel = (o1.float().mean(0) - ref.mean(0)).abs().mean() / ref.abs().mean()
    assert rel.item() < 0.5  # loose: only 8 batches of dropout noise averaged
    assert not torch.equal(o1.float(), ref.bfloat16().float())
    # LSE unaffected by dropout (dropout is post-softmax)
    o3, lse3, _ = ops.flash_attn_fwd(q, k, v, None, 1, None, 1, 0.0, True)
    assert (lse1 - lse3).abs().max().item() < 1e-5


@requires_gpu
@pytest.mark.parametrize("L", [64, 192, 256, 576])
def test_flash_bwd_parity_no_dropout(L):
    from unicore_amd import ops

    torch.manual_seed(3)
    B, H = 2, 3
    BH = B * H
    q = torch.randn(BH, L, 64, device="cuda", dtype=torch.bfloat16) * 0.2
    k, v = torch.randn_like(q), torch.randn_like(q)
    bias = torch.randn(H, L, L, device="cuda", dtype=torch.bfloat16) * 0.5
    mask = torch.zeros(B, 1, L, device="cuda", dtype=torch.bfloat16)
    mask[:, :, -9:] = -1e4

    o, lse, seed = ops.flash_attn_fwd(q, k, v, bias, 1, mask, H, 0.0, True)
    d_out = torch.randn_like(o) * 0.3
    # fused path: grads[3] is the finished (H, L, L) fp32 bias gradient
    dq, dk, dv, dbias = ops.flash_attn_bwd(
        d_out, q, k, v, o, lse, bias, 1, True, mask, H, 0.0, False, int(seed)
    )
    assert dbias.shape == (H, L, L) and dbias.dtype == torch.float32

    # fp32 reference
    qr = q.float().view(B, H, L, 64).requires_grad_(True)
    kr = k.float().view(B, H, L, 64).requires_grad_(True)
    vr = v.float().view(B, H, L, 64).requires_grad_(True)
    br = bias.float().unsqueeze(0).requires_grad_(True)
    s = qr @ kr.transpose(-1, -2) + br + mask.float().view(B, 1, 1, L)
    p = torch.softmax(s, dim=-1)
    (p @ vr).backward(d_out.float().view(B, H, L, 64))

    def cmp(a, b, tol, what):
        d = (a.float().view_as(b) - b).abs().max().item()
        scale = b.abs().max().item() + 1e-6
        assert d / scale < tol, f"{what}: {d} vs scale {scale}"

    cmp(dq, qr.grad, 0.05, "dq")
    cmp(dk, kr.grad, 0.05, "dk")
    cmp(dv, vr.grad, 0.05, "dv")
    cmp(dbias, br.grad.squeeze(0), 0.05, "dbias")


@requires_gpu
def test_flash_bwd_dropout_identity_v():
    """With V = I (L = 64) the forward output exposes the dropout keep-mask
    exactly, so the backward can be checked against an explicit-mask fp32
    reference."""
    from unicore_amd import ops

    torch.manual_seed(4)
    BH, L, p = 6, 64, 0.4
    q = torch.randn(BH, L, 64, device="cuda", dtype=torch.bfloat16) * 0.2
    k = torch.randn_like(q)
    v = torch.eye(64, device="cuda", dtype=torch.bfloat16).expand(BH, 64, 64).contiguous()

    torch.manual_seed(11)
    o, lse, seed = ops.flash_attn_fwd(q, k, v, None, 1, None, 1, p, True)
    keep = (o != 0).float()  # (BH, L, L) since O = drop(P) with V = I
    d_out = torch.randn_like(o) * 0.3
    dq, dk, dv = ops.flash_attn_bwd(
        d_out, q, k, v, o, lse, None, 1, False, None, 1, p, True, int(seed)
    )

    qr = q.float().requires_grad_(True)
    kr = k.float().requires_grad_(True)
    vr = v.float().requires_grad_(True)
    s = qr @ kr.transpose(-1, -2)
    pr = torch.softmax(s, dim=-1)
    pd = pr * keep / (1.0 - p)
    (pd @ vr).backward(d_out.float())

    def cmp(a, b, tol, what):
        d = (a.float() - b).abs().max().item()
        scale = b.abs().max().item() + 1e-6
        assert d / scale < tol, f"{what}: {d} vs scale {scale}"

    # forward itself matches the explicit-mask reference
    assert ((o.float() - pd.detach() @ vr.detach().float()).abs().max() /
            (o.float().abs().max() + 1e-6)).item() < 0.03
    cmp(dq, qr.grad, 0.06, "dq")
    cmp(dk, kr.grad, 0.06, "dk")
    cmp(dv, vr.grad, 0.06, "dv")


def _identity_block_v(BH, L, c):
    """V whose rows 64c .. 64c+63 are the identity and all others zero, so
    that O = dropout(P) V is columns 64c .. 64c+63 of dropout(P)."""
    v = torch.zeros(BH, L, 64, device="cuda", dtype=torch.bfloat16)
    v[:, 64 * c:64 * (c + 1), :] = torch.eye(64, device="cuda",
                                             dtype=torch.bfloat16)
    return v


@requires_gpu
@pytest.mark.parametrize("L,with_bias",
                         [(192, False), (192, True), (256, True), (576, True)])
def test_flash_bwd_dropout_explicit_mask(L, with_bias):
    """The identity-V trick beyond one tile.  The keep bits depend on
    (seed, row, kv) only, so L / 64 forwards from the same generator state,
    each with one 64-row identity block in V, read out the whole keep mask;
    forward and backward with a random V and that seed are then compared
    with an explicit-mask fp32 reference.  L = 192 runs dq_kres + dkv_qres,
    256 dq_k32 + dkv_qres, 576 the tiled forward, dq and dkv."""
    from unicore_amd import ops

    torch.manual_seed(5)
    B, H, p = 2, 3, 0.3
    BH = B * H
    q = torch.randn(BH, L, 64, device="cuda", dtype=torch.bfloat16) * 0.2
    k, v = torch.randn_like(q), torch.randn_like(q)
    bias = None
    if with_bias:
        bias = torch.randn(H, L, L, device="cuda", dtype=torch.bfloat16) * 0.5

    cols, seeds = [], []
    for c in range(L // 64):
        torch.manual_seed(13)
        o_c, _, seed_c = ops.flash_attn_fwd(
            q, k, _identity_block_v(BH, L, c), bias, 1, None, 1, p, True)
        cols.append(o_c != 0)
        seeds.append(int(seed_c))
    keep = torch.cat(cols, dim=-1).float()  # (BH, L, L)
    assert len(set(seeds)) == 1, seeds
    # binomial 5-sigma band around 1 - p (the 16-bit threshold moves the
    # rate by less than 2^-16)
    rate = keep.mean().item()
    sigma = math.sqrt(p * (1.0 - p) / keep.numel())
    assert abs(rate - (1.0 - p)) < 5.0 * sigma + 2.0 ** -16, (rate, sigma)

    torch.manual_seed(13)
    o, lse, seed = ops.flash_attn_fwd(q, k, v, bias, 1, None, 1, p, True)
    assert int(seed) == seeds[0]
    d_out = torch.randn_like(o) * 0.3
    dq, dk, dv = ops.flash_attn_bwd(
        d_out, q, k, v, o, lse, bias, 1, False, None, 1, p, True, int(seed)
    )

    qr = q.float().view(B, H, L, 64).requires_grad_(True)
    kr = k.float().view(B, H, L, 64).requires_grad_(True)
    vr = v.float().view(B, H, L, 64).requires_grad_(True)
    s = qr @ kr.transpose(-1, -2)
    if with_bias:
        s = s + bias.float().unsqueeze(0)
    pd = torch.softmax(s, dim=-1) * keep.view(B, H, L, L) / (1.0 - p)
    ref = pd @ vr
    ref.backward(d_out.float().view(B, H, L, 64))

    def cmp(a, b, tol, what):
        d = (a.float().view_as(b) - b).abs().max().item()
        scale = b.abs().max().item() + 1e-6
        assert d / scale < tol, f"{what}: {d} vs scale {scale}"

    cmp(o, ref.detach(), 0.03, "o")
    cmp(dq, qr.grad, 0.06, "dq")
    cmp(dk, kr.grad, 0.06, "dk")
    cmp(dv, vr.grad, 0.06, "dv")


@requires_gpu
@pytest.mark.parametrize("L", [192, 576])
def test_flash_double_run_bitwise(L):
    """Same seed, same bits: forward and backward with dropout, bias and
    mask, including the materialised bias gradient."""
    from unicore_amd import ops

    torch.manual_seed(6)
    B, H, p = 2, 3, 0.3
    q = torch.randn(B * H, L, 64, device="cuda", dtype=torch.bfloat16) * 0.2
    k, v = torch.randn_like(q), torch.randn_like(q)
    bias = torch.randn(H, L, L, device="cuda", dtype=torch.bfloat16) * 0.5
    mask = torch.zeros(B, 1, L, device="cuda", dtype=torch.bfloat16)
    mask[:, :, -9:] = -1e4
    d_out = torch.randn_like(q) * 0.3

    def run():
        torch.manual_seed(17)
        o, lse, seed = ops.flash_attn_fwd(q, k, v, bias, 1, mask, H, p, True)
        grads = ops.flash_attn_bwd(
            d_out, q, k, v, o, lse, bias, 1, True, mask, H, p, True, int(seed)
        )
        return (o, lse, *grads), int(seed)

    first, seed1 = run()
    second, seed2 = run()
    assert seed1 == seed2
    assert len(first) == 6  # o, lse, dq, dk, dv, dbias
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv", "dbias"),
                          first, second):
        assert torch.equal(a, b), name


@requires_gpu
def test_flash_bwd_rejects_bad_inputs():
    """The backward validates what the forward validates, before any launch."""
    from unicore_amd import ops

    def inputs(L):
        q = torch.randn(4, L, 64, device="cuda", dtype=torch.bfloat16)
        lse = torch.zeros(4, L, device="cuda", dtype=torch.float32)
        return dict(d_out=q.clone(), q=q, k=q.clone(), v=q.clone(),
                    o=q.clone(), lse=lse)

    def bwd(t):
        return ops.flash_attn_bwd(t["d_out"], t["q"], t["k"], t["v"], t["o"],
                                  t["lse"], None, 1, False, None, 1, 0.0,
                                  False, 0)

    t = inputs(64)
    t["d_out"] = t["d_out"].float()
    with pytest.raises(RuntimeError):
        bwd(t)
    with pytest.raises(RuntimeError):
        bwd(inputs(96))
    t = inputs(64)
    t["lse"] = torch.zeros(4, 32, device="cuda", dtype=torch.float32)
    with pytest.raises(RuntimeError):
        bwd(t)


@requires_gpu
def test_attention_module_flash_vs_materialized(monkeypatch):
    """SelfMultiheadAttention end-to-end: the flash path must match the
    materialized bmm+softmax path (bf16, p=0) including input and bias
    gradients."""
    import os

    from unicore_amd.modules import SelfMultiheadAttention
    from unicore_amd.modules import multihead_attention as mha

    monkeypatch.setenv("UNICORE_FLASH_ATTN", "1")

    torch.manual_seed(0)
    B, L, H, D = 2, 128, 4, 64
    attn = SelfMultiheadAttention(H * D, H, dropout=0.0).cuda().bfloat16()
    x = torch.randn(B, L, H * D, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    bias = (torch.randn(1, H, L, L, device="cuda", dtype=torch.bfloat16) * 0.3
            ).requires_grad_(True)
    pad = torch.zeros(B, 1, 1, L, device="cuda", dtype=torch.bfloat16)
    pad[:, :, :, -7:] = float("-inf")

    out_flash = attn(x, key_padding_mask=pad, attn_bias=bias)
    out_flash.float().pow(2).mean().backward()
    gx_flash, gb_flash = x.grad.clone(), bias.grad.clone()
    x.grad = bias.grad = None

    # direct fp32 reference instead of path-juggling
    qkv = attn.in_proj(x.detach()).float()
    q, k, v = qkv.chunk(3, dim=-1)

    def heads(t):
        return t.view(B, L, H, D).permute(0, 2, 1, 3)

    xr = x.detach().clone().requires_grad_(True)
    br = bias.detach().clone().requires_grad_(True)
    qkv_r = attn.in_proj(xr).float()
    qr, kr, vr = qkv_r.chunk(3, dim=-1)
    s = heads(qr) @ heads(kr).transpose(-1, -2) * attn.scaling
    s = s + br.float() + pad.float()
    p = torch.softmax(s, dim=-1)
    o = (p @ heads(vr)).permute(0, 2, 1, 3).reshape(B, L, H * D)
    ref = attn.out_proj(o.to(torch.bfloat16))
    ref.float().pow(2).mean().backward()

    assert (out_flash.float() - ref.float()).abs().max().item() < 3e-2
    scale = xr.grad.float().abs().max().item() + 1e-6
    assert (gx_flash.float() - xr.grad.float()).abs().max().item() / scale < 0.06
    bscale = br.grad.float().abs().max().item() + 1e-6
    assert (gb_flash.float() - br.grad.float()).abs().max().item() / bscale < 0.06


@requires_gpu
def test_flash_bwd_fused_dbias_long_seq():
    """L >= 2048 takes the fused atomic dbias path (no dS materialization);
    it must agree with the deterministic materialized fallback."""
    from unicore_amd import ops

    torch.manual_seed(9)
    B, H, L = 2, 2, 2048
    BH = B * H
    q = torch.randn(BH, L, 64, device="cuda", dtype=torch.bfloat16) * 0.2
    k, v = torch.randn_like(q), torch.randn_like(q)
    bias = torch.randn(H, L, L, device="cuda", dtype=torch.bfloat16) * 0.3

    o, lse, seed = ops.flash_attn_fwd(q, k, v, bias, 1, None, 1, 0.0, True)
    d_out = torch.randn_like(o) * 0.3
    _, _, _, dbias_fused = ops.flash_attn_bwd(
        d_out, q, k, v, o, lse, bias, 1, True, None, 1, 0.0, False, int(seed)
    )
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        _, _, _, dbias_det = ops.flash_attn_bwd(
            d_out, q, k, v, o, lse, bias, 1, True, None, 1, 0.0, False,
            int(seed)
        )
    finally:
        torch.use_deterministic_algorithms(False)
    # fused accumulates pre-rounding fp32; fallback sums bf16-rounded dS
    scale = dbias_det.abs().max().item() + 1e-6
    assert (dbias_fused - dbias_det).abs().max().item() / scale < 0.03
