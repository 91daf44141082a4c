"""Compact Evoformer-style model (BASELINE.json stress config 5).

Uni-Fold's trunk shape, original implementation: MSA row attention with a
pair bias (the fused softmax_dropout 5-D broadcast path: scores arranged
(B, H, S, L, L) so the (B, H, 1, L, L) bias maps onto the kernel's
(src_nb, outer_div) addressing with no materialized broadcast), MSA column
attention, MSA transition, outer-product-mean pair update, triangle
multiplication (outgoing + incoming) and pair transition — all through the
framework's fused LayerNorm.  ``--triangle-attention`` adds the other two
pair-stack modules, triangle self-attention around the starting and the
ending node (modules/triangle_attention.py), between the incoming triangle
multiplication and the pair transition.  Intended to run bf16 + stochastic rounding
with grad accumulation (exercising the rounding and multi-tensor kernels).
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from unicore_amd.models import (
    BaseUnicoreModel,
    register_model,
    register_model_architecture,
)
from unicore_amd import utils
from unicore_amd.modules.msa_arrange import msa_arrange, msa_merge
from unicore_amd.modules.multihead_attention import qk_scores
from unicore_amd.modules import (
    LayerNorm,
    dropout_add,
    gated_mul,
    gelu_dropout,
    softmax_dropout,
    triangle_multiply,
    outer_product_mean,
)
from unicore_amd.modules.dropout_add_ln import dropout_add_ln_pre
from unicore_amd.modules.embedding import Embedding
from unicore_amd.modules.padding_mask import build_evoformer_masks
from unicore_amd.modules.triangle_attention import TriangleAttention


def _fold_ok(*biases):
    """GPU bias folding into the fused elementwise ops (see
    transformer_encoder_layer.py): all biases present and colsum-able."""
    if os.environ.get("UNICORE_FOLD_BIAS", "1") != "1":
        return False
    from unicore_amd import ops

    if not ops.gpu_kernels_available():
        return False
    return all(b is not None and ops.colsum_supported(b.numel()) for b in biases)


class MSARowAttentionWithPairBias(nn.Module):
    def __init__(self, d_msa, d_pair, heads, dropout):
        super().__init__()
        self.heads = heads
        self.head_dim = d_msa // heads
        self.norm = LayerNorm(d_msa)
        self.pair_norm = LayerNorm(d_pair)
        self.qkv = nn.Linear(d_msa, 3 * d_msa, bias=False)
        self.pair_bias = nn.Linear(d_pair, heads, bias=False)
        self.gate = nn.Linear(d_msa, d_msa)
        self.out = nn.Linear(d_msa, d_msa)
        self.dropout = dropout
        self.scaling = self.head_dim**-0.5

    def forward(self, msa, pair, skip_out_bias=False, x_normed=None,
                key_mask=None):
        # key_mask: additive (B, 1, S, 1, L), padded residues as keys
        B, S, L, D = msa.shape
        H, Dh = self.heads, self.head_dim
        x = self.norm(msa) if x_normed is None else x_normed
        q, k, v = self.qkv(x).chunk(3, dim=-1)
        # (B, S, L, H, Dh) -> (B, H, S, L, Dh): heads OUTSIDE the msa-row dim
        # so the (B, H, 1, L, L) pair bias is a contiguous-block broadcast
        # for the fused softmax kernel
        def arrange(t):
            return msa_arrange(t, H, col=False)

        q = arrange(q) * self.scaling
        k = arrange(k)
        v = arrange(v)
        scores = qk_scores(q, k).view(B, H, S, L, L)
        bias = self.pair_bias(self.pair_norm(pair))  # (B, L, L, H)
        bias = bias.permute(0, 3, 1, 2).unsqueeze(2)  # (B, H, 1, L, L)
        attn = softmax_dropout(scores, self.dropout, self.training,
                               mask=key_mask, bias=bias)
        o = torch.bmm(attn.view(B * H * S, L, L), v)
        o = msa_merge(o, B, S, L, H, col=False)
        if _fold_ok(self.gate.bias):
            og = gated_mul(o, F.linear(x, self.gate.weight),
                           torch.zeros_like(self.gate.bias), self.gate.bias)
        else:
            og = o * torch.sigmoid(self.gate(x))
        if skip_out_bias:
            return F.linear(og, self.out.weight)
        return self.out(og)


class MSAColumnAttention(nn.Module):
    def __init__(self, d_msa, heads, dropout):
        super().__init__()
        self.heads = heads
        self.head_dim = d_msa // heads
        self.norm = LayerNorm(d_msa)
        self.qkv = nn.Linear(d_msa, 3 * d_msa, bias=False)
        self.gate = nn.Linear(d_msa, d_msa)
        self.out = nn.Linear(d_msa, d_msa)
        self.dropout = dropout
        self.scaling = self.head_dim**-0.5

    def forward(self, msa, skip_out_bias=False, x_normed=None, key_mask=None):
        # key_mask: additive (B, L, 1, 1, S), padded MSA rows as keys
        B, S, L, D = msa.shape
        H, Dh = self.heads, self.head_dim
        x = self.norm(msa) if x_normed is None else x_normed
        q, k, v = self.qkv(x).chunk(3, dim=-1)

        # attention over the S dimension for each column l
        def arrange(t):
            return msa_arrange(t, H, col=True)

        q = arrange(q) * self.scaling
        k = arrange(k)
        v = arrange(v)
        scores = qk_scores(q, k).view(B * L * H, S, S)
        if key_mask is None:
            attn = softmax_dropout(scores, self.dropout, self.training)
        else:
            # msa_arrange(col=True) orders the batches (B, L, H)
            attn = softmax_dropout(scores.view(B, L, H, S, S), self.dropout,
                                   self.training, mask=key_mask)
            attn = attn.view(B * L * H, S, S)
        o = torch.bmm(attn, v)
        o = msa_merge(o, B, S, L, H, col=True)
        if _fold_ok(self.gate.bias):
            og = gated_mul(o, F.linear(x, self.gate.weight),
                           torch.zeros_like(self.gate.bias), self.gate.bias)
        else:
            og = o * torch.sigmoid(self.gate(x))
        if skip_out_bias:
            return F.linear(og, self.out.weight)
        return self.out(og)


class Transition(nn.Module):
    def __init__(self, d, mult=4):
        super().__init__()
        self.norm = LayerNorm(d)
        self.fc1 = nn.Linear(d, d * mult)
        self.fc2 = nn.Linear(d * mult, d)

    def forward(self, x, residual=None):
        y = self.norm(x)
        if residual is not None and _fold_ok(self.fc1.bias, self.fc2.bias) \
                and y.is_cuda:
            y = F.linear(y, self.fc1.weight)
            y = gelu_dropout(y, 0.0, self.training, bias=self.fc1.bias)
            y = F.linear(y, self.fc2.weight)
            return dropout_add(y, residual, 0.0, self.training,
                               bias=self.fc2.bias)
        y = self.fc2(F.gelu(self.fc1(y)))
        return y if residual is None else residual + y

    def tail(self, y):
        """fc1 -> GELU -> fc2 WITHOUT the trailing fc2 bias: the caller's
        fused residual join folds it in (caller guarantees CUDA +
        _fold_ok(fc1.bias, fc2.bias))."""
        y = F.linear(y, self.fc1.weight)
        y = gelu_dropout(y, 0.0, self.training, bias=self.fc1.bias)
        return F.linear(y, self.fc2.weight)


class OuterProductMean(nn.Module):
    def __init__(self, d_msa, d_pair, c=32):
        super().__init__()
        self.norm = LayerNorm(d_msa)
        self.a = nn.Linear(d_msa, c)
        self.b = nn.Linear(d_msa, c)
        self.out = nn.Linear(c * c, d_pair)
        self.c = c

    def forward(self, msa, skip_out_bias=False, x_normed=None, mask=None,
                inv_norm=None):
        # mask: 0/1 (B, S, L); inv_norm: its opm_mask_inv_norm, (B, L, L)
        x = self.norm(msa) if x_normed is None else x_normed
        a = self.a(x)  # (B, S, L, c)
        b = self.b(x)
        # (B, L, L, c*c), mean over S (over the real rows under a mask)
        o = outer_product_mean(a, b, mask=mask, inv_norm=inv_norm)
        if skip_out_bias:
            return F.linear(o, self.out.weight)
        return self.out(o)


class TriangleMultiplication(nn.Module):
    def __init__(self, d_pair, c=64, outgoing=True):
        super().__init__()
        self.norm = LayerNorm(d_pair)
        self.a_proj = nn.Linear(d_pair, c)
        self.a_gate = nn.Linear(d_pair, c)
        self.b_proj = nn.Linear(d_pair, c)
        self.b_gate = nn.Linear(d_pair, c)
        self.out_norm = LayerNorm(c)
        self.out = nn.Linear(c, d_pair)
        self.gate = nn.Linear(d_pair, d_pair)
        self.outgoing = outgoing

    def forward(self, pair, p_normed=None, pair_mask=None):
        # pair_mask: 0/1 (B, I, J), multiplies a and b after gating so the
        # contraction skips padded k
        p = self.norm(pair) if p_normed is None else p_normed
        if _fold_ok(self.a_proj.bias, self.a_gate.bias, self.b_proj.bias,
                    self.b_gate.bias, self.out.bias, self.gate.bias):
            a = gated_mul(F.linear(p, self.a_proj.weight),
                          F.linear(p, self.a_gate.weight),
                          self.a_proj.bias, self.a_gate.bias,
                          row_mask=pair_mask)
            b = gated_mul(F.linear(p, self.b_proj.weight),
                          F.linear(p, self.b_gate.weight),
                          self.b_proj.bias, self.b_gate.bias,
                          row_mask=pair_mask)
        else:
            a = self.a_proj(p) * torch.sigmoid(self.a_gate(p))  # (B, I, J, c)
            b = self.b_proj(p) * torch.sigmoid(self.b_gate(p))
            if pair_mask is not None:
                a = a * pair_mask.unsqueeze(-1)
                b = b * pair_mask.unsqueeze(-1)
        o = triangle_multiply(a, b, self.outgoing)
        if _fold_ok(self.out.bias, self.gate.bias):
            return gated_mul(F.linear(self.out_norm(o), self.out.weight),
                             F.linear(p, self.gate.weight),
                             self.out.bias, self.gate.bias)
        o = self.out(self.out_norm(o))
        return o * torch.sigmoid(self.gate(p))


class EvoformerBlock(nn.Module):
    def __init__(self, d_msa, d_pair, heads, dropout,
                 triangle_attention=False, tri_attn_heads=4,
                 msa_dropout=0.0, pair_dropout=0.0):
        super().__init__()
        # shared-axis dropout of the residual joins (AlphaFold 2 Alg. 6):
        # row-wise (mask shared over dim 1) after row_attn, tri_out, tri_in
        # and tri_att_start, column-wise (dim 2) after tri_att_end
        self.msa_dropout = msa_dropout
        self.pair_dropout = pair_dropout
        self.row_attn = MSARowAttentionWithPairBias(d_msa, d_pair, heads, dropout)
        self.col_attn = MSAColumnAttention(d_msa, heads, dropout)
        self.msa_transition = Transition(d_msa)
        self.opm = OuterProductMean(d_msa, d_pair)
        self.tri_out = TriangleMultiplication(d_pair, outgoing=True)
        self.tri_in = TriangleMultiplication(d_pair, outgoing=False)
        self.pair_transition = Transition(d_pair)
        # constructed last and only on request: without the flag the
        # parameter names and the initialisation order are unchanged
        self.triangle_attention = triangle_attention
        if triangle_attention:
            self.tri_att_start = TriangleAttention(d_pair, tri_attn_heads,
                                                   dropout, starting=True)
            self.tri_att_end = TriangleAttention(d_pair, tri_attn_heads,
                                                 dropout, starting=False)

    def _join(self, y, residual, p, shared_dim):
        """Residual join of the plain chain; a plain add unless shared
        dropout is on."""
        if self.training and p > 0:
            return dropout_add(y, residual, p, True, shared_dim=shared_dim)
        return residual + y

    def forward(self, msa, pair, masks=None):
        """masks: optional padding_mask.EvoformerMasks of a padded batch."""
        # keyword arguments of the masked sub-modules; empty without masks,
        # so that every call is then the one it has always been
        k_row = k_col = k_opm = k_tri = k_start = k_end = {}
        if masks is not None:
            k_row = {"key_mask": masks.row_key}
            k_col = {"key_mask": masks.col_key}
            k_opm = {"mask": masks.msa, "inv_norm": masks.opm_inv_norm}
            k_tri = {"pair_mask": masks.pair}
            k_start = {"key_mask": masks.tri_start_key}
            k_end = {"key_mask": masks.tri_end_key}
        fold = msa.is_cuda and _fold_ok(
            self.row_attn.out.bias, self.col_attn.out.bias,
            self.msa_transition.fc1.bias, self.msa_transition.fc2.bias,
            self.opm.out.bias,
            self.pair_transition.fc1.bias, self.pair_transition.fc2.bias,
        )
        if fold and self.triangle_attention:
            fold = _fold_ok(self.tri_att_start.out.bias,
                            self.tri_att_end.out.bias)
        if fold:
            # pre-LN residual chain: each join is ONE fused kernel emitting
            # both the summed stream and the next sub-module's normed input
            # (the 6 standalone LayerNorms + 6 residual adds per block
            # collapse into the joins; only the block's first norm remains)
            t = self.training
            # shared_dim only where dropout is on: at 0 the joins are the
            # unshared ones (shared_dim=None is their default)
            md = self.msa_dropout if t else 0.0
            pd = self.pair_dropout if t else 0.0
            mrow = 1 if md > 0 else None
            prow = 1 if pd > 0 else None
            pcol = 2 if pd > 0 else None
            n = self.row_attn.norm(msa)
            y = self.row_attn(msa, pair, skip_out_bias=True, x_normed=n,
                              **k_row)
            msa, n = dropout_add_ln_pre(y, msa, self.col_attn.norm, md, t,
                                        bias=self.row_attn.out.bias,
                                        shared_dim=mrow)
            y = self.col_attn(msa, skip_out_bias=True, x_normed=n,
                              **k_col)
            msa, n = dropout_add_ln_pre(y, msa, self.msa_transition.norm, 0.0,
                                        t, bias=self.col_attn.out.bias)
            y = self.msa_transition.tail(n)
            msa, n = dropout_add_ln_pre(y, msa, self.opm.norm, 0.0, t,
                                        bias=self.msa_transition.fc2.bias)
            y = self.opm(msa, skip_out_bias=True, x_normed=n, **k_opm)
            pair, pn = dropout_add_ln_pre(y, pair, self.tri_out.norm, 0.0, t,
                                          bias=self.opm.out.bias)
            y = self.tri_out(pair, p_normed=pn, **k_tri)
            pair, pn = dropout_add_ln_pre(y, pair, self.tri_in.norm, pd, t,
                                          shared_dim=prow)
            y = self.tri_in(pair, p_normed=pn, **k_tri)
            if self.triangle_attention:
                pair, pn = dropout_add_ln_pre(y, pair, self.tri_att_start.norm,
                                              pd, t, shared_dim=prow)
                y = self.tri_att_start(pair, skip_out_bias=True, p_normed=pn,
                                       **k_start)
                pair, pn = dropout_add_ln_pre(
                    y, pair, self.tri_att_end.norm, pd, t,
                    bias=self.tri_att_start.out.bias, shared_dim=prow)
                y = self.tri_att_end(pair, skip_out_bias=True, p_normed=pn,
                                     **k_end)
                pair, pn = dropout_add_ln_pre(
                    y, pair, self.pair_transition.norm, pd, t,
                    bias=self.tri_att_end.out.bias, shared_dim=pcol)
            else:
                pair, pn = dropout_add_ln_pre(y, pair,
                                              self.pair_transition.norm, pd, t,
                                              shared_dim=prow)
            y = self.pair_transition.tail(pn)
            pair = dropout_add(y, pair, 0.0, t,
                               bias=self.pair_transition.fc2.bias)
            return msa, pair
        msa = self._join(self.row_attn(msa, pair, **k_row), msa,
                         self.msa_dropout, 1)
        msa = msa + self.col_attn(msa, **k_col)
        msa = self.msa_transition(msa, residual=msa)
        pair = pair + self.opm(msa, **k_opm)
        pair = self._join(self.tri_out(pair, **k_tri), pair,
                          self.pair_dropout, 1)
        pair = self._join(self.tri_in(pair, **k_tri), pair,
                          self.pair_dropout, 1)
        if self.triangle_attention:
            pair = self._join(self.tri_att_start(pair, **k_start),
                              pair, self.pair_dropout, 1)
            pair = self._join(self.tri_att_end(pair, **k_end), pair,
                              self.pair_dropout, 2)
        pair = self.pair_transition(pair, residual=pair)
        return msa, pair


@register_model("evoformer")
class EvoformerModel(BaseUnicoreModel):
    @staticmethod
    def add_args(parser):
        parser.add_argument("--evo-layers", type=int, metavar="N")
        parser.add_argument("--msa-dim", type=int, metavar="N")
        parser.add_argument("--pair-dim", type=int, metavar="N")
        parser.add_argument("--evo-heads", type=int, metavar="N")
        parser.add_argument("--dropout", type=float)
        parser.add_argument("--msa-dropout", type=float, metavar="P",
                            help="row-wise shared dropout (one mask per "
                                 "residue column, shared over the MSA depth) "
                                 "at the join after MSA row attention; "
                                 "AlphaFold 2 trains with 0.15")
        parser.add_argument("--pair-dropout", type=float, metavar="P",
                            help="shared dropout at the joins after both "
                                 "triangle multiplications and the starting "
                                 "node attention (row-wise) and after the "
                                 "ending node attention (column-wise); "
                                 "AlphaFold 2 trains with 0.25")
        parser.add_argument("--max-rel-pos", type=int)
        parser.add_argument("--recycle-iters", type=int,
                            help="AlphaFold-style recycling: run the block "
                                 "stack N+1 times, gradients only through "
                                 "the last pass")
        parser.add_argument("--activation-checkpoint", action="store_true",
                            help="recompute each Evoformer block in "
                                 "backward (utils.checkpoint_sequential)")
        parser.add_argument("--triangle-attention", action="store_true",
                            help="add triangle self-attention (starting and "
                                 "ending node) to every block's pair stack, "
                                 "between the incoming triangle "
                                 "multiplication and the pair transition")
        parser.add_argument("--tri-attn-heads", type=int, metavar="N",
                            help="heads of the triangle attention modules")
        parser.add_argument("--msa-padding-mask", action="store_true",
                            help="derive a padding mask from src_tokens "
                                 "(1 where a token is not pad) and mask the "
                                 "row/column/triangle attention keys, the "
                                 "outer-product mean and the triangle "
                                 "multiplications with it, so that ragged "
                                 "MSAs can be batched with padding")
        parser.add_argument("--hip-graph-blocks", action="store_true",
                            help="capture each Evoformer block as a hipGraph "
                                 "(fwd+bwd) and replay it — removes the "
                                 "per-step launch overhead of this "
                                 "launch-bound stack. Requires --dropout 0 "
                                 "(dropout kernels take their philox seed "
                                 "as a kernel argument, which a captured "
                                 "graph would freeze) and static shapes.")

    def __init__(self, args, dictionary):
        super().__init__()
        evoformer_base_architecture(args)
        self.args = args
        self.padding_idx = dictionary.pad()
        self.embed_msa = Embedding(
            len(dictionary), args.msa_dim, self.padding_idx
        )
        self.max_rel = args.max_rel_pos
        self.rel_pos_embed = nn.Embedding(2 * self.max_rel + 1, args.pair_dim)
        self.blocks = nn.ModuleList(
            [
                EvoformerBlock(args.msa_dim, args.pair_dim, args.evo_heads,
                               args.dropout,
                               triangle_attention=args.triangle_attention,
                               tri_attn_heads=args.tri_attn_heads,
                               msa_dropout=args.msa_dropout,
                               pair_dropout=args.pair_dropout)
                for _ in range(args.evo_layers)
            ]
        )
        self.final_norm = LayerNorm(args.msa_dim)
        self.lm_head = nn.Linear(args.msa_dim, len(dictionary))
        self.recycle_iters = args.recycle_iters
        self.activation_checkpoint = args.activation_checkpoint
        self.hip_graph_blocks = getattr(args, "hip_graph_blocks", False)
        self._graphed_blocks = None
        self.msa_padding_mask = getattr(args, "msa_padding_mask", False)
        assert not (self.msa_padding_mask and self.hip_graph_blocks), (
            "--hip-graph-blocks and --msa-padding-mask are mutually "
            "exclusive: the masks change with every batch, a captured graph "
            "would replay the ones it was captured with"
        )

    @classmethod
    def build_model(cls, args, task):
        return cls(args, task.dictionary)

    class _TrunkRunner(nn.Module):
        """The whole block loop as one callable, so hipGraph capture wraps
        ONE graph around every block (a graph per block pays a static-buffer
        copy of the 16 MB msa/pair tensors per block — measured slower)."""

        def __init__(self, blocks):
            super().__init__()
            self.blocks = blocks

        def forward(self, msa, pair):
            for blk in self.blocks:
                msa, pair = blk(msa, pair)
            return msa, pair

    def _graphed_trunk(self, msa, pair):
        """One fwd+bwd hipGraph over the whole trunk, captured on first use."""
        if self._graphed_blocks is None:
            assert self.args.dropout == 0, (
                "--hip-graph-blocks requires --dropout 0: the dropout "
                "kernels key philox off a kernel argument, which graph "
                "replay would freeze"
            )
            assert self.args.msa_dropout == 0 and \
                self.args.pair_dropout == 0, (
                "--hip-graph-blocks requires --msa-dropout 0 and "
                "--pair-dropout 0: the shared-dropout joins key philox off "
                "a kernel argument too"
            )
            assert not self.activation_checkpoint, (
                "--hip-graph-blocks and --activation-checkpoint are "
                "mutually exclusive"
            )
            sample = (
                msa.detach().clone().requires_grad_(True),
                pair.detach().clone().requires_grad_(True),
            )
            self._graphed_blocks = torch.cuda.make_graphed_callables(
                self._TrunkRunner(self.blocks), sample
            )
        return self._graphed_blocks(msa, pair)

    def _trunk(self, msa, pair, masks=None):
        if self.hip_graph_blocks and msa.is_cuda:
            assert masks is None, "--hip-graph-blocks takes no padding masks"
            return self._graphed_trunk(msa, pair)
        if self.activation_checkpoint and self.training:
            # recompute each block in backward; the msa/pair pair threads
            # through as the tuple state (utils.checkpoint_sequential), the
            # masks (no gradient) ride the closures
            fns = [
                (lambda b: (lambda m, p: b(m, p, masks)))(blk)
                for blk in self.blocks
            ]
            msa, pair = utils.checkpoint_sequential(fns, (msa, pair))
        else:
            for blk in self.blocks:
                msa, pair = blk(msa, pair, masks)
        return msa, pair

    def forward(self, src_tokens, msa_mask=None, **kwargs):
        # src_tokens: (B, S, L); msa_mask: optional (B, S, L), 1 = real token
        B, S, L = src_tokens.shape
        msa = self.embed_msa(src_tokens)
        masks = None
        if self.msa_padding_mask or msa_mask is not None:
            # always derived under the flag: testing it for padding first
            # would be a device sync
            if msa_mask is None:
                msa_mask = src_tokens.ne(self.padding_idx)
            masks = build_evoformer_masks(msa_mask, msa.dtype)
        pos = torch.arange(L, device=src_tokens.device)
        rel = (pos[None, :] - pos[:, None]).clamp(-self.max_rel, self.max_rel)
        pair = self.rel_pos_embed(rel + self.max_rel)  # (L, L, Dp)
        pair = pair.unsqueeze(0).expand(B, -1, -1, -1).contiguous()
        pair = pair.to(msa.dtype)
        # AlphaFold-style recycling: extra no-grad passes refine the
        # representations; only the final pass builds the autograd graph
        for _ in range(self.recycle_iters):
            with torch.no_grad():
                msa, pair = self._trunk(msa, pair, masks)
        msa, pair = self._trunk(msa, pair, masks)
        return self.lm_head(self.final_norm(msa))


@register_model_architecture("evoformer", "evoformer")
def evoformer_base_architecture(args):
    args.evo_layers = getattr(args, "evo_layers", 4)
    args.msa_dim = getattr(args, "msa_dim", 256)
    args.pair_dim = getattr(args, "pair_dim", 128)
    args.evo_heads = getattr(args, "evo_heads", 8)
    args.dropout = getattr(args, "dropout", 0.1)
    args.msa_dropout = getattr(args, "msa_dropout", None) or 0.0
    args.pair_dropout = getattr(args, "pair_dropout", None) or 0.0
    args.max_rel_pos = getattr(args, "max_rel_pos", 32)
    args.recycle_iters = getattr(args, "recycle_iters", None) or 0
    args.activation_checkpoint = getattr(args, "activation_checkpoint", False)
    args.hip_graph_blocks = getattr(args, "hip_graph_blocks", False)
    args.msa_padding_mask = getattr(args, "msa_padding_mask", False)
    args.triangle_attention = getattr(args, "triangle_attention", False)
    args.tri_attn_heads = getattr(args, "tri_attn_heads", None) or 4
