"""Masked-atom + coordinate-denoising loss for the mol_pairbias model
(BASELINE.json stress config 4).  Demonstrates a composite multi-task
UnicoreLoss: token cross-entropy on masked atoms + L2 on predicted
coordinate deltas (the Uni-Mol pretraining recipe shape)."""

import math

import torch
import torch.nn.functional as F

from unicore_amd import metrics
from unicore_amd.losses import UnicoreLoss, register_loss
from unicore_amd.modules.cross_entropy import fused_nll_loss

# Uni-Mol's normalisation of interatomic distances (Angstrom)
DIST_MEAN = 6.312
DIST_STD = 3.379


@register_loss("mol_pretrain")
class MolPretrainLoss(UnicoreLoss):
    def __init__(self, task):
        super().__init__(task)
        self.padding_idx = task.dictionary.pad()
        self.coord_loss_weight = getattr(task.args, "coord_loss_weight", 1.0)
        self.dist_loss_weight = getattr(task.args, "dist_loss_weight", 0.0)
        # Uni-Mol's norm regularisers: (weight, flag, key in the model's
        # trailing dict, logged name)
        self.norm_terms = [
            (getattr(task.args, "x_norm_loss", 0.0) or 0.0, "--x-norm-loss",
             "x_norm", "x_norm_loss"),
            (getattr(task.args, "delta_pair_repr_norm_loss", 0.0) or 0.0,
             "--delta-pair-repr-norm-loss", "delta_pair_repr_norm",
             "delta_pair_repr_norm_loss"),
        ]

    def dist_loss(self, dist, sample, masked):
        """Uni-Mol's masked distance loss: smooth L1 (sum) between the
        predicted and the normalised clean distances over pairs whose row is
        a masked atom and whose column is a real atom."""
        net = sample["net_input"]
        clean = net["src_coord"].float() + sample["coord_target"].float()
        length = (clean.unsqueeze(1) - clean.unsqueeze(2)).norm(dim=-1)
        target = (length - DIST_MEAN) / DIST_STD
        real = net["src_tokens"].ne(self.padding_idx)
        sel = masked.unsqueeze(2) & real.unsqueeze(1)
        return F.smooth_l1_loss(dist[sel].float(), target[sel], beta=1.0,
                                reduction="sum")

    def forward(self, model, sample, reduce=True):
        net_output = model(**sample["net_input"])
        # the norm regularisers travel as a trailing dict: take it off first
        norms = {}
        if isinstance(net_output[-1], dict):
            norms, net_output = net_output[-1], net_output[:-1]
        logits, coord_delta = net_output[0], net_output[1]
        if self.dist_loss_weight > 0 and len(net_output) < 3:
            raise ValueError(
                f"--dist-loss-weight {self.dist_loss_weight} needs a model "
                "that returns distances (mol_pairbias with --coord-head "
                f"equivariant --dist-head), got {len(net_output)} outputs"
            )
        target = sample["target"]
        masked = target.ne(self.padding_idx)
        sample_size = masked.int().sum()
        masked_atoms = masked
        masked = torch.where(masked.any(), masked, masked.new([True]))
        token_loss = fused_nll_loss(logits[masked], target[masked], ignore_index=self.padding_idx)
        # coordinate denoising: predict the delta back to clean positions
        coord_target = sample["coord_target"].float()
        atom_mask = sample["net_input"]["src_tokens"].ne(self.padding_idx)
        diff = (coord_delta - coord_target) * atom_mask.unsqueeze(-1)
        coord_loss = diff.pow(2).sum() / 3.0
        loss = token_loss + self.coord_loss_weight * coord_loss
        logging_output = {
            "loss": loss.data,
            "token_loss": token_loss.data,
            "coord_loss": coord_loss.data,
            "bsz": target.size(0),
            "sample_size": sample_size,
            "seq_len": target.size(1) * target.size(0),
        }
        if self.dist_loss_weight > 0:
            dist_loss = self.dist_loss(net_output[2], sample, masked_atoms)
            loss = loss + self.dist_loss_weight * dist_loss
            logging_output["loss"] = loss.data
            logging_output["dist_loss"] = dist_loss.data
        for weight, flag, key, name in self.norm_terms:
            if weight <= 0:
                continue
            if key not in norms:
                raise ValueError(
                    f"{flag} {weight} needs a model that returns "
                    f"'{key}' (mol_pairbias with {flag}), got "
                    f"{sorted(norms)}"
                )
            # a batch mean inside a loss the trainer divides by sample_size
            term = norms[key].float() * sample_size
            loss = loss + weight * term
            logging_output["loss"] = loss.data
            logging_output[name] = term.data
        return loss, sample_size, logging_output

    @staticmethod
    def reduce_metrics(logging_outputs, split="valid") -> None:
        loss_sum = sum(log.get("loss", 0) for log in logging_outputs)
        token_sum = sum(log.get("token_loss", 0) for log in logging_outputs)
        coord_sum = sum(log.get("coord_loss", 0) for log in logging_outputs)
        sample_size = sum(log.get("sample_size", 0) for log in logging_outputs)
        # sample_size can be 0 when no tokens were masked in the whole batch
        denom = sample_size if sample_size > 0 else 1
        metrics.log_scalar(
            "loss", loss_sum / denom / math.log(2), sample_size, round=3
        )
        metrics.log_scalar(
            "token_loss", token_sum / denom / math.log(2), sample_size, round=3
        )
        metrics.log_scalar("coord_loss", coord_sum / denom, sample_size, round=3)
        if any("dist_loss" in log for log in logging_outputs):
            dist_sum = sum(log.get("dist_loss", 0) for log in logging_outputs)
            metrics.log_scalar("dist_loss", dist_sum / denom, sample_size,
                               round=3)
        for name in ("x_norm_loss", "delta_pair_repr_norm_loss"):
            if any(name in log for log in logging_outputs):
                norm_sum = sum(log.get(name, 0) for log in logging_outputs)
                metrics.log_scalar(name, norm_sum / denom, sample_size,
                                   round=3)

    @staticmethod
    def logging_outputs_can_be_summed(is_train) -> bool:
        return True
