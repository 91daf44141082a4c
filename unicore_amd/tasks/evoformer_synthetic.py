"""Synthetic masked-MSA pretraining task for the Evoformer stress config
(BASELINE.json config 5): random MSAs (S sequences x L residues), 15%
masking, masked-residue prediction.

``--min-msa-depth`` / ``--min-residues`` below the fixed sizes make the
samples ragged: each draws its own (depth, length) and the collater pads the
batch to its maximum with ``pad`` (for ``--msa-padding-mask`` models)."""

import logging

import numpy as np
import torch

from unicore_amd.data import Dictionary, UnicoreDataset, data_utils
from unicore_amd.tasks import UnicoreTask, register_task

logger = logging.getLogger(__name__)


def make_residue_dictionary(n_types=26):
    d = Dictionary()
    for sym in ("[CLS]", "[PAD]", "[SEP]", "[UNK]"):
        d.add_symbol(sym, is_special=True)
    for i in range(n_types):
        d.add_symbol(f"res{i}")
    return d


class SyntheticMSADataset(UnicoreDataset):
    def __init__(self, size, n_seq, seq_len, dictionary, mask_idx, seed,
                 mask_prob=0.15, min_n_seq=None, min_seq_len=None):
        super().__init__()
        self.size = size
        self.n_seq = n_seq
        self.seq_len = seq_len
        # smaller than the fixed sizes: every sample draws its own shape
        self.min_n_seq = n_seq if min_n_seq is None else min_n_seq
        self.min_seq_len = seq_len if min_seq_len is None else min_seq_len
        assert 1 <= self.min_n_seq <= n_seq, "--min-msa-depth out of range"
        assert 1 <= self.min_seq_len <= seq_len, "--min-residues out of range"
        self.ragged = self.min_n_seq < n_seq or self.min_seq_len < seq_len
        self.dictionary = dictionary
        self.mask_idx = mask_idx
        self.seed = seed
        self.mask_prob = mask_prob
        self.epoch = 1

    def set_epoch(self, epoch, **unused):
        self.epoch = epoch

    def __len__(self):
        return self.size

    def __getitem__(self, index):
        with data_utils.numpy_seed(self.seed, self.epoch, index):
            n_seq, seq_len = self.n_seq, self.seq_len
            if self.ragged:  # extra draws only here: fixed shapes keep theirs
                n_seq = np.random.randint(self.min_n_seq, self.n_seq + 1)
                seq_len = np.random.randint(self.min_seq_len, self.seq_len + 1)
            toks = np.random.randint(5, self.mask_idx, size=(n_seq, seq_len))
            mask = np.random.rand(n_seq, seq_len) < self.mask_prob
        target = np.full_like(toks, self.dictionary.pad())
        target[mask] = toks[mask]
        src = toks.copy()
        src[mask] = self.mask_idx
        return {
            "src_tokens": torch.from_numpy(src.astype(np.int64)),
            "target": torch.from_numpy(target.astype(np.int64)),
        }


class _StackDataset(UnicoreDataset):
    """Fixed-shape samples -> stacked batch tensors."""

    def __init__(self, base, key):
        super().__init__()
        self.base = base
        self.key = key

    def __len__(self):
        return len(self.base)

    def __getitem__(self, index):
        return self.base[index][self.key]

    def collater(self, samples):
        return torch.stack(samples)

    def set_epoch(self, epoch, **unused):
        self.base.set_epoch(epoch)


class _PadStackDataset(_StackDataset):
    """Ragged (S, L) samples -> one batch padded to its maximum shape."""

    def __init__(self, base, key, pad_idx):
        super().__init__(base, key)
        self.pad_idx = pad_idx

    def collater(self, samples):
        S = max(s.shape[0] for s in samples)
        L = max(s.shape[1] for s in samples)
        out = samples[0].new_full((len(samples), S, L), self.pad_idx)
        for i, s in enumerate(samples):
            out[i, : s.shape[0], : s.shape[1]] = s
        return out


@register_task("evoformer_synthetic")
class EvoformerSyntheticTask(UnicoreTask):
    @staticmethod
    def add_args(parser):
        parser.add_argument("--dataset-size", default=64, type=int)
        parser.add_argument("--msa-depth", default=32, type=int)
        parser.add_argument("--residues", default=64, type=int)
        parser.add_argument("--mask-prob", default=0.15, type=float)
        parser.add_argument("--min-msa-depth", default=None, type=int,
                            help="below --msa-depth: each sample draws its "
                                 "depth from [min, --msa-depth] and batches "
                                 "are padded (default: the fixed depth)")
        parser.add_argument("--min-residues", default=None, type=int,
                            help="below --residues: each sample draws its "
                                 "length from [min, --residues] and batches "
                                 "are padded (default: the fixed length)")

    def __init__(self, args, dictionary):
        super().__init__(args)
        self.dictionary = dictionary
        self.seed = args.seed
        self.mask_idx = dictionary.add_symbol("[MASK]", is_special=True)
        dictionary.pad_to_multiple_(64)

    @classmethod
    def setup_task(cls, args, **kwargs):
        d = make_residue_dictionary()
        logger.info("residue dictionary: {} types".format(len(d)))
        return cls(args, d)

    def load_dataset(self, split, combine=False, **kwargs):
        from unicore_amd.data import NestedDictionaryDataset

        base = SyntheticMSADataset(
            size=self.args.dataset_size,
            n_seq=self.args.msa_depth,
            seq_len=self.args.residues,
            dictionary=self.dictionary,
            mask_idx=self.mask_idx,
            seed=self.seed + (0 if split == "train" else 1),
            mask_prob=self.args.mask_prob,
            min_n_seq=getattr(self.args, "min_msa_depth", None),
            min_seq_len=getattr(self.args, "min_residues", None),
        )
        if base.ragged:
            pad = self.dictionary.pad()

            def field(key):
                return _PadStackDataset(base, key, pad)
        else:
            def field(key):
                return _StackDataset(base, key)

        self.datasets[split] = NestedDictionaryDataset(
            {
                "net_input": {"src_tokens": field("src_tokens")},
                "target": field("target"),
            }
        )
