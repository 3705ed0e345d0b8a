"""The seeded in-memory data of tests/golden/epoch_log.json, shared by tests/golden/make_golden_epoch.py (which runs the reference's
LSTMTrainer on it) and the tests (which run rpg_ramnet_amd.trainer.SequenceTrainer on the very same tensors)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from recipe import make_item  # noqa: E402

H, W, L, K, BATCH = 32, 48, 2, 2, 2
N_TRAIN, N_VALID = 6, 4                      # sequences: three training and two validation batches of 2
METRICS = ["mse", "abs_rel_diff", "squ_rel_diff", "rms_linear", "scale_invariant_error", "mean_error", "median_error"]
CONFIG = {"name": "epoch_golden", "metrics": METRICS,
          "loss": {"type": "scale_invariant_loss", "config": {"weight": 1.0, "n_lambda": 1.0}},
          "optimizer_type": "Adam", "optimizer": {"lr": 1e-4},
          "data_loader": {"train": {"every_x_rgb_frame": K, "baseline": False}},
          "trainer": {"epochs": 2, "save_freq": 100, "verbosity": 0, "monitor": "val_loss", "monitor_mode": "min", "num_previews": 2,
                      "num_val_previews": 2, "loss_composition": ["image", "events1"], "loss_weights": [1, 1], "movie": False,
                      "still_previews": False}}


class MemoryDataset(torch.utils.data.Dataset):
    """Sequences of L packages of [C, H, W] tensors; every __getitem__ hands out fresh clones (the reference's preview code
    unsqueezes dataset items in place, lstm_trainer.py:497-500)."""

    def __init__(self, sequences):
        self.sequences = sequences

    def __len__(self):
        return len(self.sequences)

    def __getitem__(self, i):
        return [{k: v.clone() for k, v in item.items()} for item in self.sequences[i]]


def make_sequences(seed, n_seq, nan_frac):
    """Targets between 0.25 and 0.75: a smooth function of the frame (the recipe of test_hip_model._training_trajectory)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_seq):
        seq = []
        for _ in range(L):
            item = {k: v[0] for k, v in make_item(rng, 1, H, W, K, 5, 1).items()}
            tgt = 0.25 + 0.5 * torch.nn.functional.avg_pool2d(item["image"][None], 5, 1, 2)[0]
            for key in ["image"] + ["events%d" % k for k in range(K)]:
                t = tgt.clone()
                if nan_frac:
                    t[torch.from_numpy(rng.random(tuple(t.shape)) < nan_frac)] = float("nan")
                item["depth_" + key] = t
            seq.append(item)
        out.append(seq)
    return out


def loaders():
    train = torch.utils.data.DataLoader(MemoryDataset(make_sequences(41, N_TRAIN, 0.0)), batch_size=BATCH, shuffle=False)
    valid = torch.utils.data.DataLoader(MemoryDataset(make_sequences(42, N_VALID, 0.05)), batch_size=BATCH, shuffle=False)
    return train, valid
