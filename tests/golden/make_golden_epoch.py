#!/usr/bin/env python3
"""tests/golden/epoch_log.json: the `log` dicts of TWO epochs of the REFERENCE's own LSTMTrainer._train_epoch (with _valid_epoch;
RAM_Net/trainer/lstm_trainer.py:392-644) on CPU: seeded ERGB2DepthRecurrent (net_seeded_ramnet's config, every_x_rgb_frame = 2,
loss_composition ["image", "events1"]), SI loss only, B = 2, 32 x 48, L = 2, three training and two validation batches of the
in-memory data of tests/epoch_recipe.py, Adam lr 1e-4, num_previews = num_val_previews = 2, all seven metrics; writer and plotting
stubbed, movie and still previews off.  Imports the reference (build container only).
    python tests/golden/make_golden_epoch.py"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import build, import_reference, load_cfg, model_cfg  # noqa: E402
import epoch_recipe as E  # noqa: E402


class Writer:
    def __getattr__(self, name):
        return lambda *a, **k: None


def main():
    import torch._dynamo  # noqa: F401  (optimizer constructors import it lazily; it must not meet the stub modules)
    mm, sub, loss_mod, metric, etu, lt, ev = import_reference()
    lt.plot_grad_flow = lambda *a, **k: None
    lt.plot_grad_flow_bars = lambda *a, **k: None
    ramnet = load_cfg("train_e2depth_si_grad_loss_statenet_ergb.json")
    tr = E.CONFIG["trainer"]
    cfg = model_cfg(ramnet, every_x_rgb_frame=E.K, loss_composition=tr["loss_composition"])
    m = build(mm, "ERGB2DepthRecurrent", cfg)
    train, valid = E.loaders()
    t = object.__new__(lt.LSTMTrainer)
    t.model, t.loss, t.loss_params = m, loss_mod.scale_invariant_loss, dict(E.CONFIG["loss"]["config"])
    t.metrics, t.calculate_total_metrics = [getattr(metric, k) for k in E.METRICS], []
    t.every_x_rgb_frame, t.loss_composition, t.loss_weights = E.K, tr["loss_composition"], tr["loss_weights"]
    t.gpu, t.baseline, t.state_combination = torch.device("cpu"), cfg["baseline"], cfg["state_combination"]
    t.use_grad_loss, t.use_mse_loss, t.state_preview_flag, t.use_semantic_loss = False, False, False, False
    t.optimizer = torch.optim.Adam(m.parameters(), **E.CONFIG["optimizer"])
    t.data_loader, t.valid_data_loader, t.valid, t.batch_size = train, valid, True, E.BATCH
    t.verbosity, t.log_step, t.writer = 0, 1, Writer()
    t.num_previews, t.num_val_previews = tr["num_previews"], tr["num_val_previews"]
    t.movie, t.still_previews, t.grid_loss, t.record_every_N_sample = False, False, False, 5
    t.preview_indices = lt.select_evenly_spaced_elements(t.num_previews, len(train))
    t.val_preview_indices = lt.select_evenly_spaced_elements(t.num_val_previews, len(valid))
    logs = []
    for epoch in (1, 2):
        log = t._train_epoch(epoch)
        logs.append({k: v for k, v in log.items() if "previews" not in k})
        print(json.dumps(logs[-1]))
    out = {"config": E.CONFIG, "model_fixture": "net_seeded_ramnet.npz", "preview_indices": t.preview_indices,
           "val_preview_indices": t.val_preview_indices, "logs": logs}
    with open(os.path.join(HERE, "epoch_log.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("epoch_log.json")


if __name__ == "__main__":
    main()
