"""GPU: trainer.SequenceTrainer — the epoch loops of the reference's LSTMTrainer around the HIP model — against the reference's own logs
(tests/golden/epoch_log.json: two epochs of LSTMTrainer._train_epoch with _valid_epoch on the data of tests/epoch_recipe.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import epoch_recipe as E
from util import GOLDEN, build_hip_model, ref_cfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LC = ["image", "events1"]
# The project's prediction bar: element-wise 1e-3 on predictions in [0, 1].  A prediction error e <= EPS moves d = |t - p| by <= e, so
# mean / median / rms of d move by <= EPS; d / t by <= EPS / 0.25 (targets >= 0.25); d^2 / t^2 by <= 2 d EPS / t^2 <= 2 * 16 EPS;
# mean (p - t)^2 by <= 2 EPS; mean d^2 - (mean d)^2 by <= 4 EPS (d <= 1).  An entry is a sum over the 3 prediction keys of a preview.
EPS = 1e-3
METRIC_BOUND = {"mean_error": EPS, "median_error": EPS, "rms_linear": EPS, "abs_rel_diff": 4 * EPS, "squ_rel_diff": 16 * 2 * EPS, "mse": 2 * EPS,
                "scale_invariant_error": 4 * EPS}
KEYS_PER_PREVIEW = 3
LOSS_RTOL = 2e-4                 # the trajectory bound of tests/test_hip_model.py::_training_trajectory


def golden():
    with open(os.path.join(GOLDEN, "epoch_log.json")) as f:
        return json.load(f)


def make(config=None, model=None, valid=True, **kw):
    from rpg_ramnet_amd.trainer import SequenceTrainer
    cfg = json.loads(json.dumps(config or E.CONFIG))
    if model is None:
        mcfg, _ = ref_cfg("net_seeded_ramnet.npz", every_x_rgb_frame=E.K, loss_composition=LC)
        model = build_hip_model("ERGB2DepthRecurrent", mcfg)
    train, val = E.loaders()
    return SequenceTrainer(cfg, model, train, val if valid else None, **kw), cfg, model


def check_log(log, want, tag):
    for k in ("loss", "val_loss"):
        print("%s %s got %.9g reference %.9g rel %.2e" % (tag, k, log[k], want[k], abs(log[k] - want[k]) / want[k]))
        np.testing.assert_allclose(log[k], want[k], rtol=LOSS_RTOL, err_msg="%s %s" % (tag, k))
    for k in ("losses", "val_losses"):
        assert list(log[k]) == list(want[k]) == ["loss", "L_si"]
        for name in want[k]:
            np.testing.assert_allclose(log[k][name], want[k][name], rtol=LOSS_RTOL, err_msg="%s %s %s" % (tag, k, name))
    for k in ("metrics", "val_metrics"):
        assert len(log[k]) == len(E.METRICS)
        for name, got, ref in zip(E.METRICS, log[k], want[k]):
            print("%s %s %s got %.9g reference %.9g diff %.2e bound %.2e" % (tag, k, name, got, ref, abs(got - ref),
                                                                           KEYS_PER_PREVIEW * METRIC_BOUND[name]))
            assert abs(got - ref) <= KEYS_PER_PREVIEW * METRIC_BOUND[name], (tag, k, name, got, ref)


def test_two_epochs_match_the_reference_log():
    """Every loss entry at the trajectory bound, every metric entry at the bound derived from the prediction bar.  Observed on the MI355X
    (profiles/epoch_metrics_notes.md): losses within 2.4e-6 relative, metric entries within 1.3e-6 absolute — more than three orders
    below the bounds."""
    st, cfg, model = make()
    st.optimizer = torch.optim.Adam(model.parameters(), **cfg["optimizer"])
    g = golden()
    assert st.preview_indices == g["preview_indices"] and st.val_preview_indices == g["val_preview_indices"]
    for epoch, want in enumerate(g["logs"], 1):
        log = st.train_epoch(epoch)
        assert set(log) == {"loss", "losses", "metrics", "val_loss", "val_losses", "val_metrics"}
        assert not model.training                      # valid_epoch leaves the model in eval mode
        check_log(log, want, "epoch %d" % epoch)


def test_epoch_trainer_keeps_the_best_model_by_val_loss(tmp_path):
    from rpg_ramnet_amd import checkpoint as ck
    st, cfg, model = make()
    cfg["trainer"]["save_dir"] = str(tmp_path)
    st.config = cfg
    et = st.epoch_trainer()
    assert st.optimizer is et.optimizer
    g = golden()
    best = os.path.join(str(tmp_path), cfg["name"], "model_best.pth.tar")
    written, seen = [], []
    orig = st.train_epoch

    def spy(epoch):                                     # what the best checkpoint looked like when this epoch began
        seen.append(ck.load_checkpoint(best)["epoch"] if os.path.exists(best) else None)
        return orig(epoch)
    et.train_epoch = spy
    logger = et.train()
    val = [e["val_loss"] for e in g["logs"]]
    improves, m = [], float("inf")
    for i, v in enumerate(val, 1):
        if v < m:
            improves.append(i)
            m = v
    c = ck.load_checkpoint(best)
    written = [s for s in seen[1:] + [c["epoch"]]]
    assert sorted(set(written)) == improves and c["epoch"] == improves[-1]
    np.testing.assert_allclose(c["monitor_best"], min(val), rtol=LOSS_RTOL)
    entries = c["logger"].entries
    assert len(entries) == c["epoch"] and len(logger.entries) == 2
    for e in entries.values():
        assert len(e["metrics"]) == 7 and len(e["val_metrics"]) == 7 and set(e["losses"]) == {"loss", "L_si"}
    check_log(logger.entries[2], g["logs"][1], "EpochTrainer epoch 2")


def test_valid_epoch_changes_nothing():
    mcfg, _ = ref_cfg("norm_small_gru_bn.npz", every_x_rgb_frame=E.K, loss_composition=LC)
    assert mcfg["norm"] == "BN"
    model = build_hip_model("ERGB2DepthRecurrent", mcfg).train()
    st, cfg, _ = make(model=model)
    st.optimizer = torch.optim.Adam(model.parameters(), lr=1e-4)
    st.train_epoch(1)                                   # running statistics away from their initial values
    model.zero_grad(set_to_none=True)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert any(k.endswith("running_mean") and float(v.abs().max()) > 0 for k, v in before.items())
    model.train()
    log = st.valid_epoch()
    assert not model.training and np.isfinite(log["val_loss"]) and all(np.isfinite(log["val_metrics"]))
    after = model.state_dict()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    assert all(p.grad is None for p in model.parameters())


def _count_copies(fn):
    copies = []
    orig = {n: getattr(torch.Tensor, n) for n in ("cpu", "item", "tolist", "numpy")}
    try:
        for n, f in orig.items():
            setattr(torch.Tensor, n, (lambda f, n: lambda self, *a, **k: (copies.append((n, self.device.type)), f(self, *a, **k))[1])(f, n))
        out = fn()
    finally:
        for n, f in orig.items():
            setattr(torch.Tensor, n, f)
    return [c for c in copies if c[1] == "cuda"], out


def test_batch_loops_do_not_touch_the_host():
    st, cfg, model = make()
    counts = []
    for n_seq in (4, 8):                                # two and four validation batches
        st.valid_data_loader = torch.utils.data.DataLoader(E.MemoryDataset(E.make_sequences(42, n_seq, 0.05)), batch_size=E.BATCH)
        copies, log = _count_copies(st.valid_epoch)
        assert np.isfinite(log["val_loss"])
        counts.append(len(copies))
    print("device -> host copies of a valid_epoch over 2 / 4 batches:", counts)
    assert counts[0] == counts[1] == 1


def test_step_metrics_is_one_call_per_step_and_equals_per_pair_eval():
    from rpg_ramnet_amd import _hip, metrics as M
    from rpg_ramnet_amd.trainer import sequence_loss
    st, cfg, model = make(step_metrics=True)
    calls = []
    _hip.set_tracer(lambda name, fn, args: (calls.append(name), fn(*args))[1])
    try:
        log = st.valid_epoch()
    finally:
        _hip.set_tracer(None)
    n_steps = len(st.valid_data_loader)
    assert calls.count("ramnet_batch_metrics") == n_steps + 1          # one per step + the one of the previews
    # the same numbers from one eval_metrics per pair
    model.eval()
    rows = []
    with torch.no_grad():
        for sequence in st.valid_data_loader:
            _, _, parts = sequence_loss(model, sequence, LC, [1, 1], parts=True)
            assert len(parts["predictions"]) == (E.K + 1) * E.L
            rows += [M.eval_metrics(p, sequence[l]["depth_" + key], st.metrics) for l, key, p in parts["predictions"]]
    np.testing.assert_allclose(log["val_step_metrics"], np.mean(rows, axis=0), rtol=1e-12)


def test_two_ranks_log_the_same_validation_values():
    """2 ranks (gloo, both on cuda:0), each validating its shard; each child under its own time limit."""
    worker = os.path.join(ROOT, "tests", "dp_epoch_worker.py")
    port = str(29900 + os.getpid() % 300)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, worker], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT) for r in range(2)]
    outs = [p.communicate() for p in procs]
    assert [p.returncode for p in procs] == [0, 0], "\n".join(o[0][-1500:] + o[1][-1500:] for o in outs)
    res = [json.loads([l for l in o[0].splitlines() if l.startswith("{")][-1]) for o in outs]
    assert res[0]["val_loss"] == res[1]["val_loss"] and res[0]["val_metrics"] == res[1]["val_metrics"]
    assert res[0]["val_losses"] == res[1]["val_losses"]
    single = res[0]["single"]
    print("two ranks:", res[0]["val_loss"], "single process:", single["val_loss"])
    np.testing.assert_allclose(res[0]["val_loss"], single["val_loss"], rtol=1e-12)
    np.testing.assert_allclose(res[0]["val_metrics"], single["val_metrics"], rtol=1e-12)
