"""No GPU: the float64 restatement of the training metrics (tests/train_metrics_restatement.py) against the REFERENCE's own values
(tests/golden/train_metrics.npz, tests/golden/loss_metrics.npz) — the test that keeps the GPU tests of the HIP reduction honest —, the
header / binding of the new entry points, and the host logic of trainer.SequenceTrainer."""
import os
import re

import numpy as np
import pytest
import torch

import train_metrics_restatement as R
from util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The reference sums in float32 (numpy's pairwise mean, sklearn's average); the restatement sums the same float32 terms in float64.
# Largest relative difference |reference - restatement| / |restatement| over the committed pairs (train_metrics.npz + loss_metrics.npz),
# measured by tests/golden/make_golden_train_metrics.py and on loss_metrics.npz (profiles/epoch_metrics_notes.md):
MEASURED_F32_NOISE = {"mse": 8.351e-08, "abs_rel_diff": 2.561e-07, "squ_rel_diff": 1.812e-07, "rms_linear": 6.161e-08,
                      "scale_invariant_error": 8.417e-07, "mean_error": 1.876e-07}
# bound = 4 x the measured value (the summation order inside numpy / sklearn may differ between versions)
REFERENCE_BOUND = {k: 4.0 * v for k, v in MEASURED_F32_NOISE.items()}


def check_against_reference(got, want, tag, worst=None):
    """got: dict of the seven metrics; want: name -> the reference's value.  median_error bit-equal as float32, the means within
    REFERENCE_BOUND (relative)."""
    for k, ref in want.items():
        if k == "median_error":
            assert np.float32(got[k]).tobytes() == np.float32(ref).tobytes(), (tag, k, got[k], ref)
            continue
        rel = abs(float(got[k]) - float(ref)) / abs(float(ref))
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), rel)
        assert rel <= REFERENCE_BOUND[k], "%s %s: %.3e > %.3e (%r vs reference %r)" % (tag, k, rel, REFERENCE_BOUND[k], got[k], ref)


def golden_cases():
    """[(tag, prediction, target, {metric: reference value})] of both fixtures; full-size pairs are regenerated from their seeds."""
    z, out = load_golden("train_metrics.npz"), []
    for tag in list(R.SMALL_CASES) + list(R.FULL_CASES):
        if tag in R.SMALL_CASES:
            p, t = z["%s.pred" % tag], z["%s.target" % tag]
            p2, t2 = R.case_pair(tag)                       # the stored inputs ARE the seeded recipe
            assert p.tobytes() == p2.tobytes() and t.tobytes() == t2.tobytes(), tag
        else:
            p, t = R.case_pair(tag)
        out.append((tag, p, t, {k: float(z["%s.%s" % (tag, k)]) for k in R.NAMES}))
    z = load_golden("loss_metrics.npz")
    for i in range(3):
        out.append(("loss_metrics.si%d" % i, z["si%d.pred" % i], z["si%d.target" % i],
                    {k: float(z["si%d.%s" % (i, k)]) for k in R.NAMES if k != "mse"}))     # (its 'mse' is model/loss.py's, another function)
    return out


def test_restatement_matches_the_reference_metrics():
    worst = {}
    for tag, p, t, want in golden_cases():
        got = R.restate(p, t)
        if tag in R.SMALL_CASES or tag in R.FULL_CASES:
            assert got["n"] == int(load_golden("train_metrics.npz")["%s.n" % tag])
        check_against_reference(got, want, tag, worst)
    print("largest relative difference to the reference per metric:", {k: "%.3e" % v for k, v in worst.items()})


def test_fixture_covers_the_cases_the_selection_must_get_right():
    z = load_golden("train_metrics.npz")
    n = {tag: int(z["%s.n" % tag]) for tag in list(R.SMALL_CASES) + list(R.FULL_CASES)}
    assert n["n1_odd"] % 2 == 1 and n["n3_even"] % 2 == 0 and n["n3_nan20_odd"] % 2 == 1 and n["n3_nan20_even"] % 2 == 0
    p, t = R.case_pair("n3_ties_even")
    d = np.abs(t - p)
    d = np.sort(d[~np.isnan(d)])
    assert len(np.unique(d)) == 16 and d.size % 2 == 0 and d[d.size // 2 - 2] == d[d.size // 2 + 1]      # middle ranks inside a run of ties
    assert (3 * 7 * 11) % 4 != 0 and n["full_8x256x344"] == 8 * 256 * 344
    # np.median itself agrees with the bit-pattern rule on an even count whose middle elements differ
    p, t = R.case_pair("n3_even")
    assert np.float32(np.median(np.abs(t - p))) == np.float32(R.restate(p, t)["median_error"])


def test_restatement_degenerate_pairs():
    p = np.full((2, 1, 3, 4), 0.5, np.float32)
    t = np.full((2, 1, 3, 4), np.nan, np.float32)
    r = R.restate(p, t)
    assert r["n"] == 0 and all(np.isnan(r[k]) for k in R.NAMES)
    t[0] = 0.25
    r = R.restate(p, t)
    assert r["n"] == 12 and np.isnan(r["mse"]) and r["median_error"] == 0.25 and r["mean_error"] == 0.25


def test_header_declares_the_entry_points_and_the_abi_version_stays():
    from rpg_ramnet_amd import _hip
    src = open(os.path.join(ROOT, "include", "ramnet_hip.h")).read()
    assert re.search(r"size_t\s+ramnet_batch_metrics_workspace\(int G, int N, size_t npix\);", src)
    assert re.search(r"int\s+ramnet_batch_metrics\(const float \*const \*pred, const float \*const \*target, int G, int N, size_t npix,"
                     r"\s*void \*workspace,\s*double \*out, void \*stream\);", src)
    assert re.search(r"#define\s+RAMNET_ABI_VERSION\s+27\b", src)
    m = re.search(r"#define\s+RAMNET_BATCH_METRICS_TICKET_BYTES\s+(\d+)", src)
    from rpg_ramnet_amd import metrics as M
    assert m and int(m.group(1)) == M.TICKET_BYTES
    assert "ramnet_batch_metrics" in _hip.EXPORTS and "ramnet_batch_metrics_workspace" in _hip.EXPORTS
    assert os.path.exists(os.path.join(ROOT, "rpg_ramnet_amd", "csrc", "metrics.hip"))
    from rpg_ramnet_amd import build
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["metrics.hip"]


def test_batch_metrics_rejects_bad_arguments_before_any_hip_call():
    from rpg_ramnet_amd import _hip
    L = _hip.lib()
    assert L.ramnet_batch_metrics(None, None, 1, 1, 16, None, None, None) == 10001 and b"bad argument" in L.ramnet_last_error()
    assert L.ramnet_batch_metrics(4096, 4096, 1, 0, 16, 4096, 4096, None) == 10001            # N = 0
    assert L.ramnet_batch_metrics(4096, 4096, 1, 4, 1 << 30, 4096, 4096, None) == 10001       # N * npix >= 2^31
    assert L.ramnet_batch_metrics(4096, 4096, 1, 1, 16, 4100, 4096, None) == 10001            # workspace not 256-byte aligned
    assert L.ramnet_batch_metrics(None, None, 0, 1, 16, None, None, None) == 0                # G = 0: nothing to do
    assert L.ramnet_batch_metrics_workspace(0, 1, 16) == 0 and L.ramnet_batch_metrics_workspace(1, 4, 1 << 30) == 0
    small, big = L.ramnet_batch_metrics_workspace(1, 1, 16), L.ramnet_batch_metrics_workspace(48, 8, 256 * 344)
    assert 262144 < small < big < (64 << 20)


def test_metric_names_resolve_like_the_config():
    from rpg_ramnet_amd import metrics as M
    assert M.TRAIN_METRICS == R.NAMES
    assert M.resolve_metrics(["mse", "median_error"]) == ("mse", "median_error")
    with pytest.raises(NotImplementedError):
        M.resolve_metrics(["mse", "structural_similarity"])
    with pytest.raises(KeyError):
        M.resolve_metrics(["rmse"])
    with pytest.raises(KeyError):
        M.batch_metrics([torch.zeros(1, 1, 2, 2)], [torch.zeros(1, 1, 2, 2)], names=["nope"])
    with pytest.raises(ValueError):                      # no CPU fallback
        M.batch_metrics([torch.zeros(1, 1, 2, 2)], [torch.zeros(1, 1, 2, 2)])
    with pytest.raises(ValueError):
        M.batch_metrics([torch.zeros(1, 1, 2, 2)], [])


def test_preview_indices_are_the_reference_rule():
    from rpg_ramnet_amd.trainer import select_evenly_spaced_elements as sel
    import json
    assert sel(2, 3) == [0, 1] and sel(2, 2) == [0, 1] and sel(2, 4) == [1, 3] and sel(3, 10) == [1, 4, 7] and sel(2, 1) == [0, 0]
    with open(os.path.join(ROOT, "tests", "golden", "epoch_log.json")) as f:
        g = json.load(f)
    assert sel(2, 3) == g["preview_indices"] and sel(2, 2) == g["val_preview_indices"]


def test_losses_dict_carries_the_aliasing_factor_in_every_entry():
    from rpg_ramnet_amd.trainer import loss_parts
    si, gl, ml = torch.tensor(0.5, requires_grad=True), torch.tensor(0.25), torch.tensor(0.125)
    total = si + gl + ml
    d = loss_parts(2, total, si, gl, ml)
    assert list(d) == ["loss", "L_si", "L_grad", "L_mse"]
    assert [float(v) for v in d.values()] == [1.75, 1.0, 0.5, 0.25] and not any(v.requires_grad for v in d.values())
    d = loss_parts(3, si, si)
    assert list(d) == ["loss", "L_si"] and float(d["loss"]) == 1.5


def test_sequence_trainer_reads_the_config():
    import epoch_recipe as E
    import json
    from rpg_ramnet_amd.trainer import SequenceTrainer
    cfg = json.loads(json.dumps(E.CONFIG))
    model = torch.nn.Conv2d(1, 1, 1)
    model.gpu, model.every_x_rgb_frame = torch.device("cpu"), 2
    train, valid = E.loaders()
    st = SequenceTrainer(cfg, model, train, valid)
    assert st.preview_indices == [0, 1] and st.val_preview_indices == [0, 1] and st.loss_names == ["loss", "L_si"]
    assert st.metrics == tuple(E.METRICS) and st.grad_loss_weight is None and st.mse_loss is None
    with pytest.raises(RuntimeError):
        st.train_epoch(1)                                 # no optimizer yet
    cfg["grad_loss"], cfg["mse_loss"] = {"weight": 0.25}, {}
    st = SequenceTrainer(cfg, model, train)
    assert st.loss_names == ["loss", "L_si", "L_grad", "L_mse"] and st.grad_loss_weight == 0.25
    assert st.mse_loss == {"weight": 1.0, "downsampling_factor": 0.5}
    cfg["metrics"] = ["mse", "structural_similarity"]
    with pytest.raises(NotImplementedError):
        SequenceTrainer(cfg, model, train)
