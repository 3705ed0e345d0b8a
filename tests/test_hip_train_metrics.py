"""GPU: ramnet_batch_metrics (csrc/metrics.hip) and its Python surface rpg_ramnet_amd.metrics.batch_metrics / eval_metrics against the
float64 restatement fed the same fp32 inputs (tests/train_metrics_restatement.py), and against the reference's own values
(tests/golden/train_metrics.npz) at the bound of tests/test_train_metrics_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_metrics_restatement as R
from test_train_metrics_cpu import check_against_reference, golden_cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COLS = ("n", "n_target") + R.NAMES
# Kernel and restatement add the SAME fp32 terms in float64, in different orders: at most 7.2e5 terms per pair, 7.2e5 x 1.1e-16 ~ 8e-11 in the
# worst case (this is why contraction is off in metrics.hip); scale_invariant_error is a difference: absolute, against mean d^2.
REL = 1e-10


def run(pairs, names=COLS):
    from rpg_ramnet_amd import metrics as M
    out = M.batch_metrics([torch.from_numpy(p).to(DEV) for p, _ in pairs], [torch.from_numpy(t).to(DEV) for _, t in pairs], names)
    assert out.device.type == "cuda" and out.dtype == torch.float64 and tuple(out.shape) == (len(pairs), len(names))
    return out.cpu().numpy()


def check_row(row, p, t, tag):
    """One row of all columns against the restatement: counts exact, median bit-equal, the means to REL."""
    want = R.restate(p, t)
    got = dict(zip(COLS, row))
    assert got["n"] == want["n"] and got["n_target"] == want["n_target"], (tag, got["n"], want["n"])
    for k in R.NAMES:
        g, w = float(got[k]), float(want[k])
        print("%s %s kernel %.17g restatement %.17g" % (tag, k, g, w))
        if np.isnan(w):
            assert np.isnan(g), (tag, k, g)
        elif k == "median_error":
            assert np.float32(g).tobytes() == np.float32(w).tobytes() and g == float(np.float32(g)), (tag, g, w)
        elif k == "scale_invariant_error":
            assert abs(g - w) <= REL * float(want["mean_d2"]), (tag, k, g, w)
        else:
            assert abs(g - w) <= REL * abs(w), (tag, k, g, w)
    return got


def test_every_fixture_pair_alone_against_restatement_and_reference():
    for tag, p, t, ref in golden_cases():
        got = check_row(run([(p, t)])[0], p, t, tag)
        check_against_reference(got, ref, tag)


def test_all_small_pairs_of_a_shape_in_one_call():
    groups = {}
    for tag, p, t, ref in golden_cases():
        if p.size < 100000:
            groups.setdefault(p.shape, []).append((tag, p, t, ref))
    assert max(len(g) for g in groups.values()) >= 4
    for shape, g in groups.items():
        rows = run([(p, t) for _, p, t, _ in g])
        for row, (tag, p, t, ref) in zip(rows, g):
            check_against_reference(check_row(row, p, t, tag + "/batched"), ref, tag)


def test_g48_fullsize_from_seeds():
    """All (K + 1) L predictions of a B = 8, L = 8 step: 48 pairs of 8 x 1 x 256 x 344, 20 % NaN, in one call."""
    pairs = [R.seeded_pair(500 + g, (8, 1, 256, 344), 0.2) for g in range(48)]
    rows = run(pairs)
    for g in (0, 1, 17, 31, 47):
        check_row(rows[g], *pairs[g], "g48[%d]" % g)
    # every row against a one-pair call: the same bits (the join order of a pair does not depend on G)
    for g in (5, 40):
        assert run([pairs[g]])[0].tobytes() == rows[g].tobytes()


def test_degenerate_pairs_are_defined():
    from rpg_ramnet_amd import metrics as M
    nan = np.float32("nan")
    shape = (2, 1, 5, 7)                                  # N * npix = 70: not a multiple of 4
    p0 = np.full(shape, 0.5, np.float32)
    cases = {"no_valid_pixel": (p0, np.full(shape, nan, np.float32))}
    t = np.full(shape, nan, np.float32)
    t[0] = 0.25
    cases["one_sample_without_target"] = (p0, t.copy())
    t = np.full(shape, nan, np.float32)
    t[1, 0, 4, 6] = 0.75
    cases["n1"] = (p0, t.copy())
    t[0, 0, 0, 0] = 0.125
    cases["n2"] = (p0, t.copy())
    cases["all_d_equal"] = (p0, np.full(shape, 0.75, np.float32))
    cases["d_zero"] = (p0, p0.copy())
    rows = run(list(cases.values()))
    got = {tag: check_row(row, *cases[tag], tag) for tag, row in zip(cases, rows)}
    assert got["no_valid_pixel"]["n"] == 0 and all(np.isnan(got["no_valid_pixel"][k]) for k in R.NAMES)
    g = got["one_sample_without_target"]
    assert np.isnan(g["mse"]) and g["n"] == 35 and g["median_error"] == 0.25 and g["mean_error"] == 0.25
    assert got["n1"]["n"] == 1 and got["n1"]["median_error"] == 0.25
    assert got["n2"]["n"] == 2 and got["n2"]["median_error"] == float(np.float32((np.float32(0.25) + np.float32(0.375)) * np.float32(0.5)))
    assert got["all_d_equal"]["median_error"] == 0.25 and got["all_d_equal"]["scale_invariant_error"] == 0.0
    assert got["d_zero"]["median_error"] == 0.0 and got["d_zero"]["rms_linear"] == 0.0 and got["d_zero"]["n"] == 70
    # a non-finite prediction: the counts differ; eval_metrics raises as numpy's broadcast would, batch_metrics only reports
    p, t = R.case_pair("n3_nan20_even")
    p = p.copy()
    p[np.unravel_index(np.flatnonzero(~np.isnan(t))[3], t.shape)] = nan
    row = run([(p, t)], ("n", "n_target"))[0]
    assert row[1] - row[0] == 1
    with pytest.raises(ValueError):
        M.eval_metrics(torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV))
    p, t = R.case_pair("n3_nan20_even")
    ev = M.eval_metrics(torch.from_numpy(p).to(DEV), torch.from_numpy(t), ["median_error", "mse"])        # target on the host
    want = R.restate(p, t)
    assert isinstance(ev, np.ndarray) and ev.shape == (2,) and ev[0] == want["median_error"] and abs(ev[1] - want["mse"]) <= REL * want["mse"]


def test_bit_reproducible_and_workspace_needs_no_memset_between_calls():
    from rpg_ramnet_amd import metrics as M
    big = [R.seeded_pair(700 + g, (8, 1, 256, 344), 0.2) for g in range(6)]
    small = [R.case_pair(tag) for tag in ("n3_even", "n3_nan20_odd", "n3_nan20_even", "n3_ties_even")]
    tail = [R.case_pair("n3_tail")]
    M._workspaces.clear()
    a = run(big)
    assert run(big).tobytes() == a.tobytes()
    # the same workspace (allocated for the big call) serves smaller G / npix back to back, no memset in between ...
    ws = list(M._workspaces.values())[0]
    b, c, a2 = run(small), run(tail), run(big[:3])
    assert list(M._workspaces.values())[0] is ws
    # ... and each result equals the one of a fresh workspace
    for pairs, got in ((small, b), (tail, c), (big[:3], a2)):
        M._workspaces.clear()
        assert run(pairs).tobytes() == got.tobytes()
    assert a2.tobytes() == a[:3].tobytes()


def test_raw_c_abi_with_device_pointers():
    from rpg_ramnet_amd import _hip
    L = _hip.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pairs = [R.case_pair(tag) for tag in ("n3_even", "n3_ties_even")]
    ps = [torch.from_numpy(p).to(DEV) for p, _ in pairs]
    ts = [torch.from_numpy(t).to(DEV) for _, t in pairs]
    G, N, npix = 2, 3, 120
    nbytes = L.ramnet_batch_metrics_workspace(G, N, npix)
    assert nbytes > 262144
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    ptab = torch.tensor([x.data_ptr() for x in ps], dtype=torch.int64).to(DEV)
    ttab = torch.tensor([x.data_ptr() for x in ts], dtype=torch.int64).to(DEV)
    out = torch.full((G, 10), -1.0, dtype=torch.float64, device=DEV)
    ptr = lambda x: C.c_void_p(x.data_ptr())      # noqa: E731
    assert L.ramnet_batch_metrics(ptr(ptab), ptr(ttab), G, N, npix, ptr(ws), ptr(out), st) == 0, L.ramnet_last_error()
    torch.cuda.synchronize()
    rows = out.cpu().numpy()
    for row, (p, t) in zip(rows, pairs):
        check_row(row[:9], p, t, "raw")
        assert row[9] == 0.0
    assert int(ws[:262144].count_nonzero()) == 0           # the tickets are back at zero
    # rejected before anything is launched: a misaligned workspace, npix = 0
    assert L.ramnet_batch_metrics(ptr(ptab), ptr(ttab), G, N, npix, C.c_void_p(ws.data_ptr() + 4), ptr(out), st) == 10001
    assert b"bad argument" in L.ramnet_last_error()
    assert L.ramnet_batch_metrics(ptr(ptab), ptr(ttab), G, N, 0, ptr(ws), ptr(out), st) == 10001


def test_enqueues_on_the_current_stream_without_synchronising():
    from rpg_ramnet_amd import metrics as M
    pairs = [R.seeded_pair(900 + g, (8, 1, 256, 344), 0.2) for g in range(4)]
    ps = [torch.from_numpy(p).to(DEV) for p, _ in pairs]
    ts = [torch.from_numpy(t).to(DEV) for _, t in pairs]
    want = M.batch_metrics(ps, ts)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    copies = []
    orig = {n: getattr(torch.Tensor, n) for n in ("cpu", "item", "tolist", "numpy")}
    try:
        for n, f in orig.items():
            setattr(torch.Tensor, n, (lambda f, n: lambda self, *a, **k: (copies.append(n), f(self, *a, **k))[1])(f, n))
        with torch.cuda.stream(side):
            got = M.batch_metrics(ps, ts)
    finally:
        for n, f in orig.items():
            setattr(torch.Tensor, n, f)
    assert copies == [] and got.device.type == "cuda"
    side.synchronize()
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert len(M._workspaces) >= 2                         # one workspace per (device, stream)
