"""GPU: the event voxeliser of csrc/loss_voxel.hip (`ramnet_voxelize`, `ramnet_voxelize_batch`, `ramnet_voxelize_batch_sorted`,
`ramnet_voxel_indices`), every form of it called alone through the C ABI with raw pointers, cell by cell against the float64 statement
of tests/voxel_restatement.py on the rows of tests/voxel_cases.py (both anchored on the CPU by tests/test_voxel_restatement_cpu.py).

Every launch goes through `call` (tests/guarded.py): events in a float64 buffer between NaN guards, offsets in an int64 buffer between
sentinel guards, grids prefilled with the sentinel between sentinel guards.  Rules (profiles/voxel_launch_tests_notes.md §1):
  exact      dyadic rows: every vote and partial sum is exact in fp32 in any order, so every form gives the bits of the statement; cells
             without a vote and the cancelled hot cell are +0; no cell keeps its sentinel;
  derived    normal rows, cell by cell, no cell left out: k = 0 cells are +0; k = 1 cells are the vote itself, bit for bit (sorted form:
             where the vote is a multiple of 2^-40, which every vote of magnitude >= 2^-16 is); the fp32-atomic forms within
             gamma(k - 1) x sum |vote|; the sorted form within 2^-24 |exact| + k 2^-41;
  bit        the sorted form twice in a row, through both entry points, and against the restated fixed-point sum, on every row.
Each test asserts the form that served the launch (`ramnet_last_kernel`) against the geometry the CPU file states.  No bound is taken from
the kernels under test."""
import contextlib

import numpy as np
import pytest
import torch

from rpg_ramnet_amd import _hip
import voxel_cases as vc
import voxel_restatement as vr
from guarded import BADARG, F64, SENT, SENT_INT, In, Out, call, settle

pytestmark = pytest.mark.gpu

UNSUPPORTED = 10002
I64 = torch.int64
_INPUTS = {}


def last_kernel():
    return _hip.lib().ramnet_last_kernel().decode()


@contextlib.contextmanager
def option(name, value):
    L = _hip.lib()
    old = L.ramnet_get_option(name)
    assert L.ramnet_set_option(name, value) == 0
    try:
        yield
    finally:
        assert L.ramnet_set_option(name, old) == 0


def events_in(ev):
    return In(torch.tensor(np.ascontiguousarray(ev)), dtype=F64) if len(ev) else None


def inputs(name):
    """(events, offsets) of a row on the device, uploaded once and only read"""
    if name not in _INPUTS:
        lists = vc.data(name)
        off = np.cumsum([0] + [len(e) for e in lists])
        _INPUTS[name] = (events_in(np.concatenate(lists)), In(torch.tensor(off), fill=SENT_INT, dtype=I64))
    return _INPUTS[name]


def batch_args(name, entry):
    r = vc.ROWS[name]
    ev, off = inputs(name)
    grids = Out(len(r["lens"]), r["bins"] * r["H"] * r["W"])
    return [entry, ev, off, len(r["lens"]), vc.max_events(name), r["bins"], r["W"], r["H"], grids]


def launch(args, capture=False):
    """-> (grids as numpy [rows, cells], ramnet_last_kernel)"""
    if capture:                                       # recorded once on one stream (a linear graph), replayed once
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call(*args, stream=torch.cuda.current_stream().cuda_stream, defer=True)
            name = last_kernel()
        g.replay()
        settle(*args)
    else:
        call(*args)
        name = last_kernel()
    out = [a for a in args if isinstance(a, Out)][0]
    return out.value().numpy(), name


def run(name, entry="ramnet_voxelize_batch", capture=False):
    r = vc.ROWS[name]
    got, kernel = launch(batch_args(name, entry), capture)
    return got.reshape(len(r["lens"]), r["bins"], r["H"], r["W"]), kernel


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(got, ref, what):
    bad = bits(got) != bits(ref)
    if bad.any():
        at = tuple(int(i[0]) for i in np.nonzero(bad))
        raise AssertionError("%s: %d of %d cells differ, first at %s: %r != %r" % (what, int(bad.sum()), bad.size, at, float(got[at]), float(ref[at])))


def check(got, st, kind, form, what):
    """the rule of the row's data kind; st: the statement restricted to what `got` covers"""
    kept = got == np.float32(SENT)
    assert not kept.any(), "%s: %d of %d cells keep their sentinel, first at %s" % (what, int(kept.sum()), kept.size, tuple(int(i[0]) for i in np.nonzero(kept)))
    exact, k = st["exact"], st["k"]
    if form == "sorted":
        same_bits(got, st["fixed"], what + ", against the fixed-point sum")
    if kind == "dyadic":
        same_bits(got, exact.astype(np.float32), what)
        return
    assert not bits(got[k == 0]).any(), "%s: a cell without a vote is not +0" % what
    one = (k == 1) & (st["dyadic40"] if form == "sorted" else True)
    same_bits(got[one], exact[one].astype(np.float32), what + ", cells with one vote")
    bound = vr.bound_sorted(st) if form == "sorted" else vr.bound_atomic(st)
    err = np.abs(got.astype(np.float64) - exact)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print("%s (%s): max |err| %.3e, max err / bound %.3f, max k %d" % (what, form, float(err.max()), ratio, int(k.max())))
    assert np.all(err <= bound) and np.isfinite(got).all(), "%s: error %.3f x its bound" % (what, ratio)


def check_row(name, got, form, what):
    check(got, vc.statement(name), vc.ROWS[name]["kind"], form, "%s %s" % (what, name))


def expected_kernel(name, form):
    return vr.kernel_name(form, vc.ROWS[name]["geo"][form][0] if form in vc.ROWS[name]["geo"] else 0)


# ---------------------------------------------------------------------------------------- the sorted form
@pytest.mark.parametrize("name", [n for n, r in vc.ROWS.items() if r["batch"] == "sorted"])
def test_sorted_form(name):
    """ramnet_voxelize_batch by default from 2 lists; then again (the same bits), then through ramnet_voxelize_batch_sorted (the same bits)"""
    got, kernel = run(name)
    assert kernel == expected_kernel(name, "sorted")
    check_row(name, got, "sorted", "sorted form")
    again, _ = run(name)
    same_bits(again, got, "sorted form %s, second launch" % name)
    other, kernel = run(name, "ramnet_voxelize_batch_sorted")
    assert kernel == expected_kernel(name, "sorted")
    same_bits(other, got, "sorted form %s, through ramnet_voxelize_batch_sorted" % name)


@pytest.mark.parametrize("name", ["s1", "m1", "empty2", "empty16"])
def test_sorted_entry_point_alone(name):
    """one list (which ramnet_voxelize_batch leaves to the atomic form), and no events at all (a zero-fill)"""
    got, kernel = run(name, "ramnet_voxelize_batch_sorted")
    form = "sorted" if vc.max_events(name) else "zero_fill"
    assert kernel == expected_kernel(name, form)
    check_row(name, got, form, "sorted entry point")


@pytest.mark.parametrize("name", list(vc.REFUSED))
def test_sorted_entry_point_refuses(name):
    """255 bands, no row that fits, H past the record's 15 bits: RAMNET_E_UNSUPPORTED, nothing launched"""
    args = batch_args(name, "ramnet_voxelize_batch_sorted")
    refused(args, [args[-1]], rc=UNSUPPORTED, message=b"sorted form cannot take this launch")


# ---------------------------------------------------------------------------------------- the row-band forms
@pytest.mark.parametrize("name", [n for n, r in vc.ROWS.items() if r["unsorted"] == "ids"])
def test_band_form_with_ids(name):
    with option(b"voxel_sorted", 0):
        got, kernel = run(name)
    assert kernel == expected_kernel(name, "ids")
    check_row(name, got, "ids", "row bands with ids")


@pytest.mark.parametrize("name", [n for n, r in vc.ROWS.items() if r["capture"] == "idless"])
def test_band_form_idless_captured(name):
    """Inside a stream capture the library hands out no scratch: from 16 lists the bands walk the lists themselves.  (The all-empty launch
    reaches the same kernel outside a capture, and runs first: the kernel's LDS opt-in is then made before anything is recorded.)"""
    got, kernel = run("empty16")
    assert kernel == expected_kernel("empty16", "idless")
    check_row("empty16", got, "idless", "id-less row bands")
    got, kernel = run(name, capture=True)
    assert kernel == expected_kernel(name, "idless")
    check_row(name, got, "idless", "id-less row bands, captured,")


# ---------------------------------------------------------------------------------------- the global-atomic forms
@pytest.mark.parametrize("name", [n for n, r in vc.ROWS.items() if "atomic_batch" in (r["batch"], r["unsorted"])])
def test_atomic_batch_form(name):
    """what nothing else takes: one list, 255 bands, H = 32768 (by default), fewer than 16 lists with voxel_sorted = 0"""
    with option(b"voxel_sorted", 1 if vc.ROWS[name]["batch"] == "atomic_batch" else 0):
        got, kernel = run(name)
    assert kernel == "voxelize_batch_kernel"
    check_row(name, got, "atomic_batch", "atomic batch")


@pytest.mark.parametrize("name", ["a9", "s3", "m3", "empty2"])
def test_atomic_batch_form_captured(name):
    got, kernel = run(name, capture=True)
    assert kernel == expected_kernel(name, vc.ROWS[name]["capture"])
    check_row(name, got, "atomic_batch", "atomic batch, captured,")


@pytest.mark.parametrize("name", ["s1", "s3", "s2n", "m1", "m3", "a3", "a9", "t32767", "t32768"])
def test_single_list(name):
    """ramnet_voxelize on every list of the row, the empty ones included (events = NULL, a zero-fill)"""
    r, st = vc.ROWS[name], vc.statement(name)
    for g, ev in enumerate(vc.data(name)):
        grid = Out(1, r["bins"] * r["H"] * r["W"])
        call("ramnet_voxelize", events_in(ev), len(ev), r["bins"], r["W"], r["H"], grid)
        assert last_kernel() == ("voxelize_kernel" if len(ev) else "zero_fill")
        check(grid.value().numpy().reshape(r["bins"], r["H"], r["W"]), {k: a[g] for k, a in st.items()}, r["kind"], "atomic", "one list, %s[%d]" % (name, g))


@pytest.mark.parametrize("name", [n for n, r in vc.ROWS.items() if max(r["lens"])])
def test_voxel_indices(name):
    """the flat indices of both votes of every event, -1 where the vote is dropped: the events outside the image, NaN, +-inf, 1e300 included"""
    r = vc.ROWS[name]
    for g, ev in enumerate(vc.data(name)):
        if len(ev):
            il, ir = Out(1, len(ev), dtype=I64), Out(1, len(ev), dtype=I64)
            call("ramnet_voxel_indices", events_in(ev), len(ev), r["bins"], r["W"], r["H"], il, ir)
            for got, ref, side in zip((il, ir), vr.indices(ev, r["bins"], r["W"], r["H"]), ("left", "right")):
                bad = got.value().numpy().reshape(-1) != ref
                assert not bad.any(), "%s[%d] %s: %d of %d indices differ, first at event %d %r: %d != %d" % (
                    name, g, side, int(bad.sum()), bad.size, int(np.nonzero(bad)[0][0]), ev[np.nonzero(bad)[0][0]].tolist(),
                    int(got.value().numpy().reshape(-1)[bad][0]), int(ref[bad][0]))


# ---------------------------------------------------------------------------------------- arguments
def refused(args, outs, rc=BADARG, message=b"bad argument"):
    """the return code, the message, and every output as it was (guards, gaps and body)"""
    call(*args, rc=rc, defer=True)
    torch.cuda.synchronize()
    assert message in _hip.lib().ramnet_last_error(), _hip.lib().ramnet_last_error()
    for o in outs:
        o._host = None
        o.check(args[0], untouched=True)


def test_argument_checks():
    """RAMNET_E_BADARG, the message, nothing launched: the outputs keep their sentinel"""
    for entry in ("ramnet_voxelize_batch", "ramnet_voxelize_batch_sorted"):
        for name in ("s1", "s2", "a16"):
            for pos, bad in ((3, 0), (3, 65536), (5, 0), (6, 0), (7, 0), (8, None), (2, None), (1, None)):
                args = batch_args(name, entry)
                grids = args[8]
                args[pos] = bad
                refused(args, [grids])
    r, ev = vc.ROWS["s1"], vc.data("s1")[0]
    for pos, bad in ((3, 0), (4, 0), (5, 0), (6, None), (1, None)):
        grid = Out(1, r["bins"] * r["H"] * r["W"])
        args = ["ramnet_voxelize", events_in(ev), len(ev), r["bins"], r["W"], r["H"], grid]
        args[pos] = bad
        refused(args, [grid])
    for pos, bad in ((1, None), (2, 0), (3, 0), (4, 0), (5, 0), (6, None), (7, None)):
        il, ir = Out(1, len(ev), dtype=I64), Out(1, len(ev), dtype=I64)
        args = ["ramnet_voxel_indices", events_in(ev), len(ev), r["bins"], r["W"], r["H"], il, ir]
        args[pos] = bad
        refused(args, [il, ir])


# ---------------------------------------------------------------------------------------- the Python wrappers
@pytest.mark.parametrize("name", ["a16", "s3"])
def test_wrappers(name):
    from rpg_ramnet_amd import ops, voxel
    r, st = vc.ROWS[name], vc.statement(name)
    dev = torch.device("cuda:0")
    lists = [torch.tensor(np.ascontiguousarray(e)).to(dev) for e in vc.data(name)]
    ref = st["exact"].astype(np.float32)
    same_bits(voxel.events_to_voxel_grids(lists, r["bins"], r["W"], r["H"]).cpu().numpy(), ref, "events_to_voxel_grids %s" % name)
    cat, off, mx = voxel.pack_event_lists(lists, dev)
    assert mx == max(r["lens"]) and off.cpu().tolist() == np.cumsum((0,) + r["lens"]).tolist()
    out = torch.full((len(lists), r["bins"], r["H"], r["W"]), SENT, device=dev)
    assert voxel.events_to_voxel_grids_packed(cat, off, mx, r["bins"], r["W"], r["H"], out=out) is out
    same_bits(out.cpu().numpy(), ref, "events_to_voxel_grids_packed %s" % name)
    with ops.switches(deterministic=True):
        for g, ev in enumerate(lists):              # one list through the sorted form
            got = voxel.events_to_voxel_grid(ev, r["bins"], r["W"], r["H"])
            assert last_kernel() == (expected_kernel(name, "sorted") if len(ev) else "zero_fill")
            same_bits(got.cpu().numpy(), ref[g], "deterministic events_to_voxel_grid %s[%d]" % (name, g))
