"""CPU: the float64 statement of the fused scale_factor resize (tests/augment_scale_restatement.py) against what the reference executes
(torch's CPU F.interpolate after torch.flip and a slice, and the reference-generated fixture `ramnet_nocrop_scale` of
tests/golden/dataset.npz); the datasets' `defer_scale`; arguments and the C ABI as far as they need no GPU."""
import ctypes as C
import os
import random
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from recipe import FOLDERS, make_dataset_dir  # noqa: E402

import augment_scale_cases as sc  # noqa: E402
import augment_scale_restatement as asr  # noqa: E402
from rpg_ramnet_amd import augment as A  # noqa: E402
from rpg_ramnet_amd import data as D  # noqa: E402

U = 2.0 ** -24
CASE = sc.FIXTURE_CASE


# ------------------------------------------------------------------------------------------------ 1: the statement against torch
@pytest.mark.parametrize("s", sc.ANCHOR_FACTORS)
@pytest.mark.parametrize("th,tw", sc.ANCHOR_SIZES)
def test_restatement_against_torch_interpolate(th, tw, s):
    """flip + slice + F.interpolate in fp32 on the CPU against the float64 statement.  s = 0.5, 0.25: torch's coordinates are exact, three
    fp32 roundings: 4 x 2^-24 x the pixel's largest finite |tap|.  s = 0.7: torch's fp32 1 / s and coordinate carry about 3 ulp of the
    coordinate each way: 2^-24 max|tap| (6 (th + tw + 2) + 4), max|tap| over the window.  NaN masks identical."""
    H, W, top, left = th + 5, tw + 7, 3, 4
    for kind, x in (("normal", sc.normal((2, H, W), th * 1000 + tw)), ("nan", sc.with_nan(sc.normal((2, H, W), th * 1000 + tw + 1), 7))):
        for flips in (0, 1, 2, 3):
            dims = ([2] if flips & 1 else []) + ([1] if flips & 2 else [])
            win = (torch.flip(x, dims) if dims else x)[:, top:top + th, left:left + tw]
            want = F.interpolate(win[None], scale_factor=s, mode="bilinear", align_corners=False, recompute_scale_factor=False)[0]
            ref, _ = asr.exact(x.double(), H, W, th, tw, top, left, flips, s)
            assert tuple(ref.shape) == tuple(want.shape) == (2,) + asr.out_shape(th, tw, s)
            assert torch.equal(torch.isnan(ref), torch.isnan(want)), (kind, flips)
            taps = sc.largest_finite_tap(asr.ar.exact(x.double(), H, W, th, tw, top, left, flips), s)
            bound = 4 * U * taps if s in (0.5, 0.25) else U * float(taps.max()) * (6 * (th + tw + 2) + 4) * torch.ones_like(taps)
            fin = ~torch.isnan(ref)
            err = (want.double() - ref)[fin].abs()
            print("%dx%d s=%g %s flips %d: max err / bound %.3f" % (th, tw, s, kind, flips, float((err / bound[fin].clamp_min(1e-300)).max())))
            assert bool((err <= bound[fin]).all())


# ------------------------------------------------------------------------------------------------ 2, 3: the fixture, defer_scale
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = make_dataset_dir(str(tmp_path_factory.mktemp("eventscape_scale")))
    return root, sorted(os.listdir(root))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "dataset.npz"))


def test_reference_fixture_from_deferred_tensors(tree, gold):
    """the statement at 0.5 of the defer_scale=True tensors == the reference's own resized tensors, within the 0.5 bound of the anchor"""
    ds, seq, _ = sc.fixture_sequence(tree, defer_scale=True)
    assert ds.defer_scale and ds.scale_factor == 0.5
    sc.check_against_fixture(seq, gold, lambda l, key, t: asr.exact(t.double(), 20, 28, 20, 28, 0, 0, 0, 0.5)[0])


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_defer_scale_returns_full_resolution_and_the_same_random_stream(tree, gold):
    _, full, state_full = sc.fixture_sequence(tree, scale_factor=1.0)
    _, defer, state_defer = sc.fixture_sequence(tree, defer_scale=True)
    _, host, state_host = sc.fixture_sequence(tree)
    _, host_off, _ = sc.fixture_sequence(tree, defer_scale=False)
    for a, b in ((state_full, state_defer), (state_full, state_host)):
        assert a[0] == b[0] and all(np.array_equal(u, v) for u, v in zip(a[1], b[1]))
    assert len(full) == len(defer) == len(host) == 2
    name = CASE[0]
    for l, (pf, pd, ph, po) in enumerate(zip(full, defer, host, host_off)):
        assert set(pf) == set(pd) == set(ph)
        for key in pf:
            assert _same(pf[key], pd[key]), key                                       # bit for bit the scale_factor=1.0 dataset's
            want = gold["%s/%d/%s" % (name, l, key)]
            for t in (ph[key], po[key]):                                              # the default is what it was: the reference's tensors
                assert np.array_equal(t.numpy(), want, equal_nan=True), key


def test_concatenate_subfolders_hands_defer_scale_on(tree):
    root, _ = tree
    kw = dict(CASE[5], sequence_length=2)
    cat = D.concatenate_subfolders(root, "SequenceSynchronizedFramesEventsDataset", transform=None, defer_transform=True, defer_scale=True,
                                   **FOLDERS, **{k: v for k, v in kw.items()})
    assert all(d.defer_scale and d.scale_factor == 0.5 for d in cat.datasets) and cat[0][0]["events0"].shape[1:] == (20, 28)
    cat = D.concatenate_subfolders(root, "SequenceSynchronizedFramesEventsDataset", transform=None, defer_transform=True, **FOLDERS, **kw)
    assert not any(d.defer_scale for d in cat.datasets) and cat[0][0]["events0"].shape[1:] == (10, 14)
    seen = A._datasets_of(torch.utils.data.DataLoader(cat, batch_size=1))              # what AugmentedLoader's double-resize check looks at
    assert sorted(map(id, seen)) == sorted(map(id, cat.datasets))


# ------------------------------------------------------------------------------------------------ 4: arguments and ABI
def test_scale_factor_arguments():
    for bad in (0.0, -0.5, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="scale_factor"):
            A.scaled_shape(32, 32, bad)
        with pytest.raises(ValueError, match="scale_factor"):
            A.apply(torch.zeros(1, 1, 8, 8), A.Params((1.0, 0.0, 0.0, 0.0, 1.0, 0.0), 0, 0, 8, 8, True, False, False), scale_factor=bad)
    for th, tw, s in ((1, 32, 0.5), (32, 1, 0.7), (3, 3, 0.3), (224, 224, 0.004)):
        with pytest.raises(ValueError, match="no pixel left"):
            A.scaled_shape(th, tw, s)
    for s in (1.0, 1.5, 2, float("inf")):                                               # the identity path: today's launch
        assert A.scaled_shape(32, 32, s) is None
    assert A.scaled_shape(224, 224, 0.5) == (0.5, 112, 112) and A.scaled_shape(17, 23, 0.5) == (0.5, 8, 11)
    assert A.scaled_shape(32, 32, 0.7) == (0.7, 22, 22) and A.scaled_shape(17, 23, 0.7) == (0.7, 11, 16)
    for row in sc.ROWS:
        assert A.scaled_shape(row[2], row[3], row[4])[1:] == asr.out_shape(row[2], row[3], row[4])


def test_header_binding_and_abi():
    from rpg_ramnet_amd import _hip
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ramnet_hip.h")).read()
    assert re.search(r"int\s+ramnet_augment_scale_batch\(const float \*const \*src, float \*const \*dst, const int \*pidx, const float \*theta, const int \*win,"
                     r"\s*const int \*win_host, const double \*stats, const float \*bx, const float \*by, int G, int n_params, int C,"
                     r"\s*int H, int W, int th, int tw, int oh, int ow, double scale_factor, int Cpad, int nhwc, void \*stream\);", hdr)
    assert re.search(r"#define\s+RAMNET_ABI_VERSION\s+27\b", hdr)
    assert "ramnet_augment_scale_batch" in _hip.EXPORTS and set(re.findall(r"\b(ramnet_[a-z0-9_]+)\s*\(", hdr)) == set(_hip.EXPORTS)
    L = _hip.lib()
    assert L.ramnet_augment_scale_batch is not None and L.ramnet_abi_version() == 27


def test_cabi_bad_arguments_are_refused_on_the_host():
    """Every RAMNET_E_BADARG case of ramnet_augment_scale_batch, before any HIP call (dummy non-null pointers)."""
    from rpg_ramnet_amd import _hip
    L = _hip.lib()
    P = C.c_void_p(4096)
    win = (C.c_int * 4)(0, 0, 1, 0)

    def call(src=P, dst=P, theta=P, winp=P, host=None, bx=P, by=P, G=1, n=1, Cc=5, Hh=20, W=28, th=16, tw=16, oh=8, ow=8, s=0.5, cpad=8, nhwc=0):
        return L.ramnet_augment_scale_batch(src, dst, None, theta, winp, host, None, bx, by, G, n, Cc, Hh, W, th, tw, oh, ow, s, cpad, nhwc, None)

    old = (dict(src=None), dict(dst=None), dict(theta=None), dict(winp=None), dict(bx=None), dict(by=None), dict(th=0, oh=0), dict(tw=-1),
           dict(th=21), dict(tw=29), dict(cpad=4, nhwc=1), dict(cpad=6, nhwc=1), dict(Cc=0), dict(n=0), dict(G=-1), dict(G=65536))
    new = (dict(s=0.0), dict(s=-0.5), dict(s=1.0), dict(s=1.5), dict(s=float("nan")), dict(s=float("inf")), dict(oh=9), dict(oh=7), dict(ow=9),
           dict(ow=7), dict(oh=16, ow=16), dict(th=1, oh=0), dict(tw=1, ow=0), dict(s=0.05, oh=0, ow=0), dict(s=0.7, oh=8, ow=8))
    for kw in old + new:
        assert call(**kw) == 10001 and b"bad argument" in L.ramnet_last_error(), kw
    for top, left in ((5, 0), (0, 13), (-1, 0), (0, -1)):      # window outside the image, from the host copy of the table
        win[0], win[1] = top, left
        assert call(host=win) == 10001 and b"bad argument" in L.ramnet_last_error(), (top, left)
    assert call(G=0, src=None, dst=None) == 0                   # nothing to do is not an error
    assert call(G=0, s=0.7, oh=11, ow=11) == 0
