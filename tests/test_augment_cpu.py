"""CPU (no GPU): the host half of the device augmentation — augment.draw against the host transform classes (same draws, same flips,
same window, same random state afterwards), the datasets' defer_transform mode, and what draw refuses."""
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from recipe import FOLDERS, make_dataset_dir  # noqa: E402

from rpg_ramnet_amd import augment as A  # noqa: E402
from rpg_ramnet_amd import data as D  # noqa: E402

SEEDS = [int(s) for s in np.random.default_rng(7).integers(0, 2 ** 32, 200)]


def _recipe(size):
    return D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop(size)])


CASES = [
    ("recipe_260x346_224", lambda: _recipe(224), 260, 346),
    ("crop_256x344", lambda: D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop([256, 344])]), 260, 346),
    ("center_crop", lambda: D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.CenterCrop(224)]), 260, 346),
    ("flip_alone", lambda: D.RandomRotationFlip(0.0, 0.5, 0.5), 260, 346),
    ("mosaic_even", lambda: D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop(224, preserve_mosaicing_pattern=True)]), 260, 346),
    ("size_fits", lambda: D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop([260, 346])]), 260, 346),
    ("480x640", lambda: _recipe(224), 480, 640),
    ("40x56", lambda: _recipe(32), 40, 56),
]


def predicted_index(p, H, W):
    """Source index y W + x of every output pixel, from draw's flip flags and window."""
    ys = torch.arange(p.top, p.top + p.th)
    xs = torch.arange(p.left, p.left + p.tw)
    sy = (H - 1 - ys) if p.vflip else ys
    sx = (W - 1 - xs) if p.hflip else xs
    return (sy[:, None] * W + sx[None, :]).to(torch.int64)


@pytest.mark.parametrize("name,make,H,W", CASES, ids=[c[0] for c in CASES])
def test_draw_matches_host_transform_angle0(name, make, H, W):
    """Index image through the HOST transform under random.seed(seed): round() of its output is the source index draw predicts, for every
    pixel, and the random state after draw equals the state after the host call."""
    transform = make()
    index = torch.arange(H * W, dtype=torch.float32).reshape(1, H, W)
    assert int(index.max()) < 2 ** 24
    seen = set()
    for seed in SEEDS:
        random.seed(seed)
        host = transform(index)
        state_host = random.getstate()
        random.seed(12345)                                    # draw must seed by itself
        p = A.draw(transform, seed, H, W)
        assert random.getstate() == state_host, (name, seed)
        assert p.exact and tuple(host.shape) == (1, p.th, p.tw), (name, seed, p)
        assert torch.equal(torch.round(host[0]).to(torch.int64), predicted_index(p, H, W)), (name, seed, p)
        seen.add((p.hflip, p.vflip))
    assert len(seen) == 4                                     # all four flip combinations occur among the seeds


@pytest.mark.parametrize("degrees", [30, (-10, 25)])
def test_draw_rotation_theta_and_state(degrees):
    """Non-zero degrees: same random state, and theta = the first two rows of the matrix the host class builds from the same draws."""
    from math import cos, pi, sin
    rot = D.RandomRotationFlip(degrees, 0.5, 0.5)
    transform = D.Compose([rot, D.RandomCrop(224)])
    x = torch.zeros(1, 260, 346)
    for seed in SEEDS[:50]:
        random.seed(seed)
        transform(x)
        state_host = random.getstate()
        p = A.draw(transform, seed, 260, 346)
        assert random.getstate() == state_host
        random.seed(seed)                                     # the host class's own arithmetic, replayed on the same draws
        a = random.uniform(rot.degrees[0], rot.degrees[1]) * pi / 180.0
        M = torch.FloatTensor([[cos(a), -sin(a), 0], [sin(a), cos(a), 0], [0, 0, 1]])
        h, v = random.random() < 0.5, random.random() < 0.5
        if h:
            M[:, 0] *= -1
        if v:
            M[:, 1] *= -1
        assert torch.equal(torch.tensor(p.theta, dtype=torch.float32), M[:2].reshape(-1)) and (p.hflip, p.vflip) == (h, v)
        assert not p.exact and (p.th, p.tw) == (224, 224) and 0 <= p.top <= 36 and 0 <= p.left <= 122


def test_draw_none_and_bare_crops():
    state = random.getstate()
    p = A.draw(None, 5, 20, 28)
    assert random.getstate() == state and p.exact and (p.top, p.left, p.th, p.tw, p.hflip, p.vflip) == (0, 0, 20, 28, False, False)
    x = torch.arange(20 * 28, dtype=torch.float32).reshape(1, 20, 28)
    for t in (D.RandomCrop(16), D.CenterCrop(15), D.CenterCrop([16, 13], preserve_mosaicing_pattern=True)):
        for seed in SEEDS[:20]:
            random.seed(seed)
            host = t(x)
            state = random.getstate()
            p = A.draw(t, seed, 20, 28)
            assert random.getstate() == state
            assert torch.equal(host[0].to(torch.int64), predicted_index(p, 20, 28))


def test_draw_refuses_what_the_device_path_does_not_cover():
    rot, crop = D.RandomRotationFlip(0.0), D.RandomCrop(16)

    class Other:
        def __call__(self, x, is_flow=False):
            return x

    for bad, word in ((D.Compose([crop, rot]), "RandomRotationFlip"), (D.Compose([rot, rot]), "RandomRotationFlip"),
                      (D.Compose([rot, crop, D.CenterCrop(8)]), "CenterCrop"), (D.Compose([Other()]), "Other"), (Other(), "Other")):
        with pytest.raises(ValueError, match=word):
            A.draw(bad, 1, 20, 28)
    with pytest.raises(ValueError, match="is_flow"):
        A.draw(rot, 1, 20, 28, is_flow=True)
    with pytest.raises(ValueError, match="does not fit"):
        A.draw(D.RandomCrop(32), 1, 20, 28)
    raised = 0                                                 # 5 rows of slack: the draw 5 becomes the even offset 6, rows 6..22 of 21
    for seed in SEEDS[:60]:                                    # (host slicing would silently return a smaller tensor)
        random.seed(seed)
        top = random.randint(0, 5)
        try:
            p = A.draw(D.RandomCrop([16, 28], preserve_mosaicing_pattern=True), seed, 21, 28)
            assert top < 5 and p.top == top + top % 2
        except ValueError as e:
            assert top == 5 and "leave" in str(e)
            raised += 1
    assert raised > 0
    with pytest.raises(ValueError, match="leaves"):
        A.ParamTable([A.Params((1.0, 0.0, 0.0, 0.0, 1.0, 0.0), 10, 0, 16, 16, True, False, False)], 20, 28)
    with pytest.raises(ValueError, match="one size"):
        A.ParamTable([A.draw(D.CenterCrop(16), 1, 20, 28), A.draw(D.CenterCrop(8), 1, 20, 28)], 20, 28)


def test_header_and_ctypes_table_hold_the_new_entry_points():
    import re
    from rpg_ramnet_amd import _hip
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ramnet_hip.h")).read()
    declared = set(re.findall(r"\b(ramnet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_hip.EXPORTS) and {"ramnet_augment_batch", "ramnet_nonzero_stats_batch"} <= declared
    assert int(re.search(r"#define RAMNET_ABI_VERSION (\d+)", hdr).group(1)) == 27


def test_cabi_bad_arguments_are_refused_on_the_host():
    """Every RAMNET_E_BADARG case of ramnet_augment_batch, before any HIP call (dummy non-null pointers)."""
    import ctypes as C
    from rpg_ramnet_amd import _hip
    L = _hip.lib()
    P = C.c_void_p(4096)
    win = (C.c_int * 4)(0, 0, 1, 0)

    def call(src=P, dst=P, theta=P, winp=P, host=None, bx=P, by=P, G=1, n=1, Cc=5, Hh=20, W=28, th=16, tw=16, cpad=8, nhwc=0):
        return L.ramnet_augment_batch(src, dst, None, theta, winp, host, None, bx, by, G, n, Cc, Hh, W, th, tw, cpad, nhwc, None)

    for kw in (dict(src=None), dict(dst=None), dict(theta=None), dict(winp=None), dict(bx=None), dict(by=None), dict(th=0), dict(tw=-1),
               dict(th=21), dict(tw=29), dict(cpad=4, nhwc=1), dict(cpad=6, nhwc=1), dict(Cc=0), dict(n=0), dict(G=-1)):
        assert call(**kw) == 10001 and b"bad argument" in L.ramnet_last_error(), kw
    for top, left in ((5, 0), (0, 13), (-1, 0), (0, -1)):      # window outside the image, from the host copy of the table
        win[0], win[1] = top, left
        assert call(host=win) == 10001 and b"bad argument" in L.ramnet_last_error(), (top, left)
    assert call(G=0, src=None, dst=None) == 0                   # nothing to do is not an error
    assert L.ramnet_nonzero_stats_batch(None, 1, 16, P, None) == 10001
    assert L.ramnet_nonzero_stats_batch(P, 1, 18, P, None) == 10001


# ------------------------------------------------------------------------------------------------ defer_transform
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = make_dataset_dir(str(tmp_path_factory.mktemp("eventscape_aug")))
    return root, sorted(os.listdir(root))


KW = dict(sequence_length=3, step_size=2, every_x_rgb_frame=2, clip_distance=1000.0, reg_factor=5.70378)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))        # bitwise, NaN included


def test_defer_transform_returns_raw_tensors_seeds_and_the_same_random_stream(tree):
    root, names = tree
    base = os.path.join(root, names[1])
    transform = D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop(16)])
    normal = D.SequenceSynchronizedFramesEventsDataset(base, transform=transform, **FOLDERS, **KW)
    plain = D.SequenceSynchronizedFramesEventsDataset(base, transform=None, **FOLDERS, **KW)
    defer = D.SequenceSynchronizedFramesEventsDataset(base, transform=transform, defer_transform=True, **FOLDERS, **KW)
    assert len(defer) == len(normal) > 1
    for idx in range(len(normal)):
        random.seed(40 + idx)
        np.random.seed(40 + idx)
        want = normal[idx]
        state_normal = random.getstate()
        random.seed(40 + idx)
        np.random.seed(40 + idx)
        got = defer[idx]
        assert random.getstate() == state_normal                # the stream is left where the host transform leaves it
        random.seed(40 + idx)
        np.random.seed(40 + idx)
        raw = plain[idx]
        assert len(got) == len(want) == KW["sequence_length"]
        seeds = {int(p["transform_seed"]) for p in got}
        assert len(seeds) == 1                                  # ONE seed per sequence
        seed = seeds.pop()
        for pg, pw, pr in zip(got, want, raw):
            assert pg["transform_seed"].dtype == torch.int64 and pg["transform_seed"].dim() == 0
            assert set(pg) == set(pw) | {"transform_seed"} and "transform_seed" not in pw
            for key in pw:
                assert _same(pg[key], pr[key]), key             # untransformed: bitwise the transform=None dataset's
                random.seed(seed)
                assert _same(transform(pg[key]), pw[key]), key  # the reported seed reproduces the normal item on the host
    # default collation stacks the seeds to [B]
    batch = torch.utils.data.default_collate([defer[0], defer[1]])
    assert batch[0]["transform_seed"].shape == (2,) and batch[0]["events0"].shape[0] == 2


def test_defer_transform_voxel_dataset_and_concat(tree):
    root, names = tree
    base = os.path.join(root, names[0])
    t = D.RandomCrop(16)
    random.seed(3)
    a = D.VoxelGridDataset(base, "events/voxels", transform=t)[2]
    sa = random.getstate()
    random.seed(3)
    b = D.VoxelGridDataset(base, "events/voxels", transform=t, defer_transform=True)[2]
    assert random.getstate() == sa and "transform_seed" not in a
    random.seed(int(b["transform_seed"]))
    assert _same(t(b["events"]), a["events"])
    cat = D.concatenate_subfolders(root, "SequenceSynchronizedFramesEventsDataset", transform=t, defer_transform=True, **FOLDERS, **KW)
    assert "transform_seed" in cat[0][0] and cat[0][0]["events0"].shape[1:] == (20, 28)
    assert "transform_seed" not in D.concatenate_subfolders(root, "SequenceSynchronizedFramesEventsDataset", transform=t, **FOLDERS, **KW)[0][0]
