"""The rows of the `ramnet_augment_scale_batch` tests (tests/test_hip_augment_scale.py, tests/test_augment_scale_cpu.py): sizes, parameter
sets and data, seeded.  No row is chosen from what the kernel gives."""
import random

import torch

# (H, W, th, tw, s)                                     output    what it covers
ROWS = [
    (40, 56, 32, 32, 0.5),                            # 16 x 16   the 4-pixels-per-thread path (NCHW, ow % 4 == 0)
    (40, 56, 32, 32, 0.25),                           # 8 x 8     taps 4 apart, weights 0.5
    (40, 56, 32, 32, 0.7),                            # 22 x 22   non-dyadic; the first pixel's coordinate is clamped to 0
    (20, 30, 17, 23, 0.5),                            # 8 x 11    odd sizes, per-pixel path, last source row and column unused
    (20, 30, 17, 23, 0.7),                            # 11 x 16
    (9, 13, 9, 13, 0.5),                              # 4 x 6     the window is the image
    (260, 346, 224, 224, 0.5),                        # 112 x 112 the recipe
]
RECIPE = ROWS[-1]
FAST = ROWS[0]
GENERAL = [(40, 56, 32, 32, 0.5), (40, 56, 32, 32, 0.7)]
GENERAL_DEGREES = 15.0
# the factors of the CPU anchor: (d + 0.5) / s - 0.5 is never an integer for them, so torch's fp32 coordinates choose the same taps
ANCHOR_FACTORS = (0.5, 0.25, 0.7)
ANCHOR_SIZES = [(32, 32), (31, 43), (32, 48), (224, 224)]


def channels(row):
    return (5,) if row == RECIPE else (1, 5)


def row_id(row):
    return "%dx%d_%dx%d_s%g" % row


def windows(H, W, th, tw, seed):
    """[(top, left, hflip, vflip)] x 6: the four flip combinations with different random windows, then the windows' two extremes"""
    rng = random.Random(seed)
    out = [(rng.randint(0, H - th), rng.randint(0, W - tw), bool(k & 1), bool(k & 2)) for k in range(4)]
    return out + [(H - th, W - tw, True, True), (0, 0, False, True)]


def normal(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def nan_targets(shape, seed, frac=0.2):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=gen)
    x[torch.rand(shape, generator=gen) < frac] = float("nan")
    return x


def with_nan(x, seed, frac=0.2):
    x = x.clone()
    x[torch.rand(x.shape, generator=torch.Generator().manual_seed(seed)) < frac] = float("nan")
    return x


# ------------------------------------------------------------------------------------------------ the reference-generated fixture
U = 2.0 ** -24


def _fixture_case():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from recipe import DATASET_CASES
    return next(c for c in DATASET_CASES if c[0] == "ramnet_nocrop_scale")


FIXTURE_CASE = _fixture_case()        # 20 x 28 -> 10 x 14 at scale_factor 0.5, transform None, 14-21 % NaN in the targets


def largest_finite_tap(win, s):
    """[C][th][tw] float64 -> [C][oh][ow]: the largest finite |tap| of every output pixel"""
    import numpy as np
    from eval_rescale_restatement import resize_largest_tap
    return torch.from_numpy(np.stack([resize_largest_tap(p.numpy(), s) for p in win]))


def fixture_sequence(tree, **over):
    """tree: (root of recipe.make_dataset_dir, its sorted sub-directories) -> (the dataset of the fixture's case with `over` changed, its
    item under the fixture's seeds, the (random, np.random) states afterwards)"""
    import os
    import numpy as np
    from recipe import FOLDERS
    from rpg_ramnet_amd import data as D
    name, seq_i, idx, seed, spec, kw = FIXTURE_CASE
    root, names = tree
    ds = D.SequenceSynchronizedFramesEventsDataset(os.path.join(root, names[seq_i]), transform=None, **FOLDERS, **dict(kw, **over))
    random.seed(seed)
    np.random.seed(seed)
    seq = ds[idx]
    return ds, seq, (random.getstate(), np.random.get_state())


def check_against_fixture(seq, gold, resized):
    """seq: the full-resolution packages ([C][20][28] fp32 CPU tensors); resized(l, key, t) -> [C][10][14] on the CPU: equal NaN masks and
    |resized - the reference's tensor| <= 4 x 2^-24 x the pixel's largest finite |tap| (the 0.5 bound of the CPU anchor)"""
    name = FIXTURE_CASE[0]
    seen = 0
    for l, package in enumerate(seq):
        for key, t in package.items():
            if not (key.startswith("events") or key == "image" or key.startswith("depth_")):
                continue
            want = torch.from_numpy(gold["%s/%d/%s" % (name, l, key)])
            assert tuple(t.shape[1:]) == (20, 28) and tuple(want.shape[1:]) == (10, 14), key
            got = resized(l, key, t)
            assert tuple(got.shape) == tuple(want.shape), key
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (l, key)
            bound = 4 * U * largest_finite_tap(t.double(), 0.5)
            fin = ~torch.isnan(want)
            assert bool(((got.double() - want.double())[fin].abs() <= bound[fin]).all()), (l, key)
            if key.startswith("depth_"):
                assert 0.14 <= float(torch.isnan(want).float().mean()) <= 0.21, (l, key)
            seen += 1
    assert seen == len([k for k in gold.files if k.startswith(name + "/") and k.split("/")[-2].isdigit()])
