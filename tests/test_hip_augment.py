"""GPU: the device augmentation (csrc/augment.hip, rpg_ramnet_amd.augment).  Exact mode bit for bit against torch.flip + slicing; the
relations to the host transform that hold for any correct implementation; the general mode against float64; the fused nonzero
normalisation; the loader end to end; launch count; the raw C ABI."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from recipe import FOLDERS, make_dataset_dir  # noqa: E402

from rpg_ramnet_amd import _hip  # noqa: E402
from rpg_ramnet_amd import augment as A  # noqa: E402
from rpg_ramnet_amd import data as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def bits(t):
    return t.contiguous().view(torch.int32)


def flip_crop(x, p):
    """The exact transform in plain torch: x [C, H, W] -> flip, then window."""
    dims = ([2] if p.hflip else []) + ([1] if p.vflip else [])
    y = torch.flip(x, dims) if dims else x
    return y[:, p.top:p.top + p.th, p.left:p.left + p.tw]


def exact_params(hflip, vflip, top, left, th, tw):
    return A.Params((-1.0 if hflip else 1.0, 0.0, 0.0, 0.0, -1.0 if vflip else 1.0, 0.0), top, left, th, tw, True, hflip, vflip)


def nan_targets(shape, gen, frac=0.2):
    x = torch.rand(shape, generator=gen)
    x[torch.rand(shape, generator=gen) < frac] = float("nan")
    return x


SIZES = [(260, 346, 224, 224), (260, 346, 256, 344), (480, 640, 224, 224), (40, 56, 32, 32), (40, 56, 40, 56), (20, 30, 17, 23)]


@pytest.mark.parametrize("H,W,th,tw", SIZES)
@pytest.mark.parametrize("Cc", [1, 5, 10])
def test_exact_mode_bitwise(H, W, th, tw, Cc):
    """Four flip combinations with per-sample different windows in ONE batch == torch.flip + slicing, on the int32 view; N(0,1) data and
    targets with 20 % NaN; NHWC output == ops.pack_input of the NCHW output.  (20x30 -> 17x23: the path without 16-byte stores.)"""
    from rpg_ramnet_amd import ops
    gen = torch.Generator().manual_seed(H * 1000 + W + Cc)
    rng = random.Random(H + Cc)
    params = [exact_params(bool(k & 1), bool(k & 2), rng.randint(0, H - th), rng.randint(0, W - tw), th, tw) for k in range(4)]
    params += [exact_params(True, True, H - th, W - tw, th, tw), exact_params(False, True, 0, 0, th, tw)]      # the windows' extremes
    G = len(params)
    for x in (torch.randn(G, Cc, H, W, generator=gen), nan_targets((G, Cc, H, W), gen)):
        want = torch.stack([flip_crop(x[g], params[g]) for g in range(G)])
        xd = x.to(DEV)
        got = A.apply(xd, params)
        assert got.shape == want.shape and torch.equal(bits(got.cpu()), bits(want))
        nhwc = A.apply(xd, params, nhwc=True)
        assert torch.equal(bits(nhwc), bits(ops.pack_input(got, DEV)))
        wide = A.apply(xd, params, nhwc=True, cpad=16)
        assert torch.equal(bits(wide[..., :nhwc.shape[3]]), bits(nhwc)) and float(wide[..., (Cc + 3) // 4 * 4:].abs().sum()) == 0.0
    # a parameter index: tensors 0..G-1 all use set 3; and one set for every tensor
    got = A.apply(xd, params, pidx=[3] * G)
    assert torch.equal(bits(got.cpu()), bits(torch.stack([flip_crop(x[g], params[3]) for g in range(G)])))
    got = A.apply(xd, params[1])
    assert torch.equal(bits(got.cpu()), bits(torch.stack([flip_crop(x[g], params[1]) for g in range(G)])))


def dilate3(mask):
    return F.max_pool2d(mask.float()[None], 3, 1, 1)[0] > 0


@pytest.mark.parametrize("H,W,size,even", [(260, 346, 224, False), (260, 346, [256, 344], False), (480, 640, 224, False), (40, 56, 32, False),
                                           (260, 346, 224, True), (40, 56, [40, 56], False)])
def test_relation_to_the_host_transform(H, W, size, even):
    """Same seeds, the yardstick is data.Compose on the CPU: (a) device NaN mask within the host's; (b) the host's NaN mask within the
    3x3 dilation of the flipped source mask, dilated BEFORE the crop; (c) where the host is finite, |device - host| <= the host's own
    distance from the exact flip (computed with torch.flip on the CPU)."""
    transform = D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop(size, preserve_mosaicing_pattern=even)])
    gen = torch.Generator().manual_seed(H + W)
    worst = 0.0
    for seed in range(100, 108):
        x = torch.randn(1, H, W, generator=gen)
        x[torch.rand(1, H, W, generator=gen) < 0.2] = float("nan")
        random.seed(seed)
        host = transform(x)
        p = A.draw(transform, seed, H, W)
        dev = A.apply(x[None].to(DEV), p)[0].cpu()
        exact = flip_crop(x, p)
        nan_d, nan_h = torch.isnan(dev), torch.isnan(host)
        assert not bool((nan_d & ~nan_h).any())                                                   # (a)
        full = flip_crop(x, p._replace(top=0, left=0, th=H, tw=W))
        dil = dilate3(torch.isnan(full))[:, p.top:p.top + p.th, p.left:p.left + p.tw]
        assert not bool((nan_h & ~dil).any())                                                     # (b)
        fin = ~nan_h
        host_blur = (host - exact)[fin].abs()
        assert bool(((dev - host)[fin].abs() <= host_blur).all())                                 # (c)
        worst = max(worst, float(host_blur.max()))
    print("host transform's distance from the exact flip at %dx%d: %.3e" % (H, W, worst))


def _general_cases():
    cases = []
    for seed in range(8):
        cases.append(("seed%d" % seed, D.Compose([D.RandomRotationFlip(30, 0.5, 0.5), D.RandomCrop(224)]), seed))
    for deg in (7.3, -15.0, 30.0):
        for h in (0.0, 1.0):
            for v in (0.0, 1.0):
                cases.append(("deg%g_h%d_v%d" % (deg, h, v), D.Compose([D.RandomRotationFlip((deg, deg), h, v), D.RandomCrop(224)]), 1))
    return cases


def grid_sample64(x, theta, H, W):
    th64 = torch.tensor(theta, dtype=torch.float32).double().reshape(1, 2, 3)
    grid = F.affine_grid(th64, (1, x.shape[0], H, W), align_corners=False)
    return F.grid_sample(x.double()[None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0], grid[0]


@pytest.mark.parametrize("H,W", [(260, 346), (480, 640)])
def test_general_mode_against_float64(H, W):
    """Rotation + flips: |device - float64| <= 2 x |fp32 host transform - float64| on the same input (two fp32 evaluation orders of equal
    quality need not agree more closely with each other than either does with float64).  With NaN inputs the masks agree except where the
    float64 sampling coordinate lies within 1e-3 px of an integer (there rounding decides the tap set); that exclusion stays below 1 %."""
    gen = torch.Generator().manual_seed(H)
    report = []
    for name, transform, seed in _general_cases():
        x = torch.randn(2, H, W, generator=gen)
        random.seed(seed)
        host = transform(x)
        p = A.draw(transform, seed, H, W)
        assert not p.exact
        ref, grid = grid_sample64(x, p.theta, H, W)
        win = (slice(None), slice(p.top, p.top + p.th), slice(p.left, p.left + p.tw))
        ref = ref[win]
        dev = A.apply(x[None].to(DEV), p)[0].cpu()
        d_host, d_dev = float((host.double() - ref).abs().max()), float((dev.double() - ref).abs().max())
        report.append((name, d_dev, d_host))
        assert d_dev <= 2.0 * d_host, "%s %dx%d: device %.3e from float64, host %.3e" % (name, H, W, d_dev, d_host)
        nhwc = A.apply(x[None].to(DEV), p, nhwc=True)[0].cpu()
        assert torch.equal(bits(nhwc[..., :2].permute(2, 0, 1)), bits(dev)) and float(nhwc[..., 2:].abs().sum()) == 0.0
        # NaN inputs
        xn = x.clone()
        xn[torch.rand(2, H, W, generator=gen) < 0.2] = float("nan")
        refn, _ = grid_sample64(xn, p.theta, H, W)
        devn = A.apply(xn[None].to(DEV), p)[0].cpu()
        ix = ((grid[..., 0] + 1) * W - 1) / 2
        iy = ((grid[..., 1] + 1) * H - 1) / 2
        near = ((ix - ix.round()).abs() < 1e-3) | ((iy - iy.round()).abs() < 1e-3)
        near = near[win[1], win[2]]
        assert float(near.float().mean()) <= 0.01, "%s: %.2f %% of the pixels excluded" % (name, 100 * float(near.float().mean()))
        assert torch.equal(torch.isnan(devn)[:, ~near], torch.isnan(refn[win])[:, ~near]), name
        fin = ~torch.isnan(refn[win]) & ~torch.isnan(devn)
        assert float((devn.double() - refn[win])[fin].abs().max()) <= 2.0 * d_host
    for name, d_dev, d_host in report:
        print("general mode %dx%d %s: device %.3e, host %.3e from float64" % (H, W, name, d_dev, d_host))


def _event_lists(G, n, H, W, seed):
    rng = np.random.default_rng(seed)
    lists = []
    for g in range(G):
        m = n if g != 1 else 0                                   # one empty list
        ev = np.stack([np.sort(rng.random(m)), rng.integers(0, W, m).astype(np.float64), rng.integers(0, H, m).astype(np.float64),
                       rng.integers(0, 2, m).astype(np.float64)], 1)
        if g == 2:                                               # a grid with a single nonzero value: one event
            ev = np.array([[0.5, 17.0, 23.0, 1.0]])
        lists.append(ev)
    return lists


@pytest.mark.parametrize("bins", [5, 10])
def test_fused_normalisation_bitwise(bins):
    """voxelize_augmented(normalize=True) == events_to_voxel_grids_packed(normalize=True) followed by the unfused apply, bit for bit."""
    from rpg_ramnet_amd import voxel
    H, W, G = 260, 346, 5
    cat, off, mx = voxel.pack_event_lists(_event_lists(G, 200000, H, W, bins), DEV)
    transform = D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop(224)])
    params = [A.draw(transform, 50 + g, H, W) for g in range(G)]
    table = A.ParamTable(params, H, W).to(DEV)
    grids = voxel.events_to_voxel_grids_packed(cat, off, mx, bins, W, H, normalize=True)
    want = A.apply(grids, table)
    out = torch.empty(G, bins, 224, 224, device=DEV)
    scratch = A.voxel_scratch(G, bins, H, W, DEV)
    got = A.voxelize_augmented(cat, off, mx, bins, W, H, table, out=out, scratch=scratch)
    assert got.data_ptr() == out.data_ptr() and torch.equal(bits(got), bits(want))
    assert float(got[1].abs().max()) == 0.0                                                      # the empty list: nothing to normalise
    assert torch.equal(bits(got[2]), bits(A.apply(voxel.events_to_voxel_grids_packed(cat, off, mx, bins, W, H), table)[2]))   # std = 0: values unchanged
    assert float(got[0].abs().max()) > 0.5 and abs(float(grids[0][grids[0] != 0].mean())) < 1e-3
    raw = A.voxelize_augmented(cat, off, mx, bins, W, H, table, normalize=False)
    assert torch.equal(bits(raw), bits(A.apply(voxel.events_to_voxel_grids_packed(cat, off, mx, bins, W, H), table)))
    # the rotation path reads through the same normalisation
    rot = A.ParamTable([A.draw(D.Compose([D.RandomRotationFlip(20, 0.5, 0.5), D.RandomCrop(224)]), 9 + g, H, W) for g in range(G)], H, W).to(DEV)
    assert torch.equal(bits(A.voxelize_augmented(cat, off, mx, bins, W, H, rot, nhwc=True)), bits(A.apply(grids, rot, nhwc=True)))


KW = dict(sequence_length=2, step_size=2, every_x_rgb_frame=2, clip_distance=1000.0, reg_factor=5.70378)


def test_loader_end_to_end(tmp_path):
    """AugmentedLoader over the defer_transform dataset == flip + slice of the transform=None dataset's tensors with draw's parameters,
    bit for bit; sequence_loss + backward on it == on a batch built with torch.flip on the device."""
    from rpg_ramnet_amd.model.model import ERGB2DepthRecurrent
    from rpg_ramnet_amd.trainer import sequence_loss
    root = make_dataset_dir(str(tmp_path / "tree"), H=40, W=56)
    base = os.path.join(root, sorted(os.listdir(root))[0])
    transform = D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop(32)])
    defer = D.SequenceSynchronizedFramesEventsDataset(base, transform=transform, defer_transform=True, **FOLDERS, **KW)
    plain = D.SequenceSynchronizedFramesEventsDataset(base, transform=None, **FOLDERS, **KW)
    B = 2
    random.seed(77)
    np.random.seed(77)
    batches = list(A.AugmentedLoader(torch.utils.data.DataLoader(defer, batch_size=B, shuffle=False, num_workers=0), DEV, transform))
    random.seed(77)
    np.random.seed(77)
    seeds_seen = [int(defer[i][0]["transform_seed"]) for i in range(len(defer))]
    random.seed(77)
    np.random.seed(77)
    raw = [plain[i] for i in range(len(plain))]
    assert len(batches) == (len(defer) + B - 1) // B and len(batches) >= 2
    built = []
    for k, seq in enumerate(batches):
        idx = list(range(k * B, min((k + 1) * B, len(defer))))
        ps = [A.draw(transform, seeds_seen[i], 40, 56, rng=random.Random()) for i in idx]
        mine = []
        for l, item in enumerate(seq):
            assert "transform_seed" not in item
            want = {}
            for key, t in item.items():
                assert t.is_cuda and t.shape[0] == len(idx) and tuple(t.shape[2:]) == (32, 32), key
                want[key] = torch.stack([flip_crop(raw[i][l][key].to(DEV), p) for i, p in zip(idx, ps)])
                assert torch.equal(bits(t), bits(want[key])), (k, l, key)
            mine.append(want)
        built.append(mine)
    cfg = dict(num_bins_rgb=1, num_bins_events=5, skip_type="sum", recurrent_block_type="conv", state_combination="convgru", num_encoders=3,
               base_num_channels=32, num_residual_blocks=2, use_upsample_conv=True, norm="none", gpu=0, every_x_rgb_frame=2, baseline=False,
               loss_composition=["image", "events1"])
    torch.manual_seed(0)
    model = ERGB2DepthRecurrent(cfg)
    model = model.to(model.gpu).train()
    losses = []
    for seq in (batches[0], built[0]):
        model.zero_grad(set_to_none=True)
        total, _ = sequence_loss(model, seq, cfg["loss_composition"], [1, 1])
        total.backward()
        torch.cuda.synchronize()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
        losses.append(float(total.detach()))
    assert np.isfinite(losses[0]) and losses[0] == losses[1]


def test_three_launches_per_sequence():
    """B=2, L=2, K=3: 6 event-grid, 2 frame and 8 target tensors -> at most three launches; other keys pass through."""
    B, L, K, H, W = 2, 2, 3, 40, 56
    gen = torch.Generator().manual_seed(0)
    seq = []
    for l in range(L):
        item = {"image": torch.rand(B, 1, H, W, generator=gen), "depth_image": nan_targets((B, 1, H, W), gen),
                "times_image": torch.rand(B, 1, generator=gen), "transform_seed": torch.tensor([5, 6])}
        for k in range(K):
            item["events%d" % k] = torch.randn(B, 5, H, W, generator=gen)
            item["depth_events%d" % k] = nan_targets((B, 1, H, W), gen)
        seq.append(item)
    dev_seq = [{k: (v.to(DEV) if k != "transform_seed" else v) for k, v in item.items()} for item in seq]
    transform = D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop(32)])
    before = A.launch_count()
    out = A.augment_sequence(dev_seq, None, transform)
    assert 1 <= A.launch_count() - before <= 3
    assert _hip.lib().ramnet_last_kernel().startswith(b"augment_kernel")
    ps = [A.draw(transform, s, H, W, rng=random.Random()) for s in (5, 6)]
    for l in range(L):
        assert "transform_seed" not in out[l] and torch.equal(out[l]["times_image"].cpu(), seq[l]["times_image"])
        for key, t in seq[l].items():
            if key in ("times_image", "transform_seed"):
                continue
            want = torch.stack([flip_crop(t[b], ps[b]) for b in range(B)])
            assert torch.equal(bits(out[l][key].cpu()), bits(want)), (l, key)


def test_cabi_raw_launches():
    """ramnet_augment_batch with ctypes and device pointers: one exact and one general launch."""
    L = _hip.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                                     # noqa: E731
    G, Cc, H, W, th, tw = 3, 2, 20, 28, 12, 16
    gen = torch.Generator().manual_seed(3)
    x = [torch.randn(Cc, H, W, generator=gen).to(DEV) for _ in range(G)]                         # separate allocations
    y = [torch.empty(Cc, th, tw, device=DEV) for _ in range(G)]
    src = torch.tensor([t.data_ptr() for t in x], dtype=torch.int64).to(DEV)
    dst = torch.tensor([t.data_ptr() for t in y], dtype=torch.int64).to(DEV)
    bx = (torch.linspace(-1, 1, W) * (W - 1) / W).to(DEV)
    by = (torch.linspace(-1, 1, H) * (H - 1) / H).to(DEV)
    theta = torch.tensor([[-1.0, 0, 0, 0, 1, 0], [0.8, -0.6, 0, 0.6, 0.8, 0]], dtype=torch.float32)
    win = torch.tensor([[3, 5, 1, 1], [2, 4, 0, 0]], dtype=torch.int32)
    pidx = torch.tensor([0, 1, 0], dtype=torch.int32).to(DEV)
    th_d, win_d = theta.to(DEV), win.to(DEV)
    rc = L.ramnet_augment_batch(ptr(src), ptr(dst), ptr(pidx), ptr(th_d), ptr(win_d), C.c_void_p(win.data_ptr()), None, ptr(bx), ptr(by), G, 2,
                                Cc, H, W, th, tw, 0, 0, st)
    assert rc == 0, L.ramnet_last_error()
    for g in (0, 2):
        want = torch.flip(x[g], [2])[:, 3:3 + th, 5:5 + tw]
        assert torch.equal(bits(y[g]), bits(want))
    grid = F.affine_grid(theta[1].double().reshape(1, 2, 3), (1, Cc, H, W), align_corners=False)
    ref = F.grid_sample(x[1].cpu().double()[None], grid, align_corners=False)[0][:, 2:2 + th, 4:4 + tw]
    # fp32 sampling coordinates up to 28 px carry a few ulp (~1e-5 px); white noise whose neighbours differ by up to ~8 turns that into < 1e-4
    assert float((y[1].cpu().double() - ref).abs().max()) < 1e-4
    # a window outside the image in the host copy of the table: refused, nothing launched
    bad = win.clone()
    bad[1, 0] = H - th + 1
    assert L.ramnet_augment_batch(ptr(src), ptr(dst), ptr(pidx), ptr(th_d), ptr(win_d), C.c_void_p(bad.data_ptr()), None, ptr(bx), ptr(by), G, 2,
                                  Cc, H, W, th, tw, 0, 0, st) == 10001 and b"bad argument" in L.ramnet_last_error()
    assert L.ramnet_augment_batch(ptr(src), ptr(dst), ptr(pidx), ptr(th_d), ptr(win_d), None, None, ptr(bx), ptr(by), G, 2, Cc, H, W, H + 1, tw,
                                  0, 0, st) == 10001
    assert L.ramnet_augment_batch(None, ptr(dst), ptr(pidx), ptr(th_d), ptr(win_d), None, None, ptr(bx), ptr(by), G, 2, Cc, H, W, th, tw, 0, 0,
                                  st) == 10001
    assert L.ramnet_augment_batch(ptr(src), ptr(dst), ptr(pidx), ptr(th_d), ptr(win_d), None, None, ptr(bx), ptr(by), G, 2, Cc, H, W, th, tw, 1, 1,
                                  st) == 10001                                                    # C > Cpad
    # statistics entry: sums and nonzero count of every grid
    g4 = torch.randn(2, 64, device=DEV)
    g4[0, ::3] = 0.0
    stats = torch.empty(2, 3, dtype=torch.float64, device=DEV)
    assert L.ramnet_nonzero_stats_batch(ptr(g4), 2, 64, ptr(stats), st) == 0
    np.testing.assert_allclose(stats[:, 0].cpu().numpy(), g4.double().sum(1).cpu().numpy(), rtol=1e-12, atol=1e-12)
    assert [int(v) for v in stats[:, 2]] == [int((g4[0] != 0).sum()), 64]
    torch.cuda.synchronize()
