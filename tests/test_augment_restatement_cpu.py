"""CPU (no GPU): anchors of tests/augment_restatement.py and the per-row conditions that the rules of tests/test_hip_augment_launch.py rely
on (profiles/grad_loss_augment_tests_notes.md §1)."""
import random

import pytest
import torch
import torch.nn.functional as F

from rpg_ramnet_amd import augment as A
from rpg_ramnet_amd import data as D
import augment_cases as ac
import augment_restatement as ar
import reduction_restatement as rr

F64 = torch.float64


@pytest.mark.parametrize("shape", ["s1", "s2", "s4"])
def test_general_mode_against_grid_sample(shape):
    """the sample points against affine_grid in float64 (they differ by the fp32 rounding of the coordinate tables), and the bilinear
    sampling at the statement's own points against grid_sample(bilinear, zeros, align_corners=False) in float64"""
    H, W, th, tw = ac.SHAPES[shape]
    src = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3)).to(F64)
    bx, by = ar.base_coords(W), ar.base_coords(H)
    for th6, top, left, _, _ in ac.general_sets(H, W, th, tw, True):
        ix, iy, dix, diy = ar.sample_points(th6, bx, by, H, W, th, tw, top, left)
        gx, gy = (2 * ix + 1) / W - 1, (2 * iy + 1) / H - 1
        grid = F.affine_grid(th6.view(1, 2, 3), (1, 3, H, W), align_corners=False)[0, top:top + th, left:left + tw]
        assert float((grid[..., 0] - gx).abs().max()) <= 1e-6 * (1 + float(gx.abs().max())) and float((grid[..., 1] - gy).abs().max()) <= 1e-6 * (1 + float(gy.abs().max()))
        ref = F.grid_sample(src[None], torch.stack([gx, gy], -1)[None], mode="bilinear", padding_mode="zeros", align_corners=False)[0]
        val, rnd = ar.bilinear(src, ix, iy)
        assert float((val - ref).abs().max()) <= 1e-12 and bool((rnd >= 0).all())
        assert bool((dix > 0).all()) and float(dix.max()) < 1e-4 * max(1.0, float(th6.abs().max())) * W


def test_nan_taps_and_zero_padding():
    """a tap inside the image is always multiplied (0 x NaN = NaN, at integer coordinates too), a tap outside is skipped; as grid_sample"""
    src = torch.arange(12, dtype=F64).view(1, 3, 4) + 1
    src[0, 1, 2] = float("nan")
    ix = torch.tensor([[1.0, 2.0, -0.5, 3.5, -1.0, 1.5]], dtype=F64)
    iy = torch.tensor([[1.0, 0.0, 0.0, 2.0, 0.0, -2.0]], dtype=F64)
    val, _ = ar.bilinear(src, ix, iy)
    ref = F.grid_sample(src[None], torch.stack([(2 * ix + 1) / 4 - 1, (2 * iy + 1) / 3 - 1], -1)[None], mode="bilinear", padding_mode="zeros", align_corners=False)[0]
    # the second point has its NaN tap at weight exactly 0: the header's rule makes it NaN (torch's CPU grid_sample drops that tap)
    keep = torch.tensor([True, False, True, True, True, True])
    assert torch.equal(torch.isnan(val)[0, 0, keep], torch.isnan(ref)[0, 0, keep]) and float((torch.nan_to_num(val) - torch.nan_to_num(ref))[0, 0, keep].abs().max()) <= 1e-14
    assert torch.isnan(val[0, 0]).tolist() == [True, True, False, False, False, False] and val[0, 0, 2:].tolist() == [0.5, 6.0, 0.0, 0.0]


@pytest.mark.parametrize("H,W,size", [(40, 56, 32), (20, 30, 16)])
def test_exact_mode_against_the_host_transform(H, W, size):
    """data.Compose([RandomRotationFlip(0), RandomCrop]) on an index image under the seed that augment.draw is given"""
    transform = D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop(size)])
    index = torch.arange(2 * H * W, dtype=torch.float32).reshape(2, H, W)
    seen = set()
    for seed in range(24):
        random.seed(seed)
        host = transform(index)
        p = A.draw(transform, seed, H, W)
        got = ar.exact(index.to(F64), H, W, p.th, p.tw, p.top, p.left, int(p.hflip) | 2 * int(p.vflip))
        assert p.exact and torch.equal(torch.round(host).to(F64), got)
        seen.add((p.hflip, p.vflip))
    assert len(seen) == 4


def test_general_mode_against_the_host_transform():
    transform = D.Compose([D.RandomRotationFlip((25.0, 25.0), 0.5, 0.5), D.RandomCrop(16)])
    H, W = 20, 30
    x = torch.randn(2, H, W, generator=torch.Generator().manual_seed(4))
    for seed in range(6):
        random.seed(seed)
        host = transform(x)
        p = A.draw(transform, seed, H, W)
        val, bound, _ = ar.general(x.to(F64), torch.tensor(p.theta, dtype=torch.float32).to(F64), ar.base_coords(W), ar.base_coords(H), p.th, p.tw, p.top, p.left)
        assert not p.exact and float((host.to(F64) - val).abs().max()) <= 1e-4 * float(x.abs().max())


@pytest.mark.parametrize("kind", ac.STAT_KINDS)
def test_normalisation_against_the_stand_alone_statement(kind):
    src = ac._source(kind, 2, 9, 13, torch.Generator().manual_seed(8))
    out, bound = ar.normalized(src)
    ref = rr.normalize_nonzero(src)
    assert torch.equal(ar.nonzero_stats(src), rr.nonzero_stats(src))
    assert float((out - ref).abs().max()) <= 1e-14 * max(1.0, float(ref.abs().max()))
    assert (bound is None) == (kind in ("zeros", "c03", "c02")) and (bound is not None or torch.equal(out, src))
    if bound is not None:
        assert bool((out[src == 0] == 0).all()) and bool((bound[src == 0] == 0).all()) and float(bound.max()) < 1e-5


def test_layout():
    out = torch.arange(2 * 3 * 4, dtype=F64).view(2, 3, 4)
    nhwc = ar.to_layout(out, True, 4).view(3, 4, 4)
    assert torch.equal(nhwc[:, :, :2], out.permute(1, 2, 0)) and bool((nhwc[:, :, 2:] == 0).all()) and torch.equal(ar.to_layout(out, False, 0), out.view(-1))
    assert ar.clamp_window(-5, 1000, 20, 30, 17, 23) == (0, 7) and ar.clamp_window(2, 3, 20, 30, 17, 23) == (2, 3)


# ------------------------------------------------------------------------------------------------ the rows
@pytest.mark.parametrize("name", list(ac.ROWS))
def test_row_conditions(name):
    """every window fits; the parameter table serves every tensor; on finite rows every bound is finite and nothing is excluded; on NaN rows at
    most 1 % of the pixels are excluded from the comparison of the NaN masks; the normalisation bound is in range (asserted inside)"""
    r = ac.ROWS[name]
    H, W, th, tw = r["H"], r["W"], r["th"], r["tw"]
    assert r["pidx"] is not None or len(r["params"]) >= r["G"]
    assert not r["nhwc"] or (r["Cpad"] >= r["C"] and r["Cpad"] % 4 == 0)
    for t, top, left, exact, flips in r["params"]:
        assert 0 <= top <= H - th and 0 <= left <= W - tw
    has_nan = "nan" in r["kinds"]
    assert not (has_nan and r["stats"])
    covered = 0
    for gs, ref, bound, near in ac.expected(name):
        covered += len(gs)
        if bound is None:
            continue
        if not has_nan:
            assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()) and bool((bound >= 0).all())
        elif near is not None:
            print("%s set of tensors %s: %d of %d pixels excluded" % (name, gs[:3], int(near.sum()), near.numel()))
            assert int(near.sum()) <= 0.01 * near.numel()
            assert bool(torch.isnan(ref).any()) and not bool(torch.isnan(ref).all())
    assert covered == r["G"]


def test_rows_reach_what_they_are_for():
    R = ac.ROWS
    big = R["big"]
    cap = (8192 + big["G"] - 1) // big["G"]
    assert cap * 256 < big["th"] * big["tw"] and big["tw"] % 4 and (big["G"] + 127) // 128 > 32
    assert R["x_s3_c5_nchw"]["tw"] % 4 == 0 and not R["x_s3_c5_nchw"]["skew"] and R["x_s3_c5_nchw_skew"]["skew"] == 1
    assert {(r["nhwc"], r["Cpad"]) for r in R.values()} >= {(False, 0), (True, 4), (True, 8), (True, 16)} and {r["C"] for r in R.values()} >= {1, 2, 5}
    r = R["g_s4_c2_nchw"]
    for gs, ref, bound, near in ac.expected("g_s4_c2_nchw"):
        if gs == [len(r["params"]) - 1]:                     # the all-outside set
            assert not bool(ref.any()) and not bool(bound.any())
    # translations: the first / last column sampled at -0.5 / W - 0.5, just inside and just outside
    H, W, th, tw = r["H"], r["W"], r["th"], r["tw"]
    x0s = set()
    for t, top, left, _, _ in r["params"]:
        ix, iy, _, _ = ar.sample_points(t, ar.base_coords(W), ar.base_coords(H), H, W, th, tw, top, left)
        x0s |= {int(torch.floor(ix).min()), int(torch.floor(ix).max())}
    assert -1 in x0s and W - 1 in x0s
