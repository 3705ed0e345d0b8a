"""GPU: the datasets' scale_factor resize fused into the device augment launch (`ramnet_augment_scale_batch`, csrc/augment.hip;
rpg_ramnet_amd.augment's `scale_factor=`), against the float64 statement of tests/augment_scale_restatement.py on the rows of
tests/augment_scale_cases.py (both anchored on the CPU by tests/test_augment_scale_cpu.py).

Rules: exact mode |got - ref| <= 2 x 2^-24 |ref| (one rounding of a double evaluation, one ulp of slack) with equal NaN masks; general mode
the largest tolerance augment_restatement assigns to the four window values + the same term; the NHWC form is ops.pack_input of the NCHW
form bit for bit; the raw launches go through tests/guarded.py (NaN / sentinel guards around every buffer, the pointer tables frozen).
No bound is taken from the kernel under test."""
import ctypes as C
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from recipe import FOLDERS, make_dataset_dir  # noqa: E402

import augment_restatement as ar  # noqa: E402
import augment_scale_cases as sc  # noqa: E402
import augment_scale_restatement as asr  # noqa: E402
from guarded import BADARG, F64, SENT, In, Out, _bits, call, pointer_table  # noqa: E402
from rpg_ramnet_amd import _hip  # noqa: E402
from rpg_ramnet_amd import augment as A  # noqa: E402
from rpg_ramnet_amd import data as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
I32 = torch.int32
INT_FILL = 0x3FFFFFFF            # what the guards of the int32 inputs hold
GAP = 36                         # floats between the destinations of an arena (a multiple of 4: they stay 16-byte aligned)
NAME = "ramnet_augment_scale_batch"


def bits(t):
    return t.contiguous().view(torch.int32)


def last_kernel():
    return _hip.lib().ramnet_last_kernel().decode()


def exact_params(hflip, vflip, top, left, th, tw):
    return A.Params((-1.0 if hflip else 1.0, 0.0, 0.0, 0.0, -1.0 if vflip else 1.0, 0.0), top, left, th, tw, True, hflip, vflip)


def flips_of(p):
    return int(p.hflip) | (int(p.vflip) << 1)


@functools.lru_cache(maxsize=None)
def params_of(row):
    H, W, th, tw, _ = row
    return tuple(exact_params(h, v, top, left, th, tw) for top, left, h, v in sc.windows(H, W, th, tw, H * 100 + tw))


@functools.lru_cache(maxsize=None)
def reference(row, Cc, kind):
    """-> (x [6, C, H, W] fp32, ref [6, C, oh, ow] float64, tol): computed once, shared, never changed"""
    H, W, th, tw, s = row
    ps = params_of(row)
    seed = H * 1000 + W + Cc + int(s * 100)
    x = sc.normal((len(ps), Cc, H, W), seed) if kind == "normal" else sc.nan_targets((len(ps), Cc, H, W), seed)
    both = [asr.exact(x[g].double(), H, W, th, tw, p.top, p.left, flips_of(p), s) for g, p in enumerate(ps)]
    return x, torch.stack([b[0] for b in both]), torch.stack([b[1] for b in both])


# ------------------------------------------------------------------------------------------------ 5: exact mode, module level
@pytest.mark.parametrize("row", sc.ROWS, ids=sc.row_id)
def test_exact_mode(row):
    """G = 6 parameter sets in one launch (four flip combinations with different windows, the windows' two extremes), N(0,1) data and
    targets with 20 % NaN, NCHW, NHWC and cpad=16."""
    from rpg_ramnet_amd import ops
    H, W, th, tw, s = row
    oh, ow = asr.out_shape(th, tw, s)
    ps = list(params_of(row))
    for Cc in sc.channels(row):
        for kind in ("normal", "nan"):
            x, ref, tol = reference(row, Cc, kind)
            xd = x.to(DEV)
            before = A.launch_count()
            got = A.apply(xd, ps, scale_factor=s)
            assert A.launch_count() == before + 1 and last_kernel() == "augment_scale_kernel<nchw>"
            assert tuple(got.shape) == (len(ps), Cc, oh, ow)
            asr.check(got.cpu(), ref, tol, "%s C=%d %s" % (sc.row_id(row), Cc, kind))
            nhwc = A.apply(xd, ps, nhwc=True, scale_factor=s)
            assert last_kernel() == "augment_scale_kernel<nhwc>" and tuple(nhwc.shape) == (len(ps), oh, ow, (Cc + 3) // 4 * 4)
            assert torch.equal(bits(nhwc), bits(ops.pack_input(got, DEV)))
            wide = A.apply(xd, ps, nhwc=True, cpad=16, scale_factor=s)
            assert torch.equal(bits(wide[..., :nhwc.shape[3]]), bits(nhwc)) and not bool(bits(wide[..., nhwc.shape[3]:]).any())
    # one parameter set for every tensor, through a parameter index
    got = A.apply(xd, ps, pidx=[3] * len(ps), scale_factor=s)
    want = torch.stack([asr.exact(x[g].double(), H, W, th, tw, ps[3].top, ps[3].left, flips_of(ps[3]), s)[0] for g in range(len(ps))])
    asr.check(got.cpu(), want, 2 * asr.U * want.abs(), sc.row_id(row) + " pidx")
    # s >= 1: today's launch, today's result
    same = A.apply(xd, ps, scale_factor=1.0)
    assert last_kernel() == "augment_kernel<nchw>" and torch.equal(bits(same), bits(A.apply(xd, ps))) and tuple(same.shape[2:]) == (th, tw)
    with pytest.raises(ValueError, match="scale_factor"):
        A.apply(xd, ps, scale_factor=0.0)
    with pytest.raises(ValueError, match="no pixel left"):
        A.apply(xd, ps, scale_factor=0.5 / max(th, tw))


# ------------------------------------------------------------------------------------------------ raw launches
class Launch:
    """the buffers of one raw launch; `args` is what `call` gets.  srcs: [C][H][W] tensors; src_index: which source tensor g reads (default
    g); arena: the destinations in one buffer with sentinel gaps"""

    def __init__(self, srcs, params, row, Cc, nhwc=False, Cpad=0, skew=0, pidx=None, stats=None, arena=False, src_index=None):
        H, W, th, tw, s = row
        oh, ow = asr.out_shape(th, tw, s)
        P = len(params)
        self.n_out = oh * ow * (Cpad if nhwc else Cc)
        self.src = [In(x.reshape(-1)) for x in srcs]
        sp = self.src if src_index is None else [self.src[k] for k in src_index]
        G = self.G = len(sp)
        self.arena = arena
        if arena:
            self.dst = Out(G, self.n_out, ld=self.n_out + GAP)
            dp = [self.dst.ptr + 4 * (self.n_out + GAP) * g for g in range(G)]
        else:
            self.dst = [Out(1, self.n_out, skew=skew) for _ in range(G)]
            dp = self.dst
        self.tabs = pointer_table(sp, tail=1), pointer_table(dp, tail=1)
        win = torch.tensor([[p.top, p.left, int(p.exact), flips_of(p)] for p in params], dtype=I32)
        self.host_win = (C.c_int * (4 * P))(*win.reshape(-1).tolist())
        self.keep = [In(torch.tensor([p.theta for p in params], dtype=F64)), In(win, fill=INT_FILL, dtype=I32),
                     None if pidx is None else In(torch.tensor(pidx, dtype=I32), fill=INT_FILL, dtype=I32),
                     None if stats is None else In(stats.reshape(-1), dtype=F64), In(ar.base_coords(W)), In(ar.base_coords(H))]
        theta, win_in, pidx_in, st, bx, by = self.keep
        self.args = [NAME, self.tabs[0], self.tabs[1], pidx_in, theta, win_in, self.host_win, st, bx, by, G, P, Cc, H, W, th, tw, oh, ow,
                     C.c_double(s), Cpad, int(nhwc)]

    POS = {"src": 1, "dst": 2, "theta": 4, "win": 5, "host_win": 6, "bx": 8, "by": 9, "G": 10, "P": 11, "C": 12, "H": 13, "W": 14, "th": 15, "tw": 16,
           "oh": 17, "ow": 18, "s": 19, "Cpad": 20, "nhwc": 21}

    def change(self, **kw):
        for k, v in kw.items():
            self.args[self.POS[k]] = C.c_double(v) if k == "s" else v
        return self

    def outs(self):
        return [self.dst] if self.arena else self.dst

    def run(self, rc=0):
        call(*self.args, rc=rc)
        for o in self.outs():
            o._host = None
            o.check(NAME, untouched=rc != 0)
        if rc != 0:
            return None
        got = self.dst.value() if self.arena else torch.stack([o.value().view(-1) for o in self.dst])
        assert not bool((got == SENT).any()), "part of the output region keeps its sentinel"
        return got


def expected(srcs, params, row, nhwc, Cpad, src_index=None, pidx=None):
    """-> (ref, tol) [G][n_out] float64 of an exact-mode launch"""
    H, W, th, tw, s = row
    G = len(srcs) if src_index is None else len(src_index)
    done, refs, tols = {}, [], []
    for g in range(G):
        k, p = g if src_index is None else src_index[g], g if pidx is None else pidx[g]
        if (k, p) not in done:
            q = params[p]
            ref, tol = asr.exact(srcs[k].double(), H, W, th, tw, q.top, q.left, flips_of(q), s)
            done[(k, p)] = ar.to_layout(ref, nhwc, Cpad), ar.to_layout(tol, nhwc, Cpad)
        refs.append(done[(k, p)][0])
        tols.append(done[(k, p)][1])
    return torch.stack(refs), torch.stack(tols)


# ------------------------------------------------------------------------------------------------ 6: the 4-pixel path == the per-pixel path
def test_fast_path_equals_the_per_pixel_path():
    """(40, 56, 32, 32, 0.5), NCHW, exact: destinations 16-byte aligned (4 pixels per thread) and moved one float off (per pixel): same bits"""
    row = sc.FAST
    ps = list(params_of(row))
    for Cc in (1, 5):
        for kind in ("normal", "nan"):
            x, ref, tol = reference(row, Cc, kind)
            srcs = list(x)
            aligned = Launch(srcs, ps, row, Cc)
            skewed = Launch(srcs, ps, row, Cc, skew=1)
            assert all(o.ptr % 16 == 0 for o in aligned.dst) and all(o.ptr % 16 == 4 for o in skewed.dst)
            a, b = aligned.run(), skewed.run()
            assert last_kernel() == "augment_scale_kernel<nchw>"
            assert torch.equal(_bits(a), _bits(b))
            asr.check(a, ref.reshape(a.shape), tol.reshape(a.shape), "fast path C=%d %s" % (Cc, kind))
    # the normalisation goes through both paths alike
    x = sc.normal((len(ps), 2, row[0], row[1]), 5)
    x[x.abs() < 0.8] = 0.0
    stats = torch.stack([ar.nonzero_stats(t.double()) for t in x])
    a, b = Launch(list(x), ps, row, 2, stats=stats).run(), Launch(list(x), ps, row, 2, stats=stats, skew=1).run()
    assert torch.equal(_bits(a), _bits(b)) and not torch.equal(_bits(a), _bits(Launch(list(x), ps, row, 2).run()))
    H, W, th, tw, s = row
    for g, p in enumerate(ps):
        src, bound = ar.normalized(x[g].double())
        ref, tol = asr.exact(src, H, W, th, tw, p.top, p.left, flips_of(p), s, value_bound=bound)
        asr.check(a[g], ref, tol, "fast path with stats, tensor %d" % g)


# ------------------------------------------------------------------------------------------------ 7: general mode
@pytest.mark.parametrize("row", sc.GENERAL, ids=sc.row_id)
def test_general_mode(row):
    """15 degrees with the four flip combinations, finite N(0,1) data: every value within the general-mode tolerance, no NaN; the NHWC form
    is the packed NCHW form."""
    from rpg_ramnet_amd import ops
    H, W, th, tw, s = row
    deg = sc.GENERAL_DEGREES
    ps = [A.draw(D.Compose([D.RandomRotationFlip((deg, deg), float(k & 1), float(k >> 1)), D.RandomCrop((th, tw))]), 30 + k, H, W, rng=random.Random())
          for k in range(4)]
    assert not any(p.exact for p in ps) and {flips_of(p) for p in ps} == {0, 1, 2, 3}
    Cc = 2
    x = sc.normal((len(ps), Cc, H, W), 11 + int(s * 10))
    got = A.apply(x.to(DEV), ps, scale_factor=s)
    assert last_kernel() == "augment_scale_kernel<nchw>"
    bx, by = ar.base_coords(W), ar.base_coords(H)
    for g, p in enumerate(ps):
        ref, tol = asr.general(x[g].double(), torch.tensor(p.theta, dtype=F64), bx, by, th, tw, p.top, p.left, s)
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(tol).all())
        asr.check(got[g].cpu(), ref, tol, "%s general set %d" % (sc.row_id(row), g))
    nhwc = A.apply(x.to(DEV), ps, nhwc=True, scale_factor=s)
    assert torch.equal(bits(nhwc), bits(ops.pack_input(got, DEV)))
    # an exact and a general set in one launch
    mixed = [ps[0], exact_params(True, False, 1, 2, th, tw), ps[3], exact_params(False, False, 0, 0, th, tw)]
    got2 = A.apply(x.to(DEV), mixed, scale_factor=s)
    assert torch.equal(bits(got2[0]), bits(got[0]))
    for g in (1, 3):
        ref, tol = asr.exact(x[g].double(), H, W, th, tw, mixed[g].top, mixed[g].left, flips_of(mixed[g]), s)
        asr.check(got2[g].cpu(), ref, tol, "%s mixed set %d" % (sc.row_id(row), g))


# ------------------------------------------------------------------------------------------------ 8: fused normalisation
def _event_lists(G, n, H, W, seed):
    rng = np.random.default_rng(seed)
    lists = []
    for g in range(G):
        m = n if g != 1 else 0                                   # one empty list
        lists.append(np.stack([np.sort(rng.random(m)), rng.integers(0, W, m).astype(np.float64), rng.integers(0, H, m).astype(np.float64),
                               rng.integers(0, 2, m).astype(np.float64)], 1))
    return lists


def test_fused_normalisation():
    """voxelize_augmented(scale_factor=0.5, nhwc=True) on sparse event lists, 5 bins: the model's input layout at the reduced size, normalised
    with the statistics of the full grids"""
    from rpg_ramnet_amd import voxel
    H, W, th, tw, s = sc.FAST
    G, bins = 4, 5
    cat, off, mx = voxel.pack_event_lists(_event_lists(G, 1500, H, W, 1), DEV)
    ps = list(params_of(sc.FAST))[:G]
    table = A.ParamTable(ps, H, W).to(DEV)
    scratch = A.voxel_scratch(G, bins, H, W, DEV)
    got = A.voxelize_augmented(cat, off, mx, bins, W, H, table, scratch=scratch, scale_factor=s, nhwc=True)
    assert tuple(got.shape) == (G, 16, 16, 8) and last_kernel() == "augment_scale_kernel<nhwc>"
    want = A.apply(scratch["grids"], table, stats=scratch["stats"], scale_factor=s, nhwc=True)
    assert torch.equal(bits(got), bits(want))
    assert not bool(bits(got[1]).any()) and not bool(bits(got[..., bins:]).any())           # the empty list, the pad channels: +0
    grids = scratch["grids"].cpu().double()
    assert 0.0 < float((grids[0] != 0).double().mean()) < 0.5                                # sparse
    for g, p in enumerate(ps):
        src, bound = ar.normalized(grids[g])
        assert (bound is None) == (g == 1)
        ref, tol = asr.exact(src, H, W, th, tw, p.top, p.left, flips_of(p), s, value_bound=bound)
        asr.check(got[g].cpu().reshape(-1), ar.to_layout(ref, True, 8), ar.to_layout(tol, True, 8), "fused normalisation grid %d" % g)
    raw = A.voxelize_augmented(cat, off, mx, bins, W, H, table, normalize=False, scale_factor=s)
    assert torch.equal(bits(raw), bits(A.apply(scratch["grids"], table, scale_factor=s))) and tuple(raw.shape) == (G, bins, 16, 16)


# ------------------------------------------------------------------------------------------------ 9: the reference's fixture
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = make_dataset_dir(str(tmp_path_factory.mktemp("eventscape_scale_gpu")))
    return root, sorted(os.listdir(root))


def test_reference_fixture_on_the_device(tree):
    """the fixture's sequence at full resolution, uploaded, through augment_sequence(scale_factor=0.5) against the reference's own tensors"""
    gold = np.load(os.path.join(HERE, "golden", "dataset.npz"))
    ds, seq, _ = sc.fixture_sequence(tree, defer_scale=True)
    dev_seq = [{k: v[None].to(DEV) for k, v in package.items()} for package in seq]
    before = A.launch_count()
    out = A.augment_sequence(dev_seq, [0], None, scale_factor=0.5)
    assert A.launch_count() - before == len({int(v.shape[1]) for v in dev_seq[0].values()})
    sc.check_against_fixture(seq, gold, lambda l, key, t: out[l][key][0].cpu())


# ------------------------------------------------------------------------------------------------ 10: the loader
KW = dict(sequence_length=2, step_size=2, every_x_rgb_frame=2, clip_distance=1000.0, reg_factor=5.70378)


def test_loader(tree):
    """AugmentedLoader(scale_factor=0.5) over defer_transform + defer_scale datasets == the statement of the same loader's unscaled output"""
    root, _ = tree
    transform = D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop(16)])
    ds = D.concatenate_subfolders(root, "SequenceSynchronizedFramesEventsDataset", transform=transform, scale_factor=0.5, defer_transform=True,
                                  defer_scale=True, **FOLDERS, **KW)
    B = 2

    def batches(**kw):
        random.seed(77)
        np.random.seed(77)
        return list(A.AugmentedLoader(torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False, num_workers=0), DEV, transform, **kw))

    full = batches()
    before = A.launch_count()
    small = batches(scale_factor=0.5)
    launches = A.launch_count() - before
    assert len(small) == len(full) == (len(ds) + B - 1) // B >= 2
    tensors = 0
    for seq_s, seq_f in zip(small, full):
        assert len(seq_s) == len(seq_f) == KW["sequence_length"]
        for item_s, item_f in zip(seq_s, seq_f):
            assert "transform_seed" not in item_s and set(item_s) == set(item_f)
            for key, t in item_s.items():
                f = item_f[key]
                assert t.is_cuda and tuple(t.shape) == tuple(f.shape[:2]) + (8, 8) and tuple(f.shape[2:]) == (16, 16), key
                ref = torch.stack([asr.resize(u.double(), 0.5) for u in f.cpu()])
                asr.check(t.cpu(), ref, 2 * asr.U * ref.abs(), "loader " + key)
                tensors += 1
    groups = len({int(t.shape[1]) for t in small[0][0].values()})
    assert launches == groups * len(small) and launches < tensors                              # per channel-count group, not per tensor
    # a dataset that has already resized on the host: resizing again is refused
    twice = D.concatenate_subfolders(root, "SequenceSynchronizedFramesEventsDataset", transform=transform, scale_factor=0.5, defer_transform=True,
                                     **FOLDERS, **KW)
    loader = torch.utils.data.DataLoader(twice, batch_size=B)
    with pytest.raises(ValueError, match="defer_scale"):
        A.AugmentedLoader(loader, DEV, transform, scale_factor=0.5)
    A.AugmentedLoader(loader, DEV, transform)                                                  # (without the factor it is today's loader)
    with pytest.raises(ValueError, match="scale_factor"):
        A.AugmentedLoader(torch.utils.data.DataLoader(ds, batch_size=B), DEV, transform, scale_factor=float("nan"))


# ------------------------------------------------------------------------------------------------ 11: the C ABI
@pytest.mark.parametrize("nhwc,Cc,Cpad", [(False, 5, 0), (True, 5, 8), (True, 2, 4)])
@pytest.mark.parametrize("row", [sc.ROWS[0], sc.ROWS[2], sc.ROWS[3]], ids=sc.row_id)
def test_cabi_guarded(row, nhwc, Cc, Cpad):
    """every tensor in a buffer of its own between guards: exactly the output region is written, the pad channels are +0"""
    ps = list(params_of(row))
    x = sc.nan_targets((len(ps), Cc, row[0], row[1]), 17 + Cc)
    L = Launch(list(x), ps, row, Cc, nhwc=nhwc, Cpad=Cpad)
    got = L.run()
    assert last_kernel() == ("augment_scale_kernel<nhwc>" if nhwc else "augment_scale_kernel<nchw>")
    ref, tol = expected(list(x), ps, row, nhwc, Cpad)
    asr.check(got, ref, tol, "%s raw nhwc=%d" % (sc.row_id(row), nhwc))
    # a parameter index; NULL win_host
    pidx = [5, 0, 3, 3, 1, 2]
    L = Launch(list(x), ps, row, Cc, nhwc=nhwc, Cpad=Cpad, pidx=pidx).change(host_win=None)
    asr.check(L.run(), *expected(list(x), ps, row, nhwc, Cpad, pidx=pidx), "%s raw pidx" % sc.row_id(row))


BIG = [((9, 13, 9, 13, 0.5), 1),          # the issue's row: 4 x 6 pixels, one workgroup per tensor under a cap of 2
       ((40, 56, 40, 56, 0.7), 1),        # 28 x 39 = 1092 pixels on 2 workgroups = 512 threads: three trips of the per-pixel loop
       ((40, 56, 32, 32, 0.5), 10)]       # 10 x 16 x 4 = 640 items on 512 threads: two trips of the 4-pixel loop


@pytest.mark.parametrize("row,Cc", BIG, ids=[sc.row_id(r) for r, _ in BIG])
def test_grid_cap(row, Cc):
    """G = 4100 tensors in one launch (the launcher caps the grid at 2 workgroups per tensor), destinations in one arena with sentinel gaps;
    7 sources and 6 parameter sets shared among them"""
    G = 4100
    H, W, th, tw, s = row
    ps = [exact_params(h, v, top, left, th, tw) for top, left, h, v in sc.windows(H, W, th, tw, 3)]
    srcs = list(sc.nan_targets((7, Cc, H, W), 23))
    src_index, pidx = [g % 7 for g in range(G)], [g % 6 for g in range(G)]
    L = Launch(srcs, ps, row, Cc, arena=True, src_index=src_index, pidx=pidx)
    got = L.run()
    assert last_kernel() == "augment_scale_kernel<nchw>"
    asr.check(got, *expected(srcs, ps, row, False, 0, src_index, pidx), sc.row_id(row) + " G=4100")


def test_cabi_argument_checks():
    """RAMNET_E_BADARG, the message, nothing launched: every destination, table and guard as it was"""
    for row, nhwc, Cc, Cpad in ((sc.ROWS[0], False, 5, 0), (sc.ROWS[3], True, 5, 8)):
        H, W, th, tw, s = row
        oh, ow = asr.out_shape(th, tw, s)
        ps = list(params_of(row))
        srcs = list(sc.normal((len(ps), Cc, H, W), 2))
        bad = [dict(th=H + 1), dict(tw=W + 1), dict(th=0), dict(tw=0), dict(C=0), dict(H=0), dict(W=-1), dict(P=0), dict(P=-1), dict(G=-1), dict(G=65536),
               dict(src=None), dict(dst=None), dict(theta=None), dict(win=None), dict(bx=None), dict(by=None),
               dict(s=0.0), dict(s=-0.5), dict(s=1.0), dict(s=2.0), dict(s=float("nan")), dict(s=float("inf")), dict(s=-float("inf")),
               dict(oh=oh + 1), dict(oh=oh - 1), dict(ow=ow + 1), dict(ow=ow - 1), dict(oh=th, ow=tw), dict(oh=0), dict(ow=0), dict(oh=-1),
               dict(s=0.7), dict(s=0.01, oh=0, ow=0), dict(th=1, oh=0), dict(tw=1, ow=0)]
        if nhwc:
            bad += [dict(Cpad=Cc - 1), dict(Cpad=Cc // 4 * 4), dict(Cpad=6), dict(Cpad=Cpad + 2)]
        for change in bad:
            Launch(srcs, ps, row, Cc, nhwc=nhwc, Cpad=Cpad).change(**change).run(rc=BADARG)
        for k in range(len(ps)):                              # one bad window in the host copy is enough
            host = [[p.top, p.left, 1, flips_of(p)] for p in ps]
            host[k][k % 2] = -1 if k % 4 < 2 else [H - th, W - tw][k % 2] + 1
            Launch(srcs, ps, row, Cc, nhwc=nhwc, Cpad=Cpad).change(host_win=(C.c_int * (4 * len(ps)))(*sum(host, []))).run(rc=BADARG)
        L = Launch(srcs, ps, row, Cc, nhwc=nhwc, Cpad=Cpad).change(G=0)                     # no tensor: a no-op
        call(*L.args)
        for o in L.outs():
            o._host = None
            o.check(NAME, untouched=True)


# ------------------------------------------------------------------------------------------------ 12: reproducibility
def test_two_calls_give_the_same_bits_also_in_deterministic_mode():
    from rpg_ramnet_amd import ops
    for row in (sc.ROWS[0], sc.ROWS[2]):
        ps = list(params_of(row))
        x, ref, tol = reference(row, 5, "nan")
        xd = x.to(DEV)
        first = {nhwc: A.apply(xd, ps, nhwc=nhwc, scale_factor=row[4]) for nhwc in (False, True)}
        for nhwc in (False, True):
            assert torch.equal(bits(A.apply(xd, ps, nhwc=nhwc, scale_factor=row[4])), bits(first[nhwc]))
        with ops.switches(deterministic=True):
            assert ops.deterministic()
            for nhwc in (False, True):
                assert torch.equal(bits(A.apply(xd, ps, nhwc=nhwc, scale_factor=row[4])), bits(first[nhwc]))
        assert not ops.deterministic()
    # the fused normalisation on statistics joined in a fixed order
    from rpg_ramnet_amd import voxel
    H, W = sc.FAST[:2]
    cat, off, mx = voxel.pack_event_lists(_event_lists(3, 800, H, W, 2), DEV)
    table = A.ParamTable(list(params_of(sc.FAST))[:3], H, W).to(DEV)
    with ops.switches(deterministic=True):
        a = A.voxelize_augmented(cat, off, mx, 5, W, H, table, scale_factor=0.5, nhwc=True)
        b = A.voxelize_augmented(cat, off, mx, 5, W, H, table, scale_factor=0.5, nhwc=True)
    assert torch.equal(bits(a), bits(b)) and bool(a.abs().sum() > 0)


# ------------------------------------------------------------------------------------------------ 13: smoke at the reduced shape
def test_training_step_at_the_reduced_shape(tmp_path):
    """a 2-package sequence from the loader at window 64 -> 32 x 32 through trainer.sequence_loss and backward(): finite loss and gradients"""
    from rpg_ramnet_amd.model.model import ERGB2DepthRecurrent
    from rpg_ramnet_amd.trainer import sequence_loss
    root = make_dataset_dir(str(tmp_path / "tree"), n_seq=1, n_frames=8, H=72, W=88)
    transform = D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.5), D.RandomCrop(64)])
    ds = D.concatenate_subfolders(root, "SequenceSynchronizedFramesEventsDataset", transform=transform, scale_factor=0.5, defer_transform=True,
                                  defer_scale=True, **FOLDERS, **KW)
    random.seed(5)
    np.random.seed(5)
    seq = next(iter(A.AugmentedLoader(torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0), DEV, transform, scale_factor=0.5)))
    assert len(seq) == 2 and all(tuple(t.shape[2:]) == (32, 32) for item in seq for t in item.values())
    cfg = dict(num_bins_rgb=1, num_bins_events=5, skip_type="sum", recurrent_block_type="conv", state_combination="convgru", num_encoders=3,
               base_num_channels=32, num_residual_blocks=2, use_upsample_conv=True, norm="none", gpu=0, every_x_rgb_frame=2, baseline=False,
               loss_composition=["image", "events1"])
    torch.manual_seed(0)
    model = ERGB2DepthRecurrent(cfg)
    model = model.to(model.gpu).train()
    total, _ = sequence_loss(model, seq, cfg["loss_composition"], [1, 1])
    total.backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(total.detach()))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
