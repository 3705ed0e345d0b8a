"""GPU: `ramnet_augment_batch` (csrc/augment.hip), every launch alone through the C ABI with raw pointers, pixel by pixel against the float64
statement of tests/augment_restatement.py on the rows of tests/augment_cases.py (both anchored on the CPU by
tests/test_augment_restatement_cpu.py).

Every launch goes through `call` (tests/guarded.py): every source in its own buffer between NaN guards (the 4100 sources of the grid-stride
row: one arena with NaN gaps), every destination prefilled with the sentinel between sentinel guards, the two pointer tables frozen between
guards, theta / win / pidx / stats / bx / by between guards of their own.  Rules (profiles/grad_loss_augment_tests_notes.md §1):
  bit        the exact mode (NaN, -0 included); in every mode the zero padding of the NHWC channels, and whatever the statement gives with
             a bound of 0: windows sampled wholly outside the image, zero sources, sources the normalisation leaves unchanged;
  derived    the general mode on finite data, every pixel: coordinate error x the largest neighbouring difference of the zero-padded source
             around the float64 sample point, per axis, + the roundings of the four products and three adds on absolute values (+ the
             normalisation's own bound through the taps when `stats` is given);
  masks      the general mode on NaN data: the NaN masks agree wherever no coordinate lies within its error of an integer (the CPU file caps
             that share at 1 %), values as above where the neighbourhood is finite.
No bound is taken from the kernel under test."""
import ctypes as C

import pytest
import torch

from rpg_ramnet_amd import _hip
import augment_cases as ac
import augment_restatement as ar
from guarded import BADARG, F64, SENT, In, Out, _bits, assert_bits, call, pointer_table

pytestmark = pytest.mark.gpu

I32 = torch.int32
INT_FILL = 0x3FFFFFFF            # what the guards of the int32 inputs hold
GAP = 36                         # floats between the tensors of an arena (a multiple of 4: the destinations stay 16-byte aligned)


def last_kernel():
    return _hip.lib().ramnet_last_kernel().decode()


def n_out(r):
    return r["th"] * r["tw"] * (r["Cpad"] if r["nhwc"] else r["C"])


class Launch:
    """the buffers of one launch of a row; `args` is what `call` gets"""

    def __init__(self, r, srcs, arena=False, through_kernel=False, win_dev=None, win_host="same", n_params=None, stats=None):
        G, P = r["G"], len(r["params"])
        self.r, self.arena = r, arena
        nin = r["C"] * r["H"] * r["W"]
        if arena:
            self.src = In(torch.stack([s.reshape(-1) for s in srcs]), ld=nin + GAP)
            self.dst = Out(G, n_out(r), ld=n_out(r) + GAP)
            sp, dp = [self.src.ptr + 4 * (nin + GAP) * g for g in range(G)], [self.dst.ptr + 4 * (n_out(r) + GAP) * g for g in range(G)]
        else:
            self.src = [In(s.reshape(-1)) for s in srcs]
            self.dst = [Out(1, n_out(r), skew=r["skew"]) for _ in range(G)]
            sp, dp = self.src, self.dst
        self.tabs = pointer_table(sp, through_kernel, tail=1), pointer_table(dp, through_kernel, tail=1)
        win = torch.tensor([[top, left, ex, fl] for _, top, left, ex, fl in r["params"]], dtype=I32)
        win_d = win if win_dev is None else torch.tensor(win_dev, dtype=I32)
        self.host_win = None if win_host is None else (C.c_int * (4 * P))(*(win if win_host == "same" else torch.tensor(win_host, dtype=I32)).reshape(-1).tolist())
        self.keep = [In(torch.stack([p[0] for p in r["params"]])), In(win_d, fill=INT_FILL, dtype=I32),
                     None if r["pidx"] is None else In(torch.tensor(r["pidx"], dtype=I32), fill=INT_FILL, dtype=I32),
                     None if stats is None else In(stats.reshape(-1), dtype=F64), In(ar.base_coords(r["W"])), In(ar.base_coords(r["H"]))]
        theta, win_in, pidx, st, bx, by = self.keep
        self.args = ["ramnet_augment_batch", self.tabs[0], self.tabs[1], pidx, theta, win_in, self.host_win, st, bx, by, G, P if n_params is None else n_params,
                     r["C"], r["H"], r["W"], r["th"], r["tw"], r["Cpad"], int(r["nhwc"])]

    def outs(self):
        return [self.dst] if self.arena else self.dst

    def run(self, rc=0):
        call(*self.args, rc=rc)
        for o in self.outs():
            o._host = None
            o.check("ramnet_augment_batch", untouched=rc != 0)
        if rc == 0 and self.r["G"]:
            assert last_kernel() == ("augment_kernel<nhwc>" if self.r["nhwc"] else "augment_kernel<nchw>")
        return self.dst.value() if self.arena else torch.stack([o.value().view(-1) for o in self.dst])

    def untouched(self):
        for o in self.outs():
            o._host = None
            o.check("ramnet_augment_batch", untouched=True)


def check(r, got, exp, what):
    """got [G][n_out] as the device left it; exp: ac.expected_of"""
    kept = got == SENT
    assert not bool(kept.any()), "%s: %d of %d elements keep their sentinel, first at %s" % (what, int(kept.sum()), kept.numel(), kept.nonzero()[0].tolist())
    worst = 0.0
    for gs, ref, bound, near in exp:
        for j, g in enumerate(gs):
            w = "%s tensor %d" % (what, g)
            want = ar.to_layout(ref[j], r["nhwc"], r["Cpad"])
            if bound is None:
                assert_bits(got[g], want, w)
                continue
            b = ar.to_layout(bound[j], r["nhwc"], r["Cpad"])
            cmp = torch.isfinite(want) & torch.isfinite(b)
            if near is not None and not bool(cmp.all()):              # NaN data: the masks, and the values where the neighbourhood is finite
                away = ~ar.to_layout(near[None].expand(ref[j].shape).to(F64), r["nhwc"], r["Cpad"]).bool()
                bad = (torch.isnan(got[g]) != torch.isnan(want)) & away
                assert not bool(bad.any()), "%s: %d NaN of one side are numbers on the other, first at %s" % (w, int(bad.sum()), bad.nonzero()[0].tolist())
                cmp &= away
            else:
                assert bool(cmp.all()), "%s: the statement is not finite" % w
            err = (got[g][cmp].double() - want[cmp]).abs()
            assert bool(torch.isfinite(got[g][cmp]).all()) and bool((err <= b[cmp]).all()), "%s: error %.3f x its bound at %s" % (
                w, float((err / b[cmp].clamp_min(1e-300)).max()), (err > b[cmp]).nonzero()[:1].tolist())
            worst = max(worst, float((err / b[cmp].clamp_min(1e-300))[b[cmp] > 0].max()) if bool((b[cmp] > 0).any()) else 0.0)
            zero = cmp & (b == 0)
            assert_bits(got[g][zero], want[zero], w + ", where the bound is 0")
    print("%s: max err / bound %.3f" % (what, worst))


def run_row(name):
    r = ac.ROWS[name]
    L = Launch(r, ac.sources(name), through_kernel=sorted(ac.ROWS).index(name) % 2 == 1, stats=ac.stats_of(name) if r["stats"] else None)
    got = L.run()
    check(r, got, ac.expected(name), name)
    return got


# ------------------------------------------------------------------------------------------------ the rows
@pytest.mark.parametrize("name", [n for n in ac.ROWS if n.startswith("x_")])
def test_exact_mode(name):
    run_row(name)


@pytest.mark.parametrize("name", [n for n in ac.ROWS if n.startswith("g_") and not n.endswith("_nan")])
def test_general_mode(name):
    got = run_row(name)
    r = ac.ROWS[name]
    if r["pidx"] is None and not r["stats"]:             # the set that samples wholly outside the image: +0 bit for bit
        assert not bool(_bits(got[len(r["params"]) + ac.OUTSIDE]).any())


@pytest.mark.parametrize("name", [n for n in ac.ROWS if n.endswith("_nan")])
def test_general_mode_nan_masks(name):
    run_row(name)


def test_grid_stride_second_trip():
    """4100 sources of 26 x 30 -> 24 x 25 in one arena with gaps: the launcher gives each 2 workgroups = 512 threads for 600 pixels; both tables
    through ramnet_fill_pointer_table (33 chunks)"""
    name = "big"
    r = ac.ROWS[name]
    L = Launch(r, ac.sources(name), arena=True, through_kernel=True)
    got = L.run()
    check(r, got, ac.expected(name), name)


def test_nhwc_is_the_packed_nchw():
    """the NHWC destination against ops.pack_input of the NCHW destination of the same launch"""
    from rpg_ramnet_amd import ops
    for name in ("x_s2_c2_nhwc4", "g_s3_c5_nhwc8"):
        r = ac.ROWS[name]
        a = Launch(r, ac.sources(name)).run().view(r["G"], r["th"], r["tw"], r["Cpad"])
        b = Launch(dict(r, nhwc=False, Cpad=0), ac.sources(name)).run().view(r["G"], r["C"], r["th"], r["tw"])
        packed = ops.pack_input(b.to("cuda:0"), torch.device("cuda:0")).cpu()
        assert r["Cpad"] == (r["C"] + 3) // 4 * 4 and torch.equal(_bits(packed), _bits(a))


# ------------------------------------------------------------------------------------------------ the clamps
@pytest.mark.parametrize("name", ["x_s2_c2_nhwc4", "x_s3_c5_nchw", "g_s2_c2_nhwc4"])
def test_window_clamp(name):
    """a device `win` whose top / left lie outside the image: with win_host NULL the clamped window (the NaN guards of the sources hold);
    with win_host given the launch is refused"""
    base = ac.ROWS[name]
    H, W, th, tw = base["H"], base["W"], base["th"], base["tw"]
    away = [(-5, 1000), (999, -1), (-(2 ** 30), -7), (H - th + 1, W - tw + 1), (2 ** 30, 2 ** 30)]
    params = [(t, *away[k % len(away)], ex, fl) for k, (t, _, _, ex, fl) in enumerate(base["params"])]
    r = dict(base, params=params)
    srcs = ac.sources(name)
    got = Launch(r, srcs, win_host=None).run()
    exp = ac.expected_of(r, srcs)
    check(r, got, exp, name + ", windows outside")
    clamped = dict(base, params=[(t, *ar.clamp_window(top, left, H, W, th, tw), ex, fl) for t, top, left, ex, fl in params])
    again = Launch(clamped, srcs).run()
    assert torch.equal(_bits(again), _bits(got))
    Launch(r, srcs).run(rc=BADARG)
    for k in range(len(params)):                          # one bad window in the host copy is enough
        host = [[top, left, ex, fl] for _, top, left, ex, fl in clamped["params"]]
        host[k][k % 2] = -1 if k % 4 < 2 else [H - th, W - tw][k % 2] + 1
        Launch(clamped, srcs, win_host=host).run(rc=BADARG)


@pytest.mark.parametrize("name", ["x_s4_c2_nchw", "g_s2_c2_nchw_skew"])
def test_pidx_clamp(name):
    """entries of pidx out of range use the first / the last set"""
    base = ac.ROWS[name]
    P = len(base["params"])
    r = dict(base, pidx=[-1, P, -(2 ** 31), 2 ** 31 - 1, P - 1, 0][:base["G"]] + [1] * max(0, base["G"] - 6))
    srcs = ac.sources(name)
    got = Launch(r, srcs).run()
    check(r, got, ac.expected_of(r, srcs), name + ", pidx out of range")
    sets = {ac.set_of(r, g) for g in range(r["G"])}
    assert 0 in sets and P - 1 in sets


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_checks():
    """RAMNET_E_BADARG, the message, nothing launched: every destination as it was"""
    for name in ("x_s2_c2_nhwc4", "x_s4_c5_nhwc8", "g_s4_c2_nchw"):
        r = ac.ROWS[name]
        srcs = ac.sources(name)
        bad = [dict(th=r["H"] + 1), dict(tw=r["W"] + 1), dict(th=0), dict(C=0)]
        if r["nhwc"]:
            bad += [dict(Cpad=r["C"] - 1), dict(Cpad=r["C"] // 4 * 4), dict(Cpad=6), dict(Cpad=r["Cpad"] + 2)]        # Cpad < C (also as a multiple of 4), Cpad % 4 != 0
        for change in bad:
            L = Launch(r, srcs)
            for k, v in change.items():
                L.args[{"C": 12, "H": 13, "W": 14, "th": 15, "tw": 16, "Cpad": 17}[k]] = v
            L.run(rc=BADARG)
        for pos in (1, 2, 4, 5, 8, 9):                    # NULL src / dst tables, theta, win, bx, by
            L = Launch(r, srcs)
            L.args[pos] = None
            call(*L.args, rc=BADARG)
            L.untouched()
        for n_params in (0, -1):
            L = Launch(r, srcs, n_params=n_params)
            L.run(rc=BADARG)
        L = Launch(r, srcs)
        L.args[10] = -1
        L.run(rc=BADARG)


def test_no_tensors_is_a_no_op():
    r = ac.ROWS["x_s2_c2_nhwc4"]
    L = Launch(r, ac.sources("x_s2_c2_nhwc4"))
    L.args[10] = 0
    call(*L.args)
    L.untouched()
    L.args[1] = L.args[2] = None
    call(*L.args)
    L.untouched()
