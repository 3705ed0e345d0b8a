"""GPU: the batched multi-scale gradient loss of csrc/grad_loss.hip (`ramnet_grad_loss_stats`, `ramnet_grad_loss_from_stats`,
`ramnet_grad_loss_bwd`, `ramnet_fill_pointer_table`) and `ramnet_cat_batch_add` / `_masked`, every launch alone through the C ABI with raw
pointers, element by element against the float64 statement of tests/grad_loss_restatement.py on the rows of tests/grad_loss_cases.py (both
anchored on the CPU by tests/test_grad_loss_restatement_cpu.py).

Every launch goes through `call` (tests/guarded.py): every pair's prediction and target in its own buffer between NaN guards, the pointer
tables frozen between sentinel guards (written by a host copy or through ramnet_fill_pointer_table, alternating by row), the workspace of
exactly the stated size prefilled with NaN between guards, `dpred`, `stats`, `loss` and `wsum` prefilled with the sentinel.
Rules (profiles/grad_loss_augment_tests_notes.md §1):
  exact      integer rows: (S_s, C_s) equal the statement's; the loss within one fp32 rounding of it; the gradient, from counts CHOSEN by
             the test (the statement's + 5), within 5 x 2^-24 x the adjoint on absolute values (the coefficient once from double, the
             product once, three adds), and +0 bit for bit where that adjoint is 0 (under a NaN cell, cropped rows and columns);
  bit        misaligned bases against the aligned run; the other pairs of a launch with and without a pair whose scale is empty;
  derived    the normal row: sums within (2 s + 5) 2^-24 x the responses on absolute values + the double accumulation, counts exact, the
             gradient where no response within reach lies within its own bound of zero (the CPU file caps the excluded share).
No bound is taken from the kernels under test."""
import ctypes as C
import functools

import pytest
import torch

from rpg_ramnet_amd import _hip
import grad_loss_cases as gc
import grad_loss_restatement as gr
from guarded import BADARG, F64, SENT, U, In, Out, _bits, assert_bits, assert_within, call, pointer_table

pytestmark = pytest.mark.gpu

E64 = 2.0 ** -53
NAN = float("nan")


def last_kernel():
    return _hip.lib().ramnet_last_kernel().decode()


def d64(t):
    return In(t.reshape(-1), dtype=F64)


def f32t(vals):
    return torch.tensor(vals, dtype=torch.float32).to(F64)


def row(name):
    G, B, H, W, ns, _, _ = gc.ROWS[name]
    return G, B, H, W, ns


def tables(name, skew=0):
    """the pairs of a row on the device, each map in a buffer of its own, and the two pointer tables (one spare entry behind them)"""
    preds, targets = gc.data(name)
    pin, tin = [In(p.reshape(-1), skew=skew) for p in preds], [In(t.reshape(-1), skew=skew) for t in targets]
    through = sorted(gc.ROWS).index(name) % 2 == 1
    return pointer_table(pin, through, tail=1), pointer_table(tin, through, tail=1), (pin, tin)


def given_counts(name):
    """the counts the backward pass is handed: the statement's + 5, and 0 where a scale is empty"""
    c = gc.statement(name)[0][:, :, 1]
    return torch.where(c > 0, c + 5.0, c)


@functools.lru_cache(maxsize=None)
def unit_backward(name):
    """per pair (dpred, the adjoint on absolute values) of the statement at factor 1 with the given counts"""
    preds, targets = gc.data(name)
    ns, counts = gc.ROWS[name][4], given_counts(name)
    return [gr.backward(p, t, ns, counts[g], 1.0) for g, (p, t) in enumerate(zip(preds, targets))]


def workspace(G, B, H, W):
    nbytes = int(_hip.lib().ramnet_grad_loss_workspace(G, B, H, W))
    assert nbytes == gr.workspace_bytes(G, B, H, W) and nbytes % 8 == 0
    return Out(1, nbytes // 8, dtype=F64, prefill=torch.full((nbytes // 8,), NAN, dtype=F64))


def run_stats(name, skew=0, weights=None, loss=True, wsum=True, tabs=None):
    """-> (stats [G][ns][2], loss [G] or None, wsum or None) as the device left them"""
    G, B, H, W, ns = row(name)
    ptab, ttab, keep = tabs or tables(name, skew)
    ws, st = workspace(G, B, H, W), Out(1, G * ns * 2, dtype=F64)
    lo, wsu = Out(1, G) if loss else None, Out(1, 1) if wsum else None
    call("ramnet_grad_loss_stats", ptab, ttab, G, B, H, W, ns, ws, st, None if weights is None else In(weights), lo, wsu)
    assert last_kernel() == "gl_stats_kernel + gl_join_kernel"
    assert not bool(torch.isnan(ws.value()).any()), "%s: a slot of the workspace was read or left before it was written" % name
    for o in (ptab, ttab):
        o._host = None
        o.check("ramnet_grad_loss_stats")
    return st.value().view(G, ns, 2), None if lo is None else lo.value().view(-1), None if wsu is None else wsu.value().view(-1)


def check_stats(name, st):
    ref, ab = gc.statement(name)
    assert float(ab.max()) * 512 < 2 ** 53 and torch.equal(ref * 512, (ref * 512).round()), "%s: the case is not exact" % name
    bad = st != ref
    assert not bool(bad.any()), "%s: (S_s, C_s) differ at (pair, scale, which) %s: %r != %r" % (name, bad.nonzero()[0].tolist(), st[bad][:4].tolist(), ref[bad][:4].tolist())


def check_loss(name, st_ref, Bg, weights, loss, wsum, what):
    G = st_ref.shape[0]
    ref = gr.loss_from_stats(st_ref, Bg, torch.ones(G, dtype=F64) if weights is None else weights)
    if loss is not None:
        assert not bool((loss == SENT).any())
        assert torch.equal(torch.isnan(loss), torch.isnan(ref)), "%s: NaN losses %r, statement %r" % (what, loss.tolist(), ref.tolist())
        ok = ~torch.isnan(ref)
        assert_within(loss[ok], ref[ok], (U + 16 * E64) * ref[ok].abs(), what + " loss")
    if wsum is not None:
        assert loss is not None
        total = loss.double().sum()                    # the sum of the fp32 losses in double, rounded once (NaN when a pair's loss is)
        if bool(torch.isnan(total)):
            assert bool(torch.isnan(wsum).all()), "%s: wsum %r although a loss is NaN" % (what, wsum.tolist())
        else:
            assert_within(wsum, total.view(1), ((U + G * E64) * loss.double().abs().sum()).view(1), what + " wsum")


def run_bwd(name, skew=0, skew_out=0, weights=None, up=None, up_sum=None, Bg=None, Bg_dev=None, gain=1.0, counts=None, tabs=None):
    """-> dpred [G][B][H][W] as the device left it (every element written), and the factor of every pair"""
    G, B, H, W, ns = row(name)
    ptab, ttab, keep = tabs or tables(name, skew)
    counts = given_counts(name) if counts is None else counts
    st = gc.statement(name)[0].clone()
    st[:, :, 1] = counts
    dp = Out(1, G * B * H * W, skew=skew_out)
    call("ramnet_grad_loss_bwd", ptab, ttab, G, B, H, W, ns, d64(st), 0.0 if Bg is None else float(Bg), None if Bg_dev is None else d64(torch.tensor([float(Bg_dev)], dtype=F64)),
         float(gain), None if weights is None else In(weights), None if up is None else In(up), None if up_sum is None else In(torch.tensor([up_sum], dtype=F64)), dp)
    assert last_kernel() == "gl_bwd_kernel"
    got = dp.value().view(G, B, H, W)
    kept = got == SENT
    assert not bool(kept.any()), "%s: %d of %d elements of dpred keep their sentinel, first at %s" % (name, int(kept.sum()), kept.numel(), kept.nonzero()[0].tolist())
    one = torch.ones(G, dtype=F64)
    factor = ((0 * one if up is None else up) + (0.0 if up_sum is None else up_sum)) * (one if weights is None else weights) * gain * (Bg if Bg_dev is None else Bg_dev) * 2.0
    return got, factor


def check_bwd(name, got, factor, what, keep=None):
    """keep: [G][B][H][W] bool, the pixels compared (all of them when None)"""
    worst = 0.0
    for g, (grad, agrad) in enumerate(unit_backward(name)):
        ref, aref = grad * float(factor[g]), agrad * abs(float(factor[g]))
        k = torch.ones_like(ref, dtype=torch.bool) if keep is None else keep[g]
        err, bound = (got[g][k].double() - ref[k]).abs(), gr.grad_bound(aref)[k]
        ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        assert bool((err <= bound).all()) and bool(torch.isfinite(got[g]).all()), "%s dpred[%d]: error %.3f x its bound" % (what, g, ratio)
        worst = max(worst, ratio)
        zero = (aref == 0) & k
        assert_bits(got[g][zero], torch.zeros(int(zero.sum()), dtype=F64), "%s dpred[%d] where nothing arrives (NaN cells, cropped rows / columns)" % (what, g))
        assert bool((aref[torch.isnan(gc.data(name)[1][g])] == 0).all())
    print("%s dpred: max err / bound %.3f over %d pairs" % (what, worst, len(factor)))


def default_args(name):
    G = gc.ROWS[name][0]
    gen = torch.Generator().manual_seed(5)
    weights = (torch.randint(1, 9, (G,), generator=gen).to(F64) / 4.0) if sorted(gc.ROWS).index(name) % 3 else None
    up = (torch.randn(G, generator=gen).float().to(F64) + 2.0).float().to(F64).abs()
    neg = torch.arange(G) % 3 == (2 if G > 1 else sorted(gc.ROWS).index(name) % 3)         # negative upstream gradients: -0 must not come out where nothing arrives
    return weights, torch.where(neg, -up, up)


# ------------------------------------------------------------------------------------------------ the integer rows
@pytest.mark.parametrize("name", [n for n in gc.INT_ROWS if not n.startswith("empty")])
def test_exact_rows(name):
    G, B, H, W, ns = row(name)
    weights, up = default_args(name)
    tabs = tables(name)
    st, loss, wsum = run_stats(name, weights=weights, tabs=tabs)
    check_stats(name, st)
    check_loss(name, gc.statement(name)[0], B, weights, loss, wsum, name)
    got, factor = run_bwd(name, weights=weights, up=up, Bg=B, tabs=tabs)
    check_bwd(name, got, factor, name)


@pytest.mark.parametrize("which", ["inputs", "dpred", "both"])
def test_misaligned_bases(which):
    """W % 4 == 0 with the bases of pred / target one float off the 16-byte alignment (the scalar loads) and with dpred one float off (the
    scalar stores): the bits of the aligned run"""
    name = "m72x136"
    G, B, H, W, ns = row(name)
    assert W % 4 == 0
    weights, up = default_args(name)
    si, so = int(which != "dpred"), int(which != "inputs")
    st0, loss0, _ = run_stats(name, weights=weights)
    got0, factor = run_bwd(name, weights=weights, up=up, Bg=B)
    st1, loss1, _ = run_stats(name, skew=si, weights=weights)
    got1, _ = run_bwd(name, skew=si, skew_out=so, weights=weights, up=up, Bg=B)
    check_stats(name, st1)
    check_bwd(name, got1, factor, "%s, misaligned %s," % (name, which))
    assert torch.equal(_bits(st1), _bits(st0)) and torch.equal(_bits(loss1), _bits(loss0)) and torch.equal(_bits(got1), _bits(got0))


VARIANTS = {
    "up": dict(up=True), "up_sum": dict(up_sum=0.625), "both": dict(up=True, up_sum=-1.25), "weights": dict(up=True, weights=True),
    "Bg_dev": dict(up=True, Bg_dev=7.0), "Bg_host": dict(up=True, Bg=5.0), "gain": dict(up_sum=1.0, gain=0.3), "all": dict(up=True, up_sum=0.5, weights=True, Bg_dev=2.0, gain=-1.7),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["sample", "m63x66_ns2"])
def test_backward_arguments(name, variant):
    """up alone, up_sum alone, both; weights NULL and given; Bg on the host and Bg_dev (with a host Bg that must then be ignored); gain != 1"""
    G, B, H, W, ns = row(name)
    v = dict(VARIANTS[variant])
    if v.pop("up", False):
        v["up"] = f32t([1.5, -0.3, 0.7][:G])
    if v.pop("weights", False):
        v["weights"] = f32t([0.5, 1.25, 3.0][:G])
    if "Bg_dev" in v:
        v["Bg"] = -1.0
    elif "Bg" not in v:
        v["Bg"] = float(B)
    got, factor = run_bwd(name, **v)
    check_bwd(name, got, factor, "%s[%s]" % (name, variant))


@pytest.mark.parametrize("variant", ["plain", "weights", "no_loss", "no_wsum", "from_stats", "from_stats_dev"])
def test_loss_arguments(variant):
    """weights NULL and given, loss NULL, wsum NULL; the from-stats entry with Bg on the host and on the device"""
    name = "sample"
    G, B, H, W, ns = row(name)
    ref = gc.statement(name)[0]
    weights = f32t([0.5, 1.25, 3.0]) if variant != "plain" else None
    if variant.startswith("from_stats"):
        dev = variant.endswith("dev")
        for with_wsum in (True, False):
            lo, wsu = Out(1, G), Out(1, 1) if with_wsum else None
            call("ramnet_grad_loss_from_stats", d64(ref), G, ns, -3.0 if dev else 6.0, d64(torch.tensor([11.0], dtype=F64)) if dev else None, In(weights), lo, wsu)
            check_loss(name, ref, 11.0 if dev else 6.0, weights, lo.value().view(-1), wsu.value().view(-1) if with_wsum else None, "from_stats")
        return
    st, loss, wsum = run_stats(name, weights=weights, loss=variant != "no_loss", wsum=variant not in ("no_loss", "no_wsum"))
    check_stats(name, st)
    check_loss(name, ref, B, weights, loss, wsum, "%s[%s]" % (name, variant))


def test_many_pairs_loss_from_stats():
    """70 pairs through the from-stats entry: the second trip of the loss kernel's loop over pairs, and wsum over more than a wave"""
    name = "g70"
    G, B, H, W, ns = row(name)
    ref = gc.statement(name)[0]
    weights = (torch.arange(G, dtype=F64) % 5 + 1) / 4
    lo, wsu = Out(1, G), Out(1, 1)
    call("ramnet_grad_loss_from_stats", d64(ref), G, ns, 3.0, None, In(weights), lo, wsu)
    check_loss(name, ref, 3.0, weights, lo.value().view(-1), wsu.value().view(-1), "from_stats g70")


def test_empty_scale():
    """A pair with a scale that has no valid component: its loss (and wsum) NaN, the statistics, losses and gradients of the other pairs
    bit-equal to the launch without it; its own gradient finite, the statement's with that scale's coefficient 0."""
    G, B, H, W, ns = row("empty")
    weights, up = default_args("empty")
    out = {}
    for name in ("empty", "empty_without"):
        st, loss, wsum = run_stats(name, weights=weights)
        check_stats(name, st)
        check_loss(name, gc.statement(name)[0], B, weights, loss, wsum, name)
        got, factor = run_bwd(name, weights=weights, up=up, Bg=B)
        assert bool((given_counts(name) == 0).any()) == (name == "empty")
        assert bool(torch.isfinite(got).all())
        check_bwd(name, got, factor, name)
        out[name] = (st, loss, wsum, got)
    a, b = out["empty"], out["empty_without"]
    assert bool(torch.isnan(a[1][1])) and bool(torch.isnan(a[2]).all()) and not bool(torch.isnan(b[2]).any())
    for g in (0, 2):
        assert torch.equal(_bits(a[0][g]), _bits(b[0][g])) and torch.equal(_bits(a[1][g:g + 1]), _bits(b[1][g:g + 1])) and torch.equal(_bits(a[3][g]), _bits(b[3][g]))


def test_normal_row():
    name = "normal"
    G, B, H, W, ns = row(name)
    (p,), (t,) = gc.data(name)
    tabs = tables(name)
    st, loss, _ = run_stats(name, tabs=tabs)
    ref, _ = gc.statement(name)
    bounds = []
    for s, (g, ok, bound) in enumerate(gr.response_bounds(p, t, ns)):
        bounds.append(bound.sum() + 2.0 * float(ok.sum()) * E64 * g.abs().sum())
    bounds = torch.stack(bounds)
    assert torch.equal(st[0, :, 1], ref[0, :, 1]), "normal row: counts %r != %r" % (st[0, :, 1].tolist(), ref[0, :, 1].tolist())
    assert_within(st[0, :, 0], ref[0, :, 0], bounds, "normal row S_s")
    lref = gr.loss_from_stats(ref, B)
    assert_within(loss, lref, (bounds / ref[0, :, 1] * B * 2.0).mean().view(1) + (U + 16 * E64) * lref.abs(), "normal row loss")
    up = f32t([1.5])
    got, factor = run_bwd(name, up=up, Bg=B, tabs=tabs)
    keep = ~gr.unsafe_pixels(p, t, ns)
    print("normal row: %d of %d pixels compared" % (int(keep.sum()), keep.numel()))
    check_bwd(name, got, factor, name, keep=keep[None])


# ------------------------------------------------------------------------------------------------ arguments
def refused(args, outs, rc=BADARG):
    """the return code, the message, and every output as it was (guards, gaps and body)"""
    call(*args, rc=rc, defer=True)
    torch.cuda.synchronize()
    if rc:
        assert b"bad argument" in _hip.lib().ramnet_last_error(), _hip.lib().ramnet_last_error()
    for o in outs:
        o._host = None
        o.check(args[0], untouched=True)


def _stats_args(name):
    G, B, H, W, ns = row(name)
    ptab, ttab, keep = tables(name)
    outs = [workspace(G, B, H, W), Out(1, G * ns * 2, dtype=F64), Out(1, G), Out(1, 1)]
    return ["ramnet_grad_loss_stats", ptab, ttab, G, B, H, W, ns, outs[0], outs[1], None, outs[2], outs[3]], outs, keep


def _bwd_args(name):
    G, B, H, W, ns = row(name)
    ptab, ttab, keep = tables(name)
    dp = Out(1, G * B * H * W)
    st = d64(gc.statement(name)[0])
    return ["ramnet_grad_loss_bwd", ptab, ttab, G, B, H, W, ns, st, float(B), None, 1.0, None, In(torch.ones(G)), None, dp], [dp], (keep, st)


def test_argument_checks():
    """RAMNET_E_BADARG, the message, nothing launched: workspace, stats, loss, wsum and dpred as they were"""
    name = "m8x21"                                          # 8 x 21 at 4 scales; 7 rows would leave the coarsest level empty
    for pos, bad in ((7, 0), (7, 5), (5, 7), (6, 7), (1, None), (2, None), (8, None), (9, None), (3, -1), (4, 0)):
        args, outs, keep = _stats_args(name)
        args[pos] = bad
        refused(args, outs)
    for pos in (8, 9):                                      # a workspace / stats that is 4 bytes off the 8-byte alignment
        args, outs, keep = _stats_args(name)
        args[pos] = args[pos].ptr + 4
        refused(args, outs)
    for pos, bad in ((7, 0), (7, 5), (5, 7), (6, 7), (1, None), (2, None), (8, None), (15, None), (13, None), (9, 0.0), (9, -1.0)):
        args, outs, keep = _bwd_args(name)                  # 13: up = NULL with up_sum = NULL; 9: Bg <= 0 without Bg_dev
        args[pos] = bad
        refused(args, outs)
    G, B, H, W, ns = row(name)
    st = d64(gc.statement(name)[0])
    for pos, bad in ((2, -1), (2, 70000), (3, 0), (3, 5), (4, 0.0), (4, -2.0), (1, None), (7, None)):
        lo, wsu = Out(1, G), Out(1, 1)
        args = ["ramnet_grad_loss_from_stats", st, G, ns, float(B), None, None, lo, wsu]
        args[pos] = bad
        refused(args, [lo, wsu])


def test_no_pairs_is_a_no_op():
    """G = 0: success, nothing touched (NULL tables are then fine)"""
    args, outs, keep = _stats_args("m8x21")
    args[1], args[2], args[3] = None, None, 0
    refused(args, outs, rc=0)
    args, outs, keep = _bwd_args("m8x21")
    args[1], args[2], args[3] = None, None, 0
    refused(args, outs, rc=0)
    lo, wsu = Out(1, 3), Out(1, 1)
    refused(["ramnet_grad_loss_from_stats", None, 0, 4, 1.0, None, None, lo, wsu], [lo, wsu], rc=0)


# ------------------------------------------------------------------------------------------------ the pointer table
@pytest.mark.parametrize("n", [0, 1, 127, 128, 129, 300])
def test_fill_pointer_table(n):
    """chunks of 128 by kernel argument: the table bit for bit, the tail beyond n and the guards untouched"""
    ptrs = [0x7F0000000000 + 0x1010 * k + 8 for k in range(n)]
    tab = Out(1, n + 200, dtype=torch.int64)
    arr = (C.c_void_p * max(n, 1))(*ptrs)
    call("ramnet_fill_pointer_table", tab, arr, n)
    assert torch.equal(tab.value().view(-1), torch.cat([torch.tensor(ptrs, dtype=torch.int64), tab.before[tab.off + n:tab.off + n + 200]]))
    if n:
        for pos, bad in ((1, None), (2, None), (3, -1)):
            tab = Out(1, n + 200, dtype=torch.int64)
            args = ["ramnet_fill_pointer_table", tab, arr, n]
            args[pos] = bad
            refused(args, [tab])


# ------------------------------------------------------------------------------------------------ cat_batch_add
MASK_SPECIALS = [0.0, -0.0, -1.5, 1e-40, NAN, 2.0, float("inf"), -float("inf")]


def _cat_case(n, npix, C_, ld, seed):
    gen = torch.Generator().manual_seed(seed)
    parts = [torch.randn(npix, C_, generator=gen).to(F64) for _ in range(n)]
    base = torch.randn(n * npix, C_, generator=gen).to(F64)
    mask = torch.randn(n * npix, C_, generator=gen).to(F64)
    flat = mask.view(-1)
    for k, v in enumerate(MASK_SPECIALS):
        flat[(k * 5) % flat.numel()] = v
    return parts, base, mask


@pytest.mark.parametrize("npix", [1, 3, 1027])
@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_cat_batch_add(n, npix):
    """out = cat(parts) [+ base] in fp32, bit for bit; masked: a SELECT on mask > 0 (+0, -0, a negative, a denormal, NaN, +-inf in the mask;
    NaN and inf in the gradient where the mask drops it: the output there is +0, which a product with (mask > 0) would not give)"""
    for C_ in (4, 12):
        for ld, col0 in ((C_, 0), (C_ + 8, 4)):
            parts, base, mask = _cat_case(n, npix, C_, ld, 40 + n + npix + C_ + ld)
            for with_base in (False, True):
                ins = [In(p, ld=ld, col0=col0) for p in parts]
                arr = (C.c_void_p * 8)(*[i.ptr for i in ins])
                ref = torch.cat(parts).float().to(F64)
                if with_base:
                    ref = (ref + base).float().to(F64)
                out = Out(1, n * npix * C_)
                call("ramnet_cat_batch_add", arr, n, npix, C_, ld, In(base) if with_base else None, out)
                assert_bits(out.value().view(n * npix, C_), ref, "cat_batch_add n=%d npix=%d C=%d ld=%d base=%d" % (n, npix, C_, ld, with_base))
                keepm = mask > 0                                        # NaN: false
                dirty = [p.clone() for p in parts]
                cat_keep = keepm.view(n, npix, C_)
                for k, p in enumerate(dirty):                           # what the mask drops is NaN, +inf or -inf by turns
                    drop = ~cat_keep[k]
                    p[drop] = torch.tensor([NAN, float("inf"), -float("inf")], dtype=F64)[torch.arange(int(drop.sum())) % 3]
                ins = [In(p, ld=ld, col0=col0) for p in dirty]
                arr = (C.c_void_p * 8)(*[i.ptr for i in ins])
                out = Out(1, n * npix * C_)
                call("ramnet_cat_batch_add_masked", arr, n, npix, C_, ld, In(base) if with_base else None, In(mask), out)
                got = out.value().view(n * npix, C_)
                assert_bits(got[keepm], ref[keepm], "cat_batch_add_masked, kept")
                assert not bool(_bits(got[~keepm]).any()), "cat_batch_add_masked: +0 under a non-positive or NaN mask, whatever the gradient holds"
                assert 0 < int(keepm.sum()) and (n * npix * C_ < 40 or int((~keepm).sum()) >= 5)


def test_cat_batch_add_refuses():
    npix, C_ = 3, 8
    data = torch.ones(npix, C_, dtype=F64)
    ins = [In(data) for _ in range(9)]
    ok = (C.c_void_p * 9)(*[i.ptr for i in ins])
    off = (C.c_void_p * 9)(*[i.ptr + 4 * (k == 1) for k, i in enumerate(ins)])
    mask = In(torch.ones(9 * npix, C_))
    for masked in (False, True):
        for arr, n, c, ld in ((ok, 0, C_, C_), (ok, 9, C_, C_), (ok, 2, 6, 8), (ok, 2, C_, 4), (off, 2, C_, C_), (None, 2, C_, C_)):
            out = Out(1, 9 * npix * C_)
            args = ["ramnet_cat_batch_add_masked", arr, n, npix, c, ld, None, mask, out] if masked else ["ramnet_cat_batch_add", arr, n, npix, c, ld, None, out]
            refused(args, [out])
    out = Out(1, 2 * npix * C_)
    refused(["ramnet_cat_batch_add_masked", ok, 2, npix, C_, C_, None, None, out], [out])
