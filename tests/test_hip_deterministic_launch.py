"""GPU: the joins of the deterministic mode called alone through the C ABI (guarded.call / guarded.call_desc; rows and restatements in
tests/deterministic_cases.py).

Slab forms (ramnet_wgrad_desc.dw_slabs > 0 on RAMNET_ALGO_WINOGRAD24, _WINOGRAD24_2X3, _HEAD and _DIRECT, its parity view included).  Every
row is launched into a zeroed workspace of one slab MORE than ramnet_wgrad_slabs answers, three times afresh and three times into one:
  - every slab has the same bits in the three fresh runs, at least two slabs are non-zero, the slab beyond the count stays +0;
  - three launches into one workspace leave ((0 + p) + p) + p of the fresh slab p, bit for bit (plain read-modify-write);
  - ramnet_reduce_slabs gives the fp32 fold in slab order, bit for bit, and the joined gradient meets the float64 statement at the bound
    the family's own launch test applies (tests/test_hip_fold_head_launch.py, tests/test_hip_conv_launch.py: the number of terms of a sum
    does not depend on the order they are added in, so the bounds hold for the slab order as they do for the atomic one);
  - with dw_slabs = 0 the same descriptor answers through the kernel it always used.
Ordered forms of ramnet_gemm / ramnet_gemm2 (accumulate), ramnet_bias_grad, ramnet_pred_sigmoid_bwd / _linear_bwd and
ramnet_normalize_nonzero[_batch]: the same bits on every launch, the fp32 (fp64) sum of the partial rows in index order, read from the
caller's own partial buffer, bit for bit, and the float64 statement."""
import ctypes as C
import types

import pytest
import torch

import conv_restatement as cr
import deterministic_cases as dc
import fold_head_cases as fh
from guarded import F64, In, Out, _bits, assert_bits, assert_within, call, call_desc
from rpg_ramnet_amd import _hip

pytestmark = pytest.mark.gpu
U = cr.U


def _struct(f):
    s = _hip.WgradDesc()
    for k, v in f.items():
        if isinstance(v, (In, Out)):
            v = v.ptr
        if isinstance(v, list):
            for j, e in enumerate(v):
                getattr(s, k)[j] = e
        else:
            setattr(s, k, v)
    return s


def slab_protocol(fields, one, Cout, want_bias, slab_kernel, default_kernel, want_slabs=None):
    """The slab protocol of one row.  fields: descriptor fields without dw / dbias / dw_slabs; one: floats of a slab.  Returns (dw, dbias) of
    the first fresh run AFTER ramnet_reduce_slabs (slab 0 = the joined gradient) and the slab count."""
    L = _hip.lib()
    S = L.ramnet_wgrad_slabs(C.byref(_struct(fields)))
    assert S >= 2 and (want_slabs is None or S == want_slabs), S

    def launch(dw, dbias, slabs):
        f = dict(fields, dw=dw, dw_slabs=slabs)
        if want_bias:
            f["dbias"] = dbias
        call_desc("ramnet_wgrad_launch", _hip.WgradDesc, f)
        return L.ramnet_last_kernel().decode()

    def fresh():
        return Out(S + 1, one, prefill=torch.zeros(S + 1, one)), (Out(S + 1, Cout, prefill=torch.zeros(S + 1, Cout)) if want_bias else None)

    runs = []
    for _ in range(3):
        dw, dbias = fresh()
        assert launch(dw, dbias, S) == slab_kernel
        runs.append((dw, dbias))
    p, pb = runs[0][0].value(), (runs[0][1].value() if want_bias else None)
    for dw, dbias in runs[1:]:
        assert torch.equal(_bits(dw.value()), _bits(p)), "a slab differs between two launches"
        assert not want_bias or torch.equal(_bits(dbias.value()), _bits(pb)), "a bias slab differs between two launches"
    used = [bool(_bits(p[s]).any()) for s in range(S + 1)]
    assert sum(used[:S]) >= 2 and not used[S], "slabs written: %r" % used            # (on atomics everything lands in slab 0)
    assert not want_bias or (sum(bool(_bits(pb[s]).any()) for s in range(S)) >= 2 and not bool(_bits(pb[S]).any()))
    # three launches into one workspace
    dw, dbias = fresh()
    for _ in range(3):
        launch(dw, dbias, S)
    assert_bits(dw.value(), dc.accumulate(p, 3).double(), "three launches into one workspace")
    if want_bias:
        assert_bits(dbias.value(), dc.accumulate(pb, 3).double(), "three launches into one bias workspace")
    # the ordered join
    dw, dbias = runs[0]
    call("ramnet_reduce_slabs", dw, S, one)
    assert_bits(dw.value()[0], dc.ordered_join(p[:S]).double(), "ramnet_reduce_slabs: the fp32 fold in slab order")
    assert not bool(_bits(dw.value()[1:]).any()), "slabs 1.. must be +0 after the fold"
    if want_bias:
        call("ramnet_reduce_slabs", dbias, S, Cout)
        assert_bits(dbias.value()[0], dc.ordered_join(pb[:S]).double(), "ramnet_reduce_slabs on the bias slabs")
    # dw_slabs = 0: the kernel the descriptor always launched (everything in slab 0, by atomics)
    d0, b0 = fresh()
    assert launch(d0, b0, 0) == default_kernel
    assert not bool(_bits(d0.value()[1:]).any())
    return dw, dbias, S


# ---------------------------------------------------------------------------------------------------- folded decoders
@pytest.mark.parametrize("gm", [False, True], ids=["nomask", "gmask"])
@pytest.mark.parametrize("row", dc.FOLD_ROWS, ids=lambda r: "B%d-%dx%d-%d_%d" % r[:5])
@pytest.mark.parametrize("fam", sorted(dc.FOLD_FAMS))
def test_fold_wgrad_slabs(fam, row, gm):
    B, H, W, C0, Cout, want = row
    d = dc.build_fold(fam, row, gm)
    st = cr.fold_wgrad_statement(d)
    _, fabs, ntiles = cr.fold_wgrad_wino(d, fam)
    NP = 5 * (cr.FOLD_TW[fam] + 3)
    f = dict(x0=In(d.x0, ld=C0 + 4), ld0=C0 + 4, C0=C0, in_mode=_hip.IN_PLAIN, B=B, Hin=H + 4, Win=W + 4, stride=1, dout=In(d.dout, ld=Cout + 4), ldg=Cout + 4,
             Cout=Cout, Ho=H, Wo=W, HoG=2 * H, WoG=2 * W, algo=dc.FOLD_FAMS[fam], ntaps=16, dy=[t[0] for t in cr.fold_taps(0, 0)], dx=[t[1] for t in cr.fold_taps(0, 0)])
    if gm:
        f["gmask"], f["ldgm"] = In(d.gmask, ld=Cout + 8), Cout + 8
    sfx = "_2x3" if fam == "fold2x3" else ""
    targs = "<%d,%d>" % (int(gm), int(Cout % 64 != 0))
    dw, dbias, S = slab_protocol(f, 4 * NP * C0 * Cout, Cout, True, "conv_wgrad_wino24_kernel%s_slab%s" % (sfx, targs), "conv_wgrad_wino24_kernel%s%s" % (sfx, targs), want)
    assert_within(dbias.value()[0], st.dbias, (st.n_bias + 2) * U * st.dbias_abs, "%s slab form dbias" % fam)
    # the library's own unpack of slab 0 onto a non-zero gradient, the other workspaces zero: the bound of test_fold_wgrad
    gold = fh._rn(fh._gen("det_gold%d%d" % (C0, Cout)), (Cout, C0, 5, 5))
    zeros = torch.zeros(4, 16, C0, Cout, dtype=F64)
    zb = torch.zeros(2, 5 * C0, 2 * Cout, dtype=F64)
    grad = Out(1, gold.numel(), prefill=gold.reshape(-1))
    w4, wr, wc = Out(1, zeros.numel(), prefill=zeros.reshape(-1)), Out(1, zb.numel(), prefill=zb.reshape(-1)), Out(1, zb.numel(), prefill=zb.reshape(-1))
    if fam == "fold2x2":
        call("ramnet_fold_unpack_wgrad", w4, dw, wr, wc, grad, Cout, C0, C0)
    else:
        call("ramnet_fold_unpack_wgrad2x3", w4, None, dw, wr, wc, grad, Cout, C0, C0)
    ref = cr.fold_unpack_statement(gold, st.dW4, zeros, zb, zb)
    FA = cr.fold_matrix()
    babs = torch.einsum("ptk,qsl,pqtsio->oikl", FA, FA, ((ntiles + cr.R_WGRAD[fam] + 2) * U * fabs).view(2, 2, 4, 4, C0, Cout))
    assert_within(grad.value(), ref, babs + 2 * U * ref.abs(), "%s gradient after the join and the fold's unpack" % fam)
    assert not bool(_bits(dw.value()).any()), "the workspace must come back +0"


# ---------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("c", dc.HEAD_ROWS, ids=lambda c: c.name)
def test_head_wgrad_slabs(c):
    d = fh.build_head(c)
    st = cr.wgrad_statement(types.SimpleNamespace(**dict(vars(d), taps=[t[:2] for t in d.taps])))
    p = c.pitch
    f = dict(in_mode=_hip.IN_PLAIN, B=c.B, Hin=c.H, Win=c.W, C0=c.C0, ld0=c.C0 + p, x0=In(d.x0_phys, ld=c.C0 + p), stride=1, Cout=c.Cout, Ho=c.H, Wo=c.W,
             algo=_hip.ALGO_HEAD, head_cin=c.cin, dout=In(d.dout, ld=c.Cout + p), ldg=c.Cout + p, ntaps=25, dy=[t[0] for t in fh.HEAD_TAPS], dx=[t[1] for t in fh.HEAD_TAPS])
    if d.gmask is not None:
        f["gmask"], f["ldgm"] = In(d.gmask, ld=c.Cout + p + 4), c.Cout + p + 4
    tiles = -(-c.W // 32) * -(-c.H // 8) * c.B
    dw, dbias, S = slab_protocol(f, 25 * c.C0 * c.Cout, c.Cout, True, "conv_head_wgrad_kernel_slab<%d>" % c.cin, "conv_head_wgrad_kernel<%d>" % c.cin,
                                 min(tiles, dc.SLAB_CAP))
    ref = torch.zeros(25, c.C0, c.Cout, dtype=F64)
    ref[:, :c.cin] = st.dW
    rabs = torch.zeros_like(ref)
    rabs[:, :c.cin] = st.dW_abs
    assert_within(dw.value()[0], ref, (float(st.n.max()) + cr.R_WGRAD["direct"] + 2) * U * rabs, "head slab form dW %s" % c.name)     # (test_head_wgrad)
    assert_within(dbias.value()[0], st.dbias, (st.n_bias + 2) * U * st.dbias_abs, "head slab form dbias %s" % c.name)


# ---------------------------------------------------------------------------------------------------- direct
@pytest.mark.parametrize("name", dc.DIRECT_ROWS)
def test_direct_wgrad_slabs(name):
    d = dc.build_direct(name)
    st = cr.wgrad_statement(d)
    Cin, Cout, T = d.C0 + d.C1, d.Cout, len(d.taps)
    src = d.full if d.gview else d
    f = dict(x0=In(d.x0, ld=d.C0 + 4), ld0=d.C0 + 4, C0=d.C0, C1=d.C1, in_mode=d.in_mode, B=d.B, Hin=d.Hin, Win=d.Win, ntaps=T, stride=d.stride,
             dy=[t[0] for t in d.taps], dx=[t[1] for t in d.taps], dout=In(src.dout, ld=Cout + 4), ldg=Cout + 4, Cout=Cout, Ho=d.Ho, Wo=d.Wo, algo=_hip.ALGO_DIRECT)
    if d.x1 is not None:
        f["x1"], f["ld1"] = In(d.x1, ld=d.C1 + 8), d.C1 + 8
    if src.gmask is not None:
        f["gmask"], f["ldgm"] = In(src.gmask, ld=Cout + 8), Cout + 8
    if d.gview:
        f.update(zip(("gsy", "gsx", "goy", "gox", "HoG", "WoG"), d.gview))
    L = _hip.lib()
    call_desc("ramnet_wgrad_launch", _hip.WgradDesc, dict(f, dw=Out(T * Cin, Cout, prefill=torch.zeros(T * Cin, Cout))))
    default = L.ramnet_last_kernel().decode()
    assert default.startswith("conv_wgrad_kernel<")
    dw, dbias, S = slab_protocol(f, T * Cin * Cout, Cout, True, default.replace("conv_wgrad_kernel<", "conv_wgrad_kernel_slab<"), default)
    bw, bb = cr.wgrad_bound(d, st, "direct")
    assert_within(dw.value()[0], st.dW, bw, "direct slab form dW %s" % name)
    assert_within(dbias.value()[0], st.dbias, bb, "direct slab form dbias %s" % name)


# ---------------------------------------------------------------------------------------------------- ordered skinny GEMM
class _Gemm:
    def __init__(self, M, N, K, batch, trans, seed):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K, self.batch, self.trans = M, N, K, batch, trans
        ar, ac = (K, M) if trans else (M, K)
        self.A, self.B, self.C0 = dc.spread(g, (batch, ar, ac)), dc.spread(g, (batch, K, N)), dc.spread(g, (batch, M, N))
        self.lda, self.sa, self.sb, self.sc = ac, ar * ac, K * N, M * N
        self.a, self.b = In(self.A.reshape(-1, ac)), In(self.B.reshape(-1, N))

    def out(self):
        return Out(self.batch * self.M, self.N, prefill=self.C0.reshape(-1, self.N))

    def judge(self, got, part, ksplit, Mp, Np, what):
        """C = ((C0 + slice 0) + slice 1) + ... in fp32 from the launch's own partial buffer; every slice and the sum against float64"""
        A = self.A.transpose(1, 2) if self.trans else self.A
        kper = -(-(-(-self.K // ksplit)) // 32) * 32
        acc = self.C0.float()
        for ks in range(ksplit):
            sl = part[:, ks, :self.M, :self.N]
            k0, k1 = ks * kper, min(self.K, (ks + 1) * kper)
            ref = A[:, :, k0:k1] @ self.B[:, k0:k1]
            assert_within(sl, ref, (k1 - k0 + 2) * U * (A[:, :, k0:k1].abs() @ self.B[:, k0:k1].abs()), "%s: slice %d" % (what, ks))
            acc = acc + sl
        assert_bits(got.view(self.batch, self.M, self.N), acc.double(), "%s: C0 + the slices in index order, in fp32" % what)
        ref, aref = self.C0 + A @ self.B, self.C0.abs() + A.abs() @ self.B.abs()
        assert_within(got.view(self.batch, self.M, self.N), ref, (self.K + 2 + ksplit + 1) * U * aref, what)        # (the bound of test_gemm under `accumulate`)


@pytest.mark.parametrize("trans", [0, 1])
def test_gemm_ordered(trans):
    L = _hip.lib()
    M, N, K, batch, ksplit = 10, 64, 512, 2, 4
    n = L.ramnet_gemm_partial_floats(M, N, K, batch, 0, 0, 0)
    assert n == batch * ksplit * 32 * 64
    p = _Gemm(M, N, K, batch, trans, 300 + trans)
    outs = []
    for _ in range(3):
        c, part = p.out(), Out(1, n)
        call("ramnet_gemm_ordered", p.a, p.b, c, M, N, K, p.lda, N, N, trans, batch, p.sa, p.sb, p.sc, part)
        outs.append((c.value(), part.dev[part.off:part.off + n].cpu().view(batch, ksplit, 32, 64)))
    for c, _ in outs[1:]:
        assert torch.equal(_bits(c), _bits(outs[0][0])), "ramnet_gemm_ordered differs between two launches"
    p.judge(outs[0][0], outs[0][1], ksplit, 32, 64, "gemm_ordered[trans=%d]" % trans)
    # a launch that does not split (K < 256) needs no buffer and adds to C itself
    q = _Gemm(M, N, 128, batch, trans, 310 + trans)
    assert L.ramnet_gemm_partial_floats(M, N, 128, batch, 0, 0, 0) == 0
    c = q.out()
    call("ramnet_gemm_ordered", q.a, q.b, c, M, N, 128, q.lda, N, N, trans, batch, q.sa, q.sb, q.sc, None)
    A = q.A.transpose(1, 2) if trans else q.A
    assert_within(c.value().view(batch, M, N), q.C0 + A @ q.B, (128 + 4) * U * (q.C0.abs() + A.abs() @ q.B.abs()), "gemm_ordered without a split")


@pytest.mark.parametrize("trans", [0, 1])
def test_gemm2_ordered(trans):
    """the pair of a decoder layer's row and column border: two problems of different M and batch in one launch, one partial buffer"""
    L = _hip.lib()
    N, K, ksplit = 64, 512, 4
    p, q = _Gemm(10, N, K, 2, trans, 320 + trans), _Gemm(40, N, K, 1, trans, 330 + trans)
    lda = 40 if trans else K
    if trans:                                       # one leading dimension for both: the narrower A is pitched
        p.a, p.lda, p.sa = In(p.A.reshape(-1, 10), ld=40), 40, K * 40
    n = L.ramnet_gemm_partial_floats(10, N, K, 2, 40, K, 1)
    assert n == 3 * ksplit * 64 * 64
    outs = []
    for _ in range(3):
        c1, c2, part = p.out(), q.out(), Out(1, n)
        call("ramnet_gemm2_ordered", p.a, p.b, c1, 10, p.sa, p.sb, p.sc, 2, q.a, q.b, c2, 40, q.sa, q.sb, q.sc, 1, N, K, K, lda, N, N, trans, part)
        outs.append((c1.value(), c2.value(), part.dev[part.off:part.off + n].cpu().view(3, ksplit, 64, 64)))
    for c1, c2, _ in outs[1:]:
        assert torch.equal(_bits(c1), _bits(outs[0][0])) and torch.equal(_bits(c2), _bits(outs[0][1])), "ramnet_gemm2_ordered differs between two launches"
    p.judge(outs[0][0], outs[0][2][:2], ksplit, 64, 64, "gemm2_ordered first product")
    q.judge(outs[0][1], outs[0][2][2:], ksplit, 64, 64, "gemm2_ordered second product")


# ---------------------------------------------------------------------------------------------------- the other ordered joins
def _part(buf, n):
    return buf.dev[buf.off:buf.off + n].cpu()


@pytest.mark.parametrize("C_,masked", [(32, True), (12, False)])
def test_bias_grad_ordered(C_, masked):
    """db += the 256 workgroup rows in index order (fp32, from the partial buffer); npix x C terms of 25 binades, so the order of a sum shows.
    Against float64: a sum of npix terms in any order is within (npix - 1) U of the sum of the absolute values; + the rounding of the +=."""
    L = _hip.lib()
    npix = 3 * 12 * 20 + 5
    g = torch.Generator().manual_seed(400 + C_)
    dy, mask, db0 = dc.spread(g, (npix, C_)), (torch.randn(npix, C_, generator=g).to(F64) if masked else None), dc.spread(g, (C_,))
    n = L.ramnet_bias_grad_partial_floats(C_)
    assert n == 256 * C_
    outs = []
    for _ in range(3):
        db, part = Out(1, C_, prefill=db0), Out(1, n)
        call("ramnet_bias_grad_ordered", In(dy), In(mask) if masked else None, db, npix, C_, part)
        outs.append((db.value()[0], _part(part, n).view(256, C_)))
    for db, _ in outs[1:]:
        assert torch.equal(_bits(db), _bits(outs[0][0])), "ramnet_bias_grad_ordered differs between two launches"
    acc = db0.float()
    for r in range(256):
        acc = acc + outs[0][1][r]
    assert_bits(outs[0][0], acc.double(), "bias_grad_ordered: db + the rows in workgroup order")
    t = dy * (mask > 0).to(F64) if masked else dy
    assert_within(outs[0][0], db0 + t.sum(0), (npix + 2) * U * (db0.abs() + t.abs().sum(0)), "bias_grad_ordered")


@pytest.mark.parametrize("sig", [True, False], ids=["sigmoid", "linear"])
def test_pred_bwd_ordered(sig):
    """dw / db += the workgroup rows in index order (from the partial buffer), dx as the atomic form writes it; against float64 as above,
    with the dz the kernel itself forms (dy y (1 - y): two roundings, inside the + 2)"""
    L = _hip.lib()
    npix, C_ = 3 * 12 * 20 + 5, 32
    g = torch.Generator().manual_seed(410 + int(sig))
    x, w, dy = dc.spread(g, (npix, C_)), dc.spread(g, (C_,)), dc.spread(g, (npix,))
    y = torch.rand(npix, generator=g).float().to(F64)
    dw0, db0 = dc.spread(g, (C_,)), dc.spread(g, (1,))
    n = L.ramnet_pred_bwd_partial_floats()
    rows = min(512, -(-npix * 8 // 256))
    outs = []
    for ordered in (True, True, True, False):
        dw, db, dx, part = Out(1, C_, prefill=dw0), Out(1, 1, prefill=db0), Out(npix, C_), Out(1, n)
        tail = (part,) if ordered else ()
        if sig:
            call("ramnet_pred_sigmoid_bwd" + ("_ordered" if ordered else ""), In(x), C_, C_, In(w), In(y), In(dy), dx, C_, dw, db, npix, *tail)
        else:
            call("ramnet_pred_linear_bwd" + ("_ordered" if ordered else ""), In(x), C_, C_, In(w), In(dy), dx, C_, dw, db, npix, *tail)
        outs.append((dw.value()[0], db.value()[0], dx.value(), _part(part, n).view(512, 132)))
    for dw, db, dx, _ in outs[1:3]:
        assert torch.equal(_bits(dw), _bits(outs[0][0])) and torch.equal(_bits(db), _bits(outs[0][1])), "the ordered form differs between two launches"
    assert torch.equal(_bits(outs[0][2]), _bits(outs[3][2])), "dx of the ordered form is not the atomic form's"
    accw, accb = dw0.float(), db0.float()
    for r in range(rows):
        accw, accb = accw + outs[0][3][r, :C_], accb + outs[0][3][r, 128]
    assert_bits(outs[0][0], accw.double(), "pred_bwd_ordered: dw + the rows in workgroup order")
    assert_bits(outs[0][1], accb.double(), "pred_bwd_ordered: db + the rows in workgroup order")
    dz = (dy.float() * y.float() * (1.0 - y.float())).to(F64) if sig else dy
    assert_within(outs[0][0], dw0 + (dz[:, None] * x).sum(0), (npix + 3) * U * (dw0.abs() + (dz[:, None] * x).abs().sum(0)), "pred_bwd_ordered dw")
    assert_within(outs[0][1], db0 + dz.sum(), (npix + 3) * U * (db0.abs() + dz.abs().sum()), "pred_bwd_ordered db")


def test_normalize_nonzero_ordered():
    """3 grids of 5 x 12 x 20, one of them all zero, values over 25 binades with two thirds zeroed: statistics (sum, sum of squares, count) =
    the rows of the scratch in workgroup order, in fp64, bit for bit; the same bits on every launch; the normalised grids equal the atomic
    form's wherever both normalise with the same fp32 mean and deviation (the fp64 sums differ in their last bits only)."""
    L = _hip.lib()
    G, n = 3, 5 * 12 * 20
    g = torch.Generator().manual_seed(420)
    grids = dc.spread(g, (G, n)) * (torch.rand(G, n, generator=g) < 1 / 3).to(F64)
    grids[1] = 0.0
    nd = L.ramnet_nonzero_stats_scratch_doubles(G, n)
    rows = nd // (3 * G)
    assert rows == 2
    outs = []
    for _ in range(3):
        buf, stats, scratch = Out(G, n, prefill=grids), Out(G, 3, dtype=F64), Out(1, nd, dtype=F64)
        call("ramnet_normalize_nonzero_batch_ordered", buf, G, n, stats, scratch)
        outs.append((buf.value(), stats.value(), _part(scratch, nd).view(G, rows, 3)))
    for b, s, _ in outs[1:]:
        assert torch.equal(_bits(b), _bits(outs[0][0])) and torch.equal(_bits(s), _bits(outs[0][1])), "the ordered normalisation differs between two launches"
    got, stats, part = outs[0]
    assert torch.equal(_bits(stats), _bits(part[:, 0] + part[:, 1])), "stats = the scratch rows in workgroup order"
    ref = torch.stack([grids.sum(1), (grids * grids).sum(1), (grids != 0).sum(1).to(F64)], 1)
    assert torch.equal(stats[:, 2], ref[:, 2]) and float(stats[1].abs().max()) == 0.0
    assert_within(stats[:, :2], ref[:, :2], n * 2.0 ** -53 * torch.stack([grids.abs().sum(1), (grids * grids).sum(1)], 1), "nonzero statistics (fp64 sums)")
    assert not bool(_bits(got[1]).any()), "an all-zero grid stays as it is"
    for i in (0, 2):                                # the kernel's own fp32 arithmetic on its own statistics (normalize_nonzero_batch_kernel)
        cnt = stats[i, 2]
        mean = (stats[i, 0] / cnt).float()
        sd = torch.sqrt((stats[i, 1] / cnt).float() - mean * mean)
        want = torch.where(grids[i] != 0, (grids[i].float() - mean) / sd, torch.zeros(n))
        # (v - mean) is the same fp32 rounding on both sides; the deviation may differ by one ulp (mean * mean fused into the subtraction or not),
        # the quotient is rounded once: 3 U of the value, loosely
        assert_within(got[i], want.double(), 3 * U * want.double().abs(), "normalised grid %d" % i)
    # the single-grid entry point and the statistics alone: the same statistics, bit for bit
    one, s1, sc1 = Out(1, n, prefill=grids[2]), Out(1, 3, dtype=F64), Out(1, L.ramnet_nonzero_stats_scratch_doubles(1, n), dtype=F64)
    call("ramnet_normalize_nonzero_ordered", one, n, s1, sc1)
    assert torch.equal(_bits(one.value()[0]), _bits(got[2])) and torch.equal(_bits(s1.value()[0]), _bits(stats[2]))
    keep, s3, sc3 = Out(G, n, prefill=grids).freeze(), Out(G, 3, dtype=F64), Out(1, nd, dtype=F64)
    call("ramnet_nonzero_stats_batch_ordered", keep, G, n, s3, sc3)
    assert torch.equal(_bits(s3.value()), _bits(stats))
