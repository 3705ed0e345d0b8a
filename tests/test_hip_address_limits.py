"""GPU: the convolution launches at their 32-bit addressing limits (rows: tests/address_limit_cases.py, held to their limits without a GPU by
tests/test_address_limits_cpu.py; the audit behind them: profiles/address_limit_tests_notes.md).  Every row is launched alone through the C ABI
with its inflated operand in a device-resident guarded buffer (tests/guarded_big.py) that really spans the extent the descriptor names —
the refused siblings too: a missing guard shows as a wrong value or a written gap, never as an access outside an allocation.

"below" rows: the float64 statement of the descriptor (tests/conv_restatement.py), exact on the integer rows, the rules of
tests/test_hip_conv_launch.py on the cell epilogues; the kernel the family requires; guards, gaps and inputs intact.
"refused" rows: RAMNET_E_BADARG and nothing written.

One inflated operand per test, everything freed before the next; a test skips only when the device has less free memory than it needs
plus 4 GB (printed)."""
import ctypes as C
import gc
import time

import pytest
import torch

import address_limit_cases as al
import conv_restatement as cr
import guarded_big as gb
import test_hip_conv_launch as tl
import test_hip_fold_head_launch as tf
from guarded import BADARG, F64, In, Out, _bits, assert_exact, call, call_desc
from rpg_ramnet_amd import _hip

pytestmark = pytest.mark.gpu
SPARE = 4 << 30


@pytest.fixture(autouse=True)
def _free_everything():
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:               # a fault leaves the device unusable for this process: nothing more is launched on it
        pytest.exit("the device reported %s" % e, returncode=3)
    print("peak device memory %.2f GB, %.2f s" % (torch.cuda.max_memory_allocated() / 2 ** 30, time.time() - t0))
    gc.collect()
    torch.cuda.empty_cache()


def room(need):
    free, _ = torch.cuda.mem_get_info()
    if free < need + SPARE:
        print("skipped: %d bytes free, %d + %d needed" % (free, need, SPARE))
        pytest.skip("device memory: %d bytes free, %d + %d needed" % (free, need, SPARE))


class Maker:
    """the buffers of a row: the inflated operand (of every segment) on the device, the others built on the host as everywhere else"""

    def __init__(self, row):
        self.row, self.ins = row, {}

    def inp(self, op, data, ld, seg=0):
        if (op, seg) not in self.ins:
            if op == self.row.operand:
                rows = data.numel() // data.shape[-1]
                if seg == 0:
                    room(gb.nbytes(rows, ld) * getattr(self.row, "nseg", 1))
                self.ins[(op, seg)] = gb.BigIn(data, ld)
            else:
                self.ins[(op, seg)] = In(data, ld=ld)
        return self.ins[(op, seg)]

    def out(self, op, rows, cols, ld, col0, prefill):
        if op == self.row.operand:
            room(gb.nbytes(rows, ld))
            return gb.BigOut(rows, cols, ld, col0, prefill)
        return Out(rows, cols, ld=ld, col0=col0, prefill=prefill)

    def weights(self, d, fam, k):
        return tl.pack(d, fam, k)

    def fold_weights(self, w5, fam, dgrad):
        return tf.pack_fold(w5, fam, dgrad)

    def head_weights(self, d, c):
        wp = Out(1, _hip.lib().ramnet_packed_weight_elems_head(c.cin))
        call("ramnet_pack_weight_head", In(d.w_oihw.reshape(-1)), wp, c.Cout, c.cin)
        return wp.freeze()

    def inputs_intact(self, what):
        for b in self.ins.values():
            if isinstance(b, gb.BigIn):
                b.check(what)


CONV_SIDES = [(r, s) for r, s in al.SIDES if r.launch == "conv"]
WGRAD_SIDES = [(r, s) for r, s in al.SIDES if r.launch == "wgrad"]
FH_SIDES = [(r, s) for r, s in al.SIDES if r in al.FH_ROWS]


def _ids(sides):
    return ["%s-%s" % (r.name, "refused" if s else "below") for r, s in sides]


@pytest.mark.parametrize("row,refused", CONV_SIDES, ids=_ids(CONV_SIDES))
def test_conv_at_its_limit(row, refused):
    L = _hip.lib()
    d = al.conv_build(row)
    mk = Maker(row)
    f, outs = al.conv_fields(row, d, mk, refused)
    what = "%s, %s %d floats apart" % (row.name, row.operand, f[al.LD_FIELD[row.operand]])
    if refused:
        call_desc("ramnet_conv_launch", _hip.ConvDesc, f, rc=BADARG)
        mk.inputs_intact(what)
        return
    call_desc("ramnet_conv_launch", _hip.ConvDesc, f)
    name = L.ramnet_last_kernel().decode()
    tl.judge(row.case, d, cr.conv_statement(d, row.fam), outs, what)
    assert name.startswith(tl.KERNEL[row.fam]), name
    mk.inputs_intact(what)


def _segment_array(per_seg):
    arr = (_hip.WgradSeg * len(per_seg))()
    for k, one in enumerate(per_seg):
        for name, buf in one.items():
            setattr(arr[k], name, buf.ptr)
    return arr


@pytest.mark.parametrize("row,refused", WGRAD_SIDES, ids=_ids(WGRAD_SIDES))
def test_wgrad_at_its_limit(row, refused):
    """atomic form, then the slab form with the library's slab count on the same inputs: dw after the library's fold and unpack and dbias
    against the float64 statement, exact"""
    L = _hip.lib()
    algo, slabs_fn, unpack, kernel = tl.WG_FAMS[row.fam]
    d = al.wgrad_build_all(row)
    st = cr.wgrad_statement(d)
    Cin, Cout = d.Cin, row.Cout
    one = tl._ws_floats(row.fam, Cin, Cout)
    mk = Maker(row)
    for slab_form in (False, True):
        S = getattr(L, slabs_fn)(Cin, Cout) if slab_form else 1
        dw, dbias = Out(S, one, prefill=torch.zeros(S, one)), Out(S, Cout, prefill=torch.zeros(S, Cout))
        f, per_seg = al.wgrad_fields(row, d.segs, mk, dw, dbias, S if slab_form else 0, refused)
        what = "%s, %s %d floats apart, %s form" % (row.name, row.operand, f[al.LD_FIELD[row.operand]], "slab" if slab_form else "atomic")
        if row.nseg > 1:
            arr = _segment_array(per_seg)
            f["nseg"], f["segs"] = row.nseg, C.cast(arr, C.POINTER(_hip.WgradSeg))
        if refused:
            call_desc("ramnet_wgrad_launch", _hip.WgradDesc, f, rc=BADARG)
            mk.inputs_intact(what)
            continue
        call_desc("ramnet_wgrad_launch", _hip.WgradDesc, f)
        assert L.ramnet_last_kernel().decode().startswith(kernel)
        if S > 1:
            call("ramnet_reduce_slabs", dw, S, one)
            call("ramnet_reduce_slabs", dbias, S, Cout)
        assert_exact(dbias.value()[0], st.dbias, "%s dbias" % what, abs_sum=st.dbias_abs)
        grad = Out(1, Cout * Cin * 9, prefill=torch.zeros(Cout * Cin * 9))
        call(unpack, In(dw.value()[0]), grad, Cout, Cin, Cin, Cout, 0)
        ref = cr.unpack_statement(torch.zeros(Cout, Cin, 3, 3, dtype=F64), st.dW, Cout, Cin, 0).reshape(1, -1)
        assert_exact(grad.value(), ref, "%s gradient after its unpack" % what)
        mk.inputs_intact(what)


# ---------------------------------------------------------------------------------------------------- folded decoders and head
def _fold_kernel(row, dgrad):
    """the instantiation a 10 x 12 row must run (csrc/conv_wino24.hip): F(2x2,4x4) by name, F(2x3,4x4) up to its tile columns"""
    pair = int(row.Cout == 32 and row.C0 % 32 == 0 and not dgrad)
    if row.fam == "fold2x2":
        narrow = row.C0 % 32 != 0 and not dgrad          # 32-column workgroups, chunks of 8
        return r"conv_wino24_kernel<%d,%d,%d,%d>" % (2 if narrow else 4, int(dgrad), 8 if narrow else 4, pair)
    return r"conv_wino24_kernel<4,%d,\d+,%d,3%s>" % (int(dgrad), pair, ",1" if row.half else "")


def _fold_wgrad_judge(row, d, st, dw, what):
    """the library's own unpack of this launch's workspace alone (zero direct workspace and border gradients) onto a zero gradient"""
    C0, Cout = row.C0, row.Cout
    z = lambda n: Out(1, n, prefill=torch.zeros(n))
    grad, w4, wr, wc = z(Cout * C0 * 25), z(4 * 16 * C0 * Cout), z(2 * 5 * C0 * 2 * Cout), z(2 * 5 * C0 * 2 * Cout)
    if row.fam == "fold2x2":
        call("ramnet_fold_unpack_wgrad", w4, dw, wr, wc, grad, Cout, C0, C0)
    else:
        call("ramnet_fold_unpack_wgrad2x3", w4, None, dw, wr, wc, grad, Cout, C0, C0)
    zero = torch.zeros(Cout, C0, 5, 5, dtype=F64)
    ref = cr.fold_unpack_statement(zero, st.dW4, torch.zeros(4, 16, C0, Cout, dtype=F64), torch.zeros(2, 5 * C0, 2 * Cout, dtype=F64),
                                   torch.zeros(2, 5 * C0, 2 * Cout, dtype=F64))
    got = grad.value()
    assert_exact(got, ref.reshape(got.shape), "%s gradient after the fold's unpack" % what)


@pytest.mark.parametrize("row,refused", FH_SIDES, ids=_ids(FH_SIDES))
def test_fold_and_head_at_their_limits(row, refused):
    import re
    import types
    L = _hip.lib()
    c, d = al.fh_data(row)
    mk = Maker(row)
    what = "%s, %s %d floats apart" % (row.name, row.operand, al.fh_ld(row) + (4 if refused else 0))
    with tf.option(b"fold_pair", row.fold_pair), tf.option(b"fold_half_wg", row.half):
        if row.launch in ("fold_fwd", "fold_dgrad", "head_fwd"):
            cls, entry, f, outs = al.fh_fields(row, c, d, mk, refused)
            call_desc(entry, cls, f, rc=BADARG if refused else 0)
            mk.inputs_intact(what)
            if refused:
                return
            name, got = L.ramnet_last_kernel().decode(), outs["out"].value()
            if row.launch == "fold_fwd":
                st = cr.fold_statement(d, row.fam, pair=row.Cout == 32 and row.C0 % 32 == 0)
                assert cr.fold_exact_ok(st, row.fam)
                assert_exact(got, st.out.reshape(got.shape), what)
                assert re.fullmatch(_fold_kernel(row, False), name), name
            elif row.launch == "fold_dgrad":
                taps, Wt = cr.parity4_taps_weights(d.w5)
                ref, _ = cr.reduction(cr.logical_input(d), Wt, taps, 1, al.FH + 4, al.FW + 4)
                assert float(cr.parity4_wino(d.x0, d.w5, row.fam).max()) * 2.0 ** cr.GRID_BITS[row.fam] < 2 ** 24
                assert_exact(got, ref.reshape(got.shape), what)
                assert re.fullmatch(_fold_kernel(row, True), name), name
            else:
                tf.judge(c, cr.conv_statement(d, "direct"), outs["out"], what)
                assert name == "conv_head_fwd_kernel<%d>" % c.cin, name
            return
        # backward-weights: atomic form, then the slab form with the library's slab count on the same inputs
        head = row.launch == "head_wgrad"
        if head:
            st = cr.wgrad_statement(types.SimpleNamespace(**dict(vars(d), taps=[t[:2] for t in d.taps])))
            one = 25 * row.C0 * row.Cout
        else:
            st = cr.fold_wgrad_statement(d)
            assert float(cr.fold_wgrad_wino(d, row.fam)[0].max()) * 2.0 ** cr.WGRAD_GRID_BITS[row.fam] < 2 ** 24 and torch.equal(st.dW4, st.dW4.round())
            one = 4 * 5 * (cr.FOLD_TW[row.fam] + 3) * row.C0 * row.Cout
        for slab_form in (False, True):
            S = 1
            if slab_form:
                _, _, f0, _ = al.fh_fields(row, c, d, mk, refused, dw=4096, dbias=8192)
                S = L.ramnet_wgrad_slabs(C.byref(al.struct(_hip.WgradDesc, f0)))
                assert S >= 1
            dw, dbias = Out(S, one, prefill=torch.zeros(S, one)), Out(S, row.Cout, prefill=torch.zeros(S, row.Cout))
            cls, entry, f, _ = al.fh_fields(row, c, d, mk, refused, dw=dw, dbias=dbias, slabs=S if slab_form else 0)
            form = "%s, %s form" % (what, "slab" if slab_form else "atomic")
            call_desc(entry, cls, f, rc=BADARG if refused else 0)
            mk.inputs_intact(form)
            if refused:
                continue
            name = L.ramnet_last_kernel().decode()
            assert name.startswith("conv_head_wgrad_kernel" if head else "conv_wgrad_wino24_kernel" + ("_2x3" if row.fam == "fold2x3" else "")), name
            if S > 1:
                call("ramnet_reduce_slabs", dw, S, one)
                call("ramnet_reduce_slabs", dbias, S, row.Cout)
            assert_exact(dbias.value()[0], st.dbias, form + " dbias", abs_sum=st.dbias_abs)
            if head:
                ref, rabs = torch.zeros(25, row.C0, row.Cout, dtype=F64), torch.zeros(25, row.C0, row.Cout, dtype=F64)
                ref[:, :c.cin], rabs[:, :c.cin] = st.dW, st.dW_abs
                assert_exact(dw.value()[0], ref.reshape(-1), form + " dW", abs_sum=rabs.reshape(-1))
            else:
                first = Out(1, one, prefill=dw.value()[0])
                _fold_wgrad_judge(row, d, st, first, form)
                assert not bool(_bits(first.value()).any()), "the workspace must come back +0"


# ---------------------------------------------------------------------------------------------------- the callers: whole layers at the limits
import address_limit_layers as ll


class _Trace:
    """records (entry point, algo, in_mode) of every convolution launch while it is installed (_hip.set_tracer)"""

    def __init__(self):
        self.seen = set()

    def __call__(self, name, fn, args):
        if name in ("ramnet_conv_launch", "ramnet_wgrad_launch", "ramnet_conv_launch_multi"):
            d = args[0]._obj if hasattr(args[0], "_obj") else args[0][0]
            self.seen.add((name, d.algo, d.in_mode))
        return fn(*args)


def _run_layer(c, switches):
    """forward + backward of the row's layer under `switches`: ({parameter: gradient}, dx, the launches it made)"""
    from rpg_ramnet_amd import ops
    from rpg_ramnet_amd.model.submodules import ResidualBlock, UpsampleConvLayer
    dev = torch.device("cuda:0")
    P = ll.weights(c)
    from rpg_ramnet_amd.model.submodules import ConvLayer
    m = (UpsampleConvLayer(c.Cin, c.Cout, 5, padding=2) if c.layer == "decoder" else ConvLayer(c.Cin, c.Cout, 3, padding=1) if c.layer == "conv"
         else ResidualBlock(c.Cin, c.Cout)).to(dev)
    names = {"conv2d.weight": "w", "conv2d.bias": "b", "conv1.weight": "w1", "conv1.bias": "b1", "conv2.weight": "w2", "conv2.bias": "b2"}
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(P[names[k]].float())
    r = ll.reference_once(c)
    x = ll.fill_x(c, dev).requires_grad_(True)
    Ho, Wo = ll.out_map(c)
    dy = torch.zeros(c.B, Ho, Wo, c.Cout, device=dev)
    dy[r.S[:, 0].to(dev), r.S[:, 1].to(dev), r.S[:, 2].to(dev)] = r.dyv.float().to(dev)
    tr = _Trace()
    with ops.switches(**switches):
        _hip.set_tracer(tr)
        try:
            y = m(x)
            y.backward(dy)
            torch.cuda.synchronize()
        finally:
            _hip.set_tracer(None)
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    dx = x.grad
    del y, dy, m
    return grads, dx, tr.seen


LAYER_SWITCHES = {"decoder": (dict(), dict(fold_winograd_wgrad=False)), "resblock": (dict(wgrad_winograd_2x4="force"), dict(wgrad_winograd_2x4="off")),
                  "conv": (dict(wgrad_winograd_2x4="force"), dict(wgrad_winograd_2x4="off"))}


@pytest.mark.parametrize("c", ll.CASES, ids=[c.name for c in ll.CASES])
def test_layer_at_its_limit(c):
    """A whole layer on both sides of its limit (tests/address_limit_layers.py): every weight and bias gradient and dx at every pixel that
    can be non-zero equal the float64 reference exactly, dx is zero everywhere else, no launch is refused, the family is the one that can
    address the operands, and the run with the Winograd backward-weights switched off gives the same bits."""
    need = {"resblock": 18, "conv": 12, "decoder": 8}[c.layer] << 30
    room(need)
    at = c.name.endswith("_at")
    r = ll.reference_once(c)
    on, off = LAYER_SWITCHES[c.layer]
    grads, dx, seen = _run_layer(c, on)
    wg = {a for n, a, _ in seen if n == "ramnet_wgrad_launch"}
    if c.layer == "decoder":        # at the limit: four direct parity launches and the direct backward-data; below: the folded kernels
        folded = {_hip.ALGO_WINOGRAD24, _hip.ALGO_WINOGRAD24_2X3}
        assert bool(wg & folded) != at and (_hip.ALGO_DIRECT in wg) == at, seen
        assert any(m == _hip.IN_PARITY4 for _, _, m in seen) != at, seen
    else:       # (the Winograd backward-weights count the whole tensor and its halo row: the conv row one image row below 2 GB is beyond them too)
        fits = (c.B * c.H * c.W + c.W + 1) * c.Cin * 4 < al.WOOB
        assert (wg == {_hip.ALGO_DIRECT}) == (not fits) and (not fits or wg <= {_hip.ALGO_WINOGRAD_2X4, _hip.ALGO_DIRECT_SPLIT}), seen
        assert fits == (c.name == "resblock_below")
    if c.layer == "conv":           # one image of 2 GB: forward and backward-data on the direct kernel too; below it on a Winograd one
        fwd = {a for n, a, _ in seen if n == "ramnet_conv_launch"}
        assert (fwd == {_hip.ALGO_DIRECT}) == at and (at or _hip.ALGO_DIRECT not in fwd), seen
    for k, ref in r.grads.items():
        assert_exact(grads[k].cpu(), ref, "%s %s" % (c.name, k))
    flat = dx.view(-1, c.Cin)
    pix = r.dx_pix.to(flat.device)
    assert_exact(flat[pix].cpu(), r.dx, "%s dx at its %d pixels" % (c.name, pix.numel()))
    keep = flat[pix].clone()
    flat.data[pix] = 0
    assert not bool(flat.any()), "%s: dx is not zero away from the samples" % c.name
    flat.data[pix] = keep
    grads2, dx2, seen2 = _run_layer(c, off)
    assert not any(a in (_hip.ALGO_WINOGRAD24, _hip.ALGO_WINOGRAD24_2X3, _hip.ALGO_WINOGRAD_2X4) for n, a, _ in seen2 if n == "ramnet_wgrad_launch")
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), "%s: %s differs with the Winograd backward-weights off" % (c.name, k)
    assert torch.equal(dx, dx2), "%s: dx differs with the Winograd backward-weights off" % c.name


@pytest.mark.parametrize("cell", ["convgru", "convlstm", "encoder"])
def test_cells_and_encoders_take_the_direct_layout_when_told_their_operands_do_not_fit(cell, monkeypatch):
    """ops asks _wino_wgrad_fits for the recurrent cells and the space-to-depth encoders as for ConvAct and ResConv; a cell at 2 GB per
    tensor is out of reach of a quick test, so here the answer is forced on a small one: every backward-weights launch then runs the direct
    kernel (the encoder: on its materialised view), none is refused, and the gradients are those of the Winograd pass within rounding"""
    from rpg_ramnet_amd import ops
    from rpg_ramnet_amd.model.submodules import ConvGRU, ConvLSTM, ConvLayer
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    m = (ConvGRU(32, 32, 3) if cell == "convgru" else ConvLSTM(32, 32, 3) if cell == "convlstm" else ConvLayer(32, 64, 5, stride=2, padding=2)).to(dev)
    x = torch.randn(2, 16, 24, 32, device=dev)
    h = torch.randn(2, 16, 24, 32, device=dev)

    def run():
        xg = x.clone().requires_grad_(True)
        m.zero_grad()
        tr = _Trace()
        _hip.set_tracer(tr)
        try:
            out = m(xg, h) if cell == "convgru" else m(xg, (h, h * 0.5))[0] if cell == "convlstm" else m(xg)
            out = out[0] if isinstance(out, tuple) else out
            out.square().sum().backward()
            torch.cuda.synchronize()
        finally:
            _hip.set_tracer(None)
        return {k: p.grad.clone() for k, p in m.named_parameters()}, xg.grad.clone(), {(a, md) for n, a, md in tr.seen if n == "ramnet_wgrad_launch"}
    g0, dx0, wg0 = run()
    assert any(a != _hip.ALGO_DIRECT for a, _ in wg0), wg0
    monkeypatch.setattr(ops, "_wino_wgrad_fits", lambda *a, **kw: False)
    g1, dx1, wg1 = run()
    assert {a for a, _ in wg1} == {_hip.ALGO_DIRECT} and all(md != _hip.IN_S2D for _, md in wg1), wg1
    for k in g0:
        scale = float(g0[k].abs().max())
        assert float((g1[k] - g0[k]).abs().max()) <= 1e-4 * scale, k
    assert float((dx1 - dx0).abs().max()) <= 1e-4 * float(dx0.abs().max())
