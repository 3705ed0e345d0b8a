"""The one GPU process of tests/test_hip_streams.py: started fresh once per test session (library scratch is keyed by the raw stream handle
and torch hands out its pool streams round-robin, so "first use on this stream" holds only in a process that has not touched the stream).

Runs the rows of tests/stream_cases.py in their fixed order, each on a torch.cuda.Stream() of its own, and prints one JSON line per row:
{"row": id, "ok": bool, "why": assertion text or "", "conclusive": bool or null, ...}; a first line {"calibration": ...} and a last
{"done": seconds}.  An AssertionError fails its row and the worker goes on (on the default stream, before the rows: {"baseline_failed":
...} and the end); ANY other exception (a HIP call returned an error) ends the worker at once with {"fatal": ...}: nothing is launched
after a fault.

Values are held to the rule each entry point has in its own launch test (the helpers are imported from those files, no tolerance is stated
here), and every row must give the bits of the same call made on the default stream in this process (`solo`).  Rows never reuse a cached
pointer table across streams while a delay is pending: every call site builds tensors of its own (`operands`), so the tables' keys differ;
the cross-stream reuse is table_owner's alone, which synchronises the device between its two calls."""
import contextlib
import ctypes as C
import json
import os
import sys
import time
import traceback

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE), os.path.join(HERE, "golden")):          # (behind PYTHONPATH: a copied package there is the one under test)
    if p not in sys.path:
        sys.path.append(p)

from rpg_ramnet_amd import _hip, metrics as M, ops, render, voxel  # noqa: E402
import grad_loss_cases as gc  # noqa: E402
import grad_loss_restatement as gr  # noqa: E402
import metric_launch_cases as K  # noqa: E402
import render_restatement as RR  # noqa: E402
import stream_cases as sc  # noqa: E402
import voxel_cases as vc  # noqa: E402
import conv_launch_cases as cc  # noqa: E402
import conv_restatement as cr  # noqa: E402
import test_hip_conv_launch as TC  # noqa: E402
import augment_scale_cases as asc  # noqa: E402
import test_hip_augment_scale as TAS  # noqa: E402
import test_hip_grad_loss_launch as TG  # noqa: E402
import test_hip_metric_launch as TM  # noqa: E402
import test_hip_ops as TO  # noqa: E402
import test_hip_reductions as TR  # noqa: E402
import test_hip_render as TRD  # noqa: E402
import test_hip_voxel_launch as TV  # noqa: E402
from guarded import F64, SENT, SENT_BYTE, SENT_INT, In, Out, _bits, assert_exact, call  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 4


def emit(**kw):
    print(json.dumps(kw), flush=True)


def same(a, b, what):
    """two fetched results, bit for bit"""
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: output %d differs (%d bytes of %d)" % (
            what, i, int((x.view(np.uint8) != y.view(np.uint8)).sum()) if x.shape == y.shape else -1, x.nbytes)


def raw(stream):
    return stream.cuda_stream


def stream_workspace(cache, stream):
    ws = cache.get((0, raw(stream)))
    assert ws is not None, "the cache holds no workspace under (device, this stream): its keys are %r" % (sorted(cache),)
    return ws


def poison(nbytes):
    """a block of the current stream's pool that holds SENT_BYTE, handed back at once: the next torch.empty of that size on this stream
    takes it, so a result that is never written reads as 0xA5 bytes and the allocator needs no hipMalloc during the row"""
    torch.full((int(nbytes),), SENT_BYTE, dtype=torch.uint8, device=DEV)


def reserve(nbytes, tickets=0):
    """the same for a workspace: its ticket bytes 0xFF, the rest as the allocator left it.  csrc/metrics_common.hpp bm_ticket is the only
    reader of a ticket word in metrics.hip and render.hip (an atomicAdd whose old value is compared with P - 1; atomicExch puts 0 back):
    a ticket is never an index, so a workspace whose zero-fill comes late leaves results unwritten and nothing else."""
    t = torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)
    if tickets:
        t[:tickets].fill_(0xFF)
    return t.data_ptr()


# ================================================================================================ surfaces
class Surface:
    """operands(data): fresh device tensors / guarded buffers of data set 0 or 1, with `rounds` sets of outputs (built on the default
    stream; nothing here may be called while a delay is pending).  launch(o, r): enqueue on the CURRENT stream, no synchronisation.
    fetch(o, r): after a synchronisation, the outputs as numpy arrays (guards checked).  check(o, got): the launch test's value rule.
    warm(o): allocations of the row's sizes, under the stream that will run it.  tickets(stream): the caller-visible ticket words."""
    library = False

    capture_data = (1, 0)          # the data sets of the two replays: the other one first, so that a replay that reads nothing new shows
    warm_capture = False           # run the call once on the capturing stream first (torch's rule for a captured backward)

    def warm(self, o):
        """-> the address of the block reserved for the stream's workspace (ticket bytes poisoned), or None"""
        return None

    def tickets(self, stream):
        return None

    def fresh_outputs(self, o):
        """guarded outputs: a new, sentinel-filled set for another call on the same operands"""
        if "outs" in o:
            o["outs"] = self.operands(0)["outs"]

    def capture_operands(self, data):
        return self.operands(data)

    def refill(self, o, src):
        raise NotImplementedError

    def reset_outputs(self, o):
        for b in (o["outs"][0] if isinstance(o["outs"][0], tuple) else (o["outs"][0],)):
            b.dev.fill_(SENT)          # sentinel again for the next replay (guards and body hold the same value)

    def capture_check(self, o, src, got, solo, rep, kernel):
        """the value rule on the refilled data, and the bits of the eager call"""
        self.check(src_as(o, src), got, what="captured, replay %d" % rep)
        same(got, solo, "replay %d against the eager call" % rep)

    def caches(self):
        return {}

    def workspaces(self):
        """the package's workspace caches this surface takes from: one workspace per (device, stream)"""
        return []


class SiLoss(Surface):
    library = True

    def __init__(self, log):
        self.log, self.n = log, 4099
        self.name = "ramnet_si_log_loss_fwd" if log else "ramnet_si_loss_fwd"

    def operands(self, data, rounds=1):
        p, t = TR._si_data(self.n, self.log, "normal", 0.2, 300 + 10 * data)
        w, lam = (1.0 if self.log else TR.f32v(0.5)), TR.f32v(0.85)
        return dict(p=p, t=t, w=w, lam=lam, pin=In(p), tin=In(t), outs=[(Out(1, 4, dtype=F64), Out(1, 1)) for _ in range(rounds)], res=[None] * rounds)

    def args(self, o, r):
        stats, loss = o["outs"][r]
        return (self.name, o["pin"], o["tin"], self.n) + ((o["lam"],) if self.log else (o["w"], o["lam"])) + (stats, loss)

    def launch(self, o, r=0):
        call(*self.args(o, r), stream=torch.cuda.current_stream().cuda_stream or None, defer=True)

    def fetch(self, o, r=0):
        for b in o["outs"][r]:
            b._host = None
            b.check(self.name)
        stats, loss = o["outs"][r]
        return [stats.value()[:, :3].numpy(), loss.value().numpy()]

    def check(self, o, got, r=0, what=""):
        stats, loss = o["outs"][r]
        TR._si_check(stats, loss, o["p"], o["t"], self.log, "normal", o["w"], o["lam"], "%s %s" % (self.name, what))

    def refill(self, o, src):
        o["pin"].dev.copy_(src["pin"].dev)
        o["tin"].dev.copy_(src["tin"].dev)

    def capture_check(self, o, src, got, solo, rep, kernel):
        """zero-fill + atomics while capturing: test_si_forward_capture_form's rule against the one-launch form"""
        self.check(src_as(o, src), got, what="captured, replay %d" % rep)
        TR.assert_count(torch.from_numpy(got[0])[0, 2], torch.from_numpy(solo[0])[0, 2], "captured against one-launch: count")
        sb, lb = TR._si_bounds(src["p"], src["t"], self.log, src["w"], src["lam"])
        TR.assert_within(torch.from_numpy(got[0])[0, :2], torch.from_numpy(solo[0])[0, :2].double(), 2 * sb, "captured against one-launch")
        TR.assert_within(torch.from_numpy(got[1]).view(-1), torch.from_numpy(solo[1]).double().view(-1), 2 * lb.view(-1), "loss captured against one-launch")


class MseLoss(Surface):
    """ramnet_mse_loss_fwd: no scratch, a zero-fill of `stats` and atomics on it in every call; integer data, so the sums are exact and the
    bits do not depend on the arrival order"""
    B, H, W, half, name = 2, 33, 31, 0, "ramnet_mse_loss_fwd"

    def operands(self, data, rounds=1):
        p, t = TR._mse_data(self.B, self.H, self.W, "int", 0.2, 500 + 10 * data)
        return dict(p=p, t=t, pin=In(p.view(-1)), tin=In(t.view(-1)), outs=[(Out(1, 4, dtype=F64), Out(1, 1)) for _ in range(rounds)])

    def launch(self, o, r=0):
        stats, loss = o["outs"][r]
        call(self.name, o["pin"], o["tin"], self.B, self.H, self.W, self.half, stats, loss, stream=torch.cuda.current_stream().cuda_stream or None, defer=True)

    def fetch(self, o, r=0):
        for b in o["outs"][r]:
            b._host = None
            b.check(self.name)
        stats, loss = o["outs"][r]
        return [stats.value()[:, :2].numpy(), loss.value().numpy()]

    def check(self, o, got, r=0, what=""):
        TR.mse_check(torch.from_numpy(got[0]).view(-1), torch.from_numpy(got[1]), o["p"], o["t"], self.half, "int", "%s %s" % (self.name, what))

    def refill(self, o, src):
        o["pin"].dev.copy_(src["pin"].dev)
        o["tin"].dev.copy_(src["tin"].dev)


class ConvSplitK(Surface):
    """ramnet_conv_launch with splitk_ws: the 9 x 11, Cin 32, wino_ksplit 2 row of test_wino_split_reduction — arrival counters in the CALLER's
    workspace that the last arrival puts back.  first_use and second_use only; the workspace as that test prepares it (all zero)."""
    ksplit, cin = 2, 32

    def _layout(self):
        f, outs = TC.layout(self.case, self.desc, "2x2")
        return f, outs

    def operands(self, data, rounds=1):
        self.case = cc._case("ksplit%d" % self.ksplit, ("2x2",), 1, 9, 11, self.cin, 64, density=0.25)
        self.desc = cc.build(self.case)
        self.st = cr.conv_statement(self.desc, "2x2")
        assert cr.exact_ok(self.st, "2x2")
        with TV.option(b"wino_ksplit", self.ksplit):
            f, outs = self._layout()
            n = _hip.lib().ramnet_conv_splitk_floats(C.byref(TC._struct(f)))
        assert n > 64
        ws = Out(1, n, prefill=torch.zeros(n))
        f["splitk_ws"], f["splitk_floats"] = ws, n
        return dict(f=f, out=outs["out"], ws=ws, n=n)

    def fresh_outputs(self, o):
        with TV.option(b"wino_ksplit", self.ksplit):
            f, outs = self._layout()
        f["splitk_ws"], f["splitk_floats"] = o["ws"], o["n"]
        o.update(f=f, out=outs["out"])
        torch.cuda.synchronize()

    def launch(self, o, r=0):
        o["struct"] = TC._struct(o["f"])                  # (lives until the fetch)
        st = torch.cuda.current_stream().cuda_stream
        with TV.option(b"wino_ksplit", self.ksplit):
            rc = _hip.lib().ramnet_conv_launch(C.byref(o["struct"]), C.c_void_p(st) if st else None)
        assert rc == 0, ("ramnet_conv_launch", rc, _hip.lib().ramnet_last_error())

    def fetch(self, o, r=0):
        for b in [v for v in o["f"].values() if isinstance(v, Out)]:
            b._host = None
            b.check("ramnet_conv_launch")
        self.ws = o["ws"]
        return [o["out"].value().numpy()]

    def check(self, o, got, r=0, what=""):
        assert_exact(torch.from_numpy(got[0]), self.st.out, "split reduction x%d %s" % (self.ksplit, what))

    def tickets(self, stream):
        return self.ws.value()[0, :64].view(torch.int32)


class VoxelSorted(Surface):
    library = True
    names = ("m2", "s2")
    entry = "ramnet_voxelize_batch_sorted"

    def operands(self, data, rounds=1, entry=None):
        name = self.names[data]
        r = vc.ROWS[name]
        lists = vc.data(name)
        off = np.cumsum([0] + [len(e) for e in lists])
        ev, offs = TV.events_in(np.concatenate(lists)), In(torch.tensor(off), fill=SENT_INT, dtype=torch.int64)
        return dict(name=name, row=r, ev=ev, off=offs, entry=entry or self.entry,
                    outs=[Out(len(r["lens"]), r["bins"] * r["H"] * r["W"]) for _ in range(rounds)])

    def args(self, o, r):
        w = o["row"]
        return [o["entry"], o["ev"], o["off"], len(w["lens"]), vc.max_events(o["name"]), w["bins"], w["W"], w["H"], o["outs"][r]]

    def launch(self, o, r=0):
        call(*self.args(o, r), stream=torch.cuda.current_stream().cuda_stream or None, defer=True)

    def fetch(self, o, r=0):
        b = o["outs"][r]
        b._host = None
        b.check(o["entry"])
        w = o["row"]
        return [b.value().numpy().reshape(len(w["lens"]), w["bins"], w["H"], w["W"])]

    def check(self, o, got, r=0, what="", form="sorted"):
        TV.check_row(o["name"], got[0], form, "%s %s" % (o["entry"], what))

    capture_data = (0, 0)          # the lists' lengths are launch arguments: the same row, written again

    def capture_operands(self, data):
        """the sorted entry point refuses a capture: ramnet_voxelize_batch records the row's capture form"""
        return self.operands(data, entry="ramnet_voxelize_batch")

    def refill(self, o, src):
        if o["ev"] is not None:
            o["ev"].dev.copy_(src["ev"].dev)
        o["off"].dev.copy_(src["off"].dev)

    def capture_check(self, o, src, got, solo, rep, kernel):
        """global atomics on dyadic data: exact, so the bits of the eager call"""
        form = vc.ROWS[src["name"]]["capture"]
        assert kernel == TV.expected_kernel(src["name"], form), kernel
        self.check(src_as(o, src), got, what="captured, replay %d" % rep, form=form)
        same(got, solo, "replay %d against the eager call" % rep)


class BatchMetrics(Surface):
    N, npix, G = 16, 8193, 3

    def operands(self, data, rounds=1):
        assert K.BM_PLAN_ROWS[(self.N, self.npix)][0] > 1
        pairs = [K.bm_pair(400 + 10 * data + g, self.N, self.npix, nan_frac=0.2) for g in range(self.G)]
        dev = lambda a: torch.from_numpy(a).view(self.N, 1, 1, self.npix).to(DEV)
        return dict(pairs=pairs, ps=[dev(p) for p, _ in pairs], ts=[dev(t) for _, t in pairs], res=[None] * rounds)

    def nbytes(self):
        return _hip.lib().ramnet_batch_metrics_workspace(self.G, self.N, self.npix)

    def warm(self, o):
        at = reserve(self.nbytes(), M.TICKET_BYTES)
        poison(self.G * 10 * 8)
        poison(2 * self.G * 8)
        return at

    def launch(self, o, r=0):
        o["res"][r] = M.batch_metrics_table(o["ps"], o["ts"])

    def fetch(self, o, r=0):
        return [o["res"][r].cpu().numpy()]

    def check(self, o, got, r=0, what=""):
        for g, (p, t) in enumerate(o["pairs"]):
            TM.check_bm(got[0][g], p, t, "batch_metrics %s g=%d" % (what, g))

    def tickets(self, stream):
        return stream_workspace(M._workspaces, stream)[:M.TICKET_BYTES]

    def caches(self):
        return {"metrics._workspaces": M._workspaces, "metrics._tables": M._tables}

    def workspaces(self):
        return [M._workspaces]


class EvalTableRows(Surface):
    npix, G, cut, flags = K.ET_CAP_ROWS["first_at_cap"], 3, (20.0,), K.RESCALE

    def operands(self, data, rounds=1):
        assert K.et_plan(self.npix, 1, True)[1] > 1
        ps, ts, ms = K.et_pairs(500 + 10 * data, self.G, (1, self.npix), nan_frac=0.1)
        tm, pm = TM.et_inputs(ps, ts, 0)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        return dict(tm=tm, pm=pm, ms=ms, dp=[dev(p) for p in ps], dt=[dev(t) for t in ts], dm=[dev(m) for m in ms], res=[None] * rounds)

    def sizes(self):
        V = (1 + len(self.cut)) * 2
        return _hip.lib().ramnet_eval_table_ex_workspace(self.G, self.npix, len(self.cut), 1, self.flags), self.G * V * M.EVAL_ROW * 8

    def warm(self, o):
        ws, out = self.sizes()
        at = reserve(ws, M.EVAL_TICKET_BYTES)
        poison(out)
        poison(3 * self.G * 8)
        return at

    def launch(self, o, r=0):
        o["res"][r] = M.EvalTable(K.CLIP, K.REG, cutoffs=self.cut, rescale=True).add(o["dp"], o["dt"], o["dm"])

    def fetch(self, o, r=0):
        return [o["res"][r].cpu().numpy()]

    def check(self, o, got, r=0, what=""):
        for g in range(self.G):
            TM.check_et(got[0][g], o["tm"][g], o["pm"][g], o["ms"][g], self.cut, self.flags, "eval_table %s g=%d" % (what, g))

    def tickets(self, stream):
        return stream_workspace(M._eval_workspaces, stream)[:M.EVAL_TICKET_BYTES]

    def caches(self):
        return {"metrics._eval_workspaces": M._eval_workspaces}

    def workspaces(self):
        return [M._eval_workspaces]


class Render(Surface):
    shape, G, pairs = (64, 257), 3, 2
    vmin, vmax = 0.07, 0.83

    def __init__(self):
        self.lut = RR.lut_bytes()
        self.mapper = render.ColorMapper(self.vmin, self.vmax)

    def operands(self, data, rounds=1):
        rng = np.random.default_rng(11 + data)
        a = (1.4 * rng.random(self.shape) - 0.2).astype(np.float32)
        b = rng.random(self.shape).astype(np.float32)
        b[-1, -1] = np.nan
        c = rng.random(self.shape).astype(np.float32)
        c[0, 0], c[-1, -2] = 1.0, 0.0
        pairs = TRD.scale_pairs(self.shape, self.pairs, 31 + data)
        dp, dt = [TRD.to_dev(p) for p, _ in pairs], [TRD.to_dev(t) for _, t in pairs]
        want = [RR.scale_float64(M.metric_depth(p, TRD.CLIP, TRD.REG).cpu().numpy(), M.metric_depth(t, TRD.CLIP, TRD.REG).cpu().numpy()) for p, t in zip(dp, dt)]
        return dict(maps=[a, b, c], dmaps=[TRD.to_dev(m) for m in (a, b, c)], dp=dp, dt=dt, want=want, res=[None] * rounds)

    def warm(self, o):
        npix = self.shape[0] * self.shape[1]
        at = reserve(_hip.lib().ramnet_render_depth_workspace(self.G, self.pairs, npix), render.TICKET_BYTES)
        poison(5 * self.G * npix)
        poison(self.pairs * 8)
        poison((self.G + 2 * self.pairs) * 8)
        return at

    def launch(self, o, r=0):
        _, color, grey, _, scale = render.render_package(o["dmaps"], self.mapper, scale=(o["dp"], o["dt"], TRD.CLIP, TRD.REG))
        o["res"][r] = (grey, color, scale)

    def fetch(self, o, r=0):
        return [t.cpu().numpy() for t in o["res"][r]]

    def check(self, o, got, r=0, what=""):
        grey, color, scale = got
        wg, wc = TRD.restated(o["maps"], self.vmin, self.vmax, self.lut)
        assert np.array_equal(grey, wg) and np.array_equal(color, wc), "render %s: %d grey and %d colour pixels differ from the restatement" % (
            what, int((grey != wg).sum()), int((color != wc).any(axis=-1).sum()))
        n = self.shape[0] * self.shape[1]
        for g, want in enumerate(o["want"]):
            rel = abs(scale[g] - want) / abs(want)
            assert rel <= TRD.scale_bound(n), "render %s: scale %d is %.3e off the float64 sums (bound %.3e)" % (what, g, rel, TRD.scale_bound(n))

    def tickets(self, stream):
        return stream_workspace(render._workspaces, stream)[:render.TICKET_BYTES]

    def caches(self):
        return {"render._workspaces": render._workspaces}

    def workspaces(self):
        return [render._workspaces]


class GradLossBatch(Surface):
    name = "m63x66_ns4"

    def operands(self, data, rounds=1):
        """data 1: every map negated (the statistics and the loss are sums of absolute values and stay, every gradient changes its sign)"""
        name, sign = self.name, 1.0 if data == 0 else -1.0
        G, B, H, W, ns = TG.row(name)
        assert G == 3 and gr.workspace_bytes(1, 1, H, W) == 2 * 64               # two tiles per map
        preds, targets = gc.data(name)
        weights, up = TG.default_args(name)
        dev = lambda t: (sign * t).float().view(B, 1, H, W).to(DEV)
        return dict(name=name, sign=sign, dims=(G, B, H, W, ns), weights=weights, up=up, dw=None if weights is None else weights.float().to(DEV), dup=up.float().to(DEV),
                    ps=[dev(p).requires_grad_(True) for p in preds], ts=[dev(t) for t in targets], res=[None] * rounds)

    def warm(self, o):
        G, B, H, W, ns = o["dims"]
        reserve(gr.workspace_bytes(G, B, H, W))
        for n in (2 * G * 8, G * ns * 2 * 8, (G + 1) * 4, G * B * H * W * 4):
            poison(n)
            poison(n)

    def launch(self, o, r=0):
        ns = o["dims"][4]
        loss, wsum = ops.multi_scale_grad_loss_batch(o["ps"], o["ts"], weights=o["dw"], num_scales=ns, with_sum=True)
        grads = torch.autograd.grad(loss, o["ps"], grad_outputs=o["dup"])
        o["res"][r] = (ops.msg_local_stats(o["ps"], o["ts"], ns), loss.detach(), wsum.detach().view(1)) + tuple(grads)

    def fetch(self, o, r=0):
        return [t.cpu().numpy() for t in o["res"][r]]

    def check(self, o, got, r=0, what=""):
        name, (G, B, H, W, ns) = o["name"], o["dims"]
        what = "grad_loss_batch %s %s" % (name, what)
        st, loss, wsum = torch.from_numpy(got[0]), torch.from_numpy(got[1]), torch.from_numpy(got[2])
        TG.check_stats(name, st)
        TG.check_loss(name, gc.statement(name)[0], B, o["weights"], loss, wsum, what)
        counts = gc.statement(name)[0][:, :, 1]
        preds, targets = gc.data(name)
        one = torch.ones(G, dtype=F64)
        factor = o["up"] * (one if o["weights"] is None else o["weights"]) * B * 2.0          # (gain 1, no upstream gradient of the sum)
        for g in range(G):                     # check_bwd's rule, with the counts of the forward pass
            ref, aref = gr.backward(o["sign"] * preds[g], o["sign"] * targets[g], ns, counts[g], 1.0)
            ref, aref = ref * float(factor[g]), aref * abs(float(factor[g]))
            d = torch.from_numpy(got[3 + g]).view(B, H, W)
            err, bound = (d.double() - ref).abs(), gr.grad_bound(aref)
            assert bool((err <= bound).all()) and bool(torch.isfinite(d).all()), "%s dpred[%d]: error %.3f x its bound" % (
                what, g, float((err / bound.clamp_min(1e-300)).max()))
            zero = aref == 0
            assert not bool(_bits(d[zero]).any()), "%s dpred[%d]: not +0 where nothing arrives" % (what, g)

    def caches(self):
        return {"ops._msg_tables": ops._msg_tables, "ops._msg_workspaces": ops._msg_workspaces, "ops._msg_weight_cache": ops._msg_weight_cache}

    def workspaces(self):
        return [ops._msg_workspaces]

    warm_capture = True

    def refill(self, o, src):
        with torch.no_grad():
            for k in ("ps", "ts"):
                for d, s_ in zip(o[k], src[k]):
                    d.copy_(s_)

    def reset_outputs(self, o):
        pass


class PredSigmoidSI(Surface):
    """ops.PredSigmoidSI, forward and backward: ramnet_pred_sigmoid_si_fwd / _bwd join their partial sums through a scratch of the call (zeroed
    by torch.zeros on the current stream, handed from the forward to the backward launch); C = 32, seg_pix = 517, nseg = 2"""
    dims = (2, 11, 47, 32, 2)          # B, H, W, C, n: seg_pix = (B / n) H W = 517

    def operands(self, data, rounds=1):
        B, Hh, W, Cc, n = self.dims
        assert (B // n) * Hh * W == 517
        return dict(args=TO.pred_si_operands(*self.dims, seed=700 + data), res=[None] * rounds)

    def warm(self, o):
        B, Hh, W, Cc, n = self.dims
        for nbytes in (B * Hh * W * 4, _hip.lib().ramnet_pred_si_scratch_doubles(517, n) * 8, n * 32, n * 4, B * Hh * W * Cc * 4, Cc * 4, 4):
            poison(nbytes)
            poison(nbytes)

    def launch(self, o, r=0):
        outs, dx, dw, db = TO.pred_si_run(*o["args"])
        o["res"][r] = list(outs) + [dx, dw, db]

    def fetch(self, o, r=0):
        return [t.cpu().numpy() for t in o["res"][r]]

    def check(self, o, got, r=0, what=""):
        res = o["res"][r]
        TO.pred_si_check(res[:-3], res[-3], res[-2], res[-1], *o["args"])


class AugmentApply(Surface):
    """augment.apply with stats= and scale_factor on the grids of sparse event lists (test_fused_normalisation's operands and rule)"""
    G, bins = 4, 5

    def operands(self, data, rounds=1):
        H_, W_, th, tw, s = asc.FAST
        A = TAS.A
        cat, off, mx = voxel.pack_event_lists(TAS._event_lists(self.G, 1500, H_, W_, 1 + data), DEV)
        ps = list(TAS.params_of(asc.FAST))[:self.G]
        table = A.ParamTable(ps, H_, W_).to(DEV)
        scratch = A.voxel_scratch(self.G, self.bins, H_, W_, DEV)
        A.voxelize_augmented(cat, off, mx, self.bins, W_, H_, table, scratch=scratch, scale_factor=s, nhwc=True)      # (fills the grids and their statistics)
        torch.cuda.synchronize()
        return dict(ps=ps, table=table, scratch=scratch, grids=scratch["grids"].clone(), stats=scratch["stats"].clone(), host=scratch["grids"].cpu().double(),
                    res=[None] * rounds)

    def warm(self, o):
        poison(self.G * 16 * 16 * 8 * 4)
        poison(self.G * 8)
        poison(self.G * 8)

    def launch(self, o, r=0):
        o["res"][r] = TAS.A.apply(o["grids"], o["table"], stats=o["stats"], scale_factor=asc.FAST[4], nhwc=True)

    def fetch(self, o, r=0):
        return [o["res"][r].cpu().numpy()]

    def check(self, o, got, r=0, what=""):
        H_, W_, th, tw, s = asc.FAST
        out = torch.from_numpy(got[0])
        assert tuple(out.shape) == (self.G, 16, 16, 8)
        for g, p in enumerate(o["ps"]):
            src, bound = TAS.ar.normalized(o["host"][g])
            ref, tol = TAS.asr.exact(src, H_, W_, th, tw, p.top, p.left, TAS.flips_of(p), s, value_bound=bound)
            TAS.asr.check(out[g].reshape(-1), TAS.ar.to_layout(ref, True, 8), TAS.ar.to_layout(tol, True, 8), "augment.apply %s grid %d" % (what, g))


# ================================================================================================ the delay
class Delay:
    def __init__(self):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000000)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(20000000)
        b.record()
        torch.cuda.synchronize()
        self.cycles_per_ms = 20000000 / a.elapsed_time(b)
        self.ms = 20.0

    def set(self, slowest_ms):
        """20 x the slowest row's undelayed enqueue-plus-synchronise time, at least 20 ms and at most 500 ms"""
        self.ms = min(max(20.0 * slowest_ms, 20.0), 500.0)

    def start(self, stream=None, ms=None):
        """hold `stream` (default: the default stream) busy; -> an event recorded behind the delay"""
        ev = torch.cuda.Event()
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            torch.cuda._sleep(int((self.ms if ms is None else ms) * self.cycles_per_ms))
            ev.record()
        return ev


# ================================================================================================ streams
PROBE_MS = 3.0
POOL = 32             # torch hands out this many pool streams round-robin: a 33rd torch.cuda.Stream() is the first one again
STREAMS = []          # the pool, drawn once; a stream leaves it when a row takes it or its probe rejects it
UTILITY = []


def _draw():
    if not STREAMS and not UTILITY:
        seen = {}
        for _ in range(POOL):
            st = torch.cuda.Stream()
            seen.setdefault(raw(st), st)
        STREAMS.extend(seen.values())
        UTILITY.extend([STREAMS.pop(), STREAMS.pop()])
        # every first_use row needs one stream that runs beside the default stream; the runtime deals streams onto 4 hardware queues, so
        # about a quarter of the pool is rejected: the rows must leave room for that
        assert sum(k == "first_use" for _, k in sc.ROWS) <= (len(STREAMS) * 5) // 8, "more first_use rows than the stream pool can serve"


def fresh_stream(delay):
    """A stream that neither the library nor the package has seen, and that runs beside the default stream: the runtime deals streams onto a
    few hardware queues, and a stream that shares the default stream's queue waits behind the delay whatever the code under test does.
    The probe is one torch fill (no library call, no package cache) behind a short delay; a rejected stream is not offered again."""
    _draw()
    probe = torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    tried = 0
    while True:
        assert STREAMS, "no unused stream of torch's pool runs beside the default stream"
        s = STREAMS.pop(0)
        tried += 1
        behind = delay.start(ms=PROBE_MS)
        with torch.cuda.stream(s):
            probe.fill_(1.0)
        s.synchronize()
        beside = not behind.query()
        torch.cuda.synchronize()
        if beside:
            return s, tried


def utility_streams():
    """the two streams of the kinds that need no unused one (two_streams, table_owner, capture)"""
    _draw()
    return UTILITY


# ================================================================================================ row kinds
def solo(surf, data, check=True, **kw):
    """the call on the default stream, on tensors of its own -> (operands, outputs, milliseconds of enqueue + synchronise)"""
    o = surf.operands(data, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    surf.launch(o)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    got = surf.fetch(o)
    if check:
        surf.check(o, got, what="on the default stream")
    return o, got, ms


def first_use(surf, ctx, delay):
    s, tried = fresh_stream(delay)
    o = surf.operands(0)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        reserved = surf.warm(o)
    torch.cuda.synchronize()
    behind = delay.start()
    with torch.cuda.stream(s):
        surf.launch(o)
    s.synchronize()
    conclusive = not behind.query()
    torch.cuda.synchronize()
    ctx.update(stream=s, o=o, conclusive=conclusive)
    got = ctx["first"] = surf.fetch(o)
    surf.check(o, got, what="first use of a stream")
    same(got, ctx["solo"][0], "first use of a stream against the default stream")
    if not surf.library:
        assert conclusive, "the delay on the default stream had ended when the fresh stream's synchronise returned: the row shows nothing"
    if reserved is not None:
        assert stream_workspace(surf.workspaces()[0], s).data_ptr() == reserved, "the stream's workspace is not the block whose ticket bytes were poisoned"
    return dict(conclusive=conclusive, streams_probed=tried, poisoned=reserved is not None)


def second_use(surf, ctx, delay):
    assert "first" in ctx, "the first use of the stream left no result to repeat"
    s, o = ctx["stream"], ctx["o"]
    surf.fresh_outputs(o)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        surf.launch(o)
    s.synchronize()
    torch.cuda.synchronize()
    got = surf.fetch(o)
    same(got, ctx["first"], "second use of the stream against the first")
    surf.check(o, got, what="second use of a stream")
    tk = surf.tickets(s)
    if tk is not None:
        assert not bool(tk.any().item()), "a ticket word of the stream's workspace is not zero after two calls"
    return dict(tickets_checked=tk is not None)


def two_streams(surf, ctx, delay):
    """Both streams wait behind ONE delay (it sits on the first; the second waits for the event behind it), so that the eight calls, enqueued
    alternately without a host synchronisation, start together when it ends and run side by side."""
    s = utility_streams()
    o = [surf.operands(d, rounds=ROUNDS) for d in (0, 1)]
    torch.cuda.synchronize()
    for i in (0, 1):
        with torch.cuda.stream(s[i]):
            for _ in range(ROUNDS):
                surf.warm(o[i])
    torch.cuda.synchronize()
    behind = delay.start(s[0])
    s[1].wait_event(behind)
    for r in range(ROUNDS):
        for i in (0, 1):
            with torch.cuda.stream(s[i]):
                surf.launch(o[i], r)
    queued = not behind.query()
    torch.cuda.synchronize()
    for i in (0, 1):
        for r in range(ROUNDS):
            got = surf.fetch(o[i], r)
            same(got, ctx["solo"][i], "stream %d, round %d against its solo result" % (i, r))
    for i in (0, 1):
        tk = surf.tickets(s[i])
        if tk is not None:
            assert not bool(tk.any().item()), "a ticket word of stream %d's workspace is not zero" % i
    for cache in surf.workspaces():
        assert stream_workspace(cache, s[0]).data_ptr() != stream_workspace(cache, s[1]).data_ptr(), "the two streams share one workspace"
    return dict(queued_behind_the_delay=queued)


def table_owner(surf, ctx, delay):
    """structural: the device is synchronised between the two calls, so nothing here can read a table before it is filled"""
    calls = []

    def tracer(name, fn, args):
        vals = [a.value or 0 if isinstance(a, C.c_void_p) else a if isinstance(a, int) else None for a in args]
        calls.append((name, vals))
        return fn(*args)

    a, b = utility_streams()
    o = surf.operands(0)
    torch.cuda.synchronize()
    marks = []
    _hip.set_tracer(tracer)
    try:
        for s in (a, b):
            marks.append(len(calls))
            with torch.cuda.stream(s):
                surf.launch(o)
            torch.cuda.synchronize()
            same(surf.fetch(o), ctx["solo"][0], "the call on stream %s against the default stream" % ("A" if s is a else "B"))
    finally:
        _hip.set_tracer(None)
    fills, launches, checked = [], [[], []], 0          # fills: (first byte, last byte + 1, stream), in call order
    for i, (name, vals) in enumerate(calls):
        if not name.startswith("ramnet_") or name.endswith("_workspace") or not vals or vals[-1] is None:
            continue
        stream, which = vals[-1], 0 if i < marks[1] else 1
        assert stream == raw((a, b)[which]), "%s ran on stream %#x, the current stream is %#x" % (name, stream, raw((a, b)[which]))
        if name == "ramnet_fill_pointer_table":
            fills.append((vals[0], vals[0] + 8 * vals[2], stream))
            continue
        launches[which].append((name, vals))
        for p in vals[:-1]:
            if p is None or p < 4096:
                continue
            owner = [f for f in fills if f[0] <= p < f[1]]
            if owner:
                checked += 1
                assert owner[-1][2] == stream, "%s on stream %#x reads the pointer table at %#x, last filled on stream %#x" % (name, stream, p, owner[-1][2])
    assert [n for n, _ in launches[0]] == [n for n, _ in launches[1]] and launches[0], "the two calls made different launches: %r / %r" % (launches[0], launches[1])
    uploaded = 0
    for (name, va), (_, vb) in zip(*launches):
        if name == "ramnet_batch_metrics":               # its table is uploaded by a copy, not by a library call: one table per stream
            uploaded += 1
            assert va[0] != vb[0] and va[1] != vb[1], "ramnet_batch_metrics on stream B reads the table uploaded on stream A (%#x)" % va[0]
    assert checked + uploaded > 0, "no launch of this surface took a pointer table"
    return dict(table_reads_checked=checked, uploaded_tables_checked=uploaded)


def snapshot(surf):
    return {k: (len(d), sorted(id(v) for v in d.values())) for k, d in surf.caches().items()}


def capture(surf, ctx, delay):
    """captured on a side stream, replayed twice with refilled inputs; no cache entry is made or taken while capturing"""
    s = utility_streams()[1]
    o = surf.capture_operands(0)
    torch.cuda.synchronize()
    if surf.warm_capture:
        with torch.cuda.stream(s):
            surf.launch(o)
        torch.cuda.synchronize()
    before = snapshot(surf)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        surf.launch(o)
        kernel = _hip.lib().ramnet_last_kernel().decode()
    assert snapshot(surf) == before, "the capture made or replaced a cache entry: %r -> %r" % (before, snapshot(surf))
    for rep, data in enumerate(surf.capture_data):
        src = surf.capture_operands(data)
        torch.cuda.synchronize()
        surf.refill(o, src)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        surf.capture_check(o, src, surf.fetch(o), ctx["solo"][data], rep, kernel)
        surf.reset_outputs(o)
    assert snapshot(surf) == before
    return dict(replays=len(surf.capture_data))


def src_as(o, src):
    """the captured operands' buffers with the refilled data's host side (what the value rule reads)"""
    return dict(src, **{k: o[k] for k in ("outs", "res") if k in o})


KIND = dict(first_use=first_use, second_use=second_use, two_streams=two_streams, table_owner=table_owner, capture=capture)


def main():
    t0 = time.perf_counter()
    torch.cuda.set_device(0)
    surfaces = dict(si_loss=SiLoss(False), si_log_loss=SiLoss(True), mse_loss=MseLoss(), voxel_sorted=VoxelSorted(), batch_metrics=BatchMetrics(),
                    eval_table=EvalTableRows(), render=Render(), grad_loss_batch=GradLossBatch(), pred_sigmoid_si=PredSigmoidSI(), augment=AugmentApply(),
                    conv_splitk=ConvSplitK())
    assert set(surfaces) == set(sc.SURFACES) and all(surfaces[k].library == sc.SURFACES[k]["library"] for k in surfaces)
    ctx, slowest = {}, 0.0
    try:
        delay = Delay()
        for name, surf in surfaces.items():           # the default stream first: the bits every row is held to, and the undelayed times
            runs = [solo(surf, d) for d in (0, 1)]
            runs.append(solo(surf, 0, check=False))   # (warm: the time of a call whose caches exist)
            ctx[name] = dict(solo=[r[1] for r in runs[:2]])
            slowest = max(slowest, runs[2][2])
        delay.set(slowest)
        emit(calibration=dict(cycles_per_ms=delay.cycles_per_ms, slowest_undelayed_ms=slowest, delay_ms=delay.ms))
    except AssertionError as e:                       # a wrong value on the default stream: no row has anything to be held to
        emit(baseline_failed=str(e) or traceback.format_exc())
        return 1
    except BaseException:
        emit(fatal="the calls on the default stream stopped on an error", trace=traceback.format_exc())
        return 1
    for row in sc.ROWS:
        name, kind = row
        try:
            extra = KIND[kind](surfaces[name], ctx[name], delay)
            emit(row=sc.row_id(row), ok=True, why="", **extra)
        except AssertionError as e:
            emit(row=sc.row_id(row), ok=False, why=str(e) or traceback.format_exc(), conclusive=ctx[name].get("conclusive"))
        except BaseException:                             # a HIP call returned an error (or anything else unforeseen): launch nothing more
            emit(row=sc.row_id(row), ok=False, why="stopped", fatal=traceback.format_exc())
            return 1
    emit(done=time.perf_counter() - t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
