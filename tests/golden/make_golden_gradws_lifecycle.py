"""Writes tests/golden/gradws_lifecycle.json: what ConvParam does with its weight-gradient workspaces over two passes of a layer — the
layout it stamps, the size of every workspace, the slab joins / unpacks it asks the library for and what it zeroes for the next pass —
for every layout, in and out of deterministic mode (the rows below).  No GPU: the tensors live on the CPU, the launches are recorded and
not run, the host queries of the library are answered by the library.  Run at the commit whose behaviour is to be kept; the accessors it
uses (grad_ws, grad_ws_fold, grad_ws_fold24, grad_ws_fold_det, discard, _Engine.flush) exist on both sides of a change to ConvParam, and
the workspaces are listed through ConvParam.workspaces() where the commit has it, through the fields it replaced where not.

tests/test_gradws_lifecycle_cpu.py runs the same rows (run_row) on the code under test and compares."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

from convparam_trace_cases import _arg  # noqa: E402

# layer -> (output channels per weight, input channels, k, what the pass asks for)
LAYERS = {
    "k3_64_wino": ([64], 64, 3, "grad_ws_wino"),
    "k3_64_plain": ([64], 64, 3, "grad_ws"),
    "head_5_32_k5": ([32], 5, 5, "grad_ws"),
    "k5_128_64": ([64], 128, 5, "grad_ws"),
    "gru_pair_k3": ([32, 32], 64, 3, "grad_ws_wino"),
    "s2d_32_64_k5": ([64], 32, 5, "s2d"),
    "k3_64_frozen_w": ([64], 64, 3, "grad_ws_wino"),
    "fold24_64_k5": ([64], 64, 5, "fold24"),
    "fold23_64_k5": ([64], 64, 5, "fold23"),
    "fold_direct_64_k5": ([64], 64, 5, "fold_direct"),
}
# row -> (layer, deterministic, wgrad_winograd_2x4, further {switch: value} of ops.switches, end of a pass)
ROWS = {}
for _det in (False, True):
    for _w24 in ("auto", "force"):
        for _layer in LAYERS:
            if _layer != "fold_direct_64_k5" or _det:
                ROWS["%s/det%d/%s" % (_layer, _det, _w24)] = (_layer, _det, _w24, {}, "flush")
ROWS["k3_64_wino/wgrad_atomic"] = ("k3_64_wino", False, "auto", {"wgrad_slabs": False}, "flush")
ROWS["k3_64_wino/split_operands"] = ("k3_64_wino", False, "force", {"split_operands": True, "split_wgrad": True}, "flush")
ROWS["k3_64_wino/winograd_off"] = ("k3_64_wino", False, "auto", {"winograd": False}, "flush")
ROWS["k3_64_wino/discard"] = ("k3_64_wino", False, "auto", {}, "discard")


class Recorder:
    """Records every call whose last argument is the stream — integers as they are, a pointer into a workspace of the layer as
    name+floats, any other pointer as p or 0 (null) — and answers 0 without calling; host queries go through."""

    def __init__(self):
        from rpg_ramnet_amd import _hip
        self.sigs, self.calls, self.spans = _hip._SIGS, [], []

    def watch(self, cp):
        self.spans = [(n, t.data_ptr(), 4 * t.numel()) for n, t in workspaces(cp) if t is not None]

    def _ptr(self, a):
        for n, base, size in self.spans:
            if a.value is not None and base <= a.value < base + size:
                return "%s+%d" % (n, (a.value - base) // 4)
        return _arg(a)

    def __call__(self, name, fn, args):
        argtypes = self.sigs[name][1]
        if argtypes and argtypes[-1] is C.c_void_p:
            self.calls.append(name + "|" + ",".join(self._ptr(a) if isinstance(a, C.c_void_p) else _arg(a) for a in args[:-1]))
            return 0
        return fn(*args)


def workspaces(cp):
    """[(name, tensor or None)] of every gradient workspace of the layer."""
    if hasattr(cp, "workspaces"):
        return [(name, r.t) for name, r in cp.workspaces()]
    fold = cp._ws_fold or (None, None, None)
    return [("main", cp._ws), ("bias", cp._bws), ("w4", fold[0]), ("rows", fold[1]), ("cols", fold[2]), ("fold24", cp._ws_fold24),
            ("fold23", cp._ws_fold23), ("fold_direct", cp._ws_fold_det)]


def zero_runs(t):
    """[[start, length], ...] of the runs of zeros of a tensor, flat."""
    z = (t.reshape(-1) == 0).to(torch.int8)
    edge = torch.diff(z, prepend=z.new_zeros(1), append=z.new_zeros(1))
    starts, ends = (edge == 1).nonzero().flatten().tolist(), (edge == -1).nonzero().flatten().tolist()
    return [[s, e - s] for s, e in zip(starts, ends)]


def _layer(name):
    couts, cin, k, _ = LAYERS[name]
    from rpg_ramnet_amd import ops
    ws = [torch.nn.Parameter(torch.zeros(c, cin, k, k)) for c in couts]
    bs = [torch.nn.Parameter(torch.zeros(c)) for c in couts]
    if name == "k3_64_frozen_w":
        ws[0].requires_grad_(False)
    cp = ops.ConvParam(ws, bs)
    return cp.s2d() if LAYERS[name][3] == "s2d" else cp


def _ask(cp, what):
    """The accessors a backward pass of this form calls -> (the workspace its launches write, the taps and the wino24 argument of a launch)."""
    from rpg_ramnet_amd import ops
    if what in ("grad_ws", "grad_ws_wino", "s2d"):
        return cp.grad_ws(wino_ok=what != "grad_ws")[0], ops.Taps.get("conv", cp.k, cp.k // 2), False
    cp.grad_ws_fold()
    if what == "fold_direct":
        return cp.grad_ws_fold_det()[0], ops.Taps.get("fold", 4, 0, 0, 0), False
    return cp.grad_ws_fold24(what), ops.Taps.get("fold", 4, 0, 0, 0), ops._FOLD_LAYOUTS[what][1]


def run_row(row):
    """The record of one row: two passes of one layer."""
    from rpg_ramnet_amd import _hip, ops
    layer, det, w24, extra, end = ROWS[row]
    rec, st, out = Recorder(), ops._st, []
    with ops.switches(wgrad_winograd_2x4=w24, **extra, deterministic=det):
        try:
            ops._st = lambda: None
            _hip.set_tracer(rec)
            cp = _layer(layer)
            for _ in range(2):
                rec.calls = []
                ws, taps, wino24 = _ask(cp, LAYERS[layer][3])
                x0, dout = torch.zeros(1, 8, 8, cp.CinWs), torch.zeros(1, 8, 8, cp.Cout)
                d = ops._wgrad_desc_build(x0, taps, dout, ws, cp.Cout, 1, None, None, 0, _hip.IN_PLAIN, None, 0, None, None, None, None, None,
                                          None, None, 0, wino24)
                p = {"layout": list(ops._layout_of(ws)), "det_slabs": ops._det_slabs(ws), "head_cin": getattr(ws, "head_cin", 0),
                     "dw_slabs": d.dw_slabs, "algo": d.algo, "numel": {n: (None if t is None else t.numel()) for n, t in workspaces(cp)}}
                for _, t in workspaces(cp):
                    if t is not None:
                        t.fill_(1.0)
                rec.watch(cp)
                if end == "discard":
                    ops._Engine.reset()                 # (cp.discard() of every layer of the aborted pass)
                else:
                    ops._Engine.flush()
                p["calls"] = rec.calls
                p["zero_runs"] = {n: zero_runs(t) for n, t in workspaces(cp) if t is not None}
                out.append(p)
        finally:
            _hip.set_tracer(None)
            ops._st = st
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "gradws_lifecycle.json"))
    a = ap.parse_args()
    doc = {}
    for row in ROWS:
        doc[row] = run_row(row)
        print(row, [len(p["calls"]) for p in doc[row]], flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
