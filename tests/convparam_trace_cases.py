"""Workload, switch settings and call recorder shared by tests/test_hip_convparam_trace.py and the generator of its fixture
(tests/golden/make_golden_convparam_trace.py): the sequence of library launches that ConvParam's packs and weight-gradient layouts
produce, for the small ConvGRU / ConvLSTM networks of the BPTT fixtures and the narrow U-Net with folded decoders.

A record is "name|arg,arg,..." of one library call whose last argument is a stream (pure queries are left out): integers and
floats as they are, pointers as 0 (null) or p; a launch descriptor as its algo / Cout / dw_slabs / head_cin fields."""
import ctypes as C
import json

import numpy as np
import torch

from recipe import make_item
from util import build_hip_model, ref_cfg

# name -> {switch: value}, in the order ops.switches applies them.  The launch-side "force" switches ride with the backward-weights
# one: the maps of these networks are far below the sizes at which the library picks the F(2x4,3x3) / F(2x3,4x4) kernels by itself, and
# the split-operand weight gradient replaces the F(2x4,3x3) one, so it needs that layout selected first.
_FORCE = {"wgrad_winograd_2x4": "force", "winograd_2x4": "force", "fold_winograd_2x3": "force"}
SETTINGS = {
    "defaults": {},
    "wgrad_2x4_force": _FORCE,
    "split_operands": {**_FORCE, "split_operands": True, "split_wgrad": True},
    "winograd_off": {"winograd": False},
    "frozen_weight": {},
    # deterministic mode gives slabs to the direct, head and fold launches as well: with the decoders' one-launch form (F(2x2,4x4); at
    # these map sizes F(2x3,4x4) only when forced) and as four direct parity launches.  deterministic goes last in, first out: the
    # other switches refuse to change under it or it under them (the guards of the rows of ops._SWITCHES)
    "deterministic": {"deterministic": True},
    "deterministic_fold_direct": {"fold_winograd_wgrad": False, "deterministic": True},
    "deterministic_fold_2x3": {"fold_winograd_wgrad_2x3": "force", "deterministic": True},
    "wgrad_atomic": {"wgrad_slabs": False},        # the tile splits meet in slab 0 by atomic adds; the joins still run
}
DETERMINISTIC = ("deterministic", "deterministic_fold_direct", "deterministic_fold_2x3")
NETS = ("gru", "lstm", "unet")
CASES = [(net, s) for s in SETTINGS for net in NETS if s != "frozen_weight" or net == "gru"]
FROZEN = "resblocks.0.conv1.weight"          # a plain 3x3 layer: its bias still trains, the two share every launch

PACK_KINDS = {False, True, "head", "2x4", "2x4g", "2x4s", "fold", "fold24", "fold24d", "fold23", "fold23d", "border"}
LAYOUT_ALGOS = {"direct": 0, "wino": 1, "wino6": 4, "dsplit": 6}          # _hip.ALGO_* of a backward-weights launch
_PACK_OF = {"ramnet_pack_weight_wino": True, "ramnet_pack_weight_head": "head", "ramnet_pack_weight_wino2x4": "2x4",
            "ramnet_pack_weight_wino2x4_gates": "2x4g", "ramnet_pack_weight_wino2x4_split": "2x4s", "ramnet_pack_weight_fold_wino": "fold24",
            "ramnet_pack_weight_fold_wino_dgrad": "fold24d", "ramnet_pack_weight_fold_wino2x3": "fold23",
            "ramnet_pack_weight_fold_wino2x3_dgrad": "fold23d", "ramnet_pack_border_weights": "border"}
_DESC_CALLS = ("ramnet_conv_launch", "ramnet_conv_launch_multi", "ramnet_wgrad_launch")


def _desc(d):
    return "algo=%d/Cout=%d/slabs=%d/head=%d" % (d.algo, d.Cout, getattr(d, "dw_slabs", 0), d.head_cin)


def _arg(a):
    if a is None:
        return "0"
    if isinstance(a, bool):
        return str(int(a))
    if isinstance(a, (int, float)):
        return repr(a)
    if isinstance(a, C.c_void_p):
        return "p" if a.value else "0"
    if isinstance(a, bytes):
        return a.decode()
    return "p"


class Recorder:
    def __init__(self):
        from rpg_ramnet_amd import _hip
        self.sigs, self.calls = _hip._SIGS, []

    def __call__(self, name, fn, args):
        argtypes = self.sigs[name][1]
        if argtypes and argtypes[-1] is C.c_void_p:          # launches take their stream last; queries take none
            if name in _DESC_CALLS:
                d = args[0]._obj if hasattr(args[0], "_obj") else args[0]
                n = args[1] if name == "ramnet_conv_launch_multi" else 1
                head = [_desc(d[i]) for i in range(n)] if name == "ramnet_conv_launch_multi" else [_desc(d)]
                rest = args[2:-1] if name == "ramnet_conv_launch_multi" else args[1:-1]
            else:
                head, rest = [], args[:-1]
            self.calls.append(name + "|" + ",".join(head + [_arg(a) for a in rest]))
        return fn(*args)


def build(net):
    """(model in training mode, closure that runs forward + loss and returns the loss)."""
    rng = np.random.default_rng(17)
    if net == "unet":
        from rpg_ramnet_amd import ops
        cfg, z = ref_cfg("net_small_unet.npz")
        model = build_hip_model("ERGB2Depth", cfg).train()
        model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}, strict=True)
        item = make_item(rng, 2, 32, 32, 0, 1, cfg["num_bins_rgb"], True, 0.1)

        def loss():
            preds, _, _ = model(item, None, None)
            return ops.scale_invariant_loss(preds["image"], item["depth_image"].to(model.gpu))
        return model, loss
    from rpg_ramnet_amd.trainer import sequence_loss
    cfg, _ = ref_cfg("grads_seeded_ramnet.npz", state_combination="convlstm" if net == "lstm" else "convgru")
    model = build_hip_model("ERGB2DepthRecurrent", cfg).train()
    seq = [make_item(rng, 2, 32, 48, 2, 5, 1, True, 0.1)]
    return model, lambda: sequence_loss(model, seq, cfg["loss_composition"], [1, 1])[0]


def run_case(net, setting, after_first_backward=None):
    """Forward, backward, an in-place update of every trained parameter, forward and backward again: the records of the two passes."""
    from rpg_ramnet_amd import _hip, ops
    rec = Recorder()
    passes = []
    with ops.switches(**SETTINGS[setting]):
        try:
            model, loss = build(net)
            if setting == "frozen_weight":
                hit = [p for k, p in model.named_parameters() if k.endswith(FROZEN)]
                assert len(hit) == 1
                hit[0].requires_grad_(False)
            _hip.set_tracer(rec)
            for i in range(2):
                rec.calls = []
                model.zero_grad()
                loss().backward()
                torch.cuda.synchronize()
                passes.append(rec.calls)
                if i == 0:
                    if after_first_backward is not None:
                        _hip.set_tracer(None)
                        after_first_backward(model)
                        _hip.set_tracer(rec)
                    with torch.no_grad():
                        for p in model.parameters():
                            if p.grad is not None:
                                p.add_(p.grad, alpha=-1e-3)
        finally:
            _hip.set_tracer(None)
    return passes


def pack_kind(record):
    """The ConvParam pack kind that a pack launch's record stands for, None for any other call."""
    name, args = record.split("|")
    if name == "ramnet_pack_weight":
        return "fold" if args.split(",")[4] == "8" else False         # (src, dst, Cout, Cin, kh, kw, transposed, gates)
    return _PACK_OF.get(name)


def wgrad_algo(record):
    name, args = record.split("|")
    return int(args.split("/")[0][5:]) if name == "ramnet_wgrad_launch" else None


def wgrad_slabs(record):
    name, args = record.split("|")
    return int(args.split("/")[2][6:]) if name == "ramnet_wgrad_launch" else None


def encode(traces):
    """{case: [pass 1, pass 2]} -> JSON-able {"table": unique records, "cases": {case: [[index, ...], [index, ...]]}}."""
    table = {}
    cases = {k: [[table.setdefault(r, len(table)) for r in p] for p in passes] for k, passes in traces.items()}
    return {"table": list(table), "cases": cases}


def decode(doc):
    return {k: [[doc["table"][i] for i in p] for p in passes] for k, passes in doc["cases"].items()}


def dump(traces, path):
    with open(path, "w") as f:
        json.dump(encode(traces), f, separators=(",", ":"))
        f.write("\n")
