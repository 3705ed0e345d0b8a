"""Probe, reference, histories and invariants of tests/test_hip_history.py (and the manners of changing a weight that
tests/test_history_cpu.py maps to pack launches): do the gradients of a training pass depend on what the process did before it?

The probe P is one training pass — zero_grad, trainer.sequence_loss, backward, synchronize — of the models and data of
tests/test_hip_deterministic_model.py (whose helpers live here): 32 base channels, 3 encoders, 2 residual blocks, B = 2, L = 2 packages of
K = 2 event grids, 5 bins, 32 x 48, SI loss on ["image", "events1"] plus the batched gradient loss at 0.25, 20 % NaN targets.  The
reference is P on a model built fresh and loaded with the probe weights W* (ops.invalidate_descs() and ops.invalidate_packs() before it,
nothing else).  A row builds a model with OTHER weights W0, runs its history, brings the model to W* in the manner it names, runs P and
asserts the invariants (check_probe / check_state below).  In deterministic mode "equal" is equality of bits; in the default mode it is the
project's run-to-run bound (test_wgrad_side_stream_gradients: 1e-5 of the tensor maximum above a floor of 1 % of the largest gradient,
`pred.conv2d.bias` left out).  The values themselves are held to the oracle elsewhere (test_bptt_gradients_vs_oracle and the fixtures)."""
import contextlib
import copy
import ctypes as C
import sys

import numpy as np
import torch
import torch.nn as nn

from util import GOLDEN, assert_close, build_hip_model

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from recipe import make_item  # noqa: E402

B, L, K, H, W = 2, 2, 2, 32, 48
LC = ["image", "events1"]


# ------------------------------------------------------------------------------------------------ the deterministic tests' helpers
def _cfg(**over):
    cfg = dict(num_bins_rgb=1, num_bins_events=5, skip_type="sum", recurrent_block_type="conv", state_combination="convgru", num_encoders=3,
               base_num_channels=32, num_residual_blocks=2, use_upsample_conv=True, norm="none", gpu=0, every_x_rgb_frame=K, baseline=False,
               loss_composition=LC)
    cfg.update(over)
    return cfg


def _same(a, b):
    """finite, and the same bits"""
    return a.shape == b.shape and bool(torch.isfinite(a).all()) and torch.equal(a, b) and \
        torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _targets_with_nan(rng, it, frac=0.2, keep=24):
    """NaN in `frac` of every depth map, none of it in the [keep x keep] corner (3 x 3 cells of the coarsest gradient-loss scale)"""
    for k in [k for k in it if k.startswith("depth_")]:
        d = it[k].clone()
        m = torch.from_numpy(rng.random(tuple(d.shape)) < frac / (1.0 - keep * keep / float(d.shape[-2] * d.shape[-1])))
        m[..., :keep, :keep] = False
        d[m] = float("nan")
        it[k] = d
    return it


def bench_schedule(det):
    from rpg_ramnet_amd import ops
    return ops.switches(wgrad_overlap=True, decoder_overlap=True, wgrad_defer=2, deterministic=det)


def _seq(model, seed, irregular=False, batch=B, height=H, width=W, nan=True):
    rng = np.random.default_rng(seed)
    seq = []
    for _ in range(L):
        it = make_item(rng, batch, height, width, K, 5, 1, True, 0.0)
        if nan:
            it = _targets_with_nan(rng, it)
        if irregular:
            item = {k: v for k, v in it.items() if not k.startswith("depth_")}
            item["num_events"] = torch.tensor([2, 1], dtype=torch.int64)
            item["depth_events_last"], item["depth_image_last"] = it["depth_events0"], it["depth_image"]
            it = item
        seq.append({k: (v if k == "num_events" else v.to(model.gpu)) for k, v in it.items()})       # (the counts are host data)
    return seq


def _loss(model, seq, lc, unet=False):
    from rpg_ramnet_amd import ops
    from rpg_ramnet_amd.trainer import sequence_loss
    if unet:        # the feed-forward wiring has no packages: the image branch of every item, SI loss (its stand-alone operator) on the image
        return sum(ops.scale_invariant_loss(model(it, None, None)[0]["image"], it["depth_image"]) for it in seq)
    return sequence_loss(model, seq, lc, [1, 1], grad_loss_weight=0.25)[0]


def _backward(model, seq, lc, unet=False, zero=True):
    if zero:
        model.zero_grad()
    total = _loss(model, seq, lc, unet)
    total.backward()
    torch.cuda.synchronize()
    return total.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


WIRINGS = {"convgru": ("ERGB2DepthRecurrent", {}, False), "convlstm": ("ERGB2DepthRecurrent", dict(state_combination="convlstm"), False),
           "ergb2depth_tconv": ("ERGB2Depth", dict(use_upsample_conv=False), False), "irregular": ("ERGB2DepthRecurrent", {}, True)}

# ------------------------------------------------------------------------------------------------ settings
HISTORY_WIRINGS = ("convgru", "convlstm", "ergb2depth_tconv")
_FORCE = {"winograd_2x4": "force", "wgrad_winograd_2x4": "force", "fold_winograd_2x3": "force"}
_S1 = {"wgrad_overlap": True, "decoder_overlap": True, "wgrad_defer": 2}
SETTINGS = {"S1": _S1, "S2": {**_S1, **_FORCE}}       # S2: these maps are far below the sizes at which the library picks those kernels itself
# (wiring, setting, deterministic): every setting in the mode whose contract is bits, the bench schedule once more in the mode that trains
MODES = [(s, True) for s in SETTINGS] + [("S1", False)]


def schedule(setting, det):
    """deterministic goes last in (the other switches refuse to change under it)"""
    from rpg_ramnet_amd import ops
    return ops.switches(**SETTINGS[setting], deterministic=det)


class Trace:
    """The launches of a pass: (name, algo, dw_slabs, head_cin, nseg) of the descriptor launches, (name,) of the others."""

    def __init__(self):
        from rpg_ramnet_amd import _hip
        self.sigs, self.calls = _hip._SIGS, []

    def __call__(self, name, fn, args):
        argtypes = self.sigs[name][1]
        if argtypes and argtypes[-1] is C.c_void_p:
            if name in ("ramnet_conv_launch", "ramnet_wgrad_launch"):
                d = args[0]._obj if hasattr(args[0], "_obj") else args[0]
                self.calls.append((name, d.algo, getattr(d, "dw_slabs", 0), d.head_cin, getattr(d, "nseg", 0)))
            elif name == "ramnet_conv_launch_multi":
                d = args[0]._obj if hasattr(args[0], "_obj") else args[0]
                self.calls += [(name, d[i].algo, 0, d[i].head_cin, 0) for i in range(args[1])]
            else:
                self.calls.append((name,))
        return fn(*args)

    def count(self, prefix):
        return sum(1 for c in self.calls if c[0].startswith(prefix))


@contextlib.contextmanager
def traced():
    from rpg_ramnet_amd import _hip
    t = Trace()
    _hip.set_tracer(t)
    try:
        yield t
    finally:
        _hip.set_tracer(None)


def reached(wiring, setting, calls):
    """{what the setting is there for: did the reference pass reach it}: asserted all True by test_the_settings_reach_their_kernels.
    The folded decoders exist with use_upsample_conv (not in ergb2depth_tconv), the multi-segment queue in the ConvGRU cells."""
    from rpg_ramnet_amd import _hip as Hh
    wg = [c for c in calls if c[0] == "ramnet_wgrad_launch"]
    fw = [c for c in calls if c[0] in ("ramnet_conv_launch", "ramnet_conv_launch_multi")]
    fold = wiring != "ergb2depth_tconv"
    out = {"head backward-weights launch": any(c[1] == Hh.ALGO_HEAD for c in wg)}
    if fold:
        out["fold launch"] = any(c[0].startswith("ramnet_fold_unpack_wgrad") for c in calls)
    if setting == "S2":
        out["backward-weights F(2x4,3x3) with slabs"] = any(c[1] == Hh.ALGO_WINOGRAD_2X4 and c[2] > 0 for c in wg)
        out["forward F(2x4,3x3)"] = any(c[1] == Hh.ALGO_WINOGRAD_2X4 for c in fw)
        if wiring == "convgru":
            out["multi-segment launch"] = any(c[4] > 1 for c in wg)
        if fold:
            out["F(2x3,4x4)"] = any(c[1] == Hh.ALGO_WINOGRAD24_2X3 for c in calls if len(c) > 1)
    return out


# ------------------------------------------------------------------------------------------------ manners of changing a weight
def _owner(model, name):
    mod = model
    parts = name.split(".")
    for p in parts[:-1]:
        mod = getattr(mod, p)
    return mod, parts[-1]


def set_weights(model, sd, manner="load_state_dict", invalidate=True):
    """Bring every parameter of `model` to the values of `sd` (name -> tensor) in the manner named."""
    from rpg_ramnet_amd import ops
    dev = next(model.parameters()).device
    sd = {k: v.detach().to(dev).clone() for k, v in sd.items()}
    if manner == "load_state_dict":
        model.load_state_dict(sd, strict=True)
    elif manner == "assign_true":
        model.load_state_dict(sd, strict=True, assign=True)
    elif manner == "new_parameter":
        for k, p in list(model.named_parameters()):
            mod, leaf = _owner(model, k)
            setattr(mod, leaf, nn.Parameter(sd[k], requires_grad=p.requires_grad))
    elif manner == "vector_to_parameters":
        names = [k for k, _ in model.named_parameters()]
        torch.nn.utils.vector_to_parameters(torch.cat([sd[k].reshape(-1) for k in names]), model.parameters())
    else:
        for k, p in model.named_parameters():
            if manner == "copy_":
                with torch.no_grad():
                    p.copy_(sd[k])
            elif manner == "detach_copy_":
                p.detach().copy_(sd[k])
            elif manner == "data_assign":
                p.data = sd[k]
            elif manner == "data_inplace":
                p.data.copy_(sd[k])
            else:
                raise KeyError(manner)
        if manner == "data_inplace" and invalidate:
            ops.invalidate_packs()           # the documented call after a write through .data ("Changing weights")


# manner -> does the next use of a layer re-run its pack launch by itself?  (a write through .data moves neither param._version nor
# data_ptr(): ops.invalidate_packs() is the call after it)
PACKS_FOLLOW = {"load_state_dict": True, "assign_true": True, "new_parameter": True, "vector_to_parameters": True, "copy_": True,
                "detach_copy_": True, "data_assign": True, "data_inplace": False}
MANNERS = tuple(PACKS_FOLLOW)


# ------------------------------------------------------------------------------------------------ a case: wiring x setting x mode
def layers(model):
    """[(module, name, ConvParam)] of every layer that has computed, its space-to-depth and state-half views behind it."""
    out = []
    for m in model.modules():
        for name, cp in m.__dict__.get("_cps", {}).items():
            out.append((m, name, cp))
    return out


def _live(m, name):
    """The nn.Parameters that layer `name` of module m stands over NOW (the lists of model/submodules.py), and its gates."""
    if name == "c":
        return [m.conv2d.weight], [m.conv2d.bias], 1
    if name == "t":
        return [m.transposed_conv2d.weight], [m.transposed_conv2d.bias], 1
    if name in ("c1", "c2"):
        c = m.conv1 if name == "c1" else m.conv2
        return [c.weight], [c.bias], 1
    if name == "g":
        return [m.Gates.weight], [m.Gates.bias], 4
    if name == "ur":
        return [m.update_gate.weight, m.reset_gate.weight], [m.update_gate.bias, m.reset_gate.bias], 1
    assert name == "o", name
    return [m.out_gate.weight], [m.out_gate.bias], 1


def _views(cp):
    return [("", cp)] + [(n, c) for n, c in (("s2d", cp._s2d), ("state_half", cp._state_half)) if c is not None]


def check_state(model, packs=True):
    """Invariants 2-4 after a pass: every gradient workspace all zero, the split-reduction counters zero, nothing dirty or queued, every
    pack that the next launch would be served equal in bits to the pack of a fresh ConvParam over the model's LIVE parameters — at
    least one per layer, unless packs=False: after a graph capture alone, whose closing ops.invalidate_packs() leaves eager code no
    pack to be served (the graph re-runs its own)."""
    from rpg_ramnet_amd import ops
    torch.cuda.synchronize()
    assert ops._Engine.dirty == [] and ops._Engine.task == -1 and getattr(ops._Engine, "outer", []) == []
    names, counts = [], []
    found = layers(model)
    assert found
    for m, name, cp in found:
        ws, bs, gates = _live(m, name)
        fresh = ops.ConvParam(ws, bs, gates)
        compared = 0
        for vname, c in _views(cp):
            what = "%s.%s%s" % (type(m).__name__, name, "." + vname if vname else "")
            assert c._dirty is False and c._defer == [], what
            for wname, r in c.workspaces():
                if r.t is not None:
                    names.append("%s workspace %s" % (what, wname))
                    counts.append(torch.count_nonzero(r.t))
            for n, t in c._splitk.items():
                names.append("%s split-reduction counters (%d)" % (what, n))
                counts.append(torch.count_nonzero(t[:64].view(torch.int32)))
            f = fresh if not vname else getattr(fresh, vname)()
            for key, (v, pack) in c._packs.items():
                if v != c._versions(c.weights):
                    continue                    # (made for earlier values under another switch: the next use re-runs it)
                kind, transposed = (key[1], key[0]) if isinstance(key, tuple) else (key, 0)
                want = f._build_pack(kind, transposed)
                compared += 1
                for a, b in zip(pack if isinstance(pack, tuple) else (pack,), want if isinstance(want, tuple) else (want,)):
                    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                        "%s: pack %r is not the pack of the live parameters" % (what, key)
        assert compared or not packs, "%s.%s: no pack at the current versions to compare (the pass packed none?)" % (type(m).__name__, name)
    for k, p in model.named_parameters():          # the per-pass sums of the launches that have no layer workspace (ops._PassSum)
        s = ops._PassSum.get(p) if hasattr(ops, "_PassSum") else None
        if s is not None and s.t is not None:
            assert s._dirty is False and s.p() is p, k
            names.append("%s pass sum" % k)
            counts.append(torch.count_nonzero(s.t))
    bad = [n for n, c in zip(names, torch.stack(counts).tolist()) if c]
    assert not bad, "not zero after the pass: %s" % ", ".join(bad[:6])


class Case:
    def __init__(self, wiring, setting, det):
        self.wiring, self.setting, self.det = wiring, setting, det
        self.arch, over, _ = WIRINGS[wiring]
        self.cfg = _cfg(**over)
        self.unet = self.arch == "ERGB2Depth"
        self.recurrent = not self.unet

    def model(self, seed):
        return build_hip_model(self.arch, self.cfg, seed=seed).train()

    def star(self):
        """W*: the probe weights (seed 0), on the host"""
        key = ("star", self.wiring)
        if key not in _SHARED:
            _SHARED[key] = {k: v.detach().cpu().clone() for k, v in self.model(0).state_dict().items()}
        return _SHARED[key]

    def probe_seq(self, model):
        key = ("seq", self.wiring)
        if key not in _SHARED:
            _SHARED[key] = _seq(model, 11)
        return _SHARED[key]

    def P(self, model, seq=None, zero=True):
        return _backward(model, self.probe_seq(model) if seq is None else seq, LC, self.unet, zero)

    def history_pass(self, model, seed=21, **shape):
        """a pass of the history: a finite loss is all it owes (targets without NaN)"""
        loss, _ = _backward(model, _seq(model, seed, nan=False, **shape), LC, self.unet)
        assert bool(torch.isfinite(loss)), "history pass: loss %r" % float(loss)
        return loss

    def fresh_pass(self, weights):
        """P on a model built fresh and loaded with `weights`, after ops.invalidate_descs() and ops.invalidate_packs() and nothing else:
        (loss, gradients, trace)"""
        from rpg_ramnet_amd import ops
        model = self.model(3)
        model.load_state_dict({k: v.clone() for k, v in weights.items()}, strict=True)
        ops.invalidate_descs()
        ops.invalidate_packs()
        with traced() as t:
            loss, grads = self.P(model)
        check_state(model)
        return loss, grads, t.calls

    def reference(self):
        """computed once per (wiring, setting, mode), shared and left unchanged"""
        key = ("ref", self.wiring, self.setting, self.det)
        if key not in _SHARED:
            _SHARED[key] = self.fresh_pass(self.star())
        return _SHARED[key]

    def check_probe(self, got, ref, what="", scale=1.0, bits=None):
        """Invariant 1: the loss and every .grad equal the reference (x scale), the same parameters have one.  Bits in deterministic mode
        (bits=False: the run-to-run bound there too — a pass that legitimately sums in another order)."""
        loss, grads = got
        rloss, rgrads = ref[0], ref[1]
        assert set(grads) == set(rgrads), "%s parameters with a gradient: %s" % (what, sorted(set(grads) ^ set(rgrads))[:4])
        assert any(k.endswith("pred.conv2d.bias") for k in rgrads)
        if self.det if bits is None else bits:
            assert _same(loss, rloss), "%s the loss differs from the reference: %r / %r" % (what, float(loss), float(rloss))
            for k in rgrads:
                assert _same(grads[k], rgrads[k] * scale), "%s %s differs from the reference" % (what, k)
            return
        assert np.isfinite(float(loss)) and np.isfinite(float(rloss))
        np.testing.assert_allclose(float(loss), float(rloss), rtol=1e-5)
        gmax = scale * max(float(v.abs().max()) for v in rgrads.values())
        for k in rgrads:
            if not k.endswith("pred.conv2d.bias"):      # (a sum of ~1e4 terms that cancels: its own summation-order noise)
                assert bool(torch.isfinite(grads[k]).all()), k
                assert_close(grads[k].cpu().numpy(), (rgrads[k] * scale).cpu().numpy(), 1e-5, what + " " + k, floor=1e-2 * gmax)

    def differs(self, got, ref):
        """the guard of the rows that change weights: P at W0 does NOT give the reference (else stale packs could pass)"""
        assert not torch.equal(got[0], ref[0]) and any(not torch.equal(got[1][k], ref[1][k]) for k in ref[1])


_SHARED = {}


def check_deferral(setting, det):
    """The multi-segment queue against one launch per update: the ConvGRU reference pass (wgrad_defer = 2) and the same fresh pass under
    wgrad_defer = 0 — two summation orders of the same terms, held to the run-to-run bound in either mode (no bits: the segments of one
    launch share a slab join).  A queue that loses an update loses a whole time step's share of the cells' gradients."""
    from rpg_ramnet_amd import ops
    case = Case("convgru", setting, det)
    with schedule(setting, det):
        ref = case.reference()
    assert any(c[0] == "ramnet_wgrad_launch" and c[4] > 1 for c in ref[2]), "the reference pass queued nothing"
    with ops.switches(**{**SETTINGS[setting], "wgrad_defer": 0}, deterministic=det):
        loss, grads, calls = case.fresh_pass(case.star())
    assert not any(c[0] == "ramnet_wgrad_launch" and c[4] > 1 for c in calls)
    case.check_probe((loss, grads), ref, "one launch per update:", bits=False)


# ------------------------------------------------------------------------------------------------ rows
def _finish(case, model, ref=None, what="", **kw):
    got = case.P(model)
    case.check_probe(got, case.reference() if ref is None else ref, what, **kw)
    check_state(model)
    return got


def _at_w0(case):
    """a model at W0 whose first pass is P itself (and does not give the reference)"""
    model = case.model(5)
    case.differs(case.P(model), case.reference())
    check_state(model)
    return model


def row_repeat(case):
    model = case.model(5)
    set_weights(model, case.star())
    for _ in range(2):
        case.P(model)
    _finish(case, model)


def _other_batch(case, model):
    for i, b in enumerate((3, 1)):
        case.history_pass(model, seed=22 + i, batch=b)


def row_other_batch(case):
    model = case.model(5)
    _other_batch(case, model)
    set_weights(model, case.star())
    _finish(case, model)


def row_other_map(case):
    model = case.model(5)
    for i, (h, w) in enumerate(((40, 56), (16, 24))):
        case.history_pass(model, seed=24 + i, height=h, width=w)
    set_weights(model, case.star())
    _finish(case, model)


def row_switch_tour(case):
    from rpg_ramnet_amd import ops
    model = case.model(5)
    tour = [{"winograd": False}, {"wgrad_slabs": False}, {**_FORCE, "split_operands": True, "split_wgrad": True},
            {"fold_winograd_wgrad": False}, {"space_to_depth": False}]
    with ops.switches(deterministic=False):          # (first out: the others refuse to change under it)
        for i, s in enumerate(tour):
            with ops.switches(**s):
                case.history_pass(model, seed=26 + i)
    assert ops.deterministic() == case.det
    set_weights(model, case.star())
    _finish(case, model)


def _map_state(s, f):
    return type(s)(_map_state(t, f) for t in s) if isinstance(s, (list, tuple)) else f(s)


def row_aborted(case):
    """the Boom pass of test_backward_recovers_after_an_aborted_pass under wgrad_defer = 2: the state after the first package goes
    through a node whose backward raises"""
    import pytest
    from rpg_ramnet_amd import ops
    from rpg_ramnet_amd.trainer import empty_states_lstm
    model = case.model(5)
    seq = _seq(model, 30, nan=False)

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            raise RuntimeError("injected failure in backward")

    model.zero_grad()
    preds, supers, lstms = model(seq[0], None, empty_states_lstm(K))
    carried = [_map_state(s, Boom.apply) for s in supers["image"]]
    preds2, _, _ = model(seq[1], carried, lstms)
    loss = sum(ops.scale_invariant_loss(preds2[k], seq[1]["depth_" + k]) for k in LC)
    with pytest.raises(RuntimeError, match="injected failure"):
        loss.backward()
    assert ops._Engine.dirty, "the aborted pass left weight-gradient workspaces behind (this is what the row exercises)"
    if case.wiring == "convgru":
        assert any(cp._defer for cp in ops._Engine.dirty), "... and a queue of deferred cell updates"
    del preds, supers, lstms, carried, preds2, loss
    set_weights(model, case.star())
    _finish(case, model)


def row_forward_only(case):
    from rpg_ramnet_amd.trainer import empty_states_lstm
    model = case.model(5)
    seq = _seq(model, 31, nan=False)
    args = (None, None) if case.unet else (None, empty_states_lstm(K))
    model.eval()
    with torch.no_grad():
        model(seq[0], *args)
    model.train()
    if case.wiring not in NO_GRAPHED_PACKAGE:
        from rpg_ramnet_amd.graph import GraphedPackage
        g = GraphedPackage(model, seq[0])
        for it in seq:
            g(it)
        torch.cuda.synchronize()
        assert model.training
    preds, _, _ = model(seq[1], *args)        # a training-mode forward whose graph is dropped without backward
    assert all(bool(torch.isfinite(v).all()) for v in preds.values())
    del preds
    set_weights(model, case.star())
    _finish(case, model)


def row_accumulate(case):
    """P twice without zero_grad in between: every .grad is twice the reference's — in bits (doubling is exact) —, the fold's += onto a
    gradient that is not zero"""
    model = case.model(5)
    set_weights(model, case.star())
    case.check_probe(case.P(model), case.reference(), "first pass")
    case.check_probe(case.P(model, zero=False), case.reference(), "second pass", scale=2.0)
    check_state(model)


def row_frozen_then_trained(case):
    model = case.model(5)
    frozen = [p for k, p in model.named_parameters() if "encoders" in k]
    assert frozen
    for p in frozen:
        p.requires_grad_(False)
    case.history_pass(model, seed=32)
    assert all(p.grad is None for p in frozen)
    for p in frozen:
        p.requires_grad_(True)
    set_weights(model, case.star())
    _finish(case, model)


def row_adam_step(case):
    """one pass at W0 and a fused-Adam step -> W1: the packs follow the optimizer's in-place update; the reference is a fresh model
    loaded with a clone of W1"""
    model = _at_w0(case)
    w0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    opt.step()
    w1 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert all(not torch.equal(w0[k], w1[k]) for k in w1 if not k.endswith("bias")), "the step moved every weight"
    ref1 = case.fresh_pass(w1)
    case.differs((ref1[0], ref1[1]), case.reference())
    _finish(case, model, ref=ref1)


def _row_manner(manner):
    def row(case):
        model = _at_w0(case)
        set_weights(model, case.star(), manner)
        _finish(case, model)
        for k, p in model.named_parameters():        # the gradients are the live parameters' own
            assert p.grad is not None, k
    row.__name__ = "row_" + manner
    return row


def row_cpu_round_trip(case):
    model = _at_w0(case)
    set_weights(model, case.star())
    dev = model.gpu
    model.cpu()
    assert all(not p.is_cuda for p in model.parameters())
    model.to(dev)
    _finish(case, model)


def _storages(model):
    """data_ptr of every workspace and pack tensor of the model's layers"""
    out = set()
    for _, _, cp in layers(model):
        for _, c in _views(cp):
            out |= {r.t.data_ptr() for _, r in c.workspaces() if r.t is not None}
            for _, pack in c._packs.values():
                out |= {t.data_ptr() for t in (pack if isinstance(pack, tuple) else (pack,))}
    return out


def row_deepcopy(case):
    model = _at_w0(case)
    set_weights(model, case.star())
    twin = copy.deepcopy(model)
    assert layers(twin), "the copy of a warmed model is warm"
    _finish(case, twin, what="the copy:")
    _finish(case, model, what="the original:")
    a, b = _storages(model), _storages(twin)
    assert a and b and not (a & b), "a workspace or a pack is shared between a model and its copy"
    for (k, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert p is not q and p.grad is not None and q.grad is not None and p.grad.data_ptr() != q.grad.data_ptr(), k
    for m, name, cp in layers(twin):
        ws, bs, _ = _live(m, name)
        assert cp.holds(ws, bs)


def row_two_models(case):
    """the caches keyed on id(cp), id(dw), id(taps) and the per-device partial buffers with two models in one process — and in ONE pass"""
    a, b = case.model(5), case.model(6)
    case.history_pass(a, seed=33)
    case.history_pass(b, seed=34)
    for m in (a, b):
        m.zero_grad()
    sa, sb = _seq(a, 35, nan=False), _seq(a, 36, nan=False)
    total = _loss(a, sa, LC, case.unet) + _loss(b, sb, LC, case.unet)
    total.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(total))
    check_state(a)
    check_state(b)
    set_weights(a, case.star())
    _finish(case, a)


def _replay(case, g, model):
    from_graph = g()
    torch.cuda.synchronize()
    return from_graph[0].detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def row_graph_then_eager(case):
    from rpg_ramnet_amd.graph import GraphedTrainStep
    model = case.model(5)
    g = GraphedTrainStep(model, _seq(model, 37, nan=False), LC, [1, 1], grad_loss_weight=0.25)
    for _ in range(2):
        g()
    torch.cuda.synchronize()
    set_weights(model, case.star())
    _finish(case, model, what="eager after the graph:")
    g.load(case.probe_seq(model))           # the graph re-runs its packs: a replay at W* with the probe's data is P
    case.check_probe(_replay(case, g, model), case.reference(), "replay:")
    check_state(model)


def row_eager_then_graph(case):
    from rpg_ramnet_amd.graph import GraphedTrainStep
    model = case.model(5)
    _other_batch(case, model)
    set_weights(model, case.star())
    g = GraphedTrainStep(model, case.probe_seq(model), LC, [1, 1], grad_loss_weight=0.25)
    case.check_probe(_replay(case, g, model), case.reference(), "replay:")
    check_state(model, packs=False)


def row_user_stream(case):
    model = _at_w0(case)
    set_weights(model, case.star())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = case.P(model)
    torch.cuda.current_stream().wait_stream(s)
    case.check_probe(got, case.reference())
    check_state(model)


def _row_checkpoint(reentrant):
    def row(case):
        """the residual blocks under torch.utils.checkpoint: the un-checkpointed reference's gradients for every parameter.  Where the
        blocks' backward is a graph task of its own (use_reentrant=True) a block that several of them touch folds once per task — another
        summation order than the reference's one fold: bits where the trace shows as many unpack launches as the reference's, else the
        run-to-run bound and bits between two runs."""
        from torch.utils.checkpoint import checkpoint
        from rpg_ramnet_amd.model.submodules import ResidualBlock
        model = case.model(5)
        set_weights(model, case.star())
        blocks = [m for m in model.modules() if isinstance(m, ResidualBlock)]
        assert len(blocks) == 2
        for rb in blocks:
            rb.forward = (lambda x, f=type(rb).forward.__get__(rb): checkpoint(f, x, use_reentrant=reentrant))
        ref = case.reference()
        with traced() as t:
            got = case.P(model)
        unpacks = lambda calls: sum(1 for c in calls if c[0].startswith("ramnet_unpack_wgrad"))        # noqa: E731
        one_fold = unpacks(t.calls) == unpacks(ref[2])
        assert one_fold or reentrant, "a forward re-run inside the pass's own graph task folds once"
        case.check_probe(got, ref, bits=case.det and one_fold)
        check_state(model)
        again = case.P(model)
        if case.det:
            case.check_probe(again, (got[0], got[1]), "second run:")
        check_state(model)
    row.__name__ = "row_checkpoint_" + ("reentrant" if reentrant else "plain")
    return row


ROWS = {
    "repeat": row_repeat, "other_batch": row_other_batch, "other_map": row_other_map, "switch_tour": row_switch_tour,
    "aborted": row_aborted, "forward_only": row_forward_only, "accumulate": row_accumulate,
    "frozen_then_trained": row_frozen_then_trained, "adam_step": row_adam_step,
    **{m: _row_manner(m) for m in MANNERS if m != "load_state_dict"},
    "cpu_round_trip": row_cpu_round_trip, "deepcopy": row_deepcopy, "two_models": row_two_models,
    "graph_then_eager": row_graph_then_eager, "eager_then_graph": row_eager_then_graph, "user_stream": row_user_stream,
    "checkpoint_reentrant": _row_checkpoint(True), "checkpoint_plain": _row_checkpoint(False),
}
# Rows whose state a wiring does not have.  The feed-forward wiring has no packages: no state to carry through a node that raises, and
# GraphedTrainStep runs trainer.sequence_loss, which steps through packages.  (A wiring without residual blocks would leave out the
# checkpoint_* rows here; these three have two blocks each.)
LEFT_OUT = {"ergb2depth_tconv": ("aborted", "graph_then_eager", "eager_then_graph")}
# ... and the one PART of a row that two wirings do not have: the inference through graph.GraphedPackage inside `forward_only` (the graphed
# package is the ConvGRU RAM-Net's: it asserts so); the row's eval() / no_grad package and dropped training forward run for all three.
NO_GRAPHED_PACKAGE = ("convlstm", "ergb2depth_tconv")
CASES = [(w, s, d, r) for w in HISTORY_WIRINGS for s, d in MODES for r in ROWS if r not in LEFT_OUT.get(w, ())]


def case_id(c):
    return "%s-%s-%s-%s" % (c[0], c[1], "det" if c[2] else "default", c[3])


def run_row(wiring, setting, det, row):
    case = Case(wiring, setting, det)
    with schedule(setting, det):
        case.reference()
        ROWS[row](case)
