"""GPU: gradients of the event grids and frames a model is fed (INTEGRATION.md "Input gradients"), through every forward path, against the
float64 oracle run on the same tensors as float64 leaves.  The weights are those of the explicit-weight fixtures (base_num_channels = 4),
two packages each, so the state carries a gradient back into the first package's inputs; 2 x 24 x 32 (the fixtures' own size).

Tolerance: the parameter-gradient rule of tests/test_hip_model.py — max-norm 2e-3 with a floor of 1e-2 of the largest input-gradient
magnitude of the run —, the loss to rtol 1e-4."""
import json

import numpy as np
import pytest
import torch

from oracle import loss_ref, ramnet_ref
from recipe import make_item
from util import assert_close, build_hip_model, load_golden

pytestmark = pytest.mark.gpu

LC = ["image", "events1"]
# fixture -> (architecture, event grids per package, channels of an event grid, loss composition)
NETS = {"net_small_gru": ("ERGB2DepthRecurrent", 2, 5, LC), "net_small_lstm": ("ERGB2DepthRecurrent", 2, 5, LC),
        "net_small_unet": ("ERGB2Depth", 0, 6, ["image"]), "net_small_base_ergb0": ("ERGB2DepthRecurrent", 2, 6, ["image"]),
        "net_small_base_rgb": ("ERGB2DepthRecurrent", 0, 5, ["image"]), "norm_small_gru_bn": ("ERGB2DepthRecurrent", 2, 5, LC)}


def is_input(k):
    return k == "image" or (k.startswith("events") and k[6:].isdigit())


def make(name, **over):
    z = load_golden(name + ".npz")
    cfg = json.loads(str(z["config"]))
    arch, n_ev, c_ev, lc = NETS[name]
    if len(lc) > 1:
        cfg["loss_composition"] = lc
    cfg.update(over)
    model = build_hip_model(arch, cfg).train()
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}, strict=True)
    return model, cfg


def sequence(name, H=24, W=32, seed=7):
    arch, n_ev, c_ev, lc = NETS[name]
    c_img = 6 if c_ev == 6 else 1
    rng = np.random.default_rng(seed)
    return [make_item(rng, 2, H, W, n_ev, c_ev, c_img, True, 0.1) for _ in range(2)]


def with_leaves(seq, dtype=torch.float32, device=None, all64=True):
    """the sequence with every event grid and frame as a leaf of its own (float64 leaves: the targets in float64 too, unless all64=False)"""
    out = []
    for it in seq:
        new = dict(it)
        for k, v in it.items():
            if is_input(k):
                new[k] = v.detach().to(dtype=dtype, device=device if device is not None else v.device).clone().requires_grad_(True)
            elif torch.is_tensor(v) and dtype == torch.float64 and all64 and v.is_floating_point():
                new[k] = v.double()
        out.append(new)
    return out


def grads_of(seq):
    return [{k: v.grad for k, v in it.items() if is_input(k)} for it in seq]


def state64(model):
    return {k: v.detach().cpu().double().clone() for k, v in model.state_dict().items()}


def oracle(model, cfg, seq, name, sd=None):
    """(loss, gradients) of the float64 oracle with the item tensors as float64 leaves"""
    arch, _, _, lc = NETS[name]
    seq64 = with_leaves(seq, torch.float64)
    total, _ = ramnet_ref.sequence_loss(sd if sd is not None else state64(model), dict(cfg, training=True), seq64, lc, [1] * len(lc), arch=arch)
    total.backward()
    return float(total.detach()), grads_of(seq64)


def hip(model, seq, name):
    from rpg_ramnet_amd.trainer import sequence_loss
    lc = NETS[name][3]
    leaves = with_leaves(seq)
    model.zero_grad()
    total, _ = sequence_loss(model, leaves, lc, [1] * len(lc))
    total.backward()
    torch.cuda.synchronize()
    return float(total.detach()), grads_of(leaves), leaves


def same(got, ref, what, used=None):
    gmax = max(float(g.abs().max()) for d in ref for g in d.values() if g is not None)
    assert gmax > 0
    n = 0
    for l, (dg, dr) in enumerate(zip(got, ref)):
        assert set(dg) == set(dr)
        for k, r in dr.items():
            if r is None:           # an input the wiring does not read
                assert dg[k] is None or float(dg[k].abs().max()) == 0.0, (what, l, k)
                continue
            g = dg[k]
            assert g is not None, "%s: package %d %s got no gradient" % (what, l, k)
            assert tuple(g.shape) == tuple(r.shape), (what, l, k)
            assert_close(g.detach().cpu().double().numpy(), r.numpy(), 2e-3, "%s package %d %s" % (what, l, k), floor=1e-2 * gmax)
            n += 1
    assert n >= 2 and (used is None or n == used), (what, n)


_REF = {}


def reference(name):
    """the oracle's loss and gradients of a fixture's sequence, computed once"""
    if name not in _REF:
        model, cfg = make(name)
        _REF[name] = oracle(model, cfg, sequence(name), name)
    return _REF[name]


@pytest.mark.parametrize("name,used", [("net_small_gru", 6), ("net_small_lstm", 6), ("net_small_unet", 2), ("net_small_base_ergb0", 6),
                                       ("net_small_base_rgb", 2)])
def test_inputs_receive_their_gradient(name, used):
    """Fails without the feature: .grad of every event grid and frame is None there."""
    model, cfg = make(name)
    ref_loss, ref = reference(name)
    loss, got, leaves = hip(model, sequence(name), name)
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-4)
    for it in leaves:
        for k in ("events0", "image"):
            if k in it and (k == "image" or name != "net_small_base_rgb"):
                assert it[k].grad is not None and it[k].grad.shape == it[k].shape and it[k].grad.device == it[k].device, (name, k)
    same(got, ref, name, used)


@pytest.mark.parametrize("path", ["time_batched", "pass_by_pass", "direct_head_kernel_off", "irregular", "primitives"])
def test_equivalent_paths(path):
    from rpg_ramnet_amd import ops
    name = "net_small_gru"
    if path in ("time_batched", "pass_by_pass", "direct_head_kernel_off"):
        sw = dict(head_kernel=False) if path == "direct_head_kernel_off" else dict(time_batching=path == "time_batched")
        ref_loss, ref = reference(name)
        with ops.switches(**sw):
            model, cfg = make(name)
            loss, got, _ = hip(model, sequence(name), name)
        np.testing.assert_allclose(loss, ref_loss, rtol=1e-4)
        return same(got, ref, path, 6)
    model, cfg = make(name)
    sd, ncfg = state64(model), ramnet_ref.normalize_config(cfg)
    seq = sequence(name)
    B, _, H, W = seq[0]["image"].shape

    def zero_states(b):
        return [torch.zeros(b, 4 * 2 ** (i + 1), H >> (i + 1), W >> (i + 1), dtype=torch.float64) for i in range(3)]
    if path == "irregular":
        # num_events = [2, 0]: sample 0 folds both grids, sample 1 none; per-sample float64 loop of the oracle's encoder / decoder
        from rpg_ramnet_amd.trainer import sequence_loss
        lc = ["image_last", "events_last"]
        model, cfg = make(name, loss_composition=lc)
        irr = [dict({k: v for k, v in it.items() if not k.startswith("depth_")}, num_events=torch.tensor([2, 0]),
                    depth_events_last=it["depth_events0"], depth_image_last=it["depth_image"]) for it in seq]
        leaves, l64 = with_leaves(irr), with_leaves(irr, torch.float64)
        total, _ = sequence_loss(model, leaves, lc, [1, 1])
        total.backward()
        states, terms = [zero_states(1) for _ in range(B)], []
        for it in l64:
            ev_last, im_last = [], []
            for b in range(B):
                s = states[b]
                for k in range(int(it["num_events"][b])):
                    s, _ = ramnet_ref._encode(sd, ncfg, "events", it["events%d" % k][b:b + 1], s, None)
                ev_last.append(ramnet_ref._decode(sd, ncfg, s))
                s, _ = ramnet_ref._encode(sd, ncfg, "images", it["image"][b:b + 1], s, None)
                im_last.append(ramnet_ref._decode(sd, ncfg, s))
                states[b] = s
            terms += [loss_ref.scale_invariant_loss(torch.cat(im_last, 0), it["depth_image_last"]),
                      loss_ref.scale_invariant_loss(torch.cat(ev_last, 0), it["depth_events_last"])]
        ref_total = torch.stack(terms).sum() / len(l64)
        ref_total.backward()
        np.testing.assert_allclose(float(total.detach()), float(ref_total.detach()), rtol=1e-4)
        got, ref = grads_of(leaves), grads_of(l64)
        for d in ref:           # sample 1 folds no grid: its rows of the event gradients are zero, in the oracle and here
            assert float(d["events0"][1].abs().max()) == 0.0
        for d in got:
            assert float(d["events0"][0].abs().max()) > 0.0
        return same(got, ref, path, 6)
    # the primitives: update_events x 2, update_image, decode; one package, the SI loss of the last decode
    it = seq[0]
    leaves, l64 = with_leaves([it]), with_leaves([it], torch.float64)
    st = model.init_states(B, H, W)
    for k in ("events0", "events1"):
        st, _ = model.update_events(leaves[0][k], st)
    st, _ = model.update_image(leaves[0]["image"], st)
    loss = ops.scale_invariant_loss(model.decode(st), it["depth_image"].to(model.gpu))
    loss.backward()
    s = zero_states(B)
    for k in ("events0", "events1"):
        s, _ = ramnet_ref._encode(sd, ncfg, "events", l64[0][k], s, None)
    s, _ = ramnet_ref._encode(sd, ncfg, "images", l64[0]["image"], s, None)
    ref_loss = loss_ref.scale_invariant_loss(ramnet_ref._decode(sd, ncfg, s), l64[0]["depth_image"])
    ref_loss.backward()
    np.testing.assert_allclose(float(loss.detach()), float(ref_loss.detach()), rtol=1e-4)
    same(grads_of(leaves), grads_of(l64), path, 3)


def test_batch_norm_behind_the_head():
    name = "norm_small_gru_bn"
    model, cfg = make(name)
    ref_loss, ref = oracle(model, cfg, sequence(name), name)
    loss, got, _ = hip(model, sequence(name), name)
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-4)
    same(got, ref, name, 6)


def test_full_frame_mode():
    """A 20 x 22 frame, num_encoders = 3: reflect-padded to 24 x 24 inside the input repack.  The oracle runs on the ReflectionPad2d-padded
    leaves (float64) and its predictions are cropped with the CropParameters window."""
    from rpg_ramnet_amd import ops
    name = "net_small_gru"
    model, cfg = make(name)
    model.set_full_frame(True)
    seq = sequence(name, 20, 22, seed=9)
    loss, got, _ = hip(model, seq, name)
    c = ops.CropParameters(22, 20, 3)
    assert (c.height_crop_size, c.width_crop_size) == (24, 24)
    pad = torch.nn.ReflectionPad2d((c.padding_left, c.padding_right, c.padding_top, c.padding_bottom))
    l64 = with_leaves(seq, torch.float64)
    sd, prev, lstm, terms = state64(model), None, ramnet_ref.empty_states_lstm(2), []
    for it in l64:
        preds, supers, lstm = ramnet_ref.forward_recurrent(sd, cfg, {k: (pad(v) if is_input(k) else v) for k, v in it.items()}, prev, lstm)
        prev = supers["image"]
        terms += [loss_ref.scale_invariant_loss(c.crop(preds[k]), it["depth_" + k]) for k in preds if k in LC]
    ref_total = torch.stack(terms).sum() / 2
    ref_total.backward()
    np.testing.assert_allclose(loss, float(ref_total.detach()), rtol=1e-4)
    same(got, grads_of(l64), "full frame", 6)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_no_change_for_callers_who_do_not_ask():
    """Deterministic mode: the loss and every parameter gradient of a step are bit for bit the same whether or not the inputs require a
    gradient; without requires_grad the packed input has no grad_fn (and with it, it has)."""
    from rpg_ramnet_amd import ops
    from rpg_ramnet_amd.trainer import sequence_loss
    name = "net_small_gru"
    seq = sequence(name)
    with ops.switches(deterministic=True):
        res = []
        for ask in (False, True):
            model, cfg = make(name)
            s = with_leaves(seq) if ask else seq
            total, _ = sequence_loss(model, s, LC, [1, 1])
            total.backward()
            torch.cuda.synchronize()
            res.append((total.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}))
        assert torch.equal(_bits(res[0][0]), _bits(res[1][0]))
        for k in res[0][1]:
            assert torch.equal(_bits(res[0][1][k]), _bits(res[1][1][k])), k
    x = seq[0]["events0"]
    assert ops.pack_input(x, model.gpu).grad_fn is None and not ops.pack_input(x, model.gpu).requires_grad
    with torch.no_grad():
        assert ops.pack_input(x.clone().requires_grad_(True), model.gpu).grad_fn is None
    assert ops.pack_input(x.clone().requires_grad_(True), model.gpu).grad_fn is not None


def test_input_gradients_with_frozen_weights():
    """inference.input_gradients: the leaf gradients of an ordinary backward pass bit for bit (deterministic mode), every parameter's
    .grad left None, its flags restored, and no backward-weights launch (the launch accounting of tests/test_hip_partial_training.py)."""
    from rpg_ramnet_amd import _hip, inference, ops
    name = "net_small_gru"
    seq = sequence(name)
    with ops.switches(deterministic=True):
        model, cfg = make(name)
        loss, ordinary, _ = hip(model, seq, name)
        model, cfg = make(name)
        names = []

        def tracer(nm, fn, args):
            names.append(nm)
            return fn(*args)
        _hip.set_tracer(tracer)
        try:
            total, got = inference.input_gradients(model, seq, LC)
        finally:
            _hip.set_tracer(None)
        torch.cuda.synchronize()
    assert float(total) == loss and not total.requires_grad
    assert all(p.grad is None and p.requires_grad for p in model.parameters())
    wgrad = ("ramnet_wgrad_launch", "ramnet_pred_sigmoid_bwd", "ramnet_pred_sigmoid_si_bwd", "ramnet_pred_linear_bwd", "ramnet_fold_unpack_wgrad",
             "ramnet_unpack_wgrad", "ramnet_bias_grad", "ramnet_bias_grad_ordered")
    assert not [n for n in names if n in wgrad], sorted(set(names))
    packs = names.count("ramnet_nchw_to_nhwc_pad")          # (time-batched: the K grids of a package in one repack, and its frame; two packages)
    assert packs >= 4 and names.count("ramnet_head_dgrad") == packs and names.count("ramnet_nhwc_unpad_to_nchw") == packs
    for dg, do, it in zip(got, ordinary, seq):
        assert set(dg) == {"events0", "events1", "image"}
        for k in dg:
            assert dg[k].shape == it[k].shape and dg[k].device == it[k].device and dg[k].dtype == it[k].dtype
            assert torch.equal(_bits(dg[k]), _bits(do[k].to(dg[k].device))), k


def test_cpu_float64_leaves_get_cpu_float64_gradients():
    name = "net_small_gru"
    model, cfg = make(name)
    from rpg_ramnet_amd.trainer import sequence_loss
    leaves = with_leaves(sequence(name), torch.float64, all64=False)
    total, _ = sequence_loss(model, leaves, LC, [1, 1])
    total.backward()
    for it in leaves:
        for k in ("events0", "events1", "image"):
            g = it[k].grad
            assert g is not None and g.dtype == torch.float64 and g.device.type == "cpu" and g.shape == it[k].shape and float(g.abs().max()) > 0
    same(grads_of(leaves), reference(name)[1], "cpu float64 leaves", 6)


def test_caller_supplied_states_receive_gradients():
    """Leaf tensors passed as prev_super_states (NCHW, as forward() returns them): one package on top of them, against the oracle."""
    from rpg_ramnet_amd.trainer import empty_states_lstm
    from rpg_ramnet_amd import ops
    name = "net_small_gru"
    model, cfg = make(name)
    it = sequence(name)[0]
    B, _, H, W = it["image"].shape
    g = torch.Generator().manual_seed(3)
    states = [torch.randn(B, 4 * 2 ** (i + 1), H >> (i + 1), W >> (i + 1), generator=g) * 0.5 for i in range(3)]
    dev = [s.to(model.gpu).requires_grad_(True) for s in states]
    s64 = [s.double().requires_grad_(True) for s in states]
    preds, _, _ = model(it, dev, empty_states_lstm(2))
    loss = sum(ops.scale_invariant_loss(preds[k], it["depth_" + k].to(model.gpu)) for k in LC)
    loss.backward()
    rp, _, _ = ramnet_ref.forward_recurrent(state64(model), cfg, {k: v.double() for k, v in it.items()}, s64, ramnet_ref.empty_states_lstm(2))
    ref = sum(loss_ref.scale_invariant_loss(rp[k], it["depth_" + k].double()) for k in LC)
    ref.backward()
    np.testing.assert_allclose(float(loss.detach()), float(ref.detach()), rtol=1e-4)
    same([{"s%d" % i: s.grad for i, s in enumerate(dev)}], [{"s%d" % i: s.grad for i, s in enumerate(s64)}], "caller-supplied states", 3)
