"""Per-sample update masks (ramnet_conv_desc.active, ABI 25) and batches of irregular packages (ERGB2DepthRecurrent.forward with
`num_events`): the masked cell launches of every kernel family, the C ABI, the network against a float64 per-sample
loop of the oracle, padding independence, agreement with the regular path and graph replay with a rewritten device mask."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import loss_ref, ramnet_ref
from recipe import make_item
from util import assert_close, build_hip_model, nchw, ref_cfg

pytestmark = pytest.mark.gpu

TOL = 1e-3


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


@pytest.fixture(params=["igemm", "f2x2", "f2x4", "f2x4_split"])
def family(request):
    """Force each family a cell launch can take: the direct implicit GEMM, F(2x2,3x3), F(2x4,3x3), F(2x4,3x3) on split operands."""
    from rpg_ramnet_amd import ops
    with ops.switches(winograd=request.param != "igemm", winograd_2x4="force" if request.param.startswith("f2x4") else "off",
                      split_operands=request.param == "f2x4_split"):
        yield request.param


CELL_CASES = [(3, 8, 16, 64, [1, 0, 1]), (2, 16, 32, 128, [0, 1]), (4, 4, 43, 256, [0, 1, 1, 0]),
              (1, 4, 43, 256, [0]), (1, 4, 43, 256, [1])]          # (batch 1 on a coarse map: the split-reduction launch)


def _cell(kind, C):
    from rpg_ramnet_amd.model.submodules import ConvGRU, ConvLSTM
    torch.manual_seed(5)
    m = (ConvGRU if kind == "gru" else ConvLSTM)(C, C, 3)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.uniform_(-0.1, 0.1)
    return m.to(dev())


@pytest.mark.parametrize("kind", ["gru", "lstm"])
@pytest.mark.parametrize("B,H,W,C,mask", CELL_CASES)
def test_masked_cell(kind, B, H, W, C, mask, family):
    """Active samples bit-identical to the unmasked call; inactive h (and c) bit-identical to the input state (-0.0 included);
    inactive samples get dh = dh', dc = dc' and dx = 0 exactly; the weight gradients are those of the active sub-batch (float64)."""
    m = _cell(kind, C)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, H, W, C, generator=g).to(dev())
    h = torch.tanh(torch.randn(B, H, W, C, generator=g))
    h[:, ::3, ::2, ::5] = -0.0
    h = h.to(dev())
    c = torch.randn(B, H, W, C, generator=g).to(dev())
    act = torch.tensor(mask, dtype=torch.bool)
    ina = ~act
    state = h if kind == "gru" else (h, c)
    with torch.no_grad():
        ref = m(x, state)
    xg, hg, cg = (t.clone().requires_grad_(True) for t in (x, h, c))
    out = m(xg, hg if kind == "gru" else (hg, cg), active=act.to(dev()))
    outs = (out,) if kind == "gru" else out
    refs = (ref,) if kind == "gru" else ref
    ins = (h,) if kind == "gru" else (h, c)
    for o, r, i in zip(outs, refs, ins):
        assert torch.equal(bits(o)[act], bits(r)[act]), "active samples differ from the unmasked launch"
        assert torch.equal(bits(o)[ina], bits(i)[ina]), "inactive samples do not keep their state bit for bit"
    wts = [torch.randn(B, H, W, C, generator=g) for _ in outs]
    sum((o * w.to(dev())).sum() for o, w in zip(outs, wts)).backward()
    assert torch.equal(hg.grad.cpu()[ina], wts[0][ina]), "dh != dh' on inactive samples"
    assert bool((xg.grad.cpu()[ina] == 0).all()), "dx != 0 on inactive samples"
    if kind == "lstm":
        assert torch.equal(cg.grad.cpu()[ina], wts[1][ina]), "dc != dc' on inactive samples"
    if not bool(act.any()):
        for p in m.parameters():
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
        return
    # float64 oracle on the active samples alone
    sd = {"L." + k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    xa, ha, ca = (nchw(t[act.to(dev())].cpu()).double() for t in (x, h, c))
    if kind == "gru":
        r64 = (ramnet_ref.conv_gru(sd, "L", xa, ha),)
    else:
        r64 = ramnet_ref.conv_lstm(sd, "L", xa, (ha, ca))
    sum((r * nchw(w[act]).double()).sum() for r, w in zip(r64, wts)).backward()
    gmax = max(float(v.grad.abs().max()) for v in sd.values() if v.grad is not None)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        assert_close(p.grad.cpu().numpy(), sd["L." + k].grad.numpy(), TOL, "grad " + k, floor=1e-2 * gmax)


def test_cabi_masked_descriptors():
    """Masked descriptors through ctypes: a cell epilogue runs on every algorithm that takes it; a non-cell epilogue, a masked ConvLSTM
    cell without e0 and the algorithms without masked kernels are refused with RAMNET_E_BADARG."""
    from rpg_ramnet_amd import _hip as H, ops
    m = _cell("gru", 64)
    B, Hh, W, C = 2, 8, 16, 64
    x, h = torch.randn(B, Hh, W, C, device=dev()), torch.randn(B, Hh, W, C, device=dev())
    act = torch.tensor([0, 1], dtype=torch.int32, device=dev())
    cp = m._cp("ur", [m.update_gate.weight, m.reset_gate.weight], [m.update_gate.bias, m.reset_gate.bias])
    ur = torch.empty(B, Hh, W, 2 * C, device=dev())
    L = H.lib()
    taps = ops.Taps.get("conv", 3, 1)
    for algo, pack in ((H.ALGO_DIRECT, cp.pack(False, False)), (H.ALGO_WINOGRAD, cp.pack(False, True)),
                       (H.ALGO_WINOGRAD_2X4, cp.pack(False, "2x4")), (H.ALGO_WINOGRAD_2X4_SPLIT, cp.pack(False, "2x4s"))):
        d = ops._conv_desc(x, taps, pack, ur, 2 * C, x1=h, in_mode=H.IN_CAT, C1=C, bias=cp.bias(), epi=H.EPI_SIGMOID)
        d.algo, d.w, d.splitk_ws, d.splitk_floats, d.s2d_5x5 = algo, ops._p(pack), None, 0, 0
        d.active = ops._p(act)
        assert L.ramnet_conv_launch(ctypes.byref(d), ops._st()) == 0, (algo, L.ramnet_last_error())
        torch.cuda.synchronize()
        assert bool((ur[0] == 0).all()) and bool((ur[1] > 0).all()), algo
        for epi in (H.EPI_LINEAR, H.EPI_RELU):
            d.epi = epi
            assert L.ramnet_conv_launch(ctypes.byref(d), ops._st()) == H_E_BADARG, (algo, epi)
        d.epi = H.EPI_SIGMOID
    d = ops._conv_desc(x, taps, cp.pack(False, False), ur, 2 * C, x1=h, in_mode=H.IN_CAT, C1=C, bias=cp.bias(), epi=H.EPI_SIGMOID)
    d.algo, d.w, d.splitk_ws, d.splitk_floats = H.ALGO_DIRECT, ops._p(cp.pack(False, False)), None, 0
    d.active = ops._p(act)
    d.frame = 2
    assert L.ramnet_conv_launch(ctypes.byref(d), ops._st()) == H_E_BADARG
    # a masked ConvLSTM cell needs e0 = h
    lm = _cell("lstm", 64)
    lcp = lm._cp("g", [lm.Gates.weight], [lm.Gates.bias], gates=4)
    hn, cn = torch.empty_like(h), torch.empty_like(h)
    d = ops._conv_desc(x, taps, lcp.pack(False, False), hn, C, x1=h, in_mode=H.IN_CAT, C1=C, bias=lcp.bias(), epi=H.EPI_LSTM, e1=h, o1=cn)
    d.algo, d.w, d.splitk_ws, d.splitk_floats = H.ALGO_DIRECT, ops._p(lcp.pack(False, False)), None, 0
    d.active = ops._p(act)
    assert L.ramnet_conv_launch(ctypes.byref(d), ops._st()) == H_E_BADARG
    d.e0, d.lde0 = ops._p(h), C
    assert L.ramnet_conv_launch(ctypes.byref(d), ops._st()) == 0, L.ramnet_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(hn[0]), bits(h[0])) and torch.equal(bits(cn[0]), bits(h[0]))


H_E_BADARG = 10001


# ------------------------------------------------------------------------------------------------------------ network level
COUNTS = [[4, 1, 0, 2], [3, 4, 2, 1]]


def _irregular_seq(rng, counts, B, H, W, kmax, c_ev, c_img, nan_frac=0.2):
    seq = []
    for cnt in counts:
        it = make_item(rng, B, H, W, kmax, c_ev, c_img, True, nan_frac)
        item = {k: v for k, v in it.items() if not k.startswith("depth_")}
        item["num_events"] = torch.tensor(cnt, dtype=torch.int64)
        item["depth_events_last"] = it["depth_events0"]
        item["depth_image_last"] = it["depth_image"]
        seq.append(item)
    return seq


def _zero_states(cfg, B, H, W, dtype=torch.float64):
    n, base = cfg["num_encoders"], cfg["base_num_channels"]
    out = []
    for i in range(n):
        z = torch.zeros(B, base * 2 ** (i + 1), H // 2 ** (i + 1), W // 2 ** (i + 1), dtype=dtype)
        out.append((z, z.clone()) if cfg["state_combination"] == "convlstm" else z)
    return out


def _oracle_irregular(sd, cfg, seq, lc, weights):
    """The reference branch's semantics as a float64 per-sample loop of the oracle's encoder / decoder; the SI loss on the stacked
    predictions (a mean over the whole batch)."""
    cfg = ramnet_ref.normalize_config(cfg)
    B, _, H, W = seq[0]["image"].shape
    states = [_zero_states(cfg, 1, H, W) for _ in range(B)]
    terms, outs = [], []
    for item in seq:
        ev_last, im_last = [], []
        for b in range(B):
            s = states[b]
            for k in range(int(item["num_events"][b])):
                s, _ = ramnet_ref._encode(sd, cfg, "events", item["events%d" % k][b:b + 1].double(), s, None)
            ev_last.append(ramnet_ref._decode(sd, cfg, s))
            s, _ = ramnet_ref._encode(sd, cfg, "images", item["image"][b:b + 1].double(), s, None)
            im_last.append(ramnet_ref._decode(sd, cfg, s))
            states[b] = s
        preds = {"events_last": torch.cat(ev_last, 0), "image_last": torch.cat(im_last, 0)}
        outs.append(preds)
        for key, w in zip(lc, weights):
            terms.append(w * loss_ref.scale_invariant_loss(preds[key], item["depth_" + key].double()))
    return torch.stack(terms).sum() / len(seq), outs, states


def _cfg(state):
    cfg, _ = ref_cfg("net_seeded_ramnet.npz", every_x_rgb_frame=2, loss_composition=["image_last", "events_last"])
    cfg["state_combination"] = state
    return cfg


def _run(model, seq, lc):
    from rpg_ramnet_amd.trainer import sequence_loss
    return sequence_loss(model, seq, lc, [1, 1])


@pytest.mark.parametrize("state", ["convgru", "convlstm"])
def test_irregular_network_vs_oracle(state):
    """B = 4, 32 x 48, L = 2, Kmax = 4, counts with 0 and Kmax, 20 % NaN targets: loss, predictions, final states and every gradient
    against the float64 per-sample loop; the same inputs under no_grad."""
    cfg = _cfg(state)
    lc = cfg["loss_composition"]
    model = build_hip_model("ERGB2DepthRecurrent", cfg).train()
    rng = np.random.default_rng(11)
    B, H, W = 4, 32, 48
    seq = _irregular_seq(rng, COUNTS, B, H, W, 4, 5, cfg["num_bins_rgb"])
    from rpg_ramnet_amd.trainer import empty_states_lstm
    prev, lstm = None, empty_states_lstm(2)
    preds_all = []
    for item in seq:
        preds, supers, lstm = model(item, prev, lstm)
        assert list(preds) == ["events_last", "image_last"]
        assert supers["image"] is supers["image_last"]
        preds_all.append(preds)
        prev = supers["image"]
    total, _ = _run(model, seq, lc)
    model.zero_grad()
    total.backward()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    ref_total, ref_preds, ref_states = _oracle_irregular(sd, cfg, seq, lc, [1, 1])
    ref_total.backward()
    np.testing.assert_allclose(float(total.detach()), float(ref_total.detach()), rtol=1e-4)
    for got, ref in zip(preds_all, ref_preds):
        for key in ("events_last", "image_last"):
            assert_close(got[key].detach().cpu().numpy(), ref[key].detach().numpy(), TOL, key, elem_tol=TOL)
    for i, s in enumerate(prev):
        r = torch.cat([ref_states[b][i] if state == "convgru" else ref_states[b][i][0] for b in range(B)], 0)
        got = s if state == "convgru" else s[0]
        assert_close(got.detach().cpu().numpy(), r.detach().numpy(), TOL, "state %d" % i)
    gmax = max(float(v.grad.abs().max()) for v in sd.values() if v.grad is not None)
    n = 0
    for k, p in model.named_parameters():
        if sd[k].grad is None:
            continue
        n += 1
        assert p.grad is not None, k
        assert_close(p.grad.cpu().numpy(), sd[k].grad.numpy(), 2e-3, "grad " + k, floor=1e-2 * gmax)
    assert n >= 40
    with torch.no_grad():
        prev, lstm = None, empty_states_lstm(2)
        for item, ref in zip(seq, ref_preds):
            preds, supers, lstm = model(item, prev, lstm)
            prev = supers["image"]
            for key in ("events_last", "image_last"):
                assert_close(preds[key].cpu().numpy(), ref[key].detach().numpy(), TOL, "no_grad " + key, elem_tol=TOL)


def test_irregular_padding_independence():
    """Refilling the padding grids with other finite data changes nothing: predictions, states and loss bit-identical, gradients 1e-5."""
    cfg = _cfg("convgru")
    lc = cfg["loss_composition"]
    model = build_hip_model("ERGB2DepthRecurrent", cfg).train()
    rng = np.random.default_rng(12)
    seq = _irregular_seq(rng, COUNTS, 4, 32, 48, 4, 5, cfg["num_bins_rgb"])
    seq2 = []
    for item in seq:
        it = dict(item)
        for k in range(4):
            e = it["events%d" % k].clone()
            pad = torch.as_tensor([k >= int(n) for n in item["num_events"]])
            e[pad] = torch.from_numpy(rng.standard_normal(tuple(e[pad].shape)).astype(np.float32)) * 7.0
            it["events%d" % k] = e
        seq2.append(it)
    res = []
    for s in (seq, seq, seq2):          # (the repeat: run-to-run order of the backward-weights accumulation, the noise floor)
        total, _ = _run(model, s, lc)
        model.zero_grad()
        total.backward()
        with torch.no_grad():
            preds, supers, _ = model(s[0], None, None)
        res.append((total.detach(), preds, supers["image"], {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert torch.equal(bits(res[0][0]), bits(res[2][0]))
    for key in ("events_last", "image_last"):
        assert torch.equal(bits(res[0][1][key]), bits(res[2][1][key])), key
    for a, b in zip(res[0][2], res[2][2]):
        assert torch.equal(bits(a), bits(b))
    gmax = max(float(g.abs().max()) for g in res[0][3].values())
    for k in res[0][3]:
        ref = res[0][3][k].double()
        scale = max(float(ref.abs().max()), 1e-2 * gmax)
        noise = float((res[1][3][k].double() - ref).abs().max()) / scale
        err = float((res[2][3][k].double() - ref).abs().max()) / scale
        assert err <= max(1e-5, 4 * noise), "%s: rel err %.3e (repeat of the same inputs: %.3e)" % (k, err, noise)


@pytest.mark.parametrize("state", ["convgru", "convlstm"])
def test_irregular_equals_regular_when_full(state):
    """Every n_b = Kmax = K: events_last / image_last / the states agree with forward()'s events{K-1} / image (2e-5)."""
    cfg = _cfg(state)
    K = 3
    cfg["every_x_rgb_frame"] = K
    cfg["loss_composition"] = ["image", "events%d" % (K - 1)]
    model = build_hip_model("ERGB2DepthRecurrent", cfg).eval()
    rng = np.random.default_rng(13)
    it = make_item(rng, 2, 32, 48, K, 5, cfg["num_bins_rgb"])
    irr = dict(it, num_events=torch.tensor([K, K]))
    with torch.no_grad():
        p1, s1, _ = model(it, None, None)
        p2, s2, _ = model(irr, None, None)
    assert_close(p2["events_last"].cpu().numpy(), p1["events%d" % (K - 1)].cpu().numpy(), 2e-5, "events_last")
    assert_close(p2["image_last"].cpu().numpy(), p1["image"].cpu().numpy(), 2e-5, "image_last")
    for a, b in zip(s2["image_last"], s1["image"]):
        a, b = (a, b) if state == "convgru" else (a[0], b[0])
        assert_close(a.cpu().numpy(), b.cpu().numpy(), 2e-5, "state")


def test_masked_update_graph_replay():
    """A masked update_events captured with torch.cuda.graph: rewriting the device mask and replaying equals the eager call bit for bit."""
    cfg = _cfg("convgru")
    model = build_hip_model("ERGB2DepthRecurrent", cfg).eval()
    B, H, W = 3, 32, 48
    g = torch.Generator().manual_seed(4)
    ev = torch.randn(B, 5, H, W, generator=g).to(dev())
    states = [torch.randn(s.shape, generator=g).to(dev()) for s in model.init_states(B, H, W)]
    mask = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev())
    with torch.no_grad():
        model.update_events(ev, states, active=mask)          # (warm-up: packs, descriptor cache)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out, _ = model.update_events(ev, states, active=mask)
        for m in ([0, 1, 1], [1, 1, 0], [0, 0, 0]):
            mask.copy_(torch.tensor(m, dtype=torch.int32))
            graph.replay()
            torch.cuda.synchronize()
            ref, _ = model.update_events(ev, states, active=torch.tensor(m, dtype=torch.bool))
            for a, b, s in zip(out, ref, states):
                assert torch.equal(bits(a), bits(b)), m
                keep = torch.tensor(m) == 0
                assert torch.equal(bits(a)[keep], bits(s)[keep]), m


def test_irregular_full_size():
    """B = 8, Kmax = 8 at 256 x 344, forward and backward: finite, and two samples agree with their batch-1 primitive chains."""
    cfg, _ = ref_cfg("net_seeded_ramnet.npz", every_x_rgb_frame=8, loss_composition=["image_last", "events_last"])
    cfg.update(num_encoders=3, base_num_channels=32, num_bins_events=5, num_bins_rgb=1)
    model = build_hip_model("ERGB2DepthRecurrent", cfg).train()
    rng = np.random.default_rng(14)
    counts = [int(c) for c in rng.integers(1, 9, 8)]
    counts[1] = 8
    item = _irregular_seq(rng, [counts], 8, 256, 344, 8, 5, 1)[0]
    total, _ = _run(model, [item], cfg["loss_composition"])
    total.backward()
    assert bool(torch.isfinite(total))
    for p in model.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    with torch.no_grad():
        preds, supers, _ = model(item, None, None)
        for b in (0, 1):
            s = model.init_states(1, 256, 344)
            for k in range(counts[b]):
                s, _ = model.update_events(item["events%d" % k][b:b + 1], s)
            pe = model.decode(s)
            s, _ = model.update_image(item["image"][b:b + 1], s)
            pi = model.decode(s)
            assert_close(preds["events_last"][b:b + 1].cpu().numpy(), pe.cpu().numpy(), TOL, "events_last %d" % b, elem_tol=TOL)
            assert_close(preds["image_last"][b:b + 1].cpu().numpy(), pi.cpu().numpy(), TOL, "image_last %d" % b, elem_tol=TOL)
            for a, r in zip(supers["image_last"], s):
                assert_close(a[b:b + 1].cpu().numpy(), nchw(r).cpu().numpy(), TOL, "state %d" % b)
