"""ConvParam's two tables (ops._PACKS: what differs between the packs of a layer; ops._LAYOUTS: the weight-gradient layouts of a
backward pass) and the tensor-attribute protocol between grad_ws and wgrad_launch, without a device or the library."""
import pytest
import torch

from rpg_ramnet_amd import _hip as H, ops

TAPS3, TAPS5 = ops.Taps.get("conv", 3, 1), ops.Taps.get("conv", 5, 2)
ALGO = {"direct": H.ALGO_DIRECT, "wino": H.ALGO_WINOGRAD, "wino6": H.ALGO_WINOGRAD_2X4, "dsplit": H.ALGO_DIRECT_SPLIT}


def desc(dw, taps=TAPS3, Cout=64, C=64):
    x0, dout = torch.zeros(1, 8, 8, C), torch.zeros(1, 8, 8, Cout)
    return ops._wgrad_desc_build(x0, taps, dout, dw, Cout, 1, None, None, 0, H.IN_PLAIN, None, 0, None, None, None, None, None, None, None, 0, False)


def fields(d):
    return [(name, bytes(getattr(d, name)) if name in ("dy", "dx") else getattr(d, name)) for name, _ in H.WgradDesc._fields_
            if name not in ("x0", "dout", "dw", "segs")]


def test_every_symbol_of_the_tables_is_declared():
    named = [e for entry in list(ops._PACKS.values()) + list(ops._LAYOUTS.values()) for e in entry if isinstance(e, str)]
    assert len(named) == 23 + 9          # (border has no size query; the slabs of direct / wino are plain arithmetic)
    for sym in named:
        assert sym in H._SIGS, sym


def test_pack_kinds():
    assert set(ops._PACKS) == {False, True, "head", "2x4", "2x4g", "2x4s", "fold", "fold24", "fold24d", "fold23", "fold23d", "border"}
    assert len(ops._PACKS) == 12
    # the argument lists match the declared signatures: (src, dst, integers..., stream) and (integers...) of the size query
    for kind, (elems, pack, args, skip) in ops._PACKS.items():
        a = args(64, 32, 3, 1, 4)
        assert len(H._SIGS[pack][1]) == (5 if kind == "border" else 2) + len(a) + 1, kind
        if elems is not None:
            assert len(H._SIGS[elems][1]) == len(a) - skip, kind
    assert ops._PACKS["fold"][2](64, 32, 5, 0, 1) == (64, 32, 8, 8, 0, 1)


def test_layout_kinds():
    assert set(ops._LAYOUTS) == set(ALGO)
    for kind, algo in ALGO.items():
        assert ops._LAYOUTS[kind][3] == algo


@pytest.mark.parametrize("kind", sorted(ALGO))
@pytest.mark.parametrize("slabs_on", [True, False])
def test_stamped_layout_reaches_the_descriptor(kind, slabs_on):
    ws = ops._stamp_layout(torch.zeros(4), kind, 5)
    assert ops._layout_of(ws) == (kind, 5)
    assert (ws.wino, ws.wino6, ws.wg_dsplit, ws.slabs, ws.head_cin) == (kind == "wino", kind == "wino6", kind == "dsplit", 5, 0)
    with ops.switches(wgrad_slabs=slabs_on):
        d = desc(ws)
    assert d.algo == ALGO[kind]
    assert d.dw_slabs == (5 if slabs_on and kind != "direct" else 0)
    assert d.head_cin == 0


def test_hand_stamped_tensors_give_the_same_descriptors():
    plain = torch.zeros(4)
    assert ops._layout_of(plain) == ("direct", 0) and desc(plain).algo == H.ALGO_DIRECT
    a = torch.zeros(4)
    a.wino = True
    assert fields(desc(a)) == fields(desc(ops._stamp_layout(torch.zeros(4), "wino", 0)))
    assert desc(a).algo == H.ALGO_WINOGRAD and desc(a).dw_slabs == 0
    b = torch.zeros(4)
    b.wino, b.wino6 = False, True
    assert fields(desc(b)) == fields(desc(ops._stamp_layout(torch.zeros(4), "wino6", 0)))
    assert desc(b).algo == H.ALGO_WINOGRAD_2X4
    # precedence of the reader: wg_dsplit over wino6 over wino
    c = torch.zeros(4)
    c.wino = c.wino6 = True
    assert ops._layout_of(c)[0] == "wino6"
    c.wg_dsplit, c.slabs = True, 3
    assert ops._layout_of(c) == ("dsplit", 3) and desc(c).algo == H.ALGO_DIRECT_SPLIT and desc(c).dw_slabs == 3


def test_head_layer():
    ws = torch.zeros(4)
    ws.head_cin = 5
    d = desc(ws, TAPS5, Cout=32, C=8)
    assert (d.algo, d.head_cin) == (H.ALGO_HEAD, 5)
    d = desc(ops._stamp_layout(torch.zeros(4), "direct", 1, head_cin=1), TAPS5, Cout=32, C=4)
    assert (d.algo, d.head_cin, d.dw_slabs) == (H.ALGO_HEAD, 1, 0)
    assert desc(ops._stamp_layout(torch.zeros(4), "direct", 1), TAPS5, Cout=32, C=8).algo == H.ALGO_DIRECT
