"""No GPU: what the layer above the launches keeps between passes follows what the process does to the model — the host side of
tests/test_hip_history.py.  CPU tensors; the launches are recorded and not run (the recorder pattern of
tests/golden/make_golden_gradws_lifecycle.py), the host queries of the library are answered by the library.

* a layer whose nn.Parameter objects were replaced (`layer.conv2d.weight = nn.Parameter(...)`, load_state_dict(assign=True)) computes
  with, and folds into, the live ones: every ConvParam of every layer class of model/submodules.py, its s2d() and state_half() views
  included;
* the manners of changing a weight (history_cases.MANNERS), each mapped to whether the next use re-runs the pack launch;
* a backward pass inside a backward pass (torch.utils.checkpoint, use_reentrant=True) folds its own layers, once each, and discards
  nothing of the enclosing pass; a pass that raised is discarded by the next one, once."""
import ctypes as C

import pytest
import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

from history_cases import MANNERS, PACKS_FOLLOW, set_weights


class Recorder:
    """Records every call whose last argument is the stream as (name, args) and answers 0 without calling; host queries go through."""

    def __init__(self):
        from rpg_ramnet_amd import _hip
        self.sigs, self.calls = _hip._SIGS, []

    def __call__(self, name, fn, args):
        argtypes = self.sigs[name][1]
        if argtypes and argtypes[-1] is C.c_void_p:
            self.calls.append((name, args))
            return 0
        return fn(*args)

    def names(self, prefix):
        return [n for n, _ in self.calls if n.startswith(prefix)]


@pytest.fixture
def rec(monkeypatch):
    """Launches recorded, not run; everything on the calling stream (the side streams are HIP objects)."""
    from rpg_ramnet_amd import _hip, ops
    r = Recorder()
    monkeypatch.setattr(ops, "_st", lambda: None)
    with ops.switches(wgrad_overlap=False, decoder_overlap=False, fold_upsample=False):
        _hip.set_tracer(r)
        try:
            yield r
        finally:
            _hip.set_tracer(None)
            ops._Engine.reset()
    assert ops._Engine.dirty == [] and ops._Engine.task == -1 and getattr(ops._Engine, "outer", []) == []


def _layers():
    """name -> (layer, call, input channels): every layer class of model/submodules.py that owns a ConvParam."""
    from rpg_ramnet_amd.model import submodules as S
    return {
        "ConvLayer": (S.ConvLayer(8, 16, 3, 1, 1), lambda m, x: m(x), 8),
        "ConvLayer_s2d": (S.ConvLayer(32, 64, 5, 2, 2), lambda m, x: m(x), 32),          # (runs on its space-to-depth view)
        "UpsampleConvLayer": (S.UpsampleConvLayer(16, 8, 5, 1, 2), lambda m, x: m(x), 16),
        "TransposedConvLayer": (S.TransposedConvLayer(16, 8, 5, 2, 2), lambda m, x: m(x), 16),
        "ResidualBlock": (S.ResidualBlock(32, 32), lambda m, x: m(x), 32),
        "ConvLSTM": (S.ConvLSTM(32, 32, 3), lambda m, x: m(x)[0], 32),
        "ConvGRU": (S.ConvGRU(32, 32, 3), lambda m, x: m(x, None), 32),
        "RecurrentConvLayer": (S.RecurrentConvLayer(32, 32, recurrent_block_type="convgru"), lambda m, x: m(x, None)[0], 32),
        "Recurrent2ConvLayer": (S.Recurrent2ConvLayer(8, 32, 3, 1, 1, recurrent_block_type="convlstm"), lambda m, x: m(x, None)[0], 8),
    }


LAYERS = sorted(_layers())


def _pass(m, call, cin):
    x = torch.zeros(2, 8, 8, cin, requires_grad=True)
    call(m, x).sum().backward()


def _cps(m):
    return [cp for sub in m.modules() for cp in sub.__dict__.get("_cps", {}).values()]


@pytest.mark.parametrize("manner", ["new_parameter", "assign_true"])
@pytest.mark.parametrize("layer", LAYERS)
def test_a_replaced_parameter_is_the_one_computed_with_and_folded_into(rec, layer, manner):
    from rpg_ramnet_amd import ops
    torch.manual_seed(0)
    m, call, cin = _layers()[layer]
    _pass(m, call, cin)
    old = {k: p for k, p in m.named_parameters()}
    warm = _cps(m)
    assert warm and all(any(w is p for p in old.values()) for cp in warm for w in cp.weights)
    set_weights(m, {k: torch.full_like(v, 0.5) for k, v in m.state_dict().items()}, manner)
    live = {k: p for k, p in m.named_parameters()}
    assert all(live[k] is not old[k] for k in live), "the manner replaces the objects"
    m.zero_grad()
    rec.calls = []
    _pass(m, call, cin)
    cps = _cps(m)
    assert len(cps) == len(warm) and all(a is not b for a, b in zip(cps, warm))
    ids = {id(p) for p in live.values()}
    for cp in cps:
        held = list(cp.weights) + [b for b in cp.biases if b is not None]
        assert held and all(id(t) in ids for t in held), "ConvParam over parameters the layer no longer has"
        if cp.k == 5 and len(cp.weights) == 1 and cp.gates == 1:
            assert cp.s2d().weights[0] is cp.weights[0] and id(cp.s2d().biases[0]) in ids
        if cp.k == 3 and cp.Cin % 2 == 0:
            assert cp.state_half().weights[0] is cp.weights[0]
        assert not cp._dirty and cp._defer == []
    assert rec.names("ramnet_pack_"), "the new parameters were packed"
    for k, p in live.items():
        assert p.grad is not None, "%s: the fold went elsewhere" % k
        assert old[k].grad is None or old[k].grad is not p.grad
    assert ops._Engine.dirty == [] and ops._Engine.task == -1


@pytest.mark.parametrize("manner", sorted(MANNERS))
def test_which_manners_of_writing_a_weight_the_packs_follow(rec, manner):
    """history_cases.PACKS_FOLLOW: the pack launch of the next use, yes or no; after an in-place write through .data it is
    ops.invalidate_packs() that brings it."""
    from rpg_ramnet_amd import ops
    torch.manual_seed(0)
    m, call, cin = _layers()["ConvLayer"]
    with torch.no_grad():
        _ = call(m, torch.zeros(1, 8, 8, cin))
        rec.calls = []
        _ = call(m, torch.zeros(1, 8, 8, cin))
        assert rec.names("ramnet_pack_") == [], "an unchanged weight is not packed again"
        want = {k: torch.full_like(v, 0.25) for k, v in m.state_dict().items()}
        set_weights(m, want, manner, invalidate=False)
        assert all(torch.equal(m.state_dict()[k], want[k]) for k in want)
        rec.calls = []
        _ = call(m, torch.zeros(1, 8, 8, cin))
        assert bool(rec.names("ramnet_pack_")) == PACKS_FOLLOW[manner], manner
        if not PACKS_FOLLOW[manner]:
            ops.invalidate_packs()
            rec.calls = []
            _ = call(m, torch.zeros(1, 8, 8, cin))
            assert rec.names("ramnet_pack_"), "ops.invalidate_packs() is the call after a write through .data"
    assert m.cp().weights[0] is m.conv2d.weight


def _chain(monkeypatch):
    from rpg_ramnet_amd import ops
    from rpg_ramnet_amd.model.submodules import ConvLayer
    torch.manual_seed(0)
    a, b, c = (ConvLayer(16, 16, 3, 1, 1) for _ in range(3))
    discards = []
    real = ops.ConvParam.discard
    monkeypatch.setattr(ops.ConvParam, "discard", lambda self: (discards.append(self), real(self))[1])
    return a, b, c, discards


def _unpacks(rec, layers):
    """How often every layer's weight gradient was unpacked into its .grad (the second pointer of the unpack launch)."""
    grads = {m.conv2d.weight.grad.data_ptr(): i for i, m in enumerate(layers)}
    n = [0] * len(layers)
    for name, args in rec.calls:
        if name.startswith("ramnet_unpack_wgrad"):
            n[grads[args[1].value]] += 1
    return n


@pytest.mark.parametrize("reentrant", [True, False])
def test_a_backward_inside_a_backward_folds_its_own_layers_and_discards_nothing(rec, monkeypatch, reentrant):
    """a -> checkpoint(b) -> c: with use_reentrant=True b's backward is a graph task of its own inside the enclosing one, which has
    dirtied c by then; exactly one unpack per layer, no discard."""
    from rpg_ramnet_amd import ops
    a, b, c, discards = _chain(monkeypatch)
    tasks = []
    real = ops._Engine.mark.__func__
    monkeypatch.setattr(ops._Engine, "mark", classmethod(lambda cls, cp: (tasks.append(torch._C._current_graph_task_id()), real(cls, cp))[1]))
    x = torch.zeros(2, 8, 8, 16, requires_grad=True)
    c(checkpoint(b, a(x), use_reentrant=reentrant)).sum().backward()
    assert len(set(tasks)) == (2 if reentrant else 1), tasks
    assert discards == []
    assert _unpacks(rec, (a, b, c)) == [1, 1, 1]
    for m in (a, b, c):
        assert m.conv2d.weight.grad is not None and m.conv2d.bias.grad is not None
        assert not m.cp()._dirty
    assert ops._Engine.dirty == [] and ops._Engine.task == -1 and getattr(ops._Engine, "outer", []) == []


def test_a_pass_that_raised_is_discarded_by_the_next_one(rec, monkeypatch):
    from rpg_ramnet_amd import ops
    a, b, c, discards = _chain(monkeypatch)

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            raise RuntimeError("injected failure in backward")

    x = torch.zeros(2, 8, 8, 16, requires_grad=True)
    with pytest.raises(RuntimeError, match="injected failure"):
        c(Boom.apply(b(a(x)))).sum().backward()
    left = c.__dict__["_cps"]["c"]       # (c.cp() is a layer call: outside a backward pass it sweeps what an aborted one left)
    assert ops._Engine.dirty == [left] and left._dirty and discards == []
    rec.calls = []
    c(b(a(x))).sum().backward()
    assert discards == [left]
    assert _unpacks(rec, (a, b, c)) == [1, 1, 1]
    assert ops._Engine.dirty == [] and ops._Engine.task == -1 and getattr(ops._Engine, "outer", []) == []


def test_the_streaming_runner_sees_a_replaced_parameter_and_a_data_assignment():
    """graph.TimeBatchedStream._weights_version: per parameter (object, version, address), not a sum of versions."""
    from rpg_ramnet_amd.graph import TimeBatchedStream

    class Holder:
        pass
    h = Holder()
    h.model = nn.Conv2d(2, 2, 3)
    v0 = TimeBatchedStream._weights_version(h)
    assert TimeBatchedStream._weights_version(h) == v0
    h.model.weight.data = h.model.weight.data.clone()
    v1 = TimeBatchedStream._weights_version(h)
    h.model.weight = nn.Parameter(h.model.weight.detach().clone())
    v2 = TimeBatchedStream._weights_version(h)
    with torch.no_grad():
        h.model.bias.add_(1.0)
        h.model.weight.sub_(1.0)         # (a sum of versions would not see one going up ... and another parameter taking its place)
    v3 = TimeBatchedStream._weights_version(h)
    assert len({v0, v1, v2, v3}) == 4


def test_an_aborted_task_whose_callback_is_kept_alive_is_discarded_at_the_next_forward(rec, monkeypatch):
    """_Engine reads a queued callback that is still alive as an enclosing pass.  Should anything keep an aborted pass's callback alive
    (here: a list), the next forward outside any backward pass discards what it left (_Engine.sweep from _Lazy._cp): no layer stays dirty,
    every gradient of the next pass arrives."""
    from rpg_ramnet_amd import ops
    a, b, c, discards = _chain(monkeypatch)
    import functools
    kept = []

    def partial(*args):
        kept.append(functools.partial(*args))
        return kept[-1]
    monkeypatch.setattr(ops, "functools", type("F", (), {"partial": staticmethod(partial)}))

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            raise RuntimeError("injected failure in backward")

    x = torch.zeros(2, 8, 8, 16, requires_grad=True)
    with pytest.raises(RuntimeError, match="injected failure"):
        c(Boom.apply(b(a(x)))).sum().backward()
    left = c.__dict__["_cps"]["c"]
    assert len(kept) == 1 and ops._Engine.callback() is kept[0] and ops._Engine.dirty == [left] and discards == []
    rec.calls = []
    c(b(a(x))).sum().backward()
    assert discards == [left] and not left._dirty
    assert _unpacks(rec, (a, b, c)) == [1, 1, 1]
    assert ops._Engine.dirty == [] and ops._Engine.task == -1 and ops._Engine.outer == []


def test_a_model_pickles_after_a_backward_pass(rec):
    """the per-pass sums of the launches without a layer workspace (ops._PassSum) hang nothing on the nn.Parameter, whose attributes
    are pickled with it (torch.save(model))"""
    import pickle
    from rpg_ramnet_amd import ops
    m, call, cin = _layers()["TransposedConvLayer"]
    _pass(m, call, cin)
    bias = m.transposed_conv2d.bias
    assert ops._PassSum.get(bias) is not None and bias.grad is not None
    again = pickle.loads(pickle.dumps(bias))
    assert torch.equal(again, bias) and ops._PassSum.get(again) is None
    key = id(bias)
    del m, bias
    assert key not in ops._PassSum.table, "the sum goes with its parameter"
