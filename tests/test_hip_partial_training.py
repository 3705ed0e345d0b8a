"""GPU: partial training — `p.requires_grad_(False)` honoured end to end (INTEGRATION.md "Partial training").

A frozen tensor gets no .grad (so Adam over model.parameters() leaves it alone), its backward-weights launches and folds do not run,
gradients still flow through its layer, and what does train gets the gradients of the all-trainable step.  Smallest shapes that reach
every path: two packages of K = 3 event grids + 1 frame at 2 x 32 x 48, ConvGRU / ConvLSTM / BatchNorm models, time-batched and pass by
pass.  Bound between two runs of one step: the suite's own (test_hip_model.test_wgrad_side_stream_gradients): 1e-5 max-norm with a floor of
1e-2 of the largest gradient, pred.conv2d.bias (a sum that cancels to rounding noise) left out."""
import json

import numpy as np
import pytest
import torch

import epoch_recipe as E
from recipe import make_item
from util import assert_close, build_hip_model, ref_cfg

pytestmark = pytest.mark.gpu

P = "statenetphasedrecurrent."
LC = ["image", "events2"]
SETS = {
    "A": dict(train_only=[P + "resblocks.*", P + "decoders.*", P + "pred.*"]),
    "B": dict(train_only=[P + "head_events.*", P + "encoders_events.*", P + "state_combination_events.*"]),
    "C_bias": dict(freeze=["*.bias"]),
    "C_gate": dict(freeze=["*.update_gate.weight"]),
    "E": dict(train_only=[P + "pred.conv2d.*"]),
    "norm": dict(freeze=["*.norm_layer.*", "*.bn1.*", "*.bn2.*"]),          # gamma / beta of every norm layer
}
MODELS = {"gru": "net_seeded_ramnet.npz", "lstm": "net_seeded_ramnet_lstm.npz", "bn": "norm_small_gru_bn.npz"}
CASES = ([("gru", s) for s in ("A", "B", "C_bias", "C_gate", "E")] + [("lstm", s) for s in ("A", "B", "C_bias", "E")]
         + [("bn", s) for s in ("A", "B", "C_bias", "norm")])
PRED_WGRAD = ("ramnet_pred_sigmoid_bwd", "ramnet_pred_sigmoid_si_bwd", "ramnet_pred_linear_bwd")
PRED_DGRAD = ("ramnet_pred_sigmoid_dgrad", "ramnet_pred_sigmoid_si_dgrad", "ramnet_pred_linear_dgrad")


def apply_set(model, name):
    from rpg_ramnet_amd.trainer import freeze
    s = SETS[name]
    frozen = freeze(model, s["train_only"], train_only=True) if "train_only" in s else freeze(model, s["freeze"])
    assert frozen and len(frozen) < len(list(model.parameters()))
    return set(frozen)


def make(tag):
    cfg, _ = ref_cfg(MODELS[tag], every_x_rgb_frame=3, loss_composition=LC)
    return build_hip_model("ERGB2DepthRecurrent", cfg).train(), cfg


_SEQ = {}


def sequence(cfg):
    key = cfg["num_bins_rgb"]
    if key not in _SEQ:
        rng = np.random.default_rng(5)
        _SEQ[key] = [make_item(rng, 2, 32, 48, 3, 5, cfg["num_bins_rgb"], True, 0.1) for _ in range(2)]
    return _SEQ[key]


def run(model, cfg, seq=None):
    """one forward + backward; the library calls of the backward pass alone -> (loss, {name: gradient or None}, [entry points])"""
    from rpg_ramnet_amd import _hip
    from rpg_ramnet_amd.trainer import sequence_loss
    model.zero_grad()
    total, _ = sequence_loss(model, seq if seq is not None else sequence(cfg), LC, [1, 1])
    names = []

    def tracer(name, fn, args):
        names.append(name)
        return fn(*args)
    _hip.set_tracer(tracer)
    try:
        total.backward()
    finally:
        _hip.set_tracer(None)
    torch.cuda.synchronize()
    return float(total.detach()), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}, names


_REF = {}


def reference(tag, tb):
    """the all-trainable step of a model, computed once per (model, schedule)"""
    from rpg_ramnet_amd import ops
    if (tag, tb) not in _REF:
        with ops.switches(time_batching=tb):
            model, cfg = make(tag)
            _REF[tag, tb] = run(model, cfg)
    return _REF[tag, tb]


def same_gradients(got, ref, frozen, what):
    gmax = max(float(v.abs().max()) for v in ref.values())
    for k, g in got.items():
        if k in frozen or k.endswith("pred.conv2d.bias"):
            continue
        assert g is not None, k
        assert_close(g.cpu().numpy(), ref[k].cpu().numpy(), 1e-5, "%s %s" % (what, k), floor=1e-2 * gmax)


@pytest.mark.parametrize("tb", [True, False], ids=["time_batched", "pass_by_pass"])
@pytest.mark.parametrize("tag,fs", CASES, ids=["%s-%s" % c for c in CASES])
def test_frozen_tensors_get_no_gradient_and_the_rest_the_same_one(tag, fs, tb):
    from rpg_ramnet_amd import ops
    ref_loss, ref_g, ref_names = reference(tag, tb)
    with ops.switches(time_batching=tb):
        model, cfg = make(tag)
        frozen = apply_set(model, fs)
        loss, g, names = run(model, cfg)
    # 1. no .grad on a frozen tensor, and Adam over ALL parameters (what the reference's BaseTrainer builds) leaves it bit for bit
    for k, p in model.named_parameters():
        assert (p.grad is None) == (k in frozen), k
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    torch.optim.Adam(model.parameters(), lr=3e-4).step()
    for k, p in model.named_parameters():
        if k in frozen:
            assert torch.equal(p.detach().view(torch.int32), before[k].view(torch.int32)), "frozen %s moved" % k
    # 2. the same loss, the same gradients
    assert loss == ref_loss
    same_gradients(g, ref_g, frozen, "%s set %s" % (tag, fs))
    # 3. what the backward pass launched
    count = lambda ns, what: sum(n == what for n in ns)     # noqa: E731
    cell_bwd = [n for n in names if n.startswith("ramnet_gru_bwd_") or n.startswith("ramnet_lstm_bwd")]
    if fs == "E":
        assert not count(names, "ramnet_wgrad_launch") and not count(names, "ramnet_conv_launch") and not count(names, "ramnet_conv_launch_multi")
        assert not cell_bwd
    if fs == "A":
        assert not cell_bwd
        assert count(names, "ramnet_wgrad_launch") < count(ref_names, "ramnet_wgrad_launch")
    if fs == "B":
        assert not any(n in PRED_WGRAD for n in names) and sum(n in PRED_DGRAD for n in names) >= 1
        assert not count(names, "ramnet_fold_unpack_wgrad") and count(ref_names, "ramnet_fold_unpack_wgrad")
    if fs in ("C_bias", "C_gate", "norm"):      # tensors frozen beside trainable ones that share their launches: every launch still runs
        assert count(names, "ramnet_wgrad_launch") == count(ref_names, "ramnet_wgrad_launch")


def test_deferred_cell_launches_with_frozen_gates():
    """set_wgrad_defer > 1 (bench.py's schedule) on the side stream: the queue of a frozen cell stays empty, a half-frozen one flushes."""
    from rpg_ramnet_amd import ops
    with ops.switches(wgrad_overlap=True, wgrad_defer=2):
        model, cfg = make("gru")
        _, ref_g, _ = run(model, cfg)
        for fs in ("B", "C_gate"):
            model, cfg = make("gru")
            frozen = apply_set(model, fs)
            _, g, _ = run(model, cfg)
            assert all((g[k] is None) == (k in frozen) for k in g)
            same_gradients(g, ref_g, frozen, "deferred, set %s" % fs)


def test_gradual_unfreezing_takes_effect_at_the_next_forward():
    """4. freeze set A, step, unfreeze everything, step again: the second step's gradients are those of a model that was never frozen
    and holds the same weights."""
    model, cfg = make("gru")
    frozen = apply_set(model, "A")
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)
    _, g, _ = run(model, cfg)
    assert all((g[k] is None) == (k in frozen) for k in g)
    opt.step()
    for p in model.parameters():
        p.requires_grad_(True)
    twin, _ = make("gru")
    twin.load_state_dict(model.state_dict())
    _, g2, _ = run(model, cfg)
    _, gt, _ = run(twin, cfg)
    assert all(v is not None for v in g2.values())
    same_gradients(g2, gt, set(), "after unfreezing")


def test_flat_grad_reducer_over_a_partly_frozen_model(monkeypatch):
    """5. The reducer's buffer and buckets cover the trainable tensors; the end-of-pass fold meets layers wholly outside it.  The
    collectives are stood in for by no-ops (world size 1: an all-reduce is the identity), so the early issue during the fold runs."""
    from rpg_ramnet_amd import parallel
    from rpg_ramnet_amd.trainer import sequence_loss
    monkeypatch.setattr(parallel.dist, "all_reduce", lambda *a, **k: None)
    logs = {}
    for fs in (None, "A"):
        model, cfg = make("gru")
        frozen = apply_set(model, fs) if fs else set()
        red = parallel.FlatGradReducer(model)
        monkeypatch.setattr(red, "_collective", lambda: True)
        try:
            assert len(red.params) == len(list(model.parameters())) - len(frozen)
            red.zero()
            total, _ = sequence_loss(model, sequence(cfg), LC, [1, 1])
            total.backward()
            red.all_reduce()
            red.wait()
            torch.cuda.synchronize()
            for k, p in model.named_parameters():
                assert (p.grad is None) == (k in frozen), k
                if k not in frozen:
                    assert p.grad.data_ptr() == red.views[p].data_ptr()
            assert float(red.flat.abs().max()) > 0
            # every bucket left exactly once, in index order
            assert [a for a, _ in red.issue_log] == [0] + [b for _, b in red.issue_log[:-1]] and red.issue_log[-1][1] == len(red.buckets)
            logs[fs] = (list(red.issue_log), len(red.buckets), red.early_buckets)
            if fs:
                name, p = next((k, p) for k, p in model.named_parameters() if k in frozen)
                p.requires_grad_(True)
                with pytest.raises(RuntimeError, match=name.replace(".", r"\.")):
                    red.zero()
                p.requires_grad_(False)
                red.zero()
        finally:
            red.close()
    # what an all-trainable model of the same buckets logs: the decoder's buckets leave during the fold, as they do there
    assert logs["A"][1] == logs[None][1] and logs["A"][0] == logs[None][0], logs


def test_graphed_train_step_bakes_the_flags_in():
    """6. GraphedTrainStep on set A: the replay's gradients are the eager step's; a flag that changed since the capture raises."""
    from rpg_ramnet_amd.graph import GraphedTrainStep
    model, cfg = make("gru")
    frozen = apply_set(model, "A")
    seq = [{k: v.to(model.gpu) for k, v in it.items()} for it in sequence(cfg)]
    _, eager, _ = run(model, cfg, seq)
    model.zero_grad()
    g = GraphedTrainStep(model, seq, LC, [1, 1])
    g()
    torch.cuda.synchronize()
    got = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    assert all((got[k] is None) == (k in frozen) for k in got)
    same_gradients(got, {k: v for k, v in eager.items() if v is not None}, frozen, "graph replay")
    name, p = next((k, p) for k, p in model.named_parameters() if k in frozen)
    p.requires_grad_(True)
    with pytest.raises(RuntimeError, match=name.replace(".", r"\.")):
        g()
    p.requires_grad_(False)
    g()
    torch.cuda.synchronize()


def test_sequence_trainer_epoch_with_train_only():
    """7. One epoch of the loaders of tests/epoch_recipe.py with config['trainer']['train_only']: the frozen tensors come back bit for
    bit, every trainable one has moved."""
    from rpg_ramnet_amd.trainer import SequenceTrainer
    cfg = json.loads(json.dumps(E.CONFIG))
    cfg["trainer"]["train_only"] = ["*decoders*", "*pred*", "*resblocks*"]
    mcfg, _ = ref_cfg("net_seeded_ramnet.npz", every_x_rgb_frame=E.K, loss_composition=["image", "events1"])
    model = build_hip_model("ERGB2DepthRecurrent", mcfg)
    train, _ = E.loaders()
    st = SequenceTrainer(cfg, model, train, None)
    trainable = {k for k, p in model.named_parameters() if p.requires_grad}
    assert trainable and all(any(s in k for s in ("decoders", "pred", "resblocks")) for k in trainable)
    assert set(st.frozen) == {k for k, _ in model.named_parameters()} - trainable and st.frozen
    st.optimizer = torch.optim.Adam(model.parameters(), **cfg["optimizer"])
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    log = st.train_epoch(1)
    torch.cuda.synchronize()
    assert np.isfinite(log["loss"])
    for k, p in model.named_parameters():
        same = torch.equal(p.detach().view(torch.int32), before[k].view(torch.int32))
        assert same == (k not in trainable), k
