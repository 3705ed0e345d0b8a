"""Host logic of partial training: trainer.freeze on a plain nn.Module, the config keys the trainers read, the flag checks of the
reducer, and the loud failure of ops.ensure_grad on a frozen tensor.  No GPU."""
import json

import pytest
import torch


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.enc = torch.nn.ModuleList([torch.nn.Conv2d(1, 2, 3), torch.nn.Conv2d(2, 2, 3)])
        self.dec = torch.nn.Conv2d(2, 1, 3)
        self.pred = torch.nn.Conv2d(1, 1, 1)


def trainable(m):
    return [n for n, p in m.named_parameters() if p.requires_grad]


def test_freeze_resolves_fnmatch_patterns_over_parameter_names():
    from rpg_ramnet_amd.trainer import freeze
    m = Net()
    assert freeze(m, ["enc.*"]) == ["enc.0.weight", "enc.0.bias", "enc.1.weight", "enc.1.bias"]
    assert trainable(m) == ["dec.weight", "dec.bias", "pred.weight", "pred.bias"]
    assert freeze(m, "*.bias") == ["enc.0.bias", "enc.1.bias", "dec.bias", "pred.bias"]      # a single pattern; already frozen ones are named again
    assert trainable(m) == ["dec.weight", "pred.weight"]
    m = Net()
    assert freeze(m, ["enc.[0].weight", "pred.w*"]) == ["enc.0.weight", "pred.weight"]
    with pytest.raises(KeyError):                   # patterns are case-sensitive
        freeze(m, ["ENC.*"])


def test_freeze_train_only_freezes_everything_else():
    from rpg_ramnet_amd.trainer import freeze
    m = Net()
    frozen = freeze(m, ["dec.*", "pred.*"], train_only=True)
    assert frozen == ["enc.0.weight", "enc.0.bias", "enc.1.weight", "enc.1.bias"]
    assert trainable(m) == ["dec.weight", "dec.bias", "pred.weight", "pred.bias"]
    assert freeze(m, ["pred.bias"], train_only=True) == frozen + ["dec.weight", "dec.bias", "pred.weight"]      # never un-freezes: calls compose
    assert trainable(m) == ["pred.bias"]


def test_freeze_refuses_a_pattern_without_a_match_before_touching_anything():
    from rpg_ramnet_amd.trainer import freeze
    m = Net()
    for kw in (dict(), dict(train_only=True)):
        with pytest.raises(KeyError, match="decoder"):
            freeze(m, ["enc.*", "decoder.*"], **kw)
        assert len(trainable(m)) == 8


def test_trainers_read_the_two_config_keys():
    """The stub model of test_train_metrics_cpu.test_sequence_trainer_reads_the_config; absent keys = every tensor trains."""
    import epoch_recipe as E
    from rpg_ramnet_amd.trainer import SequenceTrainer, apply_freeze_config

    def stub():
        model = torch.nn.Conv2d(1, 1, 1)
        model.gpu, model.every_x_rgb_frame = torch.device("cpu"), 2
        return model
    train, _ = E.loaders()
    cfg = json.loads(json.dumps(E.CONFIG))
    model = stub()
    st = SequenceTrainer(cfg, model, train)
    assert st.frozen == [] and trainable(model) == ["weight", "bias"]
    cfg["trainer"]["freeze"] = ["bias"]
    model = stub()
    st = SequenceTrainer(cfg, model, train)
    assert st.frozen == ["bias"] and trainable(model) == ["weight"]
    cfg["trainer"].pop("freeze")
    cfg["trainer"]["train_only"] = ["b*"]
    model = stub()
    st = SequenceTrainer(cfg, model, train)
    assert st.frozen == ["weight"] and trainable(model) == ["bias"]
    assert apply_freeze_config(model, cfg) == ["weight"]                  # idempotent
    cfg["trainer"]["train_only"] = ["nothing*"]
    with pytest.raises(KeyError):
        SequenceTrainer(cfg, stub(), train)


def test_epoch_trainer_applies_the_keys_before_it_builds_the_optimizer(tmp_path):
    import epoch_recipe as E
    from rpg_ramnet_amd.trainer import EpochTrainer
    cfg = json.loads(json.dumps(E.CONFIG))
    cfg["trainer"]["save_dir"] = str(tmp_path)
    cfg["trainer"]["train_only"] = ["pred.*"]
    m = Net()
    et = EpochTrainer(m, cfg, lambda epoch: {"loss": 1.0, "val_loss": 1.0})
    assert et.frozen == [n for n, _ in m.named_parameters() if not n.startswith("pred.")] and trainable(m) == ["pred.weight", "pred.bias"]
    # the optimizer still holds every parameter, as the reference's does (checkpoints keep the reference layout); it skips what has no .grad
    assert sum(len(g["params"]) for g in et.optimizer.param_groups) == 8
    before = [p.detach().clone() for p in m.parameters()]
    for p in m.parameters():
        if p.requires_grad:
            p.grad = torch.ones_like(p)
    et.optimizer.step()
    for (n, p), b in zip(m.named_parameters(), before):
        assert torch.equal(p.detach(), b) == (not n.startswith("pred.")), n


def test_ensure_grad_refuses_a_frozen_tensor():
    from rpg_ramnet_amd import ops
    p = torch.nn.Parameter(torch.zeros(3))
    assert ops.ensure_grad(p) is p.grad and p.grad is not None
    q = torch.nn.Parameter(torch.zeros(3), requires_grad=False)
    with pytest.raises(AssertionError, match="frozen"):
        ops.ensure_grad(q)
    assert q.grad is None


def test_reducer_refuses_a_flag_that_changed_since_construction():
    from rpg_ramnet_amd.parallel import FlatGradReducer
    from rpg_ramnet_amd.trainer import freeze
    m = Net()
    frozen = freeze(m, ["enc.*"])
    red = FlatGradReducer(m, overlap=False)
    assert len(red.params) == 4 and red.flat.numel() == sum(p.numel() for n, p in m.named_parameters() if n not in frozen)
    red.zero()
    assert all((p.grad is None) == (n in frozen) for n, p in m.named_parameters())
    m.enc[1].bias.requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"enc\.1\.bias"):
        red.zero()
    m.enc[1].bias.requires_grad_(False)
    m.dec.weight.requires_grad_(False)
    with pytest.raises(RuntimeError, match=r"dec\.weight"):
        red.zero()


def test_header_declares_the_dgrad_entry_points_and_the_abi_version_stays():
    import os
    import re
    from rpg_ramnet_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "ramnet_hip.h")).read()
    for name in ("ramnet_pred_sigmoid_dgrad", "ramnet_pred_linear_dgrad", "ramnet_pred_sigmoid_si_dgrad"):
        assert re.search(r"\bint %s\(" % name, src) and name in _hip.EXPORTS
    assert int(re.search(r"#define RAMNET_ABI_VERSION (\d+)", src).group(1)) == 27
