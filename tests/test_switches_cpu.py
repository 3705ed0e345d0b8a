"""No GPU: the switch table of rpg_ramnet_amd.ops — its rows and defaults, the environment variables that seed five of them, the setters that
bench.py, the tests and the tools call, the refusals, ops.switches' save-and-restore and the rows that the launch-descriptor caches depend on."""
import inspect
import json
import os
import subprocess
import sys

import pytest

from rpg_ramnet_amd import _hip, ops

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
# the values of the module globals (and of the library's options) before there was a table
DEFAULTS = {
    "abl_skip_wgrad": False, "winograd": True, "wgrad_slabs": True, "winograd_2x4": "auto", "wgrad_winograd_2x4": "auto", "fold_upsample": True,
    "fold_winograd": True, "fold_winograd_wgrad": True, "fold_pair": True, "fold_winograd_2x3": "auto", "fold_half_wg": "auto",
    "fold_winograd_wgrad_2x3": "auto", "fold_dgrad": True, "gru_bwd_fused": True, "gru_materialize_hr": True, "split_operands": False,
    "split_wgrad": False, "winograd_split": 1, "head_kernel": True, "space_to_depth": True, "space_to_depth_fused": True,
    "space_to_depth_2x4": True, "cell_state_half": "auto", "cell_state_half_min_pix": 0, "wgrad_overlap": False, "decoder_overlap": False,
    "branch_overlap": False, "wgrad_defer": 0, "time_batching": True, "time_batch_max_decodes": 0, "relu_premask": True, "si_fusion": True,
    "grad_loss_batched": True, "desc_cache": True, "deterministic": False,
}
ENV = {"RAMNET_ABL_SKIP_WGRAD": ("abl_skip_wgrad", "1"), "RAMNET_GRU_HR": ("gru_materialize_hr", "0"), "RAMNET_SPLIT_WGRAD": ("split_wgrad", "1"),
       "RAMNET_DESC_CACHE": ("desc_cache", "0"), "RAMNET_S2D_2X4": ("space_to_depth_2x4", "0")}
ONE_ARGUMENT = ["set_branch_overlap", "set_decoder_overlap", "set_deterministic", "set_fold_dgrad", "set_fold_upsample", "set_fold_winograd",
                "set_fold_winograd_2x3", "set_fold_winograd_wgrad", "set_fold_winograd_wgrad_2x3", "set_grad_loss_batched", "set_gru_bwd_fused",
                "set_gru_materialize_hr", "set_relu_premask", "set_si_fusion", "set_space_to_depth", "set_space_to_depth_fused",
                "set_split_operands", "set_split_wgrad", "set_wgrad_defer", "set_wgrad_overlap", "set_wgrad_slabs", "set_wgrad_winograd_2x4",
                "set_winograd", "set_winograd_split",
                # (called by nothing outside the package today, setters all the same)
                "set_fold_pair", "set_fold_half_wg", "set_head_kernel", "set_space_to_depth_2x4"]
TWO_ARGUMENTS = {"set_winograd_2x4": ("mode", "min_wgs"), "set_time_batching": ("on", "max_decodes"), "set_cell_state_half": ("mode", "min_pix")}
GETTERS = ["get_winograd", "deterministic", "get_split_operands", "get_split_wgrad", "get_fold_upsample", "get_head_kernel", "decoder_overlap",
           "branch_overlap", "wgrad_defer", "get_space_to_depth", "time_batch_max_decodes", "time_batching", "get_relu_premask", "si_fusion",
           "grad_loss_batched"]
IN_KEY = {"winograd", "winograd_2x4", "split_operands", "head_kernel", "space_to_depth_2x4", "fold_winograd_2x3",       # forward / backward-data
          "wgrad_slabs"}                                                                                                   # backward-weights (+ head_kernel)
INVALIDATE = {"split_operands": 1, "winograd_split": 1, "fold_pair": 1}          # invalidate_descs() calls of one change
FLIP = {"auto": "off", "off": "auto"}


def _fresh(env):
    e = {k: v for k, v in os.environ.items() if k not in ENV}
    e.update(env)
    out = subprocess.run([sys.executable, "-W", "ignore", "-c", "import json; from rpg_ramnet_amd import ops; print(json.dumps(ops.switch_values()))"],
                         cwd=ROOT, env=e, check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def _other(name):
    """A value of the row's domain that differs from the current one."""
    v = ops.switch_values()[name]
    return (not v) if isinstance(v, bool) else FLIP[v] if isinstance(v, str) else v + 2


def test_rows_and_defaults_in_a_fresh_process():
    assert _fresh({}) == DEFAULTS
    assert list(ops.switch_values()) == list(DEFAULTS)


@pytest.mark.parametrize("var", sorted(ENV))
def test_the_environment_seeds_its_row(var):
    name, text = ENV[var]
    want = dict(DEFAULTS)
    want[name] = not DEFAULTS[name]
    assert _fresh({var: text}) == want


def test_the_environment_names_and_the_defaults_own_spelling():
    assert {r.env: n for n, r in ops._SWITCHES.items() if r.env} == {var: name for var, (name, _) in ENV.items()}
    assert _fresh({var: "1" if DEFAULTS[name] else "0" for var, (name, _) in ENV.items()}) == DEFAULTS


def test_every_setter_and_getter_is_there_with_its_arguments():
    for name in ONE_ARGUMENT:
        p = list(inspect.signature(getattr(ops, name)).parameters.values())
        assert len(p) == 1 and p[0].default is inspect.Parameter.empty and p[0].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, name
        assert getattr(ops, name).__name__ == name
    for name, args in TWO_ARGUMENTS.items():
        p = inspect.signature(getattr(ops, name)).parameters
        assert tuple(p) == args and p[args[1]].default is None, name
    for name in ONE_ARGUMENT + list(TWO_ARGUMENTS):
        assert getattr(ops, name).__doc__ == ops._SWITCHES[name[4:]].doc
    for name in GETTERS:
        assert not inspect.signature(getattr(ops, name)).parameters
    assert callable(ops.set_finalize_hook) and callable(ops.invalidate_descs) and callable(ops.invalidate_packs)
    assert {"set_" + n for n, r in ops._SWITCHES.items() if r.setter} | set(TWO_ARGUMENTS) == set(ONE_ARGUMENT) | set(TWO_ARGUMENTS)
    for name, row in ops._SWITCHES.items():                          # the hot path's globals hold the values
        if row.var is not None:
            assert getattr(ops, row.var) == ops.switch_values()[name], name


def test_out_of_domain_values_raise_what_they_raised():
    before = ops.switch_values()
    for setter in (ops.set_winograd_2x4, ops.set_wgrad_winograd_2x4, ops.set_fold_winograd_2x3, ops.set_fold_winograd_wgrad_2x3, ops.set_cell_state_half):
        with pytest.raises(AssertionError):
            setter("on")
    with pytest.raises(KeyError):
        ops.set_fold_half_wg("on")
    for n in (-1, _hip.WGRAD_MAX_SEGMENTS + 1):
        with pytest.raises(AssertionError):
            ops.set_wgrad_defer(n)
    with pytest.raises(KeyError):
        with ops.switches(no_such_switch=True):
            pass
    assert ops.switch_values() == before
    with ops.switches(wgrad_defer=_hip.WGRAD_MAX_SEGMENTS):
        assert ops.wgrad_defer() == _hip.WGRAD_MAX_SEGMENTS
    with ops.switches(deterministic=True):
        with pytest.raises(RuntimeError, match=r"^set_wgrad_slabs\(False\) has no deterministic form: the atomic join of the backward-weights tile splits "
                                               r"contradicts set_deterministic\(True\)$"):
            ops.set_wgrad_slabs(False)
        with pytest.raises(RuntimeError, match=r"^set_grad_loss_batched\(False\) has no deterministic form: the unbatched multi-scale gradient loss joins by "
                                               r"atomic adds \(set_deterministic\(True\) is on\)$"):
            ops.set_grad_loss_batched(False)
    with ops.switches(wgrad_slabs=False, grad_loss_batched=False):
        with pytest.raises(RuntimeError, match=r"^set_deterministic\(True\) needs the slab join of the backward-weights launches: set_wgrad_slabs\(True\) first$"):
            ops.set_deterministic(True)                     # (the slab guard comes first)
    with ops.switches(grad_loss_batched=False):
        with pytest.raises(RuntimeError, match=r"^set_deterministic\(True\) needs the batched multi-scale gradient loss: set_grad_loss_batched\(True\) first$"):
            ops.set_deterministic(True)
    assert ops.switch_values() == before


NON_DEFAULT = dict(winograd_2x4="off", split_operands=True, wgrad_defer=3, fold_half_wg="force", fold_pair=False, winograd_split=4, wgrad_overlap=True,
                   time_batch_max_decodes=2, gru_bwd_fused=False)
INSIDE = dict(winograd_2x4="force", split_operands=False, wgrad_defer=7, fold_half_wg="off", fold_pair=True, winograd_split=0, wgrad_overlap=False,
              time_batch_max_decodes=5, gru_bwd_fused=True)


def _subset(names):
    v = ops.switch_values()
    return {n: v[n] for n in names}


def test_switches_puts_back_what_was_there():
    before = ops.switch_values()
    with ops.switches(**NON_DEFAULT):                   # (itself a check: everything returns to `before` at the end)
        start = ops.switch_values()
        assert _subset(NON_DEFAULT) == NON_DEFAULT and ops._WINO_2X4 == "off" and ops._WGRAD_DEFER == 3
        with ops.switches(**INSIDE):
            assert _subset(INSIDE) == INSIDE
        assert ops.switch_values() == start
        with pytest.raises(ZeroDivisionError):
            with ops.switches(**INSIDE):
                assert _subset(INSIDE) == INSIDE
                1 / 0
        assert ops.switch_values() == start
    assert ops.switch_values() == before


def test_switches_applies_in_order_and_restores_in_reverse():
    before = ops.switch_values()
    with ops.switches(wgrad_slabs=True, grad_loss_batched=True, deterministic=True):
        assert ops.deterministic() is True
        with ops.switches(deterministic=False, wgrad_slabs=False):         # un-nests deterministic -> wgrad_slabs, re-nests wgrad_slabs -> deterministic
            assert ops.switch_values()["wgrad_slabs"] is False and ops.deterministic() is False
        assert ops.deterministic() is True and ops._WGRAD_SLABS is True
    assert ops.switch_values() == before
    calls = []
    real = ops._set_switch
    ops._set_switch = lambda name, value: (calls.append((name, value)), real(name, value))[1]
    try:
        with ops.switches(wgrad_defer=2, winograd=False, wgrad_winograd_2x4="force"):
            pass
    finally:
        ops._set_switch = real
    assert calls == [("wgrad_defer", 2), ("winograd", False), ("wgrad_winograd_2x4", "force"),
                     ("wgrad_winograd_2x4", "auto"), ("winograd", True), ("wgrad_defer", 0)]


def test_a_refused_value_leaves_everything_as_it_was():
    with ops.switches(wgrad_defer=5, fold_half_wg="off"):
        before = ops.switch_values()
        with pytest.raises(RuntimeError, match="needs the slab join"):
            with ops.switches(wgrad_defer=9, fold_half_wg="force", wgrad_slabs=False, deterministic=True):
                raise AssertionError("the body must not run")
        assert ops.switch_values() == before
        assert before["wgrad_slabs"] is True and before["deterministic"] is False and before["wgrad_defer"] == 5


def test_library_held_rows_come_back_in_the_library():
    get = _hip.lib().ramnet_get_option
    names = (b"fold_pair", b"wino_ksplit", b"fold_half_wg", b"wgrad_wino_nf", b"ordered_only")
    with ops.switches(fold_pair=False, winograd_split=3, fold_half_wg="force", wgrad_overlap=True, deterministic=True):
        prior = [get(n) for n in names]
        assert prior == [0, 3, 1, 2, 1]
        with ops.switches(fold_pair=True, winograd_split=False, fold_half_wg="auto", wgrad_overlap=False, deterministic=False):
            assert [get(n) for n in names] == [1, 0, 2, 1, 0]
        assert [get(n) for n in names] == prior
    assert [get(n) for n in names] == [1, 1, 2, 1, 0]


def test_the_key_rows_and_the_invalidating_rows():
    assert {n for n, r in ops._SWITCHES.items() if r.key} == IN_KEY
    assert {n: len([f for f in r.invalidates if f == "invalidate_descs"]) for n, r in ops._SWITCHES.items() if r.invalidates} == INVALIDATE
    assert ops._SWITCHES["fold_pair"].invalidates == ("invalidate_packs", "invalidate_descs")
    before = ops.switch_values()
    for name in DEFAULTS:
        if name == "deterministic":
            continue
        key, epoch, packs = ops._SWITCH_KEY, ops._DESC_EPOCH, ops._PACK_EPOCH
        with ops.switches(**{name: _other(name)}):
            assert (ops._SWITCH_KEY != key) == (name in IN_KEY), name
            assert ops._DESC_EPOCH - epoch == INVALIDATE.get(name, 0), name
            assert ops._PACK_EPOCH - packs == (name == "fold_pair"), name
        assert ops._SWITCH_KEY == key and ops._DESC_EPOCH - epoch == 2 * INVALIDATE.get(name, 0), name
    key, epoch = ops._SWITCH_KEY, ops._DESC_EPOCH
    with ops.switches(deterministic=True):
        assert ops._SWITCH_KEY == key and ops._DESC_EPOCH == epoch
    ops.set_winograd_2x4(before["winograd_2x4"])
    assert ops._DESC_EPOCH == epoch                     # (only min_wgs makes set_winograd_2x4 invalidate; no test changes the library's threshold)
    assert ops.switch_values() == before
