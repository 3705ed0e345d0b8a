"""No GPU: tests/stream_cases.py against the code.  Every module-level dict or list of the package's launch modules whose name starts
with `_`, and every static container or thread_local of csrc/, has a record (what it owes to its stream) or a reason why it is no device
state; a new cache without either fails here."""
import importlib
import os
import re

import stream_cases as sc

MODULES = ("ops", "metrics", "render", "augment", "voxel")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rpg_ramnet_amd", "csrc")
DECL = re.compile(r"\bstatic\s+(?:thread_local\s+)?std::(?:map|unordered_map|unordered_set)\s*<.*>\s*(\w+)\s*;|\bthread_local\s+[\w:]+\s+(\w+)\s*[\[=;]")
FIELDS = ("owner", "names", "key", "init", "resets", "capture", "rows")


def recorded_names():
    return {n for r in sc.RECORDS for n in r["names"]}


def package_state():
    out = []
    for m in MODULES:
        mod = importlib.import_module("rpg_ramnet_amd." + m)
        out += ["%s.%s" % (m, k) for k, v in vars(mod).items() if k.startswith("_") and not k.startswith("__") and isinstance(v, (dict, list))]
    return out


def csrc_state():
    out = []
    for f in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, f)) as fh:
            for line in fh:
                if line.lstrip().startswith("//"):
                    continue
                for m in DECL.finditer(line):
                    out.append((f, m.group(1) or m.group(2)))
    return out


def test_every_package_cache_has_a_record_or_a_reason():
    found = package_state()
    assert "ops._msg_tables" in found and "metrics._tables" in found and "render._workspaces" in found and "augment._ptrs" in found    # (the walk sees them)
    names = recorded_names()
    missing = [n for n in found if n not in names and n not in sc.NOT_DEVICE_STATE]
    assert not missing, "module-level state without a record in tests/stream_cases.py: %s" % missing
    both = [n for n in found if n in names and n in sc.NOT_DEVICE_STATE]
    assert not both, both
    stale = [n for n in list(sc.NOT_DEVICE_STATE) + [n for n in names if n.split(".")[0] in MODULES] if n not in found]
    assert not stale, "entries of tests/stream_cases.py that name nothing in the package: %s" % stale
    assert all(len(why) > 10 for why in sc.NOT_DEVICE_STATE.values())


def test_every_static_container_of_csrc_has_a_record_or_a_reason():
    found = csrc_state()
    assert ("loss_voxel.hip", "bufs") in found and ("pointwise.hip", "ev") in found and ("pointwise.hip", "g_err") in found        # (the walk sees them)
    missing = [k for k in found if k not in sc.CSRC_RECORDED and k not in sc.CSRC_NOT_DEVICE_STATE]
    assert not missing, "static state of csrc/ without a record in tests/stream_cases.py: %s" % missing
    names = recorded_names()
    for k, recs in sc.CSRC_RECORDED.items():
        assert found.count(k) == len(recs), "%s: %d declarations, %d records" % (k, found.count(k), len(recs))
        assert all(r in names for r in recs), (k, recs)
    stale = [k for k in sc.CSRC_NOT_DEVICE_STATE if k not in found]
    assert not stale, stale


def test_the_walk_of_csrc_finds_a_new_container():
    text = ["static std::map<int, float *> cache;", "    static thread_local std::unordered_map<int, hipEvent_t> pool;", "static thread_local char buf[96] = \"\";",
            "    static std::unordered_set<unsigned long long> seen;", "// static std::map<int, int> commented;"]
    got = [m.group(1) or m.group(2) for line in text if not line.lstrip().startswith("//") for m in DECL.finditer(line)]
    assert got == ["cache", "pool", "buf", "seen"]


def test_records_are_complete_and_rows_exist():
    required = ["si_scratch.bufs", "voxel_id_scratch.bufs", "allow_full_lds.done", "ramnet_stream_fork.ev", "metrics._workspaces", "metrics._eval_workspaces",
                "metrics._tables", "render._workspaces", "ColorMapper._tables", "ops._msg_tables", "ops._msg_workspaces", "ops._msg_weight_cache", "ops._CONSTS",
                "augment._coords", "augment._ptrs", "ConvParam.packs", "ConvParam._splitk", "ConvParam._part", "ConvParam gradient workspaces"]
    names = recorded_names()
    assert all(n in names for n in required), [n for n in required if n not in names]
    for r in sc.RECORDS:
        assert set(r) == set(FIELDS) and all(r[f] for f in FIELDS[:6]), r["owner"]
        assert all(s in sc.SURFACES for s in r["rows"]), (r["owner"], r["rows"])
    layer = [r for r in sc.RECORDS if r["key"] == "layer"]
    assert len(layer) == 4 and all(r["init"] == sc.LAYER_CONTRACT for r in layer)
    # (no rows of their own, history_cases.row_user_stream runs them; the split-K counters in a caller's workspace have the issue's one surface)
    assert all(r["rows"] == (("conv_splitk",) if r["names"] == ("ConvParam._splitk",) else ()) for r in layer)


def test_rows_are_well_formed():
    assert len(set(sc.ROWS)) == len(sc.ROWS)
    for s, k in sc.ROWS:
        assert s in sc.SURFACES and k in sc.KINDS
    for s, d in sc.SURFACES.items():
        kinds = [k for t, k in sc.ROWS if t == s]
        assert kinds[:2] == ["first_use", "second_use"], s         # (second_use repeats the call of first_use on its stream)
        assert set(d) == {"library", "entry", "shape"}
    # the delayed kinds never share a cached pointer table across streams: cross-stream reuse is table_owner's alone (it synchronises the device)
    covered = {s for r in sc.RECORDS for s in r["rows"]}
    assert covered | set(sc.STATELESS) == set(sc.SURFACES) and not covered & set(sc.STATELESS), (covered, set(sc.SURFACES))
    assert [k for s, k in sc.ROWS if s == "conv_splitk"] == ["first_use", "second_use"]
    # the entries that document a capture path have a capture row
    for s in ("si_loss", "voxel_sorted", "grad_loss_batch"):
        assert (s, "capture") in sc.ROWS
