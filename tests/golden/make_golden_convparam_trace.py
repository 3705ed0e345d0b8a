"""Writes tests/golden/convparam_trace.json: the library launches of the small networks under every weight-gradient layout (the
cases of tests/convparam_trace_cases.py).  Run on the GPU at the commit whose behaviour is to be kept — the fixture then records
that behaviour, not the code under test — and only with names that exist on both sides of a change to ConvParam.

--hashes FILE also lists a SHA-256 of every pack tensor and of every parameter gradient after the first backward pass of each case
(bit-identity checks by hand: run twice to see which tensors reproduce at all, then once on the changed code)."""
import argparse
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import convparam_trace_cases as cases  # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def hashes_of(model, prefix, out):
    for mname, m in model.named_modules():
        for cname, cp in sorted(getattr(m, "_cps", {}).items()):
            for tag, c in (("", cp), (".s2d", getattr(cp, "_s2d", None)), (".state_half", getattr(cp, "_state_half", None))):
                for key, (_, packed) in sorted(getattr(c, "_packs", {}).items(), key=lambda kv: str(kv[0])):
                    for i, t in enumerate(packed if isinstance(packed, tuple) else (packed,)):
                        out.append("%s pack %s.%s%s %s[%d] %s" % (prefix, mname, cname, tag, key, i, sha(t)))
    for k, p in model.named_parameters():
        if p.grad is not None:
            out.append("%s grad %s %s" % (prefix, k, sha(p.grad)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "convparam_trace.json"))
    ap.add_argument("--hashes", default=None)
    a = ap.parse_args()
    traces, lines = {}, []
    for net, setting in cases.CASES:
        name = "%s/%s" % (net, setting)
        traces[name] = cases.run_case(net, setting, (lambda m: hashes_of(m, name, lines)) if a.hashes else None)
        print(name, [len(p) for p in traces[name]], flush=True)
    cases.dump(traces, a.out)
    flat = [r for passes in traces.values() for p in passes for r in p]
    packs = {cases.pack_kind(r) for r in flat} - {None}
    algos = {cases.wgrad_algo(r) for r in flat}
    print("pack kinds missing:", cases.PACK_KINDS - packs, "layouts missing:", [k for k, v in cases.LAYOUT_ALGOS.items() if v not in algos])
    if a.hashes:
        with open(a.hashes, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
