"""Compare the gfx950 device code of one kernel family between two object files, instruction for instruction.

    python tools/compare_kernel_isa.py OLD.o NEW.o conv_wino_r6_kernel

Each object's fat binary is extracted (llvm-objcopy), unbundled (clang-offload-bundler), disassembled (llvm-objdump -d -C) and split by
symbol.  Symbols that contain the family name are matched by their demangled name with trailing DEFAULT template arguments ignored (a kernel of the old object that is
`kernel<4, 1, false>` matches `kernel<4, 1, false, false>` of the new one), so a template argument added with a default does not hide a
comparison.  Addresses and raw encodings are dropped; branch targets are kept as offsets from the symbol's start.  Prints one line per
kernel (same / DIFFERENT / only in one object) and exits non-zero when a kernel present in both differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def device_disassembly(obj):
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=" + fat, "--output=" + co], check=True)
        return subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", "--no-show-raw-insn", co], check=True, capture_output=True,
                              text=True).stdout


def kernels(obj, family):
    out, name, start = {}, None, 0
    for line in device_disassembly(obj).splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            name = m.group(2) if family in m.group(2) else None
            start = int(m.group(1), 16)
            if name:
                out[name] = []
            continue
        if name is None or not line.strip():
            continue
        ins = re.sub(r"//.*$", "", line).strip()
        ins = re.sub(r"<[^>]*\+0x([0-9a-f]+)>", lambda t: "<+0x%s>" % t.group(1), ins)      # branch targets: offset inside the symbol
        if ins:
            out[name].append(ins)
    return out


def key(dem):
    m = re.search(r"<(.*?)>\(", dem)
    args = [a.strip() for a in m.group(1).split(",")] if m else []
    while args and args[-1] == "false":
        args.pop()
    return dem.split("<")[0] + "<" + ",".join(args) + ">"


def main():
    old, new, family = sys.argv[1:4]
    ko, kn = kernels(old, family), kernels(new, family)
    bo = {key(n): ko[n] for n in ko}
    bn = {key(n): kn[n] for n in kn}
    bad = 0
    for k in sorted(set(bo) | set(bn)):
        if k not in bo:
            print("%-60s only in NEW (%d instructions)" % (k, len(bn[k])))
        elif k not in bn:
            print("%-60s only in OLD" % k)
            bad += 1
        elif bo[k] == bn[k]:
            print("%-60s same (%d instructions)" % (k, len(bo[k])))
        else:
            print("%-60s DIFFERENT (%d vs %d instructions)" % (k, len(bo[k]), len(bn[k])))
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
