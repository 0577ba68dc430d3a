"""Per-kernel ISA comparison of one csrc/*.hip file between two trees (a refactor's evidence):
  python scripts/isa_kernel_diff.py <tree A> <tree B> sra_fast.hip
Compiles the file of each tree for the device only with the Makefile's CXXFLAGS (read from tree B's
csrc/Makefile, ARCH and EXTRA at their defaults) plus --offload-device-only -S, then prints, per kernel
symbol, whether the instruction text is identical (comment lines, blank lines and assembler
directives ignored) and the metadata of both trees: .vgpr_count, .sgpr_count,
.group_segment_fixed_size, .private_segment_fixed_size, .vgpr_spill_count.  Needs hipcc, no GPU."""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("rgbx_semantic_segmentation_amd", "csrc")
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count")


def cxxflags(tree):
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1)
    return hipcc, flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()


def assembly(tree, name, hipcc, flags, out):
    r = subprocess.run([hipcc, *flags, "--offload-device-only", "-S", name, "-o", os.path.abspath(out)],
                       cwd=os.path.join(tree, CSRC), stderr=subprocess.PIPE, text=True)
    sys.stderr.write("".join(l for l in r.stderr.splitlines(True) if "--hip-link" not in l))   # device-only: no link step
    r.check_returncode()
    return open(out).read().split("\n")


def kernels(lines):
    """{symbol: (instruction lines, {metadata field: value})} of every kernel the metadata lists"""
    first = lines.index("amdhsa.kernels:") + 1
    entries = []
    for l in lines[first:]:
        if not l.startswith("  "):                  # the next top-level key ends the kernel list
            break
        m = re.match(r"^  [- ] \.(\w+):\s+(\S+)$", l)    # a kernel's own keys: 4 columns in, "- " on its first
        if l.startswith("  - "):
            entries.append({})
        if m:
            entries[-1][m.group(1)] = m.group(2)
    out = {}
    for m in entries:
        name = m["name"]
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
        # .LBB<function index>_<block>: the index is the kernel's position in the file, not its code
        text = [re.sub(r"\.LBB\d+_", ".LBB_", l.strip()) for l in lines[start + 1:end]]
        out[name] = ([l.split(";")[0].rstrip() for l in text if l and (l[0] not in ";." or l.startswith(".LBB"))], m)
    return out


def demangle(names):
    r = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True)
    short = r.stdout.split("\n") if r.returncode == 0 else names
    return dict(zip(names, (s.replace("(anonymous namespace)::", "").replace("__hip_bfloat16", "bf16")
                            .replace("_Float16", "f16") for s in short)))


def main():
    a, b, name = sys.argv[1:4]
    hipcc, flags = cxxflags(b)
    with tempfile.TemporaryDirectory() as tmp:
        ka = kernels(assembly(a, name, hipcc, flags, os.path.join(tmp, "a.s")))
        kb = kernels(assembly(b, name, hipcc, flags, os.path.join(tmp, "b.s")))
    nice = demangle(sorted(set(ka) | set(kb)))
    print(f"# {name}: A = {a}, B = {b}; per kernel: instruction text, then A -> B of " + ", ".join(FIELDS))
    same = 0
    for sym in sorted(nice, key=nice.get):
        if sym not in ka or sym not in kb:
            print(f"{nice[sym]}: only in {'A' if sym in ka else 'B'}")
            continue
        (ia, ma), (ib, mb) = ka[sym], kb[sym]
        ident = ia == ib
        same += ident
        verdict = "identical" if ident else f"DIFFERS ({len(ia)} -> {len(ib)} instructions)"
        print(f"{nice[sym]}: {verdict}; " + " ".join(
            (ma[f] if ma[f] == mb[f] else f"{ma[f]}->{mb[f]}") for f in FIELDS))
    print(f"# {same} of {len(nice)} kernels identical")


if __name__ == "__main__":
    main()
