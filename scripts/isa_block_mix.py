"""Instruction mix per basic block of one kernel in a device assembly listing, the way the counts in
profiles/dw_window/README.md were taken:
  hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --offload-device-only -S csrc/dwconv.hip -o dw.s
  python scripts/isa_block_mix.py dw.s <mangled kernel name> [min instructions of a listed block]
Prints one line per basic block (label, then class=count), the kernel's total, and its
.vgpr_count / .private_segment_fixed_size from the metadata."""
import collections
import re
import sys


def classes(op):
    c = []
    if op.startswith("v_"):
        c.append("valu")
    if op.startswith("v_pk_fma"):
        c.append("pk_fma")
    if op.startswith(("v_pk_mul", "v_pk_add")):
        c.append("pk_muladd")
    if op.startswith(("v_lshlrev_b32", "v_and_b32", "v_cvt_f32_f16")):
        c.append("unpack")
    if op.startswith("v_rcp"):
        c.append("rcp")
    if op.startswith("v_exp"):
        c.append("exp")
    if op.startswith("v_med3"):
        c.append("med3")
    if op.startswith("v_mov"):
        c.append("mov")
    if op.startswith(("ds_read", "ds_load")):
        c.append("ds_read")
    if op.startswith(("ds_write", "ds_store")):
        c.append("ds_write")
    if op.startswith("global_load"):
        c.append("gload")
    if op.startswith("global_store"):
        c.append("gstore")
    if op.startswith("scratch_"):
        c.append("scratch")
    return c


def main():
    path, sym = sys.argv[1], sys.argv[2]
    least = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    blocks, cur = [], ["entry", collections.Counter()]
    for l in lines[start + 1:end]:
        s = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            blocks.append(cur)
            cur = [m.group(1), collections.Counter()]
        if not s or s[0] in ";." or m:
            continue
        op = s.split()[0]
        cur[1]["total"] += 1
        for c in classes(op):
            cur[1][c] += 1
    blocks.append(cur)
    whole = collections.Counter()
    for name, c in blocks:
        whole.update(c)
        if c["total"] >= least:
            print(f"{name:12s}", " ".join(f"{k}={v}" for k, v in sorted(c.items())))
    print("whole kernel", " ".join(f"{k}={v}" for k, v in sorted(whole.items())))
    meta = next(i for i, l in enumerate(lines) if l.strip() == f".name:           {sym}")
    for l in lines[meta:meta + 12]:
        if "vgpr_count" in l or "private_segment_fixed_size" in l or "vgpr_spill" in l:
            print(l.strip())


if __name__ == "__main__":
    main()
