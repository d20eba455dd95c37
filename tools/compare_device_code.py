#!/usr/bin/env python3
"""Are two builds' kernels the same machine code?  For each object file given, extracts the gfx950 code object from
both build directories (as tools/kernel_reachability.py does) and compares:
  - the set of kernel symbols,
  - each kernel's `llvm-objdump -d` text with addresses and encodings removed,
  - each kernel's metadata from `llvm-readelf --notes` (registers, spills, LDS, scratch, ...).

usage: compare_device_code.py <build dir A> <build dir B> [object ...]   (default: rs_kernels.o rs_kernels_f32.o)
e.g.   compare_device_code.py /path/to/base/roadsurf_amd/build roadsurf_amd/build
exit status 0: identical; 1: a difference (listed)."""
import bisect
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size", "wavefront_size",
        "max_flat_workgroup_size", "uses_dynamic_stack")


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fat}",
                    f"--output={co}", "--unbundle"], check=True)
    return co


def symbols(co):
    """[(address, name)] of the code object's symbols with a size, sorted"""
    out = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
    syms = []
    for line in out.splitlines():
        f = line.split()
        if len(f) >= 8 and f[0].rstrip(":").isdigit() and f[3] in ("OBJECT", "FUNC") and int(f[2], 0 if f[2].startswith("0x") else 10):
            syms.append((int(f[1], 16), f[7]))
    return sorted(syms)


def kernels(co):
    """{symbol: ((disassembly lines, the same with symbolic addresses), metadata dict)}.  Addresses, encodings and
    branch labels are dropped.  In the second form the PC-relative address of a global (s_getpc_b64 s[a:b];
    s_add_u32 sa, sa, lo; s_addc_u32 sb, sb, hi) is replaced by the symbol it points into: where the layout of the
    code object moved (it follows the order in which kernels are instantiated) the literal differs, the symbol does
    not.  (An address formed as `table - k` lands in whatever lies before the table: the plain form is the exact
    one, the symbolic form the one that survives a new layout.)"""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    meta = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: (re.search(r"\." + k + r":\s+(\S+)", block) or [None, None])[1] for k in META}
    syms = symbols(co)
    addrs = [a for a, _ in syms]

    def symbolic(target):
        i = bisect.bisect_right(addrs, target) - 1
        return f"<{syms[i][1]}+{target - syms[i][0]:#x}>" if i >= 0 else f"<{target:#x}>"

    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co],
                         capture_output=True, text=True, check=True).stdout
    code, sym, cur, pc, hi = {}, {}, None, {}, set()
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur, pc, hi = m.group(1), {}, set()
            code[cur], sym[cur] = [], []
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if cur is None or not m:
            continue  # blank lines, "..." runs of padding
        op, args, addr = m.group(1), [x.strip() for x in m.group(2).split(",")], int(m.group(3), 16)
        code[cur].append(op + " " + ", ".join(args))
        g = re.fullmatch(r"s\[(\d+):(\d+)\]", args[0]) if op == "s_getpc_b64" else None
        if g:
            pc[int(g.group(1))] = addr + 4
        elif op == "s_add_u32" and len(args) == 3 and args[0] == args[1] and args[0][1:].isdigit() \
                and int(args[0][1:]) in pc and args[2].startswith("0x"):
            r = int(args[0][1:])
            lo = int(args[2], 16)
            args[2] = symbolic(pc.pop(r) + (lo - (1 << 32) if lo >= 1 << 31 else lo))
            hi.add(r + 1)
        elif op == "s_addc_u32" and len(args) == 3 and args[0] == args[1] and args[0][1:].isdigit() \
                and int(args[0][1:]) in hi:
            hi.discard(int(args[0][1:]))
            args[2] = "<hi>"
        sym[cur].append(op + " " + ", ".join(args))
    return {k: ((code.get(k, []), sym.get(k, [])), meta[k]) for k in meta}


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    objs = sys.argv[3:] or ["rs_kernels.o", "rs_kernels_f32.o"]
    bad = 0
    for obj in objs:
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            ka = kernels(code_object(os.path.join(a_dir, obj), ta))
            kb = kernels(code_object(os.path.join(b_dir, obj), tb))
        for name in sorted(set(ka) ^ set(kb)):
            print(f"{obj}: {name} only in {'A' if name in ka else 'B'}")
            bad += 1
        same = 0
        for name in sorted(set(ka) & set(kb)):
            (ca, ma), (cb, mb) = ka[name], kb[name]
            if ma != mb:
                print(f"{obj}: {name}: metadata differs: "
                      + ", ".join(f"{k} {ma[k]} -> {mb[k]}" for k in META if ma[k] != mb[k]))
                bad += 1
            elif ca[0] != cb[0] and ca[1] != cb[1]:
                print(f"{obj}: {name}: code differs ({len(ca[0])} -> {len(cb[0])} instructions)")
                bad += 1
            else:
                same += 1
        print(f"{obj}: {same} kernels identical (code and metadata), {len(set(ka) | set(kb)) - same} not")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
