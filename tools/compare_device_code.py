#!/usr/bin/env python3
"""Are two builds' kernels the same machine code?  For each object file given, extracts the gfx950 code object from
both build directories (as tools/kernel_reachability.py does) and compares:
  - the set of kernel symbols,
  - each kernel's `llvm-objdump -d` text with addresses and encodings removed,
  - each kernel's metadata from `llvm-readelf --notes` (registers, spills, LDS, scratch, ...).

usage: compare_device_code.py <build dir A> <build dir B> [object ...]   (default: rs_kernels.o rs_kernels_f32.o)
e.g.   compare_device_code.py /path/to/base/roadsurf_amd/build roadsurf_amd/build
exit status 0: identical; 1: a difference (listed)."""
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
    """({address: name} of the functions, [(address, name)] of the data objects other than kernel descriptors,
    {address: symbol+addend} of the GOT slots)"""
    out = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "-r", "--wide", co],
                         capture_output=True, text=True, check=True).stdout
    funcs, data, got = {}, [], {}
    for line in out.splitlines():
        f = line.split()
        if len(f) >= 8 and f[0].rstrip(":").isdigit() and int(f[2], 0 if f[2].startswith("0x") else 10):
            if f[3] == "FUNC":
                funcs[int(f[1], 16)] = f[7]
            elif f[3] == "OBJECT" and not f[7].endswith(".kd"):
                data.append((int(f[1], 16), f[7]))
        elif len(f) >= 5 and f[2] == "R_AMDGPU_ABS64":
            got[int(f[0], 16)] = "".join(f[4:])
    return funcs, sorted(set(data)), got


def kernels(co):
    """{symbol: ((disassembly lines, the same with symbolic addresses), metadata dict)}.  Addresses, encodings and
    branch labels are dropped.  In the second form the PC-relative address of a global (s_getpc_b64 s[a:b];
    s_add_u32 sa, sa, lo; s_addc_u32 sb, sb, hi) is replaced by what it points to, so that it survives a new layout
    of the code object (the layout follows the order in which kernels are instantiated, and their lengths): a GOT
    slot by the symbol the slot holds, the start of a function by its name, any other address by its signed offset
    from every data object.  The compiler forms `table - k` as readily as `table + k`, and a build may lay the data
    objects out in another order, so such an address is the same in both builds when it is the same offset from
    some data object in both (match())."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    meta = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: (re.search(r"\." + k + r":\s+(\S+)", block) or [None, None])[1] for k in META}
    funcs, data, got = symbols(co)

    def symbolic(target):
        if target in got:
            return f"<got:{got[target]}>"
        if target in funcs:
            return f"<{funcs[target]}>"
        return frozenset((name, target - addr) for addr, name in data)

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
        target = None
        if g:
            pc[int(g.group(1))] = addr + 4
        elif op == "s_add_u32" and len(args) == 3 and args[0] == args[1] and args[0][1:].isdigit() \
                and int(args[0][1:]) in pc and args[2].startswith("0x"):
            r = int(args[0][1:])
            lo = int(args[2], 16)
            target = symbolic(pc.pop(r) + (lo - (1 << 32) if lo >= 1 << 31 else lo))
            args[2] = target if isinstance(target, str) else "<data>"
            hi.add(r + 1)
        elif op == "s_addc_u32" and len(args) == 3 and args[0] == args[1] and args[0][1:].isdigit() \
                and int(args[0][1:]) in hi:
            hi.discard(int(args[0][1:]))
            args[2] = "<hi>"
        text = op + " " + ", ".join(args)
        sym[cur].append((text, target) if isinstance(target, frozenset) else text)
    return {k: ((code.get(k, []), sym.get(k, [])), meta[k]) for k in meta}


def match(a, b):
    """two symbolic disassemblies: the same lines, each data address the same offset from some data object in both"""
    return len(a) == len(b) and all(
        x == y or (isinstance(x, tuple) and isinstance(y, tuple) and x[0] == y[0] and bool(x[1] & y[1]))
        for x, y in zip(a, b))


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
            elif ca[0] != cb[0] and not match(ca[1], cb[1]):
                print(f"{obj}: {name}: code differs ({len(ca[0])} -> {len(cb[0])} instructions)")
                bad += 1
            else:
                same += 1
        print(f"{obj}: {same} kernels identical (code and metadata), {len(set(ka) | set(kb)) - same} not")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
