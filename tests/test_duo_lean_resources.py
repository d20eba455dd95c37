"""No GPU: the registers, spills and LDS that let five wavefronts of the LEAN knot-reading step kernel share a SIMD,
and the chain kernels that have to fit beside them.

A SIMD of gfx950 has 512 vector registers per lane: five wavefronts fit when each is allocated at most 96
(RS_DUO_LEAN_WAVES, rs_kernels.hip), and they leave 32 for the kernels of the re-sort chain that run between two
step launches of a plan.  The LDS admits ten workgroups per CU below 16 384 B each.  None of that is
a language rule: a new value held across the time loop puts the allocator back to spilling into it.  The figures are
read from the kernel metadata of the device code - the code objects inside roadsurf_amd/build/*.o where a build
newer than the sources left them, else a device-only compile to assembly with the Makefile's flags - by the regular
expression of tools/compare_device_code.py."""
import functools
import glob
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roadsurf_amd", "csrc")
LEAN_KNOTS = ("_ZN2rs15step_kernel_duoILi15ELb0ELi1ELb0ELb0ELb0ELb0EEEvNS_8StepArgsE",  # bench.py's headline instance
              "_ZN2rs15step_kernel_duoILi15ELb1ELi1ELb0ELb0ELb0ELb0EEEvNS_8StepArgsE")  # ... with the history score
VGPR_GRANULE = 8  # registers are allocated in blocks of eight per lane
# the links of the chain between two step launches that fit in what five step wavefronts leave: (source, name pattern)
CHAIN = [("rs_kernels", r"forecast_key_kernel"), ("rs_cluster", r"cs_hist_kernel"), ("rs_cluster", r"cs_binscan_kernel"), ("rs_cluster", r"cs_scatter_kernel"),
         ("rs_cluster", r"apply_kernelId")]  # apply_kernel<double>


def _hipflags():
    mk = open(os.path.join(ROOT, "roadsurf_amd", "Makefile")).read()
    m = re.search(r"^HIPFLAGS \?= (.*?\\\n.*?)$", mk, re.M)
    return m.group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()


def _blocks(text):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import compare_device_code as cdc
    meta = {}
    for block in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: (re.search(r"\." + k + r":\s+(\S+)", block) or [None, None])[1] for k in cdc.META}
    return meta


@functools.lru_cache(None)
def _metadata(unit):
    """{kernel symbol: metadata} of roadsurf_amd/csrc/<unit>.hip's gfx950 code"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import compare_device_code as cdc
    obj = os.path.join(ROOT, "roadsurf_amd", "build", unit + ".o")
    deps = glob.glob(os.path.join(CSRC, "*")) + [os.path.join(ROOT, "include", "roadsurf.h"),
                                                 os.path.join(ROOT, "roadsurf_amd", "Makefile")]
    with tempfile.TemporaryDirectory() as tmp:
        if os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(d) for d in deps):
            co = cdc.code_object(obj, tmp)
            text = subprocess.run([f"{cdc.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True,
                                  check=True).stdout
        else:
            asm = os.path.join(tmp, unit + ".s")
            subprocess.check_call(["hipcc"] + _hipflags() + ["--cuda-device-only", "-S", "-w",
                                                             os.path.join(CSRC, unit + ".hip"), "-o", asm],
                                  stderr=subprocess.DEVNULL, cwd=os.path.join(ROOT, "roadsurf_amd"))
            text = open(asm).read()
    return _blocks(text)


@pytest.mark.parametrize("symbol", LEAN_KNOTS, ids=["headline", "history_score"])
def test_the_lean_knot_reading_instances_fit_five_wavefronts_on_a_simd(symbol):
    m = _metadata("rs_kernels")[symbol]
    print(symbol, m)
    assert int(m["vgpr_count"]) <= 96
    assert int(m["vgpr_spill_count"]) == 0
    assert int(m["private_segment_fixed_size"]) == 0
    assert int(m["group_segment_fixed_size"]) <= 16384


@pytest.mark.parametrize("unit,pattern", CHAIN, ids=[p for _, p in CHAIN])
def test_the_chain_kernels_fit_beside_five_step_wavefronts(unit, pattern):
    hits = {k: v for k, v in _metadata(unit).items() if re.search(pattern, k)}
    assert len(hits) == 1, (pattern, sorted(hits))
    (name, m), = hits.items()
    print(name, m)
    allocated = -(-int(m["vgpr_count"]) // VGPR_GRANULE) * VGPR_GRANULE
    assert allocated <= 32
    assert int(m["vgpr_spill_count"]) == 0 and int(m["private_segment_fixed_size"]) == 0
