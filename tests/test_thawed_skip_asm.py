"""No GPU: the compiler still branches round layer_vsh's frozen/thawed select where a wavefront is thawed throughout.

layer_step tells layer_vsh when every active lane of the wavefront has the layer thawed, and layer_vsh then skips
the per-lane select between the frozen constant and the water polynomials (a literal and two v_cndmask_b32 per
layer).  What keeps the optimiser from folding that branch back into the selects is an empty asm statement, which
no language rule protects: this test compiles the step kernels for gfx950 with the Makefile's flags (device code
only, to assembly) and has tools/asm_attrib.py read the headline instance - every one of its fifteen selects must
stand in a block that a scalar branch jumps over."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "_ZN2rs15step_kernel_duoILi15ELb0ELi1ELb0ELb0ELb0ELb0EEEvNS_8StepArgsE"


def _hipflags():
    mk = open(os.path.join(ROOT, "roadsurf_amd", "Makefile")).read()
    m = re.search(r"^HIPFLAGS \?= (.*?\\\n.*?)$", mk, re.M)
    flags = m.group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "")
    return flags.split()


def test_every_select_of_the_headline_instance_sits_behind_a_scalar_branch(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import asm_attrib
    flags = _hipflags()
    assert "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags
    asm = str(tmp_path / "rs_kernels.s")
    subprocess.check_call(["hipcc"] + flags + ["--cuda-device-only", "-S", "-w",
                                               os.path.join(ROOT, "roadsurf_amd", "csrc", "rs_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    found, bad = asm_attrib.check_thawed_skip(asm, HEADLINE)
    assert found == 15  # one select per layer: 13 on the ground wave, 2 on the surface wave
    assert bad == 0
