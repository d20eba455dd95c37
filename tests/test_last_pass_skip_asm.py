"""No GPU: the compiler still branches round the final stability correction of the two-wavefront kernels' loop.

model_step_fluxes_prepped evaluates the correction of the loop's exit pass only where the wavefront's tail is alive or
a lane's Stab does not prove the sign the dry-tail tests need (rs_physics_body.inc, DRY TAIL: THE LAST PASS).  What
keeps the optimiser from hoisting the correction over that wave-uniform test is an empty asm statement, which no
language rule protects: this test compiles the step kernels for gfx950 with the Makefile's flags (device code only,
to assembly, with line tables) and has tools/asm_attrib.py read the headline instance - the instructions inlined from
the final `bl_arm` must begin in a block that a scalar branch jumps over, and the square root and the logarithm
must be among them."""
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


def test_the_final_correction_of_the_headline_instance_sits_behind_a_scalar_branch(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import asm_attrib
    flags = _hipflags()
    assert "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags
    asm = str(tmp_path / "rs_kernels.s")
    subprocess.check_call(["hipcc"] + flags + ["--cuda-device-only", "-gline-tables-only", "-S", "-w",
                                               os.path.join(ROOT, "roadsurf_amd", "csrc", "rs_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL, cwd=os.path.join(ROOT, "roadsurf_amd"))
    found, guarded = asm_attrib.check_last_pass_skip(asm, HEADLINE)
    assert found >= 40  # both arms, the square root's and the logarithm's sequences: about eighty instructions
    assert guarded
