"""Which step kernel a launch takes (roadsurf_amd/csrc/rs_step_select.hpp), on the host compiler alone: every
instance the GPU suite reaches is the answer for some shape, no shape names anything else, and one row per decision
the launchers made before the table existed - with its grid, workgroup size and dynamic LDS."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roadsurf_amd", "csrc")
REACH = os.path.join(ROOT, "profiles", "r06_kernel_reachability.txt")

DRIVER = r"""
#include "rs_step_select.hpp"
#include <cstdio>
#include <iostream>
using namespace rs;
static const char *name_of(StepKernel k) {
  switch (k) {
#define NAME(id, ...) case StepKernel::id: return #__VA_ARGS__;
    RS_STEP_KERNELS_F64(NAME) RS_STEP_KERNELS_F32(NAME)
#undef NAME
    default: return "NONE";
  }
}
int main(int argc, char **) {
  if (argc > 1) { /* the table itself */
#define LIST(id, ...) std::puts(#__VA_ARGS__);
    RS_STEP_KERNELS_F64(LIST) RS_STEP_KERNELS_F32(LIST)
    return 0;
  }
  long long f32, nl, src, full, sky, depth, cpl, a32, diag, score, variant, npoints, wave_n, list, nlist;
  while (std::cin >> f32 >> nl >> src >> full >> sky >> depth >> cpl >> a32 >> diag >> score >> variant >> npoints
         >> wave_n >> list >> nlist) {
    StepShape s;
    s.f32 = f32; s.nlayers = (int32_t)nl; s.src = (StepSource)src; s.full = full; s.sky = sky; s.depth = depth;
    s.cpl = (StepCoupling)cpl; s.a32 = a32; s.diag = diag; s.score = score; s.variant = (int32_t)variant;
    s.npoints = npoints; s.wave_n = (int32_t)wave_n; s.cpl_list = list; s.cpl_nlist = (int32_t)nlist;
    const StepLaunch l = select_step(s);
    std::printf("%s|%u|%u|%u\n", name_of(l.kernel), l.grid, l.block, l.lds);
  }
  return 0;
}
"""

FIELDS = ("f32", "nl", "src", "full", "sky", "depth", "cpl", "a32", "diag", "score", "variant", "npoints", "wave_n",
          "list", "nlist")
DEFAULT = dict(f32=0, nl=15, src=0, full=0, sky=0, depth=0, cpl=0, a32=1, diag=0, score=1, variant=0,
               npoints=1_000_000, wave_n=0, list=0, nlist=0)
WINDOW, KNOTS, RAW = 0, 1, 2
NONE, GENERAL, CHUNK, REPLAY = 0, 1, 2, 3
AUTO, REG, LDS, DUO, HYBRID = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def select(tmp_path_factory):
    d = tmp_path_factory.mktemp("step_select")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"), "-o", exe],
                   check=True)

    def run(shapes):
        text = "".join(" ".join(str(int(s[k])) for k in FIELDS) + "\n" for s in shapes)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(shapes)
        return [(n, int(g), int(b), int(l)) for n, g, b, l in (line.split("|") for line in out)]

    run.table = subprocess.run([exe, "table"], capture_output=True, text=True, check=True).stdout.splitlines()
    return run


def reached_instances():
    return {line.strip() for line in open(REACH) if re.match(r"rs(32)?::step_kernel", line)}


def test_every_reached_instance_is_selected_and_nothing_else(select):
    reached = reached_instances()
    assert len(reached) == 57
    assert sorted(select.table) == sorted(reached)  # one table row per instance
    grid = dict(f32=(0, 1), nl=(8, 15, 32), src=(WINDOW, KNOTS, RAW), full=(0, 1), sky=(0, 1), depth=(0, 1),
                cpl=(NONE, GENERAL, CHUNK, REPLAY), a32=(0, 1), diag=(0, 1), score=(0, 1),
                variant=(AUTO, REG, LDS, DUO, HYBRID), npoints=(1000, 1_000_000), wave_n=(0,), list=(0, 1),
                nlist=(300,))
    shapes = [dict(zip(grid, v)) for v in itertools.product(*grid.values())]
    got = {r[0] for r in select(shapes)}
    assert got - {"NONE"} == reached


def row(**kw):
    s = dict(DEFAULT)
    s.update(kw)
    return s


def duo(score, src, full, sky=False, cpl=False, replay=False):
    b = lambda x: "true" if x else "false"
    return f"rs::step_kernel_duo<15, {b(score)}, {src}, {b(full)}, {b(sky)}, {b(cpl)}, {b(replay)}>"


def reg(full, score, a32):
    return f"rs::step_kernel_reg<15, {'true' if full else 'false'}, {'true' if score else 'false'}, " \
           f"{'true' if a32 else 'false'}>"


def g(n, per=256):
    return (n + per - 1) // per


L64 = lambda nl: nl * 256 * 8  # the LDS profile, fp64
L32 = lambda nl: nl * 256 * 4  # ... fp32
M = 1_000_000

ROWS = [
    # RS_DUO_MAX_POINTS: AUTO takes two wavefronts per 64 points up to 65 536 points (LEAN, FULL, sky view)
    (row(npoints=65536), (duo(1, 0, 0), 1024, 128, 0)),
    (row(npoints=65537), (reg(0, 1, 1), 257, 256, 0)),
    (row(npoints=65536, full=1), (duo(1, 0, 1), 1024, 128, 0)),
    (row(npoints=65537, full=1), ("rs::step_kernel_hybrid<true, true>", 257, 256, 0)),
    (row(npoints=65536, full=1, sky=1), (duo(1, 0, 1, sky=1), 1024, 128, 0)),
    (row(npoints=65537, full=1, sky=1), ("rs::step_kernel_sky_h<4>", 257, 256, 0)),
    (row(npoints=65536, wave_n=1040), (duo(1, 0, 0), 1040, 128, 0)),  # a wave table sets the grid
    (row(npoints=65536, score=0), (duo(0, 0, 0), 1024, 128, 0)),
    # NLayers: 15 in registers / hybrid, 8 and 32 in LDS
    (row(), (reg(0, 1, 1), g(M), 256, 0)),
    (row(nl=8), ("rs::step_kernel_lds<false, false>", g(M), 256, L64(8))),
    (row(nl=32), ("rs::step_kernel_lds<false, false>", g(M), 256, L64(32))),
    (row(nl=8, full=1), ("rs::step_kernel_lds<true, false>", g(M), 256, L64(8))),
    (row(nl=32, npoints=1000), ("rs::step_kernel_lds<false, false>", g(1000), 256, L64(32))),
    (row(nl=8, full=1, sky=1), ("rs::step_kernel_sky<false>", g(M), 256, L64(8))),
    (row(nl=32, full=1, sky=1, npoints=1000), ("rs::step_kernel_sky<false>", g(1000), 256, L64(32))),
    # a32: the instances with 32-bit window offsets, and not the two-wavefront flavour without them
    (row(a32=0), (reg(0, 1, 0), g(M), 256, 0)),
    (row(a32=0, full=1), ("rs::step_kernel_hybrid<true, false>", g(M), 256, 0)),
    (row(a32=0, score=0, full=1), ("rs::step_kernel_hybrid<false, false>", g(M), 256, 0)),
    (row(a32=1, score=0, full=1), ("rs::step_kernel_hybrid<false, true>", g(M), 256, 0)),
    (row(a32=0, npoints=1000), (reg(0, 1, 0), g(1000), 256, 0)),
    (row(a32=0, npoints=1000, full=1, sky=1), ("rs::step_kernel_sky_h<4>", g(1000), 256, 0)),
    # diagnostics: the instance that carries bl_diagnose, in every family
    (row(diag=1, npoints=1000), ("rs::step_kernel_lds<true, true>", g(1000), 256, L64(15))),
    (row(diag=1, variant=DUO, npoints=1000), ("rs::step_kernel_lds<true, true>", g(1000), 256, L64(15))),
    (row(diag=1, variant=REG), ("rs::step_kernel_lds<true, true>", g(M), 256, L64(15))),
    (row(diag=1, full=1, sky=1, npoints=1000), ("rs::step_kernel_sky<true>", g(1000), 256, L64(15))),
    (row(diag=1, full=1, cpl=GENERAL), ("rs::step_kernel_coupled<true>", g(M), 256, L64(15))),
    (row(diag=0, full=1, cpl=GENERAL), ("rs::step_kernel_coupled<false>", g(M), 256, L64(15))),
    # forced variants; "not this launch: as AUTO"; the register profile at NL != 15 has no instance
    (row(variant=REG), (reg(0, 1, 1), g(M), 256, 0)),
    (row(variant=REG, full=1, score=0), (reg(1, 0, 1), g(M), 256, 0)),
    (row(variant=REG, nl=8), ("NONE", 0, 256, 0)),
    (row(variant=LDS), ("rs::step_kernel_lds<false, false>", g(M), 256, L64(15))),
    (row(variant=LDS, full=1, npoints=1000), ("rs::step_kernel_lds<true, false>", g(1000), 256, L64(15))),
    (row(variant=DUO), (duo(1, 0, 0), g(M, 64), 128, 0)),
    (row(variant=DUO, full=1), (duo(1, 0, 1), g(M, 64), 128, 0)),
    (row(variant=DUO, a32=0), (reg(0, 1, 0), g(M), 256, 0)),
    (row(variant=DUO, a32=0, full=1), ("rs::step_kernel_hybrid<true, false>", g(M), 256, 0)),
    (row(variant=DUO, full=1, depth=1), ("rs::step_kernel_hybrid<true, true>", g(M), 256, 0)),
    (row(variant=DUO, nl=8), ("rs::step_kernel_lds<false, false>", g(M), 256, L64(8))),
    (row(variant=HYBRID, full=1), ("rs::step_kernel_hybrid<true, true>", g(M), 256, 0)),
    (row(variant=HYBRID, full=1, npoints=1000), ("rs::step_kernel_hybrid<true, true>", g(1000), 256, 0)),
    (row(variant=HYBRID), (reg(0, 1, 1), g(M), 256, 0)),
    (row(variant=HYBRID, nl=8, full=1), ("rs::step_kernel_lds<true, false>", g(M), 256, L64(8))),
    # an output depth: never the two-wavefront flavour
    (row(full=1, depth=1, npoints=1000), ("rs::step_kernel_hybrid<true, true>", g(1000), 256, 0)),
    (row(full=1, depth=1, sky=1, npoints=1000), ("rs::step_kernel_sky_h<4>", g(1000), 256, 0)),
    # sky view with and without the two-wavefront flavour
    (row(full=1, sky=1, npoints=1000), (duo(1, 0, 1, sky=1), g(1000, 64), 128, 0)),
    (row(full=1, sky=1, npoints=1000, score=0), (duo(0, 0, 1, sky=1), g(1000, 64), 128, 0)),
    (row(full=1, sky=1, npoints=1000, variant=LDS), (duo(1, 0, 1, sky=1), g(1000, 64), 128, 0)),
    (row(full=1, sky=1), ("rs::step_kernel_sky_h<4>", g(M), 256, 0)),
    # coupling: rs_hip_step's rounds (general kernel), lock-step chunks and replay rounds
    (row(full=1, cpl=GENERAL, list=1, nlist=300), ("rs::step_kernel_coupled<false>", 2, 256, L64(15))),
    (row(full=1, cpl=GENERAL, list=1, nlist=0), ("rs::step_kernel_coupled<false>", 0, 256, L64(15))),
    (row(full=1, cpl=GENERAL, sky=1, npoints=1000), ("rs::step_kernel_coupled<false>", g(1000), 256, L64(15))),
    (row(full=1, cpl=GENERAL, nl=8), ("rs::step_kernel_coupled<false>", g(M), 256, L64(8))),
    (row(full=1, cpl=CHUNK), ("rs::step_kernel_cpl_h<3, false>", g(M), 256, 0)),
    (row(full=1, cpl=CHUNK, sky=1), ("rs::step_kernel_cpl_h<3, true>", g(M), 256, 0)),
    (row(full=1, cpl=CHUNK, nl=8), ("rs::step_kernel_cpl<false>", g(M), 256, L64(8))),
    (row(full=1, cpl=CHUNK, nl=8, sky=1), ("rs::step_kernel_cpl<true>", g(M), 256, L64(8))),
    (row(full=1, cpl=REPLAY, list=1, nlist=300), ("rs::step_kernel_cpl_replay_h<3, false>", 2, 256, 0)),
    (row(full=1, cpl=REPLAY, list=1, nlist=300, sky=1), ("rs::step_kernel_cpl_replay_h<3, true>", 2, 256, 0)),
    (row(full=1, cpl=REPLAY, list=1, nlist=300, nl=8), ("rs::step_kernel_cpl_replay<false>", 2, 256, L64(8))),
    (row(full=1, cpl=REPLAY, list=1, nlist=300, nl=32, sky=1),
     ("rs::step_kernel_cpl_replay<true>", 2, 256, L64(32))),
    (row(full=1, cpl=REPLAY, list=0), ("rs::step_kernel_cpl_replay_h<3, false>", 0, 256, 0)),
    (row(full=1, cpl=REPLAY, list=1, nlist=0), ("rs::step_kernel_cpl_replay_h<3, false>", 0, 256, 0)),
    # the raw series of the driver path: chunks with and without sky view and coupling, replay rounds
    (row(src=RAW, full=1), (duo(1, 2, 1), g(M, 64), 128, 0)),
    (row(src=RAW, full=1, score=0), (duo(0, 2, 1), g(M, 64), 128, 0)),
    (row(src=RAW, full=1, sky=1), (duo(1, 2, 1, sky=1), g(M, 64), 192, 0)),
    (row(src=RAW, full=1, sky=1, score=0), (duo(0, 2, 1, sky=1), g(M, 64), 192, 0)),
    (row(src=RAW, full=1, wave_n=20000), (duo(1, 2, 1), 20000, 128, 0)),
    (row(src=RAW, full=1, cpl=CHUNK), (duo(1, 2, 1, cpl=1), g(M, 64), 128, 0)),
    (row(src=RAW, full=1, cpl=CHUNK, score=0), (duo(1, 2, 1, cpl=1), g(M, 64), 128, 0)),
    (row(src=RAW, full=1, cpl=CHUNK, sky=1), (duo(1, 2, 1, sky=1, cpl=1), g(M, 64), 192, 0)),
    (row(src=RAW, full=1, cpl=REPLAY, list=1, nlist=100), (duo(1, 2, 1, cpl=1, replay=1), 2, 128, 0)),
    (row(src=RAW, full=1, cpl=REPLAY, list=1, nlist=0), (duo(1, 2, 1, cpl=1, replay=1), 0, 128, 0)),
    (row(src=RAW, full=1, cpl=REPLAY, list=1, nlist=100, sky=1), ("NONE", 0, 256, 0)),
    (row(src=RAW, full=1, nl=8), ("NONE", 0, 256, 0)),
    # the knots, LEAN and FULL, both precisions
    (row(src=KNOTS), (duo(1, 1, 0), g(M, 64), 128, 0)),
    (row(src=KNOTS, full=1), (duo(1, 1, 1), g(M, 64), 128, 0)),
    (row(src=KNOTS, score=0), (duo(0, 1, 0), g(M, 64), 128, 0)),
    (row(src=KNOTS, full=1, score=0, wave_n=16000), (duo(0, 1, 1), 16000, 128, 0)),
    (row(src=KNOTS, nl=8), ("NONE", 0, 256, 0)),
    (row(f32=1, src=KNOTS), ("rs32::step_kernel_f32duo<1, true, false, false>", g(M, 128), 128, 0)),
    (row(f32=1, src=KNOTS, full=1), ("rs32::step_kernel_f32duo<1, true, true, false>", g(M, 128), 128, 0)),
    (row(f32=1, src=KNOTS, score=0), ("rs32::step_kernel_f32duo<1, false, false, false>", g(M, 128), 128, 0)),
    (row(f32=1, src=KNOTS, full=1, score=0, wave_n=99),
     ("rs32::step_kernel_f32duo<1, false, true, false>", g(M, 128), 128, 0)),
    # fp32 windows: two points per lane; REG / LDS forced: one point per lane; the general kernel for coupling,
    # an output depth (stream or tsurfOutputDepth), and FULL or sky view at NLayers != 15
    (row(f32=1), ("rs32::step_kernel_f32duo<0, true, false, false>", g(M, 128), 128, 0)),
    (row(f32=1, score=0, npoints=1000), ("rs32::step_kernel_f32duo<0, false, false, false>", g(1000, 128), 128, 0)),
    (row(f32=1, full=1), ("rs32::step_kernel_f32duo<0, true, true, false>", g(M, 128), 128, 0)),
    (row(f32=1, full=1, variant=LDS), ("rs32::step_kernel_f32duo<0, true, true, false>", g(M, 128), 128, 0)),
    (row(f32=1, full=1, score=0), ("rs32::step_kernel_f32duo<0, false, true, false>", g(M, 128), 128, 0)),
    (row(f32=1, full=1, sky=1), ("rs32::step_kernel_f32duo<0, true, true, true>", g(M, 128), 128, 0)),
    (row(f32=1, sky=1, score=0), ("rs32::step_kernel_f32duo<0, false, true, true>", g(M, 128), 128, 0)),
    (row(f32=1, variant=DUO), ("rs32::step_kernel_f32duo<0, true, false, false>", g(M, 128), 128, 0)),
    (row(f32=1, variant=HYBRID), ("rs32::step_kernel_f32duo<0, true, false, false>", g(M, 128), 128, 0)),
    (row(f32=1, variant=REG), ("rs32::step_kernel_f32_lds", g(M), 256, L32(15))),
    (row(f32=1, variant=LDS), ("rs32::step_kernel_f32_lds", g(M), 256, L32(15))),
    (row(f32=1, nl=8), ("rs32::step_kernel_f32_lds", g(M), 256, L32(8))),
    (row(f32=1, full=1, cpl=GENERAL), ("rs32::step_kernel_f32_coupled", g(M), 256, L32(15))),
    (row(f32=1, full=1, cpl=GENERAL, sky=1, nl=32), ("rs32::step_kernel_f32_coupled", g(M), 256, L32(32))),
    (row(f32=1, full=1, depth=1), ("rs32::step_kernel_f32_coupled", g(M), 256, L32(15))),
    (row(f32=1, full=1, depth=1, npoints=1000, variant=LDS), ("rs32::step_kernel_f32_coupled", g(1000), 256, L32(15))),
    (row(f32=1, full=1, nl=8), ("rs32::step_kernel_f32_coupled", g(M), 256, L32(8))),
    (row(f32=1, full=1, sky=1, nl=32), ("rs32::step_kernel_f32_coupled", g(M), 256, L32(32))),
    (row(f32=1, sky=1, nl=8), ("rs32::step_kernel_f32_coupled", g(M), 256, L32(8))),
    (row(f32=1, full=1, cpl=CHUNK), ("NONE", 0, 256, 0)),
    (row(f32=1, src=RAW, full=1), ("NONE", 0, 256, 0)),
    # the dressed wavefronts of tests/test_hip_sky_cpl_waves.py: 1 280 points with sky view, with coupling (1 120 of
    # them with coupling on: what a replay round lists at most), with both, at 15 and 12 layers, through the driver
    (row(full=1, sky=1, npoints=1280), (duo(1, 0, 1, sky=1), 20, 128, 0)),
    (row(full=1, sky=1, npoints=1280, score=0), (duo(0, 0, 1, sky=1), 20, 128, 0)),
    (row(full=1, sky=1, npoints=1280, a32=0), ("rs::step_kernel_sky_h<4>", 5, 256, 0)),
    (row(full=1, sky=1, npoints=1280, nl=12), ("rs::step_kernel_sky<false>", 5, 256, L64(12))),
    (row(src=RAW, full=1, sky=1, npoints=1280), (duo(1, 2, 1, sky=1), 20, 192, 0)),
    (row(full=1, cpl=GENERAL, npoints=1280), ("rs::step_kernel_coupled<false>", 5, 256, L64(15))),
    (row(full=1, cpl=CHUNK, npoints=1280), ("rs::step_kernel_cpl_h<3, false>", 5, 256, 0)),
    (row(full=1, cpl=REPLAY, npoints=1280, list=1, nlist=1120), ("rs::step_kernel_cpl_replay_h<3, false>", 5, 256, 0)),
    (row(full=1, cpl=GENERAL, npoints=1280, list=1, nlist=1120), ("rs::step_kernel_coupled<false>", 5, 256, L64(15))),
    (row(full=1, cpl=CHUNK, npoints=1280, nl=12), ("rs::step_kernel_cpl<false>", 5, 256, L64(12))),
    (row(full=1, cpl=REPLAY, npoints=1280, nl=12, list=1, nlist=1120),
     ("rs::step_kernel_cpl_replay<false>", 5, 256, L64(12))),
    (row(full=1, cpl=GENERAL, npoints=1280, nl=12, list=1, nlist=1120),
     ("rs::step_kernel_coupled<false>", 5, 256, L64(12))),
    (row(full=1, cpl=CHUNK, sky=1, npoints=1280), ("rs::step_kernel_cpl_h<3, true>", 5, 256, 0)),
    (row(full=1, cpl=REPLAY, sky=1, npoints=1280, list=1, nlist=1120),
     ("rs::step_kernel_cpl_replay_h<3, true>", 5, 256, 0)),
    (row(full=1, cpl=CHUNK, sky=1, npoints=1280, nl=12), ("rs::step_kernel_cpl<true>", 5, 256, L64(12))),
    (row(full=1, cpl=REPLAY, sky=1, npoints=1280, nl=12, list=1, nlist=1120),
     ("rs::step_kernel_cpl_replay<true>", 5, 256, L64(12))),
    (row(src=RAW, full=1, cpl=CHUNK, npoints=1280), (duo(1, 2, 1, cpl=1), 20, 128, 0)),
    (row(src=RAW, full=1, cpl=REPLAY, npoints=1280, list=1, nlist=1280), (duo(1, 2, 1, cpl=1, replay=1), 20, 128, 0)),
    (row(src=RAW, full=1, cpl=CHUNK, sky=1, npoints=1280), (duo(1, 2, 1, sky=1, cpl=1), 20, 192, 0)),
    (row(f32=1, full=1, sky=1, npoints=1280), ("rs32::step_kernel_f32duo<0, true, true, true>", 10, 128, 0)),
    (row(f32=1, full=1, sky=1, npoints=1280, score=0), ("rs32::step_kernel_f32duo<0, false, true, true>", 10, 128, 0)),
    (row(f32=1, full=1, cpl=GENERAL, npoints=1280), ("rs32::step_kernel_f32_coupled", 5, 256, L32(15))),
]


@pytest.mark.parametrize("shape,want", ROWS, ids=lambda v: None if isinstance(v, dict) else v[0])
def test_row(select, shape, want):
    assert select([shape])[0] == want, shape
