#!/usr/bin/env python3
"""Static instruction counts of one kernel, attributed to source lines.

usage: asm_attrib.py file.s kernel_mangled_name [--by func|line]
       asm_attrib.py file.s kernel_mangled_name --valu [--src roadsurf_amd/csrc]

file.s = `hipcc --cuda-device-only -gline-tables-only -S` output (the Makefile's HIPFLAGS otherwise).  Every
instruction is charged to the innermost .loc in force (file, line); lines are then grouped by file (or listed one
by one) so that one can see where the vector, scalar, memory and branch instructions of the time loop come from.
Static counts: a block that runs once per step counts once, the boundary-layer loop body counts once too.

--valu: the vector instructions of the TIME LOOPS alone (the loops that hold a workgroup barrier: the two
wavefronts' per-step loops of step_kernel_duo), by source REGION and opcode class, weighted by how often each
region runs per step.  The region of an instruction comes from the whole inline chain the compiler prints behind
its .loc (`; a.inc:165:45 @[ a.inc:873:9 @[ k.hip:1641:25 ] ]`): the functions those lines lie in are looked up in
the sources (--src) and the first rule of REGIONS that a frame satisfies names the region.  WEIGHTS holds the run
frequencies (profiles/r05_wave_stats*.txt); the weighted sum is the model's vector instructions
per 64 point-steps, to be set against SQ_INSTS_VALU.  The rules name functions and pieces of source text
('snow_here', 'ka_[', 'PSIM = R4(0.6)'): they follow the sources as they are and have to be kept up with them - the
rules that matched no instruction are listed under the table, and a rule that used to match and no longer does
is a rule to repair.

--check-thawed-skip: exit status 1 unless every select between layer_vsh's frozen constant and its polynomials
(the v_mov_b32 of 0x413d7ae0, the high word of 920 x 2100, with its two v_cndmask_b32) stands in a block that a
scalar branch (s_cbranch_scc*) jumps over - what the empty asm statement in layer_vsh is there to keep.

--check-last-pass-skip (file.s with line tables, -gline-tables-only): exit status 1 unless the final stability
correction of model_step_fluxes_prepped (the instructions inlined from its `bl_arm<false>(mt, Stab, x);`) begins in
a block that a scalar branch (s_cbranch_scc*, s_cbranch_vcc*) jumps over - what the empty asm statement in front of
it is there to keep.
"""
import collections
import os
import re
import sys


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op.startswith("s_cbranch") or op in ("s_branch", "s_setpc_b64", "s_swappc_b64"):
        return "branch"
    if op in ("s_waitcnt", "s_nop"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "scratch_", "buffer_", "flat_")):
        return "vmem"
    return "other"


VALU_CLASSES = ("f64", "cndmask", "mov", "cmp", "lane", "cvt", "int")


def valu_class(op):
    """fp64 arithmetic (v_rcp/v_rsq/v_ldexp/v_min/v_max included) | v_cndmask_b32 | v_mov_b32/_b64 and
    v_accvgpr_* | v_cmp* | v_readfirstlane/v_readlane/v_writelane | v_cvt* | integer and bit operations"""
    if op.startswith(("v_mov_", "v_accvgpr_")):
        return "mov"
    if op.startswith("v_cndmask"):
        return "cndmask"
    if op.startswith("v_cmp"):
        return "cmp"
    if op.startswith(("v_readfirstlane", "v_readlane", "v_writelane")):
        return "lane"
    if op.startswith("v_cvt"):
        return "cvt"
    if "_f64" in op:
        return "f64"
    return "int"


# ---- --valu: regions and weights --------------------------------------------------------------------------------------
# (function a frame lies in, substring of that frame's source line or None, wave or None) -> region; first match wins,
# frames are tried from the innermost outwards.  wave: "surface" / "ground" = the frame chain passes through
# duo_surface / duo_ground.
FINAL_ARM = "bl_arm<false>(mt, Stab, x);"  # model_step_fluxes_prepped's final stability correction, by its source text
FINAL_REGION = "boundary-layer: final correction (skipped where every lane is dead and Stab proves the sign)"
EAIR_REGION = "CalcLE: EAir (skipped where every lane is dry and warmer than the air)"
ESURF_REGION = "CalcLE: ESurf (skipped where every lane is dry and warmer than the air)"
TAIL_REGION = "CalcLE: tail (skipped where every lane is dry and evaporating)"
# (function, substring) that names the region from ANY frame of the chain, before the innermost-first rules below:
# the final correction is bl_arm, rs_log and rs_sq like every pass's, told apart by the line it is inlined from
OUTER = [
    ("model_step_fluxes_prepped", FINAL_ARM, FINAL_REGION),
]
REGIONS = [
    ("boundary_layer_ieee", None, None, "guard (IEEE redo, out of line)"),
    ("knot_forcing", None, None, "knot interpolation"),
    ("knot_begin", None, None, "knot interpolation"),
    ("rs_sy_hour", None, None, "knot interpolation"),
    ("precipitation_to_storage", None, None, "precipitation (CalcPrecType)"),
    ("forcing_prep_head", None, None, "ForcingPrep"),
    ("check_values_forcing", None, None, "ForcingPrep"),
    ("forcing_prep_tail", None, None, "ForcingPrep"),
    ("forcing_prep", None, None, "ForcingPrep"),
    ("duo_put_prep", None, None, "mailbox put"),
    ("duo_get_prep", None, None, "mailbox get"),
    ("check_values_tsurf", None, None, "CheckValues (surface temperature)"),
    ("air_vapour_pressure", None, None, EAIR_REGION),
    ("rs_log", None, None, "boundary-layer pass: unstable arm, log (two paths, one taken)"),
    ("model_step_fluxes_prepped", "boundary_layer_ieee", None, "guard (IEEE redo, out of line)"),
    ("model_step_fluxes_prepped", "__builtin_inf", None, "ESurf / fluxes"),
    ("dry_tail_signs", None, None, "CalcLE: dry-tail tests"),
    ("dry_tail_le", None, None, "CalcLE: dry-tail tests"),
    ("dry_tail_warm", None, None, "CalcLE: dry-tail tests"),
    ("dry_tail_dry", None, None, "CalcLE: dry-tail tests"),
    ("dry_tail_warm_t", None, None, "CalcLE: dry-tail tests"),
    ("dry_tail_psychc", None, None, "CalcLE: dry-tail tests"),
    ("model_step_fluxes_prepped", "dry_tail_psychc", None, "CalcLE: dry-tail tests"),
    ("le_numerator", None, None, ESURF_REGION),
    ("model_step_fluxes_prepped", "psychrometric", None, TAIL_REGION),
    ("model_step_fluxes_prepped", "rs_wave_all", None, "CalcLE: dry-tail tests"),
    ("model_step_fluxes_prepped", "RAero", None, TAIL_REGION),
    ("model_step_fluxes_prepped", "WatDen", None, TAIL_REGION),
    ("model_step_fluxes_prepped", "lfus", None, TAIL_REGION),
    ("model_step_fluxes_prepped", "fx.le > ", None, TAIL_REGION),
    ("model_step_fluxes_prepped", "ESurf", None, ESURF_REGION),
    ("model_step_fluxes_prepped", "s.tsurf < 0", None, ESURF_REGION),
    ("bl_arm", "rs_log", None, "boundary-layer pass: unstable arm"),
    ("bl_arm", "PSIM = R4(0.6)", None, "boundary-layer pass: unstable arm"),
    ("bl_arm", None, None, "boundary-layer pass"),
    ("bl_pass", None, None, "boundary-layer pass"),
    ("bl_iteration", None, None, "boundary-layer pass"),
    ("fluxes_post", None, None, "ESurf / fluxes"),
    ("model_step_fluxes_prepped", None, None, "ESurf / fluxes"),
    ("layer_vsh", None, "surface", "layers 1-2: thawed arm"),
    ("layer_vsh", None, "ground", "layers 3-15: thawed arm"),
    ("layer_step", "rs_div(", "surface", "layers 1-2: thawed arm"),
    ("layer_step", "rs_div(", "ground", "layers 3-15: thawed arm"),
    ("layer_step", "RS_DIVC(", "surface", "layers 1-2: thawed arm"),
    ("layer_step", "capDZF", "surface", "layers 1-2: frozen arm"),
    ("layer_step", "hs1F", "surface", "layers 1-2: frozen arm"),
    ("layer_step", "capDZF", "ground", "layers 3-15: frozen arm"),
    ("layer_step", None, "surface", "layers 1-2: flux and update"),
    ("layer_step", None, "ground", "layers 3-15: flux and update"),
    ("melting", None, None, "melting"),
    ("road_condition", "alb", None, "albedo"),
    ("road_condition", "IceSum", None, "albedo"),
    ("road_condition", "bare", None, "storages: bare-road test and shortcut"),
    ("road_condition", "verycold", None, "storages: bare-road test and shortcut"),
    ("road_condition", None, None, "storages"),
    ("model_step_ground", None, "surface", "layers 1-2: flux and update"),
    ("store_outputs", None, None, "output stores"),
    ("output_row", None, None, "output stores"),
    ("blank_rows", None, None, "output stores"),
    ("duo_surface", None, None, "loop control, mailbox values, state (surface wave)"),
    ("duo_ground", None, None, "loop control, mailbox values, state (ground wave)"),
]
# runs per wave-step of one copy of the region's code.  The compiler peels four boundary-layer passes and keeps a
# rolled loop for the rest (6.21 passes per wave-step: 4 x 1 + 1 x 2.21); a region that sits in that inner loop gets
# BL_ROLLED automatically.  Thirteen copies of the layer code on the ground wave, two on the surface wave, one each.
BL_ROLLED = 6.21 - 4.0
THAWED = 6.2 / 13.0  # 5.4 - 7 of 13 layers take the thawed arm
# (layer_vsh's select between the frozen constant and the polynomials - a literal and two v_cndmask_b32 that only a
# wavefront with frozen AND thawed points in the layer runs - has no line of its own in the line table: it is
# charged with the thawed arm, at the thawed arm's weight, which overstates it)
WEIGHTS = {
    "guard (IEEE redo, out of line)": 0.0,
    "knot interpolation": 1.0,          # (the per-interval reload inside it runs every 120th index: see RELOAD)
    "precipitation (CalcPrecType)": 0.034,
    # profiles/r05_wave_stats.txt: 0.6176 of the passes a wavefront issues have a lane on the unstable arm; log's
    # table path runs in 0.3334 of the passes and its polynomial path in 0.4005 (0.6176 - 0.3334 + 0.1163 on both):
    # every instruction of rs_log belongs to one of the two, charged at their mean
    "boundary-layer pass: unstable arm": 0.6176,
    "boundary-layer pass: unstable arm, log (two paths, one taken)": 0.367,
    "layers 1-2: thawed arm": THAWED, "layers 3-15: thawed arm": THAWED,
    "layers 1-2: frozen arm": 1.0 - THAWED, "layers 3-15: frozen arm": 1.0 - THAWED,
    # profiles/r09_dry_tail_counts.txt: every lane dry and evaporating in 0.6458 of the wave-steps, dry and warmer than
    # the air by the margin in 0.4406
    # profiles/r10_last_pass_counts.txt: the final correction is skipped in 0.6458 of the wave-steps (every wave-step
    # in which all lanes are dead: no Stab at or below stabSafe there), and the tail runs where it is not
    TAIL_REGION: 1.0 - 0.6458,
    FINAL_REGION: 1.0 - 0.6458,
    # two copies each of ESurf's and EAir's code: in front of the loop (a wavefront that is not all-warm: 1 - 0.4406)
    # and in the tail (all-warm and not skipped: no such wave-step on the bench workload) - the mean of the two
    ESURF_REGION: 0.5 * (1.0 - 0.4406),
    EAIR_REGION: 0.5 * (1.0 - 0.4406),
    "melting": 0.10,
    "storages": 1.0 - 0.615,            # the bare-road shortcut takes 61.5 % of the wave-steps
    "albedo": 1.0 - 0.615,
}
RELOAD = ("ka_[", "kb_[", "K.dv[q]", "K.ph0 =", "K.ph1 =", "has_b", "kcur = k",
          "K.hour", "K.night =")  # knot_forcing's once-per-interval block (any line that names K.hour: its per-index use is a scalar copy)
SNOW, ICE = 0.06, 0.10  # of the wave-steps carry snow / ice (storages' sub-blocks, by their source text)


def functions_of(src_dir):
    """{file name: sorted [(first line, function name)]} of the device functions and lambdas in the sources"""
    out = {}
    pat = re.compile(r"^\s*(?:template\s*<[^>]*>\s*)?(?:static\s+)?(?:__device__|__global__)\b")
    name_pat = re.compile(r"\b([A-Za-z]\w*)\s*\(")  # (a lambda belongs to the function it is written in)
    for name in os.listdir(src_dir):
        if not name.endswith((".hip", ".hpp", ".h", ".inc")):
            continue
        rows, lines = [], open(os.path.join(src_dir, name), errors="replace").read().split("\n")
        for i, ln in enumerate(lines, 1):
            if pat.match(ln) and ";" not in ln.split("{")[0]:
                names = [n for n in name_pat.findall(ln.split("{")[0]) if not n.startswith("__")]
                if names:
                    rows.append((i, names[0]))
        out[name] = (rows, lines)
    return out


MATCHED = set()


def frame_info(funcs, fname, line):
    rows, lines = funcs.get(os.path.basename(fname), ([], []))
    fn = None
    for first, name in rows:
        if first <= line:
            fn = name
        else:
            break
    return fn, (lines[line - 1] if 0 < line <= len(lines) else "")


def region_of(frames, funcs):
    """(region or None, frame infos); None: nothing but line 0 - a copy the compiler made, charged where it stands"""
    info = [frame_info(funcs, f, l) for f, l in frames if l > 0]
    if not info:
        return None, info
    fns = [fn for fn, _ in info]
    wave = "surface" if "duo_surface" in fns else "ground" if "duo_ground" in fns else None
    for fn, text in info:
        for rfn, sub, region in OUTER:
            if fn == rfn and sub in text:
                MATCHED.add((rfn, sub, None, region))
                return region, info
    for fn, text in info:
        for rule in REGIONS:
            rfn, sub, rwave, region = rule
            if fn == rfn and (sub is None or sub in text) and (rwave is None or rwave == wave):
                MATCHED.add(rule)
                return region, info
    return "other (%s)" % (fns[-1] if fns and fns[-1] else "?"), info


def valu_table(path, kernel, src_dir):
    funcs = functions_of(src_dir)
    # pass 1: the kernel's lines, its blocks' loops
    body, inside = [], False
    for ln in open(path):
        if ln.startswith(kernel + ":"):
            inside = True
            continue
        if inside:
            if ln.startswith(".Lfunc_end"):
                break
            body.append(ln.rstrip("\n"))
    loop_of, parent, cur_loop, barrier_loops = {}, {}, None, set()
    blocks = []  # (outermost loop or None, innermost loop or None, [(op, frames)])
    frames = []
    cur = None
    i = 0
    while i < len(body):
        ln = body[i]
        m = re.match(r"^(\.LBB\d+_\d+):|^; %bb\.\d+:", ln)
        if m:
            label = m.group(1)
            text = ln
            j = i + 1
            while j < len(body) and re.match(r"^\s+;", body[j]) and not body[j].lstrip().startswith("; %bb"):
                text += " " + body[j]
                j += 1
            inner = outer = None
            mh = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", text)
            mp = re.search(r"Parent Loop (BB\d+_\d+) Depth=1", text)
            if "Loop Header" in text and label:
                inner = label[2:]
                outer = mp.group(1) if mp else inner
            elif mh:
                inner = mh.group(1)
                outer = mp.group(1) if mp else (inner if mh.group(2) == "1" else parent.get(inner))
            if inner and outer:
                parent.setdefault(inner, outer)
            cur = (outer, inner, [])
            blocks.append(cur)
            i = j
            continue
        m = re.match(r"\s*\.loc\s+\d+\s+\d+.*?;\s*(.*)$", ln)
        if m:
            frames = [(a, int(b)) for a, b in re.findall(r"([\w./+-]+):(\d+):\d+", m.group(1))]
        else:
            m = re.match(r"\s+([a-z_0-9]+)", ln)
            if m and not ln.lstrip().startswith((".", ";")) and cur is not None:
                op = m.group(1)
                cur[2].append((op, frames))
                if op == "s_barrier" and cur[0]:
                    barrier_loops.add(cur[0])
        i += 1
    # pass 2: the vector instructions of the time loops
    table = collections.defaultdict(lambda: collections.defaultdict(collections.Counter))  # region -> weight -> class
    last_region = "other (?)"
    for outer, inner, ins in blocks:
        if outer not in barrier_loops:
            continue
        rolled = inner != outer
        for op, fr in ins:
            if not op.startswith("v_"):
                continue
            region, info = region_of(fr, funcs)
            if region is None:
                region = last_region
            last_region = region
            w = WEIGHTS.get(region, 1.0)
            texts = " ".join(t for _, t in info)
            if region == "knot interpolation" and any(s in texts for s in RELOAD):
                region, w = "knot interpolation: new interval (every 120th index)", 1.0 / 120.0
            if region == "storages":
                if "snow_here" in texts or "SnowTran" in texts or "WatSnowRat" in texts:
                    region, w = "storages: snow blocks", SNOW
                elif "ice_here" in texts or "freezes" in texts:
                    region, w = "storages: ice blocks", ICE
            if rolled and region.startswith(("boundary-layer", "ESurf", "other")):
                w *= BL_ROLLED
                region += " [rolled loop]"
            table[region][w][valu_class(op)] += 1
    print(f"{'region':62s} {'weight':>6s} " + " ".join(f"{c:>7s}" for c in VALU_CLASSES) + f" {'static':>7s} {'weighted':>8s}")
    tot_s, tot_w, tot_c = 0, 0.0, collections.Counter()
    for region in sorted(table, key=lambda r: -sum(w * sum(c.values()) for w, c in table[r].items())):
        for w, c in sorted(table[region].items()):
            n = sum(c.values())
            tot_s += n
            tot_w += n * w
            for k, v in c.items():
                tot_c[k] += v * w
            print(f"{region[:62]:62s} {w:6.3f} " + " ".join(f"{c[k]:7d}" for k in VALU_CLASSES) + f" {n:7d} {n * w:8.1f}")
    print(f"{'TOTAL (weighted by class; static; weighted)':62s} {'':6s} " + " ".join(f"{tot_c[k]:7.1f}" for k in VALU_CLASSES)
          + f" {tot_s:7d} {tot_w:8.1f}")
    idle = [r for r in REGIONS + [(f, t, None, r) for f, t, r in OUTER] if r not in MATCHED]
    if idle:
        print("rules that matched no instruction of this kernel's time loops: "
              + "; ".join(f"{r[0]}{' ~ ' + repr(r[1]) if r[1] else ''}{' @' + r[2] if r[2] else ''}" for r in idle))


def check_thawed_skip(path, kernel):
    """(selects found, selects NOT jumped over by a scalar branch): the blocks that materialise 920 x 2100 for
    layer_vsh's select (tests/test_thawed_skip_asm.py compiles the kernels and calls this)"""
    inside, prev_op, block_guarded, found, bad = False, None, False, 0, 0
    for ln in open(path):
        if ln.startswith(kernel + ":"):
            inside = True
            continue
        if not inside:
            continue
        if ln.startswith(".Lfunc_end"):
            break
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", ln):
            block_guarded = prev_op is not None and prev_op.startswith("s_cbranch_scc")
            continue
        m = re.match(r"\s+([a-z_0-9]+)\s*(.*)", ln)
        if not m or ln.lstrip().startswith((".", ";")):
            continue
        if m.group(1).startswith("v_mov_b32") and "0x413d7ae0" in m.group(2):
            found += 1
            bad += 0 if block_guarded else 1
        prev_op = m.group(1)
    return found, bad


def check_last_pass_skip(path, kernel, src_dir=None):
    """(vector instructions of the final stability correction, True where the block its first one stands in is
    jumped over by a scalar branch); path: assembly with line tables (tests/test_last_pass_skip_asm.py compiles the
    kernels and calls this)"""
    src_dir = src_dir or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "roadsurf_amd", "csrc")
    funcs = functions_of(src_dir)
    inside, prev_op, block_guarded, frames, found, guarded = False, None, False, [], 0, False
    for ln in open(path):
        if ln.startswith(kernel + ":"):
            inside = True
            continue
        if not inside:
            continue
        if ln.startswith(".Lfunc_end"):
            break
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", ln):
            block_guarded = prev_op is not None and prev_op.startswith(("s_cbranch_scc", "s_cbranch_vcc"))
            continue
        m = re.match(r"\s*\.loc\s+\d+\s+\d+.*?;\s*(.*)$", ln)
        if m:
            frames = [(a, int(b)) for a, b in re.findall(r"([\w./+-]+):(\d+):\d+", m.group(1))]
            continue
        m = re.match(r"\s+([a-z_0-9]+)\s*(.*)", ln)
        if not m or ln.lstrip().startswith((".", ";")):
            continue
        if m.group(1).startswith("v_") and any(fn == "model_step_fluxes_prepped" and FINAL_ARM in text
                                               for fn, text in (frame_info(funcs, f, l) for f, l in frames if l > 0)):
            if found == 0:
                guarded = block_guarded
            found += 1
        prev_op = m.group(1)
    return found, guarded


def main():
    path, kernel = sys.argv[1], sys.argv[2]
    if "--check-last-pass-skip" in sys.argv:
        found, guarded = check_last_pass_skip(path, kernel)
        print(f"{found} vector instructions of the final stability correction in {kernel}, "
              f"{'behind' if guarded else 'NOT behind'} a scalar branch")
        sys.exit(0 if found and guarded else 1)
    if "--check-thawed-skip" in sys.argv:
        found, bad = check_thawed_skip(path, kernel)
        print(f"{found} frozen/thawed selects in {kernel}, {bad} of them not behind a scalar branch")
        sys.exit(1 if bad or not found else 0)
    if "--valu" in sys.argv:
        src = sys.argv[sys.argv.index("--src") + 1] if "--src" in sys.argv else \
            os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "roadsurf_amd", "csrc")
        valu_table(path, kernel, src)
        return
    by = "line" if "--by" in sys.argv and sys.argv[sys.argv.index("--by") + 1] == "line" else "file"
    files = {}
    cur = (0, 0)
    inside = False
    counts = collections.defaultdict(lambda: collections.Counter())
    for ln in open(path):
        m = re.match(r"\s*\.file\s+(\d+)\s+\"[^\"]*\"\s+\"([^\"]+)\"", ln)
        if m:
            files[int(m.group(1))] = m.group(2)
            continue
        if ln.startswith(kernel + ":"):
            inside = True
            continue
        if not inside:
            continue
        if ln.startswith(".Lfunc_end"):
            break
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", ln)
        if m:
            cur = (int(m.group(1)), int(m.group(2)))
            continue
        m = re.match(r"\s+([a-z_0-9]+)", ln)
        if not m or ln.lstrip().startswith((".", ";")):
            continue
        op = m.group(1)
        cls = classify(op)
        if cls == "other":
            continue
        key = (files.get(cur[0], "?"), cur[1]) if by == "line" else files.get(cur[0], "?")
        counts[key][cls] += 1
    tot = collections.Counter()
    keys = sorted(counts, key=lambda k: -sum(counts[k].values()))
    print(f"{'where':50s} {'valu':>6s} {'salu':>6s} {'smem':>6s} {'branch':>6s} {'wait':>6s} {'lds':>5s} {'vmem':>5s}")
    for k in keys:
        c = counts[k]
        tot.update(c)
        name = f"{k[0]}:{k[1]}" if by == "line" else k
        print(f"{name:50s} {c['valu']:6d} {c['salu']:6d} {c['smem']:6d} {c['branch']:6d} {c['wait']:6d} {c['lds']:5d} {c['vmem']:5d}")
    print(f"{'TOTAL':50s} {tot['valu']:6d} {tot['salu']:6d} {tot['smem']:6d} {tot['branch']:6d} {tot['wait']:6d} {tot['lds']:5d} {tot['vmem']:5d}")


if __name__ == "__main__":
    main()
