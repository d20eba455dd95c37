/*
 * rs_physics.hpp — one RoadSurf time step for one point, as device code.
 *
 * One point per lane.  The ground temperature profile is reached through a
 * small accessor (registers for the NLayers-specialised kernel, an LDS column
 * for the generic one); every other piece of carried state is a scalar in
 * VGPRs.  Layer constants come from RsConstants (kernel argument -> SGPRs).
 *
 * Arithmetic contract: fp64, IEEE + - * / sqrt in the
 * reference's evaluation order, no FMA contraction (the translation unit is
 * compiled with -ffp-contract=off), every unsuffixed Fortran literal is REAL(4)
 * and enters as R4(x) = (double)x##f.  exp/log are the only operations that are
 * not bit-defined by IEEE; see rs_math.hpp.
 *
 * The reference splits this work over ~20 subroutines that communicate through
 * derived types; here it is fused into one pass with the dead stores removed:
 *   - GCond, HS(2:), GroundFlux, SnowIceRat, WetSnowFrozen, Rain/SnowIntensity,
 *     PrecType, Tdew, SensibleHeatFlux are never read on this path;
 *   - condDZ is constant in time and comes from RsConstants;
 *   - VSH/capDZ/flux/update of a layer are one loop body with a rolling flux
 *     instead of three loops over heap/array temporaries
 *     (src/BalanceModel.f90:109 allocates Gflux every call);
 *   - atm%BLCond need not be carried: it only seeds BLCond_Old at j = 1 and the
 *     loop cannot exit before j = 5 (src/BoundaryLayer.f90:67,92).
 * Each block cites the reference lines it restates.
 */
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/roadsurf.h"
#include "rs_math.hpp"
#include "rs_consts_dev.h"


#define RS_REAL double
#define RS_NS rs
/* the constants are read as constant memory (scalar loads): rs_kernels.hip, consts_of */
#define RS_CONSTS RsConstantsDev __attribute__((address_space(4)))
/* a / b with b uniform and its reciprocal in the constant block */
#define RS_DIVC(a, b, rb) rs_div_u(a, b, c.rb)
/* ---- the fp64 flavour's side of rs_general_body.inc (the fp32 one: the head of rs_kernels_f32.hip) ---- */
#define RS_SECANT_DIV(a, b) ((a) / (b)) /* Coupling_control's secant: the IEEE quotient, as the reference forms it */
#define RS_PROFILE_PIN 1                /* RegProfile::pin holds the new profile in place (see there) */
#define RS_CPL_SLOTS(c) true            /* the coupling slots of the state block are written and read by every plan */
#define RS_CPL_DECAY_TABLE 1            /* the coupling decay from the plan's table (RsConstantsDev::cpl_tab) */
#define RS_RELAX_TABLE 1                /* the relaxation factor likewise (RsConstantsDev::relax_tab) */
#define RS_GEN_PREFETCH 1               /* the general loop fetches the next index's forcing half a step early */
#define RS_GEN_FP64_FEATURES 1          /* diagnostics, write-back of the in-place input edits, the cpl_stop park */
#define RS_INIT_KERNEL init_kernel      /* the name of the kernel that makes the initial state */
#define RS_INIT_ANCHOR R4(-99.9)        /* the relaxation anchors' seed, src/Initialization.f90:377-379 */
#define RS_INIT_ZERO_TAIL 1             /* init zeroes the profile slots behind NLayers */
#define RS_BL_GUARD 1
#define RS_MELTDEN c.meltDen /* WatMHeat*WatDens, the same IEEE product formed once on the host */
#define RS_BARE_FAST(c) ((c).bareFastOk != 0) /* rs_consts_dev.h */
#define RS_PREC_FAST(c) ((c).precFastOk != 0)
#define RS_CHK(c, i, lit) ((c).chk[i])         /* rs_consts_dev.h: CheckValues' bounds */
#define R4(x) ((double)(x##f))
#ifndef RS_NO_FROZEN_TABLE
#define RS_FROZEN_TABLE 1 /* layer_step: capDZ of a layer that is frozen in all 64 points from RsConstantsDev::capDZF */
#endif
/* the five per-layer constants of layer_step next to one another (RsConstantsDev::lk): one scalar load per
 * layer instead of one per table (-DRS_NO_LAYER_ROWS: the tables of RsConstants) */
#ifndef RS_NO_LAYER_ROWS
#define RS_LK(c, j, name) ((c).lk[j].name)
#else
#define RS_LK(c, j, name) ((c).name[j])
#endif
#ifndef RS_NO_HCW_TABLE
#define RS_HCW_TABLE 1 /* layer_vsh: the water polynomials' coefficients from RsConstantsDev::hcw */
#endif
#define RS_STAB_UPPER(x) rs_min_one(x) /* bl_iteration: the stability parameter's upper clamp, one v_min_f64 in the stable arm */
/* CalcLE's tail skipped for a wavefront in which the reference zeroes it in every point (rs_physics_body.inc, DRY
 * TAIL; the argument there rests on this flavour's correctly rounded arithmetic).  A/B builds: -DRS_NO_DRY_TAIL_SKIP
 * is the text without either stage, -DRS_NO_DRY_ESURF_SKIP the first stage alone.
 * On top of both stages, for the two-wavefront kernels (model_step_fluxes_prepped):
 *   RS_BL_LAST       the boundary-layer loop carries Stab, and the stability correction of its exit pass is evaluated
 *                    only where the tail is alive or Stab does not prove the sign it is needed for
 *                    (-DRS_NO_BL_LAST_SKIP: the correction at the end of every pass, as it stood)
 *   RS_EAIR_SURFACE  the air's vapour pressure is formed by the surface wave, where a wavefront needs it, instead of
 *                    by the ground wave for every index (-DRS_NO_EAIR_SURFACE: worked out ahead and mailed)
 * These two stay defined: rs_kernels.hip's mailbox follows them. */
#ifndef RS_NO_DRY_TAIL_SKIP
#define RS_DRY_TAIL 1
#if !defined(RS_NO_DRY_ESURF_SKIP) && !defined(RS_EXP_SURFACE_LIGHT) && !defined(RS_EXP_PIPE1)
#define RS_DRY_ESURF 1
#if !defined(RS_NO_BL_LAST_SKIP) && !defined(RS_EXP_STAB_CHAIN)
#define RS_BL_LAST 1
#endif
#ifndef RS_NO_EAIR_SURFACE
#define RS_EAIR_SURFACE 1
#endif
#endif
#endif
#include "rs_physics_body.inc"
#undef RS_DRY_TAIL
#undef RS_DRY_ESURF
#undef RS_STAB_UPPER
#undef RS_FROZEN_TABLE
#undef RS_HCW_TABLE
#undef RS_LK
/* (RS_REAL, R4, RS_DIVC and the rs_general_body.inc macros above stay defined: rs_kernels.hip includes that text) */
#undef RS_NS
#undef RS_CONSTS
#undef RS_BL_GUARD
#undef RS_MELTDEN
#undef RS_BARE_FAST
#undef RS_PREC_FAST
#undef RS_CHK

#include "rs_skyview.hpp" /* sky_view_radiation */
