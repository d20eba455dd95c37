/* rs_physics_body.inc - the model physics, written once and instantiated per arithmetic
 * type by rs_physics.hpp (RS_REAL = double, namespace rs: the parity path) and by
 * rs_kernels_f32.hip (RS_REAL = float, namespace rs32: BASELINE config 5).
 * Needs: RS_REAL, RS_NS, RS_CONSTS, R4(x). */
namespace RS_NS {

/* Scalar carried state of one point (SURVEY.md Appendix B). */
struct Scalars {
  RS_REAL tnw1, tnw2; /* TmpNw(1:2) */
  RS_REAL tsurf;      /* surf%TsurfAve */
  RS_REAL wat, snow, ice, ice2, dep;
  RS_REAL q2melt, t4melt, albedo;
  RS_REAL tair_end, vz_end, rh_end; /* relaxation anchors */
  bool verycold, failed;
};

/* Forcing of one time index. */
struct Forcing {
  RS_REAL tair, tdew, vz, rhz, prec, sw, lw, tsurfobs, depth;
  int32_t phase, hour;
};

/* Temperature at depth (src/BalanceModel.f90:390-417); T(k) = Tmp(k), k=1..N,
 * tbot = Tmp(N+1).  Selects instead of a data-dependent index so the register
 * profile never needs dynamic indexing. */
template <class Prof>
__device__ __forceinline__ RS_REAL temp_at_depth(const RS_CONSTS &c, const Prof &T, RS_REAL tbot,
                                                RS_REAL depth) {
  const int N = T.nlayers();
  if (rs_fabs(depth - R4(0.0)) < R4(0.00001)) return T.get(1);
  if (depth > c.ZDpth[N + 1]) return tbot;
  RS_REAL r = 0.0;
  bool found = false;
#pragma unroll
  for (int k = 1; k <= N; ++k) {
    const RS_REAL zk = c.ZDpth[k], zk1 = c.ZDpth[k + 1];
    if (!found && depth > zk && depth <= zk1) {
      const RS_REAL tk = T.get(k);
      const RS_REAL tk1 = (k == N) ? tbot : T.get(k + 1);
      r = tk + rs_div((depth - zk) * (tk1 - tk), zk1 - zk);
      found = true;
    }
  }
  return r;
}

template <class Prof>
__device__ __forceinline__ RS_REAL surface_temperature(const RS_CONSTS &c, const Prof &T,
                                                      RS_REAL tbot, RS_REAL depth) {
  if (depth >= 0) return temp_at_depth(c, T, tbot, depth);
  return (T.get(1) + T.get(2)) / R4(2.0);
}

/* src/Cond.f90:143-249 + src/Storage.f90:9-29 */
__device__ __forceinline__ void precipitation_to_storage(const RS_CONSTS &c, const MathTab &mt,
                                                         Scalars &s, int32_t phase,
                                                         RS_REAL &prec_ts, RS_REAL tair, RS_REAL rhz) {
  RS_REAL rain = R4(0.0), snow = R4(0.0);
  bool interpret = true;
  if ((RS_REAL)phase > c.MissValI) {
    interpret = false;
    if (prec_ts <= c.MinPrecmm) {
      prec_ts = R4(0.0);
    } else {
      switch (phase) {
        case 0: case 1: case 4: case 5: rain = prec_ts; break;
        case 2: snow = prec_ts / R4(2.); rain = snow; break;
        case 3: case 6: snow = prec_ts; break;
        default: interpret = true;
      }
    }
  }
  if (interpret) {
    if (prec_ts <= c.MinPrecmm) {
      prec_ts = R4(0.0);
      rain = R4(0.0);
      snow = R4(0.0);
    } else {
      const RS_REAL pexp = R4(22.0) - R4(2.7) * tair - R4(0.20) * rhz;
      const RS_REAL prain = rs_div(R4(1.0), R4(1.0) + rs_exp(mt, pexp));
      if (prain < c.PLimSnow) {
        snow = prec_ts;
        rain = R4(0.0);
      } else if (prain > c.PLimRain) {
        rain = prec_ts;
        snow = R4(0.0);
      } else {
        snow = prec_ts / R4(2.);
        rain = snow;
      }
    }
  }
  s.wat = s.wat + rain;
  s.snow = s.snow + snow;
}

/* src/BoundaryLayer.f90:3-109 (+ calcRaero :112-131, CalcLE :134-190), in three pieces so
 * that a kernel can run the fixed-point loop its own way (the trip count is 5 for 80 % of the
 * point-steps and up to 35 for the rest: tools/bl_iterations.py):
 *   bl_setup      :50-62   air properties and the loop invariants
 *   bl_iteration  :64-96   one pass of the loop body; returns true where the loop exits
 *   bl_finish     calcRaero, CalcLE
 * boundary_layer() below is the plain composition. */
struct BlInv { /* per-point values the loop only reads */
  RS_REAL dT, den0, vkvz, avk;
#ifdef RS_EXP_STAB_CHAIN
  RS_REAL kinv; /* 1 / (den0 vkvz^3) */
#endif
};
struct BlVar { /* carried by the loop */
  RS_REAL PSIM, PSIH, BLCond;
};
struct BlAux { /* needed again after the loop */
  RS_REAL AirDens, AirHCap, PsychC, WatDen;
};

#ifndef RS_BL_MAXIT
#define RS_BL_MAXIT 40
#endif
#ifndef RS_LAYER_GROUP
#define RS_LAYER_GROUP 4 /* layers per group of constant loads in model_step_ground (0: no grouping) */
#endif

template <bool IEEE = false>
__device__ __forceinline__ void bl_setup(const RS_CONSTS &c, RS_REAL tsurf, RS_REAL tair,
                                         RS_REAL vz, BlInv &v, BlVar &x, BlAux &a) {
  const RS_REAL TaK = tair + R4(273.15);
  a.AirDens = rs_dv<IEEE>(R4(100000.0), R4(287.05) * TaK);
  const RS_REAL dK = (TaK - R4(250.0)) * (TaK - R4(250.0));
  a.AirHCap = R4(1005.0) + (IEEE ? rs_dv<true>(dK, R4(3364.)) : RS_DIVC(dK, R4(3364.), r_3364));
  const RS_REAL AirVCap = a.AirHCap * a.AirDens;
  a.PsychC = R4(0.1) * (R4(0.00063) * TaK + R4(0.47496));
  a.WatDen = R4(-0.0050) * tsurf * tsurf + R4(0.0079) * tsurf + R4(1000.0028);
  /* loop invariants of :78-79, same association as the reference */
  v.dT = tsurf - tair;
  v.den0 = AirVCap * (tair + R4(273.15));
  v.vkvz = c.VK_Const * vz;
  v.avk = AirVCap * c.VK_Const;
#ifdef RS_EXP_STAB_CHAIN
  v.kinv = rs_div((RS_REAL)1.0, v.den0 * (v.vkvz * v.vkvz * v.vkvz));
#endif
  x.PSIM = R4(0.0);
  x.PSIH = R4(0.0);
  x.BLCond = 0.0;
}

/* -VK*ZRefT*Grav of :78, associated as the reference does; uniform, evaluated once per loop */
__device__ __forceinline__ RS_REAL bl_stab_num(const RS_CONSTS &c) {
  return -c.VK_Const * c.ZRefT * c.Grav;
}

/* One pass is two halves: bl_pass (:66-80: UStar, BLCond, Stab, and the exit test of :92, which reads nothing of what
 * follows) and bl_arm (:83-89: the stability correction from Stab, which only the NEXT pass and calcRaero read). */
template <bool IEEE = false>
__device__ __forceinline__ bool bl_pass(const RS_CONSTS &c, const BlInv &v, BlVar &x, int j, RS_REAL stab_num,
                                        RS_REAL &Stab) {
  const RS_REAL ConvLim = R4(0.001);
  const RS_REAL BLCond_Old = x.BLCond;
  RS_REAL UStar;
  if (!IEEE && j == 1) {
    /* first pass: PSIM = PSIH = +0.0 (:62), and d + 0.0 == d for the nonzero d that plan creation
     * insists on, so both denominators are the uniform logarithms themselves */
    UStar = RS_DIVC(v.vkvz, c.logUstar, r_logUstar);
    x.BLCond = RS_DIVC(v.avk * UStar, c.logCond, r_logCond);
  } else {
    UStar = rs_dvb<IEEE>(v.vkvz, c.logUstar + x.PSIM);
    x.BLCond = rs_dvb<IEEE>(v.avk * UStar, c.logCond + x.PSIH);
  }
#ifdef RS_EXP_STAB_CHAIN
  /* (experiment build, tools/experiments/r6_stab_chain.sh - NOT the reference's bits) an upper bound of what a
   * shorter dependent chain in the stable arm can buy a small shard: 1 / (den0 UStar^3) = a^3 / (den0 vkvz^3) with
   * a = logUstar + PSIM, known seven operations before UStar - here taken as the reciprocal itself (no Newton step,
   * no remainder, no correction: three levels fewer than the exact variant DESIGN.md 8 item 4 describes could have) */
  const RS_REAL a_ = (!IEEE && j == 1) ? c.logUstar : c.logUstar + x.PSIM;
  Stab = (stab_num * x.BLCond * v.dT) * ((a_ * a_ * a_) * v.kinv);
#else
  Stab = rs_dvb<IEEE>(stab_num * x.BLCond * v.dT, v.den0 * (UStar * UStar * UStar));
#endif
  return (j >= 5) && (rs_fabs(x.BLCond - BLCond_Old) < ConvLim);
}

template <bool IEEE = false>
__device__ __forceinline__ void bl_arm(const MathTab &mt, RS_REAL Stab, BlVar &x, bool *unstable = nullptr) {
  /* The clamp `if (Stab > 1) Stab = 1` (:80) only ever acts on a Stab that takes the stable arm: Stab > 1 is
   * Stab > 0, and a NaN fails both tests and goes on unclamped, as it must - the guard of boundary_layer() lives
   * on it.  RS_STAB_UPPER is that clamp inside the arm (rs_physics.hpp: one v_min_f64 instead of a compare, a
   * literal and two selects in every pass); a flavour without it clamps in front, as the reference writes it. */
#ifndef RS_STAB_UPPER
  if (Stab > 1) Stab = 1;
#endif
  if (Stab > 0) {
#ifdef RS_STAB_UPPER
    x.PSIH = R4(4.7) * RS_STAB_UPPER(Stab);
#else
    x.PSIH = R4(4.7) * Stab;
#endif
    x.PSIM = x.PSIH;
  } else {
    x.PSIH = R4(-2.0) * rs_log(mt, (R4(1.0) + rs_sq<IEEE>(R4(1.0) - R4(16.0) * Stab)) / R4(2.0));
    x.PSIM = R4(0.6) * x.PSIH;
    if (unstable) *unstable = true;
  }
}

template <bool IEEE = false>
__device__ __forceinline__ bool bl_iteration(const RS_CONSTS &c, const MathTab &mt,
                                             const BlInv &v, BlVar &x, int j, RS_REAL stab_num,
                                             bool *unstable = nullptr) {
  RS_REAL Stab;
  const bool done = bl_pass<IEEE>(c, v, x, j, stab_num, Stab);
  bl_arm<IEEE>(mt, Stab, x, unstable);
  return done;
}

#ifdef RS_DRY_TAIL
/* DRY TAIL.  CalcLE ends with `if (le > 0 .and. wat <= 0) then le = 0; evap = 0` (src/BoundaryLayer.f90:186-189): a
 * dry surface that would evaporate does not.  A wavefront in which that rule fires in every point - most of the
 * bench workload's: the bare-road shortcut of road_condition needs evap == 0 in all 64 - skips what the rule throws
 * away: calcRaero's division and clamp, le's and evap's divisions, the latent-heat select and the water density.
 *
 * dry_tail_le says, from signs and classes alone (every test is false on a NaN), that the reference's le comes out
 * of its division positive, so that the rule fires and leaves le = +0.0, evap = +0.0.  With
 *   N = AirVCap*(ESurf - EAir)   positive and NORMAL  (>= 2^-1022, finite)
 *   raNum = (logMom + PSIM)*(logHeat + PSIH) > 0      (+inf allowed)
 *   raDen = VK^2*VZ              positive and finite
 *   0 < PsychC < 1
 * the IEEE quotient raNum/raDen is in [+0, +inf] and not a NaN (neither 0/0 nor inf/inf can occur), the clamp leaves
 * RAero in [+0, 30], D = PsychC*RAero is in [+0, 30) and le = N/D is +inf for D = 0 and at least 2^-1022/30 > 2^-1074
 * otherwise: positive, never an underflowed +0 (which the rule would leave alone, with evap = +0/(lat*WatDen) at the
 * mercy of lat and WatDen).  `le > 0` holds, `wat <= 0` is tested as the reference tests it, both results are +0.0
 * whatever lat, WatDen and DTSecs are.  The bare sequence's NaN where IEEE gives +inf or 0 (the GUARD below) needs no
 * thought here: the guard's redo is the IEEE evaluation this argument is about, and ends in the same two zeros.
 *
 * dry_tail_warm says the same without ESurf, for a surface warmer than the air:
 *   -100 < tair,  tair + 0.01 <= tsurf < 100,  EAir not a NaN  (and the tests on wat, raNum, raDen above).
 * Both Magnus curves rise with T above -237.3 and -265.5 degrees, the one over ice lies below the one over water for
 * T < 0 and meets it at 0, and d ln E / dT = a*b/(T + b)^2 is at least 0.036 / K below 100 degrees: the exact
 * ESurf(tsurf) exceeds the exact saturation pressure at tair by 3.6e-4 of itself.  The computed values carry a few
 * ulp each (as*T and T + bs rounded, a correctly rounded quotient of magnitude < 20, rs_exp within an ulp of exp, one
 * product): below 1e-14 relative, ten orders under the gap.  hum <= 1 after its clamp and rounding is monotone, so
 * the computed EAir = hum*ESat <= ESat < ESurf (a negative hum makes EAir <= 0 < ESurf, -inf included).  On that
 * range of tair, AirDens is in (0.9, 2.1), AirHCap in [1005, 1010], PsychC in (0.058, 0.071) and ESurf - EAir >=
 * 3.6e-4 * 1e-6, so N is normal or +inf (EAir = -inf) and le = N/D positive or +inf as above: zeroed.  (With the
 * humidity's limit taken as the reference's MIN takes it - a NaN reads 1.0, forcing_prep_tail - EAir cannot be a
 * NaN on that range of tair; the test stands so that the argument does not lean on it.)
 *
 * THE LAST PASS (RS_BL_LAST, model_step_fluxes_prepped).  The stability correction at the end of the loop's exit pass
 * (:83-89) is read once, by calcRaero, whose RAero feeds only le: where the rule fires it is computed for the sign of
 * raNum alone.  The loop therefore carries Stab, a pass j >= 2 begins with bl_arm on the Stab of pass j-1 - the same
 * operations on the same operands in the same order for every lane, minus the arm of its exit pass - and every test
 * above that does not read raNum is made BEFORE the loop (dry_tail_dry, dry_tail_warm_t, and ESurf, N and PsychC where
 * some lane is not warm).  Behind the loop the sign of raNum is PROVEN from Stab, no longer computed:
 *   Stab > 0:  PSIH = PSIM = 4.7*min(Stab, 1) in (0, 4.7]; both factors are at least their logarithms.
 *   stabSafe < Stab <= 0 (-0 included):  the exact PSIH(Stab) = -2 ln((1 + sqrt(1 - 16 Stab))/2) falls with -Stab and
 *     equals -min(logHeat/2, logMom/1.2) at stabSafe (rs_consts_dev.h), so logHeat + PSIH >= logHeat/2 and logMom +
 *     0.6 PSIH >= logMom/2 exactly; rs_sq and rs_log are within a few ulp, and the half that is left is 1e15 ulp.
 * stabSafe exists only for logMom, logHeat positive and finite (a NaN otherwise: the compare fails in every lane), so
 * both computed factors are positive and finite and their product is positive (at worst +inf, which dry_tail_signs
 * allows) - what `raNum > 0` asked.  A NaN Stab compares false.  Everything else rests on what stood above: a lane's
 * proof is its own, stage 1's or stage 2's, so a wavefront of both kinds skips too.  Where a lane is alive or its Stab
 * is at or below stabSafe, the arm runs for the wavefront and the tail follows as the reference writes it, rule and
 * all, with no second skip.  The GUARD sees le = +0.0 in a skipped wavefront and the blcond it always saw; a bare
 * sequence's NaN in the final Stab fails the compare and arrives in le through the arm as before.
 *
 * EAIR ON DEMAND (RS_EAIR_SURFACE).  Stage 2's `EAir == EAir` is a statement about EAir's inputs: with -100 < tair <
 * 100 (tair < tsurf < 100) the Magnus quotient is below 20 in magnitude and ESat is positive and finite;
 * rs_min_num_one returns 1.0 for a NaN and never a NaN; so EAir = hum*ESat is a number or -inf (hum = -inf), the case
 * the argument above covers - never a NaN.  The surface wave forms EAir from the mailed tair and rhz, by
 * air_vapour_pressure as forcing_prep_tail did, only in a wavefront that needs it. */
__device__ __forceinline__ bool dry_tail_dry(RS_REAL wat, RS_REAL raDen) {
  return (wat <= R4(0.0)) && rs_is_pos_finite(raDen);
}
__device__ __forceinline__ bool dry_tail_warm_t(RS_REAL tsurf, RS_REAL tair) {
  return (tair > R4(-100.0)) && (tsurf < R4(100.0)) && (tsurf >= tair + R4(0.01));
}
__device__ __forceinline__ bool dry_tail_psychc(RS_REAL PsychC) { return (PsychC > R4(0.0)) && (PsychC < R4(1.0)); }
__device__ __forceinline__ bool dry_tail_signs(RS_REAL wat, RS_REAL raNum, RS_REAL raDen) {
  return (wat <= R4(0.0)) && (raNum > R4(0.0)) && rs_is_pos_finite(raDen);
}
__device__ __forceinline__ bool dry_tail_le(bool signs, RS_REAL N, RS_REAL PsychC) {
  return signs && rs_is_pos_normal(N) && (PsychC > R4(0.0)) && (PsychC < R4(1.0));
}
__device__ __forceinline__ bool dry_tail_warm(bool signs, RS_REAL tsurf, RS_REAL tair, RS_REAL EAir) {
  return signs && (tair > R4(-100.0)) && (tsurf < R4(100.0)) && (tsurf >= tair + R4(0.01)) && (EAir == EAir);
}
#ifdef RS_BL_STATS
/* [49] wave-steps in which dry_tail_le holds in every active lane, [50] lane-steps in which it holds; [51], [52] the
 * same for dry_tail_warm ([0], [1] are the totals) */
__device__ __forceinline__ void dry_tail_count(bool le_dry, bool warm) {
  const unsigned long long act = __builtin_amdgcn_ballot_w64(true), m1 = __builtin_amdgcn_ballot_w64(le_dry),
                           m2 = __builtin_amdgcn_ballot_w64(warm);
  if ((unsigned long long)__builtin_ctzll(act) == (unsigned long long)(threadIdx.x & 63u)) {
    if (m1 == act) atomicAdd(&rs::g_bl_stats[49], 1ull);
    atomicAdd(&rs::g_bl_stats[50], (unsigned long long)__builtin_popcountll(m1));
    if (m2 == act) atomicAdd(&rs::g_bl_stats[51], 1ull);
    atomicAdd(&rs::g_bl_stats[52], (unsigned long long)__builtin_popcountll(m2));
  }
}
#endif
#endif

template <bool IEEE = false>
__device__ __forceinline__ void bl_finish(const RS_CONSTS &c, const MathTab &mt, const BlAux &a,
                                          const BlVar &x, RS_REAL tsurf, RS_REAL tair, RS_REAL vz,
                                          RS_REAL rhz, RS_REAL wat, RS_REAL &le, RS_REAL &evap) {
#ifdef RS_DRY_TAIL
  /* the text below in the order the skips need: what the tests read first, what they skip last */
  const RS_REAL raNum = (c.logMom + x.PSIM) * (c.logHeat + x.PSIH), raDen = c.VK_Const * c.VK_Const * vz;
  const bool signs = dry_tail_signs(wat, raNum, raDen); /* (IEEE: the guard's redo runs the whole text) */
#if defined(RS_DRY_ESURF) && defined(RS_EAIR_SURFACE) /* (EAIR ON DEMAND: the air's vapour pressure behind the test) */
  if (!IEEE && rs_wave_all(signs && dry_tail_warm_t(tsurf, tair))) {
    le = R4(0.0);
    evap = R4(0.0);
    return;
  }
#endif
  const RS_REAL aa = (tair < 0) ? R4(21.875) : R4(17.269);
  const RS_REAL ba = (tair < 0) ? R4(265.5) : R4(237.3);
  const RS_REAL ESat = R4(0.61078) * rs_exp(mt, rs_dv<IEEE>(aa * tair, tair + ba));
  const RS_REAL EAir = rs_min_num_one(R4(0.01) * rhz) * ESat; /* (Min's NaN rule: forcing_prep_tail) */
#if defined(RS_DRY_ESURF) && !defined(RS_EAIR_SURFACE)
  if (!IEEE && rs_wave_all(dry_tail_warm(signs, tsurf, tair, EAir))) {
    le = R4(0.0);
    evap = R4(0.0);
    return;
  }
#endif
  const RS_REAL as = (tsurf < 0) ? R4(21.875) : R4(17.269);
  const RS_REAL bs = (tsurf < 0) ? R4(265.5) : R4(237.3);
  const RS_REAL ESurf = R4(0.61078) * rs_exp(mt, rs_dv<IEEE>(as * tsurf, tsurf + bs));
  const RS_REAL N = a.AirDens * a.AirHCap * (ESurf - EAir);
  if (!IEEE && rs_wave_all(dry_tail_le(signs, N, a.PsychC))) {
    le = R4(0.0);
    evap = R4(0.0);
    return;
  }
  if (!IEEE) asm volatile(""); /* keeps the skip a branch, as in layer_vsh */
  RS_REAL RAero = rs_dvb<IEEE>(raNum, raDen);
  if (RAero > R4(30.0)) RAero = R4(30.);
  le = rs_dvb<IEEE>(N, a.PsychC * RAero);
#else /* the flavours without the skip (fp32, -DRS_NO_DRY_TAIL_SKIP): the statements in the order they had, which the
         compiler's schedule follows - the fp32 kernels stay the machine code they were */
  RS_REAL RAero = rs_dvb<IEEE>((c.logMom + x.PSIM) * (c.logHeat + x.PSIH), c.VK_Const * c.VK_Const * vz);
  if (RAero > R4(30.0)) RAero = R4(30.);

  /* Magnus formula over ice (T < 0) or water: one exp per temperature, the
   * coefficients are selected instead of the whole expression being branched */
  const RS_REAL as = (tsurf < 0) ? R4(21.875) : R4(17.269);
  const RS_REAL bs = (tsurf < 0) ? R4(265.5) : R4(237.3);
  const RS_REAL ESurf = R4(0.61078) * rs_exp(mt, rs_dv<IEEE>(as * tsurf, tsurf + bs));
  const RS_REAL aa = (tair < 0) ? R4(21.875) : R4(17.269);
  const RS_REAL ba = (tair < 0) ? R4(265.5) : R4(237.3);
  const RS_REAL ESat = R4(0.61078) * rs_exp(mt, rs_dv<IEEE>(aa * tair, tair + ba));
  RS_REAL hum = R4(0.01) * rhz;
  if (hum > R4(1.0)) hum = R4(1.0);
  const RS_REAL EAir = hum * ESat;
  le = rs_dvb<IEEE>(a.AirDens * a.AirHCap * (ESurf - EAir), a.PsychC * RAero);
#endif
  /* (both latent heats read as scalars, the lane picks a value: see SetDayDependendVariables) */
  const RS_REAL lvap = c.LVap, lfus = c.LFus;
  const RS_REAL lat = (tsurf >= R4(0.0)) ? lvap : lfus;
  evap = rs_dvb<IEEE>(le, lat * a.WatDen) * R4(1000.0) * c.DTSecs;
  if ((le > R4(0.0)) && (wat <= R4(0.0))) {
    le = R4(0.0);
    evap = R4(0.0);
  }
}

/* TRIPS: also report the scheduling hint of rs_hip_recluster (passes, unstable branch taken) -
 * a few vector instructions per pass that a plan sorted by forecast does not need */
template <bool IEEE, bool TRIPS = true>
__device__ __forceinline__ void boundary_layer_impl(const RS_CONSTS &c, const MathTab &mt,
                                                    RS_REAL tsurf, RS_REAL tair, RS_REAL vz,
                                                    RS_REAL rhz, RS_REAL wat, RS_REAL &blcond,
                                                    RS_REAL &le, RS_REAL &evap, int32_t &trips) {
  BlInv v;
  BlVar x;
  BlAux a;
  bl_setup<IEEE>(c, tsurf, tair, vz, v, x, a);
  const RS_REAL stab_num = bl_stab_num(c);
  int j = 1;
  bool unstable = false;
  for (; j <= RS_BL_MAXIT; ++j)
    if (bl_iteration<IEEE>(c, mt, v, x, j, stab_num, TRIPS ? &unstable : nullptr)) break;
  /* scheduling hint (rs_hip_recluster): passes, +64 if any of them took the log/sqrt branch */
  trips = TRIPS ? j + (unstable ? 64 : 0) : 5;
  blcond = x.BLCond;
  bl_finish<IEEE>(c, mt, a, x, tsurf, tair, vz, rhz, wat, le, evap);
}

#if RS_BL_GUARD
/* the guard's slow path: out of line, arguments and results by value (in registers), so that it
 * costs the hot loop neither registers, nor scratch traffic, nor instruction-cache footprint */
struct BlOut {
  RS_REAL blcond, le, evap;
};
#ifndef RS_GUARD_ATTR
#define RS_GUARD_ATTR __attribute__((noinline))
#endif
__device__ RS_GUARD_ATTR BlOut boundary_layer_ieee(const RS_CONSTS *c, const uint64_t *expT,
                                                   const double *logT, const double *K,
                                                   RS_REAL tsurf, RS_REAL tair, RS_REAL vz,
                                                   RS_REAL rhz, RS_REAL wat) {
  MathTab mt;
  mt.expT = expT;
  mt.logT = logT;
  mt.K = K;
  mt.S = (RS_NS::MathCoef)RS_NS::c_gl_scoef;
  asm volatile("" : "+s"(mt.S));
  BlOut o;
  int32_t trips;
  boundary_layer_impl<true>(*c, mt, tsurf, tair, vz, rhz, wat, o.blcond, o.le, o.evap, trips);
  return o;
}
#endif

/* Outputs: blcond, le (LE_Flux), evap (EvapmmTS).
 *
 * GUARD.  The divisions and the square root above run the bare Newton sequences of rs_math.hpp,
 * which return the IEEE result for finite nonzero operands of moderate exponent but NaN where
 * IEEE division returns +-inf or 0 (x/0, x/inf, inf/x).  Almost every denominator on this path
 * is bounded away from zero by CheckValues and by the parameter domain that plan creation
 * enforces (rs_consts_dev.h) - except the ones of this loop: logUstar + PSIM and logCond + PSIH
 * cancel to zero for a strongly unstable profile (PSIM, PSIH run to about -4 for |Ts - Ta| ~ 100 K
 * in calm air), den0*UStar^3 and VK^2*VZ are zero for VZ = 0 with a zero calm limit, and at the
 * final index (lastValues: no CheckValues) the forcing is unchecked.  The reference then carries
 * on with inf/0 as IEEE defines them (clamps such as `Stab > 1`, `RAero > 30` turn them back into
 * finite numbers).  A NaN of the bare sequence survives every later pass and both clamps, so it
 * shows in BLCond or in LE: such a lane - practically never, and wave-uniformly skipped - is
 * redone with IEEE division and square root, which is exact for every operand. */
template <bool TRIPS = true>
__device__ __forceinline__ void boundary_layer(const RS_CONSTS &c, const MathTab &mt,
                                               RS_REAL tsurf, RS_REAL tair, RS_REAL vz, RS_REAL rhz,
                                               RS_REAL wat, RS_REAL &blcond, RS_REAL &le,
                                               RS_REAL &evap, int32_t &trips) {
  boundary_layer_impl<false, TRIPS>(c, mt, tsurf, tair, vz, rhz, wat, blcond, le, evap, trips);
#if RS_BL_GUARD && !defined(RS_IEEE_DIV) && !defined(RS_DIV_CHECK) && !defined(RS_NO_BL_GUARD) && !defined(RS_BL_FIXUP)
  if (!(rs_fabs(blcond) < __builtin_inf()) || !(rs_fabs(le) < __builtin_inf())) {
    const BlOut o = boundary_layer_ieee(&c, mt.expT, mt.logT, mt.K, tsurf, tair, vz, rhz, wat);
    blcond = o.blcond;
    le = o.le;
    evap = o.evap;
  }
#endif
}

/* Volumetric heat capacity of layer j from its (stale) TmpNw value
 * (src/BalanceModel.f90:215-236). */
/* all_thawed: the caller knows that T >= 0 in every active lane of the wavefront (layer_step's ballot): the
 * select below would pick the polynomials' product everywhere and is skipped - a real branch, three vector
 * instructions shorter per layer (a literal and two selects) */
__device__ __forceinline__ RS_REAL layer_vsh(const RS_CONSTS &c, int j, RS_REAL T, bool all_thawed = false) {
  /* both branches are a dozen flops: evaluate the water polynomials
   * unconditionally and select, so 15 layers cost no branches */
  const RS_REAL tmp2 = T * T;
#ifdef RS_HCW_TABLE
  /* the eight REAL(4) coefficients from the plan's constant block (one wide scalar load for the layer)
   * instead of two scalar moves each (rs_consts_dev.h) */
  const RS_REAL RooW = c.hcw[0] * tmp2 + c.hcw[1] * T + c.hcw[2];
  const RS_REAL CW = c.hcw[3] * tmp2 * tmp2 - c.hcw[4] * tmp2 * T + c.hcw[5] * tmp2 - c.hcw[6] * T + c.hcw[7];
#else
  const RS_REAL RooW = R4(-0.0050) * tmp2 + R4(0.0079) * T + R4(1000.0028);
  const RS_REAL CW = R4(0.0000102) * tmp2 * tmp2 - R4(0.0017169) * tmp2 * T +
                    R4(0.11516) * tmp2 - R4(3.4739) * T + R4(4217.2);
#endif
  /* one select of the product instead of one per factor: 920 * 2100 is exact */
  RS_REAL CHWT = RooW * CW;
  if (!all_thawed) {
#ifdef RS_FROZEN_TABLE /* (the callers that ballot) */
    /* Keeps the arm a branch: left to itself the optimiser turns it back into the two selects it replaces.
     * Nothing in the language promises that; `tools/asm_attrib.py file.s kernel --check-thawed-skip` fails where
     * a compiler no longer branches round the select (the attribution workflow of profiles/r07_valu_attribution.txt
     * runs it). */
    asm volatile("");
#endif
    CHWT = (T >= 0) ? CHWT : R4(920.0) * R4(2100.0);
  }
  return RS_LK(c, j, dryCap) + RS_LK(c, j, WCont) * CHWT;
}

/* src/Storage.f90:319-402.  Writes T(1), T(2) (the new profile) and q2melt.
 * The TsurfAve assignment at :389-394 is overwritten unconditionally at
 * src/BalanceModel.f90:78-84 and is dropped. */
template <class Prof>
__device__ __forceinline__ void melting(Scalars &s, Prof &T, RS_REAL hstor, RS_REAL hs1,
                                        bool in_coupling_phase, RS_REAL last_tsurf_obs) {
  if ((s.snow > R4(0.0)) || (s.ice > R4(0.0)) || (s.ice2 > R4(0.0))) {
    if ((hstor <= R4(0.00001)) || (s.tsurf <= s.t4melt) || (s.q2melt <= 0) ||
        (in_coupling_phase && last_tsurf_obs < s.t4melt)) {
      if (s.tsurf < R4(0.5)) {
        s.q2melt = R4(0.0);
        return;
      } else if (s.tsurf > R4(2.0)) {
        const RS_REAL QAvail = hs1 * (T.get(1) - s.t4melt);
        if (QAvail < s.q2melt) s.q2melt = QAvail;
        return;
      }
    }
    const RS_REAL QAvail = hs1 * (T.get(1) - s.t4melt);
    if (s.q2melt >= QAvail) {
      s.q2melt = QAvail;
      T.set(1, s.t4melt + R4(0.01));
      T.set(2, s.t4melt + R4(0.01));
    } else {
      const RS_REAL QLeftOver = QAvail - s.q2melt;
      T.set(1, s.t4melt + rs_div(QLeftOver, hs1));
      T.set(2, s.t4melt + R4(0.01));
    }
  } else {
    s.q2melt = R4(0.0);
  }
}

/* src/Cond.f90:69-103 + src/Cond.f90:9-65 + src/Storage.f90:33-314,409-432 +
 * src/Cond.f90:105-139: wear factors, the four storages, melt heat for the next
 * step, albedo for the next step. */
__device__ __forceinline__ void road_condition(const RS_CONSTS &c, Scalars &s, RS_REAL evap, bool real = false) {
#ifdef RS_EXP_SURFACE_LIGHT /* (experiment build, tools/experiments/r6_surface_light.sh - wrong physics: an upper bound of
                               what taking this block off the surface wavefront's chain can buy a small shard;
                               `real`: -DRS_EXP_SURFACE_MOVED's stand-in work on the ground wavefront) */
  if (!real) {
    if (s.verycold && (s.tsurf > c.TLimColdH)) s.verycold = false;
    s.albedo = c.AlbDry;
    return;
  }
#endif
  /* A wavefront whose roads are all bare and dry (78 % of the point-steps of the BASELINE workload;
   * the plan order keeps such points together): with the five storages +0.0 and no evaporation or
   * condensation every branch below either is not taken or stores the +0.0 it found - WaterStorage
   * 0 - f*(+-0) = +0, nothing to wear, melt or freeze, the clamps leave 0 alone as long as the
   * upper limits are not negative (RS_BARE_FAST: checked once per plan) - Q2Melt = 0, T4Melt as it
   * was, albedo of the dry road.  What is left is the VeryCold hysteresis (src/Cond.f90:34-39). */
  {
    const bool bare = rs_is_pos_zero(s.wat) && rs_is_pos_zero(s.snow) && rs_is_pos_zero(s.ice) &&
                      rs_is_pos_zero(s.ice2) && rs_is_pos_zero(s.dep) && evap == R4(0.0);
#ifdef RS_BL_STATS
    {
      const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
      const bool nosnow = rs_is_pos_zero(s.snow), noice = rs_is_pos_zero(s.ice) && rs_is_pos_zero(s.ice2);
      const bool nodep = rs_is_pos_zero(s.dep) && !(evap < R4(0.0)), nowat = rs_is_pos_zero(s.wat);
      const bool u11 = __builtin_amdgcn_ballot_w64(bare) == act, u12 = __builtin_amdgcn_ballot_w64(nosnow) == act,
                 u13 = __builtin_amdgcn_ballot_w64(noice) == act, u14 = __builtin_amdgcn_ballot_w64(nodep) == act,
                 u15 = __builtin_amdgcn_ballot_w64(nowat) == act,
                 u16 = __builtin_amdgcn_ballot_w64(nosnow && noice && nodep) == act;
      if ((unsigned long long)__builtin_ctzll(act) == (unsigned long long)(threadIdx.x & 63u)) {
        atomicAdd(&rs::g_bl_stats[10], 1ull);
        if (u11) atomicAdd(&rs::g_bl_stats[11], 1ull);
        if (u12) atomicAdd(&rs::g_bl_stats[12], 1ull);
        if (u13) atomicAdd(&rs::g_bl_stats[13], 1ull);
        if (u14) atomicAdd(&rs::g_bl_stats[14], 1ull);
        if (u15) atomicAdd(&rs::g_bl_stats[15], 1ull);
        if (u16) atomicAdd(&rs::g_bl_stats[16], 1ull);
      }
    }
#endif
    if (RS_BARE_FAST(c) && rs_wave_all(bare)) {
      if (s.verycold && (s.tsurf > c.TLimColdH)) s.verycold = false;
      if (!s.verycold && (s.tsurf < c.TLimColdL)) s.verycold = true;
      s.q2melt = R4(0.0);
      s.albedo = c.AlbDry;
      return;
    }
  }
  /* A wavefront none of whose roads has snow (the plan order keeps the storage classes together; on the bench
   * workload the roads that are not bare mostly carry frost): with Snowmms = +0.0 every statement of
   * SnowStorage either tests Snowmms > 0 or leaves +0.0 as it is (Snowmms < MinSnowmms stores the +0.0 it found,
   * Snowmms > MaxSnowmms needs a negative limit: RS_BARE_FAST) and nobody reads SnowTran, WatSnowRat or the
   * wet-snow flag - the block is skipped, exactly.  Likewise IceStorage below. */
#ifdef RS_NO_STORAGE_SKIP /* (A/B build) */
  const bool snow_here = true;
#else
  const bool snow_here = !(RS_BARE_FAST(c) && rs_wave_all(rs_is_pos_zero(s.snow)));
#endif
  /* WearFactors */
  RS_REAL SnowTran = R4(0.0);
  if (snow_here) {
    SnowTran = c.wSnowTran * s.snow;
    SnowTran = (SnowTran > R4(0.01)) ? SnowTran : R4(0.01);
    if (s.snow < R4(0.2)) SnowTran = SnowTran * 3;
    SnowTran = SnowTran * c.Tph;
  }
  RS_REAL IceWear = c.wIce * s.ice;
  IceWear = (IceWear > R4(0.01)) ? IceWear : R4(0.01);
  IceWear = IceWear * c.Tph;
  RS_REAL IceWear2 = c.wIce2 * s.ice2;
  IceWear2 = (IceWear2 > R4(0.01)) ? IceWear2 : R4(0.01);
  IceWear2 = IceWear2 * c.Tph;
  RS_REAL DepWear = c.wDep * s.dep;
  DepWear = (DepWear > R4(0.01)) ? DepWear : R4(0.01);
  DepWear = DepWear * c.Tph;
  RS_REAL WatWear = c.wWat * s.wat;
  WatWear = (WatWear > R4(0.06)) ? WatWear : R4(0.06);
  WatWear = 10 * WatWear * c.Tph;

  /* RoadCond head: hysteresis (:34-39); SnowType reset to dry (:32) */
  bool wet = false;
  if (s.verycold && (s.tsurf > c.TLimColdH)) s.verycold = false;
  if (!s.verycold && (s.tsurf < c.TLimColdL)) s.verycold = true;

  /* WaterStorage, src/Storage.f90:33-84 */
  if ((s.snow <= R4(0.0)) && (s.ice <= R4(0.0)) && (s.dep <= R4(0.0)) && (s.tsurf > c.TLimDew)) {
    if (s.wat > c.MaxPormms)
      s.wat = s.wat - evap;
    else
      s.wat = s.wat - c.PorEvaF * evap;
  }
  if (s.wat > R4(0.0)) {
    if (s.wat < c.WWearLim) WatWear = R4(0.0);
    if (s.wat > c.WWetLim)
      s.wat = s.wat - WatWear;
    else
      s.wat = s.wat - c.DampWearF * WatWear;
  }
  if (s.wat < c.MinWatmms) s.wat = R4(0.0);
  if (s.wat > c.MaxWatmms) s.wat = c.MaxWatmms;
  RS_REAL ext = s.wat - c.MaxPormms;
  ext = (ext > R4(0.)) ? ext : R4(0.);

  /* SnowStorage, src/Storage.f90:88-196 */
  if (snow_here) {
    RS_REAL WatSnowRat;
    const RS_REAL RDummy = ext + s.snow;
    if (RDummy > R4(0.001))
      WatSnowRat = rs_div(ext, RDummy);
    else
      WatSnowRat = R4(0.0);
    if (s.snow > R4(0.0)) {
      if (WatSnowRat > c.WetSnowFormR) wet = true;
      if (s.dep > R4(0.0)) {
        s.ice = s.ice + s.dep;
        s.dep = R4(0.0);
      }
      if ((s.q2melt > R4(0.0)) && (s.tsurf >= c.TLimMeltSnow)) {
        const RS_REAL Melted = RS_DIVC(s.q2melt * c.DTSecs, RS_MELTDEN, r_meltDen);
        s.snow = s.snow - R4(1000.) * Melted;
        s.wat = s.wat + R4(1000.) * Melted;
      }
    }
    if (s.snow > R4(0.0)) {
      s.snow = s.snow - SnowTran;
      s.ice = s.ice + c.wSnow2Ice * SnowTran;
      s.ice2 = s.ice2 + c.wSnow2Ice * SnowTran;
    }
    if ((s.snow > R4(0.0)) && wet) {
      if (WatSnowRat > c.WetSnowMeltR) {
        s.wat = s.wat + s.snow;
        s.snow = R4(0.0);
      }
      if (s.tsurf < c.TLimFreeze) {
        s.ice = s.ice + s.snow + s.wat;
        s.ice2 = s.ice2 + s.snow + s.wat;
        s.snow = R4(0.0);
        s.wat = R4(0.0);
      }
    }
    if (s.snow < c.MinSnowmms) s.snow = R4(0.0);
    if (s.snow > c.MaxSnowmms) s.snow = s.snow - (c.MaxSnowmms / R4(2.));
  }

  /* IceStorage, src/Storage.f90:199-267.  Skipped for a wavefront in which no road has ice of either kind NOW
   * (SnowStorage may just have made some) and no water is about to freeze: every statement then tests a
   * storage > 0, or stores the +0.0 it found, or needs a negative upper limit. */
  const bool freezes = s.tsurf < c.TLimFreeze && s.wat > R4(0.0);
#ifdef RS_NO_STORAGE_SKIP
  const bool ice_here = true;
#else
  const bool ice_here = !(RS_BARE_FAST(c) && rs_wave_all(rs_is_pos_zero(s.ice) && rs_is_pos_zero(s.ice2) && !freezes));
#endif
  if (ice_here) {
    if (freezes) {
      s.ice = s.ice + s.wat;
      s.ice2 = s.ice2 + s.wat;
      s.wat = R4(0.0);
    }
    if ((s.snow <= R4(0.)) && (s.ice > R4(0.))) {
      if ((s.q2melt > R4(0.0)) && (s.tsurf >= c.TLimMeltIce)) {
        const RS_REAL Melted = RS_DIVC(s.q2melt * c.DTSecs, RS_MELTDEN, r_meltDen);
        s.ice = s.ice - R4(1000.) * Melted;
        s.ice2 = s.ice2 - R4(1000.) * Melted;
        s.wat = s.wat + R4(1000.) * Melted;
      }
    }
    if (s.ice > R4(0.)) s.ice = s.ice - IceWear;
    if (s.ice2 > R4(0.)) s.ice2 = s.ice2 - IceWear2;
    if (s.ice < c.MinIcemms) s.ice = R4(0.0);
    if (s.ice > c.MaxIcemms) s.ice = c.MaxIcemms;
    if (s.ice2 < c.MinIcemms) s.ice2 = R4(0.0);
    if (s.ice2 > c.MaxIcemms) s.ice2 = c.MaxIcemms;
  }

  /* DepositStorage, src/Storage.f90:271-314 */
  if (evap < R4(0.0)) s.dep = s.dep - evap;
  if (s.tsurf > c.TLimMeltDep) {
    s.wat = s.wat + s.dep;
    s.dep = R4(0.0);
  }
  if ((s.snow <= R4(0.0)) && (s.dep > 0)) s.dep = s.dep - DepWear;
  if (s.dep < c.MinDepmms) s.dep = R4(0.0);
  if (s.dep > c.MaxDepmms) {
    s.wat = s.wat + (s.dep - c.MaxDepmms);
    s.dep = c.MaxDepmms;
  }

  /* RoadCond tail, src/Cond.f90:61-62 */
  if (s.wat < c.MinWatmms) s.wat = R4(0.0);
  if (s.wat > c.MaxWatmms) s.wat = c.MaxWatmms;

  /* A wavefront that skipped both blocks has Snowmms = Icemms = Icemms2 = +0.0 in every lane still: no melt heat
   * (Q2Melt = 0, T4Melt as it was), and CalcAlbedo's IceSum = 0.5 (0 + 0) + Depositmms is the deposit itself. */
  if (!snow_here && !ice_here) {
    s.q2melt = R4(0.0);
    const RS_REAL IceMax = R4(1.5);
    RS_REAL alb = c.AlbDry;
    if (s.dep > R4(0.01)) {
      if (s.dep < IceMax)
        alb = c.AlbDry + RS_DIVC(s.dep, IceMax, r_IceMax) * (c.AlbSnow - c.AlbDry);
      else
        alb = c.AlbSnow;
    }
    s.albedo = alb;
    return;
  }
  /* NewMeltFreezeHeat, src/Storage.f90:409-432 */
  s.q2melt = R4(0.0);
  if (s.snow > R4(0.0)) {
    s.q2melt = RS_DIVC(RS_MELTDEN * RS_DIVC(s.snow, R4(1000.), r_1000), c.DTSecs, r_DTSecs);
    s.t4melt = c.TLimMeltSnow;
  }
  if ((s.snow <= R4(0.0)) && (s.ice > R4(0.0))) {
    s.q2melt = RS_DIVC(RS_MELTDEN * RS_DIVC(s.ice, R4(1000.), r_1000), c.DTSecs, r_DTSecs);
    s.t4melt = c.TLimMeltIce;
  }
  if (s.q2melt < R4(0.0)) s.q2melt = R4(0.0);

  /* CalcAlbedo, src/Cond.f90:105-139 */
  {
    RS_REAL IceSum = R4(0.5) * (s.ice + s.ice2) + s.dep;
    const RS_REAL IceMax = R4(1.5);
    if (IceSum < R4(0.0)) IceSum = R4(0.0);
    RS_REAL alb = c.AlbDry;
    if (s.snow > R4(0.01) && s.snow > s.ice) {
      alb = c.AlbSnow;
    } else if (s.ice > R4(0.01) || s.dep > R4(0.01)) {
      if (IceSum < IceMax)
        alb = c.AlbDry + RS_DIVC(IceSum, IceMax, r_IceMax) * (c.AlbSnow - c.AlbDry);
      else
        alb = c.AlbSnow;
    }
    s.albedo = alb;
  }
}

/* roadModelOneStep (examples/example1/src/Simulation.f90:120-172) with
 * BalanceModelOneStep (src/BalanceModel.f90:7-86) inlined, in two halves so that
 * the caller can issue the next time index's forcing loads between them.
 * On entry: tair/vz/rhz/prec_ts are the current atm values (after
 * SetCurrentValues / relaxation / lastValues), T is Tmp(1..N) possibly with obs
 * forcing applied, s.tsurf is up to date. */
struct Fluxes {
  RS_REAL blcond, le, evap, rnet, trffric;
  int32_t trips; /* passes of the boundary-layer loop (+64: the unstable branch was taken):
                    a scheduling hint, not model state */
};

/* What the coupling machinery feeds into a step (src/BalanceModel.f90:44-45,71-73);
 * off the coupling path: coefficients 1.0, not in a coupling phase. */
struct CouplingInputs {
  RS_REAL sw_cof = 1.0, lw_cof = 1.0, last_tsurf_obs = 0.0;
  bool in_phase = false;
};

/* first half: precipitation -> storages, day/night, boundary layer, net radiation.
 * fluxes_pre / fluxes_post are the parts before and after the boundary-layer loop. */
__device__ __forceinline__ void fluxes_pre(const RS_CONSTS &c, const MathTab &mt, Scalars &s,
                                           RS_REAL tair, RS_REAL &vz, RS_REAL rhz, RS_REAL prec_ts,
                                           int32_t phase, int32_t hour, Fluxes &fx) {
  /* A wavefront without precipitation at this index (the plan order keeps the dry, bare roads
   * together): prec = +-0 gives PrecInTStep = +-0 <= MinPrecmm, so both branches of CalcPrecType set
   * Rain = Snow = 0 and the storages get + 0.0 (src/Cond.f90:187-188,222-223, src/Storage.f90:24-27) -
   * nothing changes as long as MinPrecmm is not negative (RS_PREC_FAST: checked once per plan). */
  if (!(RS_PREC_FAST(c) && rs_wave_all(prec_ts == R4(0.0))))
    precipitation_to_storage(c, mt, s, phase, prec_ts, tair, rhz);

  /* SetDayDependendVariables, src/BalanceModel.f90:354-387 */
  /* all four constants are read first (scalar loads) and the lane then picks VALUES; written as
   * an if/else over the loads, the compiler merges the arms into one load from a per-lane address
   * of the constants block: a vector memory round trip in the middle of the step */
  const RS_REAL calmN = c.CalmLimNgt, calmD = c.CalmLimDay, fricN = c.TrfFricNgt,
                fricD = c.TrFfricDay;
  const bool night = ((RS_REAL)hour >= c.NightOn) || ((RS_REAL)hour <= c.NightOff);
  const RS_REAL calm = night ? calmN : calmD;
  fx.trffric = night ? fricN : fricD;
  if (vz < calm) vz = calm;
}

__device__ __forceinline__ void fluxes_post(const RS_CONSTS &c, const Scalars &s, RS_REAL sw,
                                            RS_REAL lw, const CouplingInputs &cp, Fluxes &fx) {
  /* CalcRNet, src/BalanceModel.f90:282-307 (SwRadCof = LwRadCof = 1.0 off the
   * coupling path; x*1.0 is exact, so the compiler drops the factors there) */
  const RS_REAL TsurfK = s.tsurf + R4(273.15);
  const RS_REAL TsurfK2 = TsurfK * TsurfK;
  const RS_REAL RBB = c.Emiss * c.SB_Const * (TsurfK2 * TsurfK2);
  fx.rnet = (R4(1.) - s.albedo) * sw * cp.sw_cof + c.Emiss * lw * cp.lw_cof - RBB;
}

template <bool TRIPS = true>
__device__ __forceinline__ Fluxes model_step_fluxes(const RS_CONSTS &c, const MathTab &mt,
                                                    Scalars &s, RS_REAL tair, RS_REAL vz, RS_REAL rhz,
                                                    RS_REAL prec_ts, RS_REAL sw, RS_REAL lw,
                                                    int32_t phase, int32_t hour,
                                                    const CouplingInputs &cp = CouplingInputs()) {
  Fluxes fx;
  fluxes_pre(c, mt, s, tair, vz, rhz, prec_ts, phase, hour, fx);
  boundary_layer<TRIPS>(c, mt, s.tsurf, tair, vz, rhz, s.wat, fx.blcond, fx.le, fx.evap, fx.trips);
  fluxes_post(c, s, sw, lw, cp, fx);
  return fx;
}

/* ---- the part of a time step that depends on the forcing alone --------------------------------------
 * (two wavefronts per 64 points, rs_kernels.hip step_kernel_duo: the ground wave works it out one index
 * AHEAD and hands it over through LDS, so that the surface wave's chain starts at the surface state.)
 * Every value is formed by the expression, in the operand order, that the one-wave path uses:
 * SetCurrentValues' VZ(1) floor, the precipitation per step (src/InputOutput.f90:111,186), CheckValues'
 * forcing tests (:45-84), CalcPrecType (src/Cond.f90:143-249), SetDayDependendVariables
 * (src/BalanceModel.f90:354-387), the air properties and loop invariants of CalcBLCondAndLE
 * (src/BoundaryLayer.f90:50-62,78-79) and the vapour pressure of the air (CalcLE, :160-170). */
struct ForcingPrep {
  RS_REAL tair, vz, rhz; /* vz: after the VZ(1) floor and the calm limit */
  RS_REAL rain, snow;    /* what PrecipitationToStorage adds to the water and snow storages */
  RS_REAL trffric;
  RS_REAL AirDens, AirHCap, PsychC, den0, vkvz, avk;
  RS_REAL AirVCap = 0; /* AirHCap x AirDens: what the two-wavefront mailbox carries of the two (duo_get_prep) */
#ifndef RS_EAIR_SURFACE /* (with it: air_vapour_pressure of tair and rhz, where model_step_fluxes_prepped needs it) */
  RS_REAL EAir;
#endif
  RS_REAL sw, lw;
  bool bad; /* CheckValues' verdict on the forcing (the surface-temperature test is the surface wave's) */
  bool night = false; /* SetDayDependendVariables' branch: which traffic friction and calm limit the index gets */
  bool stop = false;  /* the sky view's sun position left its domain (rs_physics.hpp sky_view_radiation) */
  bool bad_rw = false; /* coupling replays: CheckValues' verdict on the forcing of the index BEHIND the point's
                          coupling window, which the reference's loop has just seen when it rewinds (step_kernel_duo<REPLAY>) */
  RS_REAL tsurfobs = R4(-9999.9); /* FULL: the observation SetCurrentValues forces on Tmp(1:2) at this index, or missing */
  /* What model_step_fluxes_prepped first reads behind the boundary-layer loop (or in a wavefront whose dry tail is
   * alive), through accessors: a caller whose ForcingPrep lies in memory that stays put for the whole step hands
   * over a type that fetches them THERE instead of holding them across the loop (rs_kernels.hip DuoLatePrep). */
  __device__ __forceinline__ RS_REAL rhz_late() const { return rhz; }
  __device__ __forceinline__ RS_REAL vz_late() const { return vz; }
  __device__ __forceinline__ RS_REAL sw_late() const { return sw; }
  __device__ __forceinline__ RS_REAL lw_late() const { return lw; }
};

__device__ __forceinline__ bool check_values_forcing(const RS_CONSTS &c, const Forcing &f) {
  const RS_REAL hi100 = rs_fmax(f.tair, f.vz);
  const RS_REAL lo01 = rs_fmin(rs_fmin(f.rhz, f.sw), rs_fmin(f.lw, f.prec));
  return (hi100 > RS_CHK(c, 0, R4(100.0))) | (lo01 < RS_CHK(c, 1, R4(-0.1))) |
         (f.tair < RS_CHK(c, 2, R4(-90.0))) | (f.rhz > RS_CHK(c, 3, R4(120.0))) |
         (f.vz < RS_CHK(c, 4, R4(-1.0))) | (f.sw > RS_CHK(c, 5, R4(4000.0))) |
         (f.lw > RS_CHK(c, 6, R4(1000.0))) | (f.prec > RS_CHK(c, 7, R4(500.0)));
}

/* ... and CheckValues' test of the surface temperature ("Abnormal surface temperature", :78-82) */
__device__ __forceinline__ bool check_values_tsurf(const RS_CONSTS &c, RS_REAL tsurf) {
  return rs_fabs(tsurf) > RS_CHK(c, 0, R4(100.0));
}

/* First half of the forcing's share of a step: SetCurrentValues' VZ(1) floor and CheckValues' forcing
 * tests.  i: the 1-based time index of the forcing; checked: i < SimLen (CheckValues does not run at the
 * last); has_tdew: the dew-point test of the FULL feature set (:59-62).  Returns VZ after the floor. */
__device__ __forceinline__ RS_REAL forcing_prep_head(const RS_CONSTS &c, const Forcing &f, int32_t i,
                                                     bool checked, bool has_tdew, bool &bad) {
  RS_REAL vz = f.vz;
  if (i == 1 && vz < R4(0.4)) vz = R4(0.4); /* src/Initialization.f90:121-123 */
  bad = false;
  if (checked) {
    Forcing chk = f;
    chk.vz = vz;
    bad = check_values_forcing(c, chk);
    if (has_tdew) bad = bad | (f.tdew < -90) | (f.tdew > R4(100.0));
  }
  return vz;
}

/* CalcLE's vapour pressure of the air (src/BoundaryLayer.f90:160-172), Magnus over ice or water at tair times the
 * limited humidity */
__device__ __forceinline__ RS_REAL air_vapour_pressure(const MathTab &mt, RS_REAL tair, RS_REAL rhz) {
  const RS_REAL aa = (tair < 0) ? R4(21.875) : R4(17.269);
  const RS_REAL ba = (tair < 0) ? R4(265.5) : R4(237.3);
  const RS_REAL ESat = R4(0.61078) * rs_exp(mt, rs_dv<false>(aa * tair, tair + ba));
  /* Min((0.01*Rhz), 1.0), src/BoundaryLayer.f90:172: the compiled reference's MIN returns the other operand where
   * one is a NaN - a NaN humidity (CheckValues lets it through) reads as saturated air - and so does v_min_f64 */
  return rs_min_num_one(R4(0.01) * rhz) * ESat;
}

/* Second half, from the air temperature, wind speed and humidity the step will use (the FULL feature
 * set relaxes them between the two halves, src/Relaxation.f90).  NIGHT_U: the caller hands over the day/night
 * verdict in night_u - the comparison below on the same hour, made once for a run of indices that share the
 * hour (the knot-reading source: one hour for all points, one per knot interval) - and f.hour is not read. */
template <bool NIGHT_U = false>
__device__ __forceinline__ ForcingPrep forcing_prep_tail(const RS_CONSTS &c, const MathTab &mt, const Forcing &f,
                                                         RS_REAL tair, RS_REAL vz, RS_REAL rhz, bool bad,
                                                         bool night_u = false) {
  ForcingPrep q;
  RS_REAL prec_ts = RS_DIVC(f.prec, (RS_REAL)3600.0, r_3600) * c.DTSecs;
  q.bad = bad;
  /* PrecipitationToStorage without the storages: the same function on two zeros */
  {
    Scalars z;
    z.wat = R4(0.0);
    z.snow = R4(0.0);
#ifdef RS_BL_STATS
    {
      const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
      const bool dry = __builtin_amdgcn_ballot_w64(prec_ts == R4(0.0)) == act;
      if ((unsigned long long)__builtin_ctzll(act) == (unsigned long long)(threadIdx.x & 63u)) {
        atomicAdd(&rs::g_bl_stats[17], 1ull);
        if (!dry) atomicAdd(&rs::g_bl_stats[18], 1ull);
      }
    }
#endif
    if (!(RS_PREC_FAST(c) && rs_wave_all(prec_ts == R4(0.0))))
      precipitation_to_storage(c, mt, z, f.phase, prec_ts, tair, rhz);
    q.rain = z.wat; /* 0 + Rain and 0 + Snow are Rain and Snow */
    q.snow = z.snow;
  }
  const RS_REAL calmN = c.CalmLimNgt, calmD = c.CalmLimDay, fricN = c.TrfFricNgt, fricD = c.TrFfricDay;
  const bool night = NIGHT_U ? night_u : ((RS_REAL)f.hour >= c.NightOn) || ((RS_REAL)f.hour <= c.NightOff);
  const RS_REAL calm = night ? calmN : calmD;
  q.trffric = night ? fricN : fricD;
  q.night = night;
  if (vz < calm) vz = calm;
  q.tair = tair;
  q.vz = vz;
  q.rhz = rhz;
  const RS_REAL TaK = tair + R4(273.15);
  q.AirDens = rs_dv<false>(R4(100000.0), R4(287.05) * TaK);
  const RS_REAL dK = (TaK - R4(250.0)) * (TaK - R4(250.0));
  q.AirHCap = R4(1005.0) + RS_DIVC(dK, R4(3364.), r_3364);
  const RS_REAL AirVCap = q.AirHCap * q.AirDens;
  q.PsychC = R4(0.1) * (R4(0.00063) * TaK + R4(0.47496));
  q.den0 = AirVCap * (tair + R4(273.15));
  q.vkvz = c.VK_Const * vz;
  q.avk = AirVCap * c.VK_Const;
#ifndef RS_EAIR_SURFACE
  q.EAir = air_vapour_pressure(mt, tair, rhz);
#endif
  q.sw = f.sw;
  q.lw = f.lw;
  return q;
}

template <bool NIGHT_U = false>
__device__ __forceinline__ ForcingPrep forcing_prep(const RS_CONSTS &c, const MathTab &mt, const Forcing &f,
                                                    int32_t i, bool checked, bool night_u = false) {
  bool bad;
  const RS_REAL vz = forcing_prep_head(c, f, i, checked, false, bad);
  return forcing_prep_tail<NIGHT_U>(c, mt, f, f.tair, vz, f.rhz, bad, night_u);
}

#ifdef RS_BL_STATS
/* the boundary-layer loop's counters (rs_math.hpp g_bl_stats): the step, each pass, the trip counts */
struct BlStatsStep {
  unsigned long long act;
  bool first;
};
__device__ __forceinline__ BlStatsStep bl_stats_step() {
  const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
  const bool first = (unsigned long long)__builtin_ctzll(act) == (unsigned long long)(threadIdx.x & 63u);
  if (first) {
    atomicAdd(&rs::g_bl_stats[0], 1ull);
    atomicAdd(&rs::g_bl_stats[1], (unsigned long long)__builtin_popcountll(act));
  }
  return BlStatsStep{act, first};
}
/* h0: PSIH before the pass; x: after the pass and its arm */
__device__ __forceinline__ void bl_stats_pass(const BlStatsStep &st, int j, RS_REAL h0, const BlVar &x) {
  const unsigned long long act = st.act;
  const bool first = st.first;
  { /* which arms of the pass ran: the stable one, the unstable one with log's polynomial / table path */
    const bool uns = !(x.PSIH > R4(0.0)), far = x.PSIH < R4(-0.1254);
    const unsigned long long mu = __builtin_amdgcn_ballot_w64(uns), mf = __builtin_amdgcn_ballot_w64(far),
                             ma = __builtin_amdgcn_ballot_w64(true);
    if ((unsigned long long)__builtin_ctzll(ma) == (unsigned long long)(threadIdx.x & 63u)) {
      atomicAdd(&rs::g_bl_stats[19], 1ull);
      atomicAdd(&rs::g_bl_stats[48], (unsigned long long)__builtin_popcountll(ma));
      atomicAdd(&rs::g_bl_stats[46], (unsigned long long)__builtin_popcountll(mu));
      atomicAdd(&rs::g_bl_stats[47], (unsigned long long)__builtin_popcountll(mf));
      if (mu) atomicAdd(&rs::g_bl_stats[20], 1ull);
      if (mf && (mu & ~mf)) atomicAdd(&rs::g_bl_stats[21], 1ull);
      if (mu && (ma & ~mu)) atomicAdd(&rs::g_bl_stats[22], 1ull);
      if (mf) atomicAdd(&rs::g_bl_stats[23], 1ull);
    }
  }
  if (j >= 2 && j <= 4) {
    const bool same = __double_as_longlong((double)h0) == __double_as_longlong((double)x.PSIH);
    const unsigned long long ms = __builtin_amdgcn_ballot_w64(same);
    if (first) {
      if (ms == act) atomicAdd(&rs::g_bl_stats[j], 1ull);
      atomicAdd(&rs::g_bl_stats[3 + j], (unsigned long long)__builtin_popcountll(ms));
    }
  }
}
__device__ __forceinline__ void bl_stats_trips(const BlStatsStep &st, int j) {
  const bool first = st.first;
  { /* trip counts: the lane's, and the wavefront's (how many passes it issued) */
    const int trips = j > RS_BL_MAXIT ? RS_BL_MAXIT : j;
    int wmax = trips, wsum = trips;
    for (int o = 32; o > 0; o >>= 1) {
      const int other = __shfl_xor(wmax, o, 64);
      wmax = other > wmax ? other : wmax;
      wsum += __shfl_xor(wsum, o, 64);
    }
    auto bin = [](int t) { return t <= 8 ? t - 5 : t <= 12 ? 4 : t <= 20 ? 5 : t < 40 ? 6 : 7; };
    for (int b = 0; b < 8; ++b) {
      const unsigned long long mb = __builtin_amdgcn_ballot_w64(bin(trips) == b);
      if (first && mb) atomicAdd(&rs::g_bl_stats[32 + b], (unsigned long long)__builtin_popcountll(mb));
    }
    {
      const int nh = __builtin_popcountll(__builtin_amdgcn_ballot_w64(trips > 20));
      if (first && nh > 0) atomicAdd(&rs::g_bl_stats[40 + (nh == 1 ? 0 : nh <= 3 ? 1 : nh <= 7 ? 2 : nh <= 15 ? 3 : nh <= 31 ? 4 : 5)], 1ull);
    }
    if (first) {
      atomicAdd(&rs::g_bl_stats[9], (unsigned long long)wsum);
      atomicAdd(&rs::g_bl_stats[8], (unsigned long long)wmax);
      atomicAdd(&rs::g_bl_stats[24 + bin(wmax)], 1ull);
    }
  }
}
#endif

/* model_step_fluxes from a ForcingPrep: the storages take the precipitation, the boundary-layer loop
 * starts from the handed-over invariants, CalcLE from the handed-over vapour pressure of the air (or, EAIR ON DEMAND,
 * from the handed-over air temperature and humidity). */
/* TRIPS: 0 no scheduling hint, 1 the history score's (passes, +64 where a pass took the unstable branch), 2 the
 * pass count alone (the loop's own counter: nothing per pass) */
#ifdef RS_BL_LAST
/* CalcLE's numerator AirVCap*(ESurf - EAir) (src/BoundaryLayer.f90:160-176); the product AirDens x AirHCap arrives
 * as AirVCap, EAir by the mailbox or from the mailed tair and rhz (EAIR ON DEMAND) */
template <class Q>
__device__ __forceinline__ RS_REAL le_numerator(const MathTab &mt, RS_REAL tsurf, const Q &q) {
  const RS_REAL as = (tsurf < 0) ? R4(21.875) : R4(17.269);
  const RS_REAL bs = (tsurf < 0) ? R4(265.5) : R4(237.3);
  const RS_REAL ESurf = R4(0.61078) * rs_exp(mt, rs_dv<false>(as * tsurf, tsurf + bs));
#ifdef RS_EAIR_SURFACE
  const RS_REAL EAir = air_vapour_pressure(mt, q.tair, q.rhz_late());
#else
  const RS_REAL EAir = q.EAir;
#endif
  return q.AirVCap * (ESurf - EAir);
}
/* forcing_prep_tail's expression on forcing_prep_tail's value: three operations where a wavefront needs them */
__device__ __forceinline__ RS_REAL psychrometric(RS_REAL tair) {
  return R4(0.1) * (R4(0.00063) * (tair + R4(273.15)) + R4(0.47496));
}
#ifdef RS_BL_STATS
/* [53] wave-steps in which every active lane is dead by its own tests (the sign of raNum apart), [54] wave-steps in
 * which the final stability correction is skipped, [55] of those, with a lane that left the loop on the unstable
 * side (the sqrt and the log that are not evaluated), [56] wave-steps in which every lane is dry and warm */
__device__ __forceinline__ void bl_last_count(bool dead, bool skip, bool all_warm, RS_REAL Stab) {
  const unsigned long long act = __builtin_amdgcn_ballot_w64(true), mu = __builtin_amdgcn_ballot_w64(!(Stab > R4(0.0)));
  if ((unsigned long long)__builtin_ctzll(act) == (unsigned long long)(threadIdx.x & 63u)) {
    if (dead) atomicAdd(&rs::g_bl_stats[53], 1ull);
    if (skip) atomicAdd(&rs::g_bl_stats[54], 1ull);
    if (skip && mu) atomicAdd(&rs::g_bl_stats[55], 1ull);
    if (all_warm) atomicAdd(&rs::g_bl_stats[56], 1ull);
  }
}
#endif

/* The flavour with THE LAST PASS (DRY TAIL): tests, loop on Stab, then the skip or the final correction and the tail */
template <int TRIPS = 1, class Q = ForcingPrep>
__device__ __forceinline__ Fluxes model_step_fluxes_prepped(const RS_CONSTS &c, const MathTab &mt,
                                                            Scalars &s, const Q &q,
                                                            const CouplingInputs &cp = CouplingInputs()) {
  Fluxes fx;
  s.wat = s.wat + q.rain;
  s.snow = s.snow + q.snow;
  fx.trffric = q.trffric;
  BlInv v;
  BlVar x;
  v.dT = s.tsurf - q.tair;
  v.den0 = q.den0;
  v.vkvz = q.vkvz;
  v.avk = q.avk;
  x.PSIM = R4(0.0);
  x.PSIH = R4(0.0);
  x.BLCond = 0.0;
  const RS_REAL stab_num = bl_stab_num(c);
  /* the dry-tail tests that do not read the loop's result: a lane is `dead` by stage 2 (warm) or by stage 1 */
  const RS_REAL raDen = c.VK_Const * c.VK_Const * q.vz;
  const bool dry = dry_tail_dry(s.wat, raDen);
  const bool warm = dry && dry_tail_warm_t(s.tsurf, q.tair);
  const bool all_warm = rs_wave_all(warm);
  RS_REAL N = R4(0.0);
  bool dead = true;
#ifdef RS_BL_STATS
  const bool need_n = true; /* (the counters of dry_tail_count want stage 1's verdict in every wave-step) */
#else
  const bool need_n = !all_warm;
#endif
  if (need_n) {
    asm volatile(""); /* keeps the skip a branch, as in layer_vsh */
    N = le_numerator(mt, s.tsurf, q);
    dead = rs_wave_all(warm || (dry && rs_is_pos_normal(N) && dry_tail_psychc(psychrometric(q.tair))));
  }
  RS_REAL Stab = R4(0.0);
  int j = 1;
  bool unstable = false;
#ifdef RS_BL_STATS
  { /* (the arm at the end of every pass, as bl_iteration has it: the counters look at each pass's correction) */
    const BlStatsStep st = bl_stats_step();
    for (; j <= RS_BL_MAXIT; ++j) {
      const RS_REAL h0 = x.PSIH;
      const bool done = bl_pass<false>(c, v, x, j, stab_num, Stab);
      bl_arm<false>(mt, Stab, x, TRIPS == 1 ? &unstable : nullptr);
      bl_stats_pass(st, j, h0, x);
      if (done) break;
    }
    bl_stats_trips(st, j);
  }
#else
  for (; j <= RS_BL_MAXIT; ++j) {
    if (j >= 2) bl_arm<false>(mt, Stab, x, TRIPS == 1 ? &unstable : nullptr);
    if (bl_pass<false>(c, v, x, j, stab_num, Stab)) break;
  }
  if (TRIPS == 1 && !(Stab > R4(0.0))) unstable = true; /* the exit pass's branch, without taking it */
#endif
  fx.trips = TRIPS == 1 ? j + (unstable ? 64 : 0) : TRIPS == 2 ? (j > RS_BL_MAXIT ? RS_BL_MAXIT : j) : 5;
  fx.blcond = x.BLCond;
  const bool skip = dead && rs_wave_all(Stab > c.stabSafe);
#ifdef RS_BL_STATS
  {
    const RS_REAL raNum = (c.logMom + x.PSIM) * (c.logHeat + x.PSIH);
    dry_tail_count(dry_tail_le(dry_tail_signs(s.wat, raNum, raDen), N, psychrometric(q.tair)), warm && (raNum > R4(0.0)));
    bl_last_count(dead, skip, all_warm, Stab);
  }
#endif
  if (skip) {
    fx.le = R4(0.0);
    fx.evap = R4(0.0);
  } else {
    asm volatile(""); /* keeps the skip a branch, as in layer_vsh */
#ifndef RS_BL_STATS
    bl_arm<false>(mt, Stab, x);
#endif
    const RS_REAL raNum = (c.logMom + x.PSIM) * (c.logHeat + x.PSIH);
    if (!need_n) N = le_numerator(mt, s.tsurf, q);
    const RS_REAL WatDen = R4(-0.0050) * s.tsurf * s.tsurf + R4(0.0079) * s.tsurf + R4(1000.0028);
    RS_REAL RAero = rs_dvb<false>(raNum, raDen);
    if (RAero > R4(30.0)) RAero = R4(30.);
    fx.le = rs_dvb<false>(N, psychrometric(q.tair) * RAero);
    const RS_REAL lvap = c.LVap, lfus = c.LFus;
    const RS_REAL lat = (s.tsurf >= R4(0.0)) ? lvap : lfus;
    fx.evap = rs_dvb<false>(fx.le, lat * WatDen) * R4(1000.0) * c.DTSecs;
    if ((fx.le > R4(0.0)) && (s.wat <= R4(0.0))) {
      fx.le = R4(0.0);
      fx.evap = R4(0.0);
    }
  }
#if RS_BL_GUARD && !defined(RS_IEEE_DIV) && !defined(RS_DIV_CHECK) && !defined(RS_NO_BL_GUARD) && !defined(RS_BL_FIXUP)
  if (!(rs_fabs(fx.blcond) < __builtin_inf()) || !(rs_fabs(fx.le) < __builtin_inf())) {
    const BlOut o = boundary_layer_ieee(&c, mt.expT, mt.logT, mt.K, s.tsurf, q.tair, q.vz_late(), q.rhz_late(), s.wat);
    fx.blcond = o.blcond;
    fx.le = o.le;
    fx.evap = o.evap;
  }
#endif
  fluxes_post(c, s, q.sw_late(), q.lw_late(), cp, fx);
  return fx;
}
#else
template <int TRIPS = 1, class Q = ForcingPrep>
__device__ __forceinline__ Fluxes model_step_fluxes_prepped(const RS_CONSTS &c, const MathTab &mt,
                                                            Scalars &s, const Q &q,
                                                            const CouplingInputs &cp = CouplingInputs()) {
  Fluxes fx;
  s.wat = s.wat + q.rain;
  s.snow = s.snow + q.snow;
  fx.trffric = q.trffric;
  BlInv v;
  BlVar x;
  BlAux a;
  a.PsychC = q.PsychC;
#ifndef RS_DRY_TAIL /* (with the skip: in the tail, where the skip covers it) */
  const RS_REAL WatDen = R4(-0.0050) * s.tsurf * s.tsurf + R4(0.0079) * s.tsurf + R4(1000.0028);
#endif
  v.dT = s.tsurf - q.tair;
  v.den0 = q.den0;
  v.vkvz = q.vkvz;
  v.avk = q.avk;
#ifdef RS_EXP_STAB_CHAIN
  v.kinv = rs_div((RS_REAL)1.0, v.den0 * (v.vkvz * v.vkvz * v.vkvz));
#endif
  x.PSIM = R4(0.0);
  x.PSIH = R4(0.0);
  x.BLCond = 0.0;
  const RS_REAL stab_num = bl_stab_num(c);
  int j = 1;
  bool unstable = false;
#ifdef RS_BL_STATS
  {
    const BlStatsStep st = bl_stats_step();
    for (; j <= RS_BL_MAXIT; ++j) {
      const RS_REAL h0 = x.PSIH;
      const bool done = bl_iteration<false>(c, mt, v, x, j, stab_num, TRIPS == 1 ? &unstable : nullptr);
      bl_stats_pass(st, j, h0, x);
      if (done) break;
    }
    bl_stats_trips(st, j);
  }
#else
#ifdef RS_EXP_PIPE1 /* (probe: the surface's vapour pressure - independent of the loop - in the block of the peeled first pass) */
  const RS_REAL as_ = (s.tsurf < 0) ? R4(21.875) : R4(17.269);
  const RS_REAL bs_ = (s.tsurf < 0) ? R4(265.5) : R4(237.3);
  const RS_REAL ESurf_ = R4(0.61078) * rs_exp(mt, rs_dv<false>(as_ * s.tsurf, s.tsurf + bs_));
  (void)bl_iteration<false>(c, mt, v, x, 1, stab_num, TRIPS == 1 ? &unstable : nullptr);
  j = 2;
#endif
  for (; j <= RS_BL_MAXIT; ++j)
    if (bl_iteration<false>(c, mt, v, x, j, stab_num, TRIPS == 1 ? &unstable : nullptr)) break;
#endif
  fx.trips = TRIPS == 1 ? j + (unstable ? 64 : 0) : TRIPS == 2 ? (j > RS_BL_MAXIT ? RS_BL_MAXIT : j) : 5;
  fx.blcond = x.BLCond;
  do { /* bl_finish with EAir handed over */
    const RS_REAL raNum = (c.logMom + x.PSIM) * (c.logHeat + x.PSIH), raDen = c.VK_Const * c.VK_Const * q.vz;
#ifdef RS_DRY_TAIL
    const bool signs = dry_tail_signs(s.wat, raNum, raDen);
#endif
#ifdef RS_DRY_ESURF
#ifdef RS_EAIR_SURFACE
    const bool warm = signs && dry_tail_warm_t(s.tsurf, q.tair);
#else
    const bool warm = dry_tail_warm(signs, s.tsurf, q.tair, q.EAir);
#endif
#ifndef RS_BL_STATS
    if (rs_wave_all(warm)) {
      fx.le = R4(0.0);
      fx.evap = R4(0.0);
      break;
    }
#endif
#endif
    const RS_REAL as = (s.tsurf < 0) ? R4(21.875) : R4(17.269);
    const RS_REAL bs = (s.tsurf < 0) ? R4(265.5) : R4(237.3);
#ifdef RS_EXP_SURFACE_LIGHT
    const RS_REAL ESurf = R4(0.61078) + (as + bs) * R4(0.0001) * s.tsurf;
#elif defined(RS_EXP_PIPE1)
    const RS_REAL ESurf = ESurf_;
    (void)as; (void)bs;
#else
    const RS_REAL ESurf = R4(0.61078) * rs_exp(mt, rs_dv<false>(as * s.tsurf, s.tsurf + bs));
#endif
#ifdef RS_EAIR_SURFACE
    const RS_REAL EAir = air_vapour_pressure(mt, q.tair, q.rhz_late());
#else
    const RS_REAL EAir = q.EAir;
#endif
    /* (AirDens x AirHCap x (...) is (AirDens x AirHCap) x (...): the product arrives as AirVCap) */
    const RS_REAL N = q.AirVCap * (ESurf - EAir);
#ifdef RS_DRY_TAIL
    const bool le_dry = dry_tail_le(signs, N, a.PsychC);
#if defined(RS_BL_STATS) && defined(RS_DRY_ESURF)
    dry_tail_count(le_dry, warm);
#endif
    if (rs_wave_all(le_dry)) {
      fx.le = R4(0.0);
      fx.evap = R4(0.0);
      break;
    }
    asm volatile(""); /* keeps the skip a branch, as in layer_vsh */
    const RS_REAL WatDen = R4(-0.0050) * s.tsurf * s.tsurf + R4(0.0079) * s.tsurf + R4(1000.0028);
#endif
    RS_REAL RAero = rs_dvb<false>(raNum, raDen);
    if (RAero > R4(30.0)) RAero = R4(30.);
    fx.le = rs_dvb<false>(N, a.PsychC * RAero);
    const RS_REAL lvap = c.LVap, lfus = c.LFus;
    const RS_REAL lat = (s.tsurf >= R4(0.0)) ? lvap : lfus;
    fx.evap = rs_dvb<false>(fx.le, lat * WatDen) * R4(1000.0) * c.DTSecs;
    if ((fx.le > R4(0.0)) && (s.wat <= R4(0.0))) {
      fx.le = R4(0.0);
      fx.evap = R4(0.0);
    }
  } while (false);
#if RS_BL_GUARD && !defined(RS_IEEE_DIV) && !defined(RS_DIV_CHECK) && !defined(RS_NO_BL_GUARD) && !defined(RS_BL_FIXUP)
  if (!(rs_fabs(fx.blcond) < __builtin_inf()) || !(rs_fabs(fx.le) < __builtin_inf())) {
    const BlOut o = boundary_layer_ieee(&c, mt.expT, mt.logT, mt.K, s.tsurf, q.tair, q.vz_late(), q.rhz_late(), s.wat);
    fx.blcond = o.blcond;
    fx.le = o.le;
    fx.evap = o.evap;
  }
#endif
  fluxes_post(c, s, q.sw_late(), q.lw_late(), cp, fx);
  return fx;
}
#endif /* RS_BL_LAST */

/* One layer of CalcHCapHCond + calcCapDZCondDZ + calcProfile fused (src/BalanceModel.f90:189-251,
 * 132-155, 90-129): heat capacity from the (stale) TmpNw value, capDZ, the flux to the layer below,
 * the explicit update.  tj = Tmp(j), tnext = Tmp(j+1), Gprev = the flux from the layer above (in:
 * G(j-1), out: G(j)).  hs1: where to leave HS(1) (layer 1 only). */
__device__ __forceinline__ RS_REAL layer_step(const RS_CONSTS &c, int j, RS_REAL tj, RS_REAL tstale,
                                              RS_REAL tnext, RS_REAL &Gprev, RS_REAL *hs1) {
#ifdef RS_FROZEN_TABLE
  /* capDZ travels NEGATED (ncap = -capDZ: the quotient as it comes out of the division, the frozen table's value
   * with its sign flipped on the scalar unit) and the update multiplies by -ncap: the sign is an operand modifier
   * of the multiplication, the same product bit for bit, instead of a vector instruction per thawed layer at the
   * point where the two arms join. */
  RS_REAL ncap;
  /* every lane of the wavefront has the layer frozen (NaN compares as frozen in layer_vsh too): the
   * plan's constants (rs_consts_dev.h).  The forecast sort's ground digit lines the points up by frost
   * depth, so that this is the common case where the ground is frozen at all - and a layer that is not frozen
   * in every point is mostly thawed in every point, which layer_vsh is told. */
  const unsigned long long thawed = __builtin_amdgcn_ballot_w64(tstale >= 0);
#ifdef RS_EXP_SURFACE_LIGHT
  if (j <= 2) {
    ncap = -RS_LK(c, j, capDZF);
    if (hs1) *hs1 = c.hs1F;
  } else
#endif
  if (thawed == 0ull) {
    ncap = -RS_LK(c, j, capDZF);
    if (hs1) *hs1 = c.hs1F;
  } else {
    const RS_REAL vsh = layer_vsh(c, j, tstale, thawed == __builtin_amdgcn_ballot_w64(true));
    if (hs1) *hs1 = RS_DIVC(vsh * c.HSfac1, c.twoDT, r_twoDT);
    ncap = rs_div((RS_REAL)1.0, RS_LK(c, j, DyC) * vsh);
  }
  const RS_REAL G = RS_LK(c, j, condDZ) * (tnext - tj);
  const RS_REAL tn = tj + c.DTSecs * (-ncap * (G - Gprev));
#else
  const RS_REAL vsh = layer_vsh(c, j, tstale);
  if (hs1) *hs1 = RS_DIVC(vsh * c.HSfac1, c.twoDT, r_twoDT);
  const RS_REAL capDZ = -rs_div((RS_REAL)1.0, RS_LK(c, j, DyC) * vsh);
  const RS_REAL G = RS_LK(c, j, condDZ) * (tnext - tj);
  const RS_REAL tn = tj + c.DTSecs * (capDZ * (G - Gprev));
#endif
  Gprev = G;
  return tn;
}

/* second half: ground profile, melting, new surface temperature, storages.
 * depth_i is modelInput%depth(i). */
/* DEPTH = false: neither tsurfOutputDepth nor depth(i) can be >= 0 (the LEAN feature set): the
 * surface temperature is the mean of the two top layers, no search of the grid is compiled in. */
template <class Prof, class Stale = Prof, bool DEPTH = true>
__device__ __forceinline__ void model_step_ground(const RS_CONSTS &c, Scalars &s, Prof &T,
                                                  RS_REAL tbot, RS_REAL tair, const Fluxes &fx,
                                                  RS_REAL depth_i,
                                                  const CouplingInputs &cp = CouplingInputs(),
                                                  const Stale *stale_all = nullptr) {
  const int N = T.nlayers();
  /* CalcHCapHCond + calcCapDZCondDZ + calcProfile fused
   * (src/BalanceModel.f90:189-251, 132-155, 90-129) */
  const RS_REAL t1old = T.get(1), t2old = T.get(2);
  const RS_REAL Sens = fx.blcond * (tair - t1old);
  RS_REAL Gprev = fx.rnet - fx.le + fx.trffric + Sens;
  RS_REAL hs1 = 0.0;
  /* The layer constants are read through a pointer that is laundered every RS_LAYER_GROUP layers: the
   * scalar loads of a group cannot be issued before the group starts, so the compiler does not fetch
   * all four tables of all layers up front (64 scalar registers, which pushes the masks that live
   * across this block into VGPR lanes: 18 v_writelane/v_readlane per step) */
  const RS_CONSTS *cl = &c;
#pragma unroll
  for (int j = 1; j <= N; ++j) {
    if (Prof::kUnrolled && RS_LAYER_GROUP > 0 && j > 1 && (j - 1) % RS_LAYER_GROUP == 0)
      asm volatile("" : "+s"(cl)); /* (profiles whose layer loop is not unrolled fetch per iteration anyway) */
    const RS_REAL tj = T.get(j);
    /* TmpNw(j) as CalcHCapHCond sees it (src/BalanceModel.f90:215): equal to Tmp(j) except
     * for layers 1-2 after observation forcing, and for EVERY layer on the first step after
     * a coupling restore (Tmp is restored, TmpNw is not: src/Coupling.f90:245-247) */
    const RS_REAL tstale = stale_all ? stale_all->get(j) : (j == 1) ? s.tnw1 : (j == 2) ? s.tnw2 : tj;
    const RS_REAL tnext = (j == N) ? tbot : T.get(j + 1);
    T.set(j, layer_step(*cl, j, tj, tstale, tnext, Gprev, (j == 1) ? &hs1 : nullptr));
  }
  T.pin();

  /* calcHStor, src/BalanceModel.f90:311-322 */
  const RS_REAL T1Ave = (t1old + R4(3.) * t2old) / R4(4.);
  const RS_REAL TN1Ave = (T.get(1) + R4(3.) * T.get(2)) / R4(4.);
  const RS_REAL hstor = hs1 * (TN1Ave - T1Ave);

  melting(s, T, hstor, hs1, cp.in_phase, cp.last_tsurf_obs);

  /* Tmp = TmpNw; new TsurfAve (src/BalanceModel.f90:60-84) */
  s.tnw1 = T.get(1);
  s.tnw2 = T.get(2);
  if (DEPTH) {
    const RS_REAL depth = (c.tsurfOutputDepth >= R4(0.0)) ? c.tsurfOutputDepth : depth_i;
    s.tsurf = surface_temperature(c, T, tbot, depth);
  } else {
    s.tsurf = (T.get(1) + T.get(2)) / R4(2.0);
  }

  road_condition(c, s, fx.evap);
}

/* CheckValues, src/InputOutput.f90:45-84 (sky-view checks: see the general kernel) */
/* Every comparison is evaluated (`|`, not `||`): compares and their ORs on the scalar unit instead
 * of a ladder of divergent branches, and tests against the SAME bound share one compare through
 * max/min - `a > h | b > h` is `max(a, b) > h`, also for a NaN operand, which the reference does not
 * reject either (x < lo and x > hi are both false) and which v_max/v_min_f64 drop: 64 -> 30
 * instructions per step. */
__device__ __forceinline__ bool check_values(const RS_CONSTS &c, const Forcing &f, RS_REAL tsurf,
                                             bool has_tdew) {
  const RS_REAL hi100 = rs_fmax(f.tair, f.vz);                              /* > 100 */
  const RS_REAL lo01 = rs_fmin(rs_fmin(f.rhz, f.sw), rs_fmin(f.lw, f.prec)); /* < -0.1 */
  /* RS_CHK(i, literal): the bound, from the plan's constant block where there is one (eight doubles,
   * one scalar load, instead of two scalar moves per fp64 literal) */
  bool bad = (hi100 > RS_CHK(c, 0, R4(100.0))) | (lo01 < RS_CHK(c, 1, R4(-0.1))) |
             (f.tair < RS_CHK(c, 2, R4(-90.0))) | (f.rhz > RS_CHK(c, 3, R4(120.0))) |
             (f.vz < RS_CHK(c, 4, R4(-1.0))) | (f.sw > RS_CHK(c, 5, R4(4000.0))) |
             (f.lw > RS_CHK(c, 6, R4(1000.0))) | (f.prec > RS_CHK(c, 7, R4(500.0)));
  if (has_tdew) bad = bad | (f.tdew < -90) | (f.tdew > R4(100.0));
  bad = bad | (rs_fabs(tsurf) > RS_CHK(c, 0, R4(100.0)));
  return bad;
}

}  // namespace RS_NS
