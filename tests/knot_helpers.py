"""Caller-made hourly knots through the knot-reading launches (rs_hip_step_knots) for tests/test_hip_knots.py, and
the plain references of tests/test_knot_reference.py (a plain module: no fixture, no pytest setting, no GPU at
import).

The reference everywhere is ``golden_helpers.expand_knots`` - IEEE float64 in numpy - followed by the CPU checker
(``reference``).  Nothing a kernel under test produces is an input of the reference or of the run: the index-1
window of ``init_state`` is the numpy expansion's first row, uploaded.
"""
from __future__ import annotations

import types
from fractions import Fraction

import numpy as np

import golden_helpers as gh
import oracle_helpers as oh

BLOCK_FIELDS = ("tair", "tdew", "vz", "rhz", "prec", "sw", "lw", "tsurf0", "phase")  # include/roadsurf.h, rs_synth.h
DUO = 3  # the two-wavefront variant: step_kernel_duo
OUT = oh.F64_OUT


def start_of(start_hour: int):
    return (2024, 1, 10, int(start_hour), 0, 0)


def knot_block(K: dict, np_pad: int) -> np.ndarray:
    """K[field][n, nk] (+ phase [n, nk], tsurf0 [n]) -> [nk][9][np_pad] float64 in the library's field order;
    the columns behind n hold zeros."""
    n, nk = K["tair"].shape
    assert np_pad >= n
    blk = np.zeros((nk, len(BLOCK_FIELDS), np_pad))
    for q, name in enumerate(BLOCK_FIELDS):
        if name == "tsurf0":
            blk[:, q, :n] = np.asarray(K["tsurf0"], np.float64)[None, :]
        else:
            blk[:, q, :n] = np.asarray(K[name], np.float64).T
    return blk


def expand(K: dict, simlen: int, spk: int = 120, start_hour: int = 0) -> dict:
    """golden_helpers.expand_knots with the clock started at start_hour (an infinite knot makes 0 * inf on the
    way to a value numpy's rule then replaces by the knot: no warning for it)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return gh.expand_knots(K, simlen, spk, start=start_of(start_hour))


def reference(f: dict, settings, params, locals_):
    """(outputs [n][SimLen], first failed index [n]: 0 or the 1-based index behind which every row is -9999.0)."""
    ora, _, _ = oh.run_oracle("ref" if oh.have_ref() else "port", f, settings, params, locals_)
    return ora, first_blank(ora)


def first_blank(out: dict) -> np.ndarray:
    """The index at which a point was failed, from its rows: the failing index's own row is still saved, every
    later row reads -9999.0 (Simulation.f90:58) - so the 1-based index of the last saved row, where a later row is
    blank."""
    blank = np.ones(out["tsurf"].shape, bool)
    for k in OUT:
        blank &= out[k] == -9999.0
    L = blank.shape[1]
    tail = np.flip(np.cumprod(np.flip(blank, 1), 1), 1).astype(bool)  # blank from here to the end
    nblank = tail.sum(axis=1)
    return np.where(nblank > 0, L - nblank, 0).astype(np.int32)


def is_full(settings, locals_) -> bool:
    return bool(settings.use_relaxation or settings.force_tsurf or any(l.InitLenI > 1 for l in locals_))


def run_knots(K: dict, settings, params, locals_, *, precision: int = 64, chunks, order: str, start_hour: int = 0,
              spk: int = 120, source: str = "knots"):
    """The block through rs_hip_step_knots in launches of ``chunks`` indices (the last launch takes what is left;
    a single int: every launch that long).  order "natural": the order row stays the identity; "forecast": a
    recluster_forecast from knot rows between launches, exactly workload.SyntheticRun._resort's calls.  Per-point
    parameter arrays are gathered through the order row for every launch and the outputs mapped back through it.
    source "window": the same launches through rs_hip_expand_forcing_ordered + rs_hip_step (the A/B partner).
    Returns dict(out [n][SimLen] per field, failed, first_failed [n], orders [launch][n], moved)."""
    import torch
    from roadsurf_amd import abi, device, lib, workload

    assert order in ("natural", "forecast") and source in ("knots", "window")
    assert order == "natural" or spk == workload.SPK
    if isinstance(locals_, abi.LocalParameters):
        locals_ = [locals_] * K["tair"].shape[0]
    n, L = K["tair"].shape[0], int(settings.SimLen)
    f32 = precision == 32
    wdt = torch.float32 if f32 else torch.float64
    plan = device.Plan(n, settings, params, 0)
    plan.set_variant(DUO)
    if f32:
        plan.set_precision(32)
    plan.set_history_score(False)
    dev, npad = plan.device, plan.np_pad
    knots = torch.from_numpy(knot_block(K, npad)).to(dev)
    spec = lib.RsSynthSpec(0, 0, spk, start_hour)
    full = is_full(settings, locals_)

    # index 1 for the init kernel: the first row of the numpy expansion
    f1 = expand(K, 1, spk, start_hour)
    win0 = device.ForcingWindow.empty(1, npad, dev, optional=("tdew", "tsurfobs"), dtype=wdt)
    for name, t in win0.tensors.items():
        if t is None or name == "hour":
            continue
        t.zero_()
        t[0, :n] = torch.from_numpy(np.ascontiguousarray(f1[name][:, 0])).to(dev).to(t.dtype)
    win0.tensors["hour"][0] = int(f1["hour"][0])

    start = start_of(start_hour)
    tb = plan.uniform_tbottom(*start[:3])
    per_point = {"initlen": (np.array([l.InitLenI for l in locals_], np.int32), torch.int32),
                 "tair_relax": (np.array([l.tair_relax for l in locals_]), torch.float64),
                 "vz_relax": (np.array([l.VZ_relax for l in locals_]), torch.float64),
                 "rh_relax": (np.array([l.RH_relax for l in locals_]), torch.float64)}

    def params_in(order_row):
        """RsPointParams in the slot order of order_row (slot -> point)."""
        if not full:
            return plan.point_params(tb)
        v = {}
        for name, (a, dt) in per_point.items():
            t = torch.zeros((npad,), dtype=dt, device=dev)
            t[:n] = torch.from_numpy(np.ascontiguousarray(a[order_row])).to(dev)
            v[name] = t
        relax = bool(settings.use_relaxation)
        return plan.point_params(tb, v["initlen"], *([v["tair_relax"], v["vz_relax"], v["rh_relax"]] if relax else []))

    if isinstance(chunks, int):
        chunks = [chunks] * ((L + chunks - 1) // chunks)
    launches, t0 = [], 1
    for c in chunks:
        if t0 > L:
            break
        ns = min(int(c), L - t0 + 1)
        launches.append((t0, ns))
        t0 += ns
    if t0 <= L:
        launches.append((t0, L - t0 + 1))
    rows = max(ns for _, ns in launches)
    out = device.OutputWindow.empty(rows, npad, dev, dtype=wdt)
    win = None
    if source == "window":
        win = device.ForcingWindow.empty(rows, npad, dev, optional=("tdew", "tsurfobs") if full else (), dtype=wdt)

    # what workload.SyntheticRun._resort reads of its object: the same calls, from this block's knot rows
    # (the workload keeps one knot behind the series' last, hours + 2: its preview of the last window names it)
    kn_sort = knots if knots.shape[0] >= (L - 1) // spk + 2 else torch.cat([knots, knots[-1:]])
    sorter = types.SimpleNamespace(plan=plan, simlen=L, resort=True, forecast=True, chunk=0, spec=spec, knots=kn_sort,
                                   precip_bit=True, previews_in_window=True, forecast_alpha=0.5,
                                   forecast_mode=workload.DEFAULT_FORECAST_MODE)

    plan.reset_order()
    ident = np.arange(n)
    pp = params_in(ident)
    plan.init_state(win0, pp)
    got = {k: np.full((n, L), np.nan, np.float32 if f32 else np.float64) for k in OUT}
    orders, moved = [], 0
    try:
        for c, (t0, ns) in enumerate(launches):
            plan.sync()
            row = plan.order().cpu().numpy()[:n].astype(np.int64)
            orders.append(row)
            if not np.array_equal(np.sort(row), ident):  # nothing can be mapped back: the caller asserts on orders
                break
            moved += int((row != ident).sum())
            pp = params_in(row)
            if source == "knots":
                plan.step_knots(spec, knots, out, pp, t0, ns, out_row0=t0 - 1)
            else:
                plan.expand_ordered(spec, knots, win, t0, ns)
                plan.step(win, out, pp, t0, ns, out_row0=t0 - 1)
            plan.sync()
            for k in OUT:
                got[k][row, t0 - 1:t0 - 1 + ns] = out.tensors[k][:ns, :n].cpu().numpy().T
            if order == "forecast" and c + 1 < len(launches):
                sorter.chunk = launches[c + 1][1]
                workload.SyntheticRun._resort(sorter, t0 + ns)
        plan.sync()
        res = {"out": got, "failed": plan.failed_count(), "first_failed": plan.first_failed_index(),
               "orders": orders, "moved": moved}
    finally:
        plan.close()
    return res


# ---- the flavours a hand-made knot block is sent through ------------------------------------------------------
# (entry, ...): "knots" / "window" - run_knots with that source, natural order; "points" - device.run_points with
# (variant, lean_if_possible, chunked).  Launches of FLAVOUR_CHUNK indices where chunked.  Which step-kernel
# instance each of them takes at 15 layers is pinned by tests/test_step_selection.py; the module docstring of
# tests/test_hip_storage_waves.py names them.
FLAVOUR_CHUNK = 60
FLAVOURS = [("knots",), ("window",)] + [("points", v, lean, chunked) for v in (1, 2, 3, 4) for lean in (True, False)
                                        for chunked in (False, True)]
FLAVOURS_F32 = [("knots",), ("window",), ("points", 0, True, True), ("points", 0, False, True)]


def flavour_id(fl) -> str:
    if fl[0] != "points":
        return fl[0]
    return f"variant{fl[1]}_{'lean' if fl[2] else 'full'}_{'chunks' if fl[3] else 'whole'}"


def run_flavour(fl, K: dict, f: dict, settings, params, locals_, *, start_hour: int, precision: int = 64):
    """The knot block K (and its numpy expansion f, for the entries that take a forcing window from the host) through
    one flavour: (outputs [n][SimLen], first failed index [n] - the plan's own for run_knots, read from the blank
    rows for run_points, whose count of failed points must agree with them)."""
    if fl[0] in ("knots", "window"):
        res = run_knots(K, settings, params, locals_, precision=precision, chunks=FLAVOUR_CHUNK, order="natural",
                        start_hour=start_hour, source=fl[0])
        assert res["moved"] == 0
        return res["out"], np.asarray(res["first_failed"], np.int32)
    from roadsurf_amd import device
    _, variant, lean, chunked = fl
    got, nfail = device.run_points(f, settings, params, locals_, chunk=FLAVOUR_CHUNK if chunked else 0,
                                   variant=variant, lean_if_possible=lean, precision=precision, device=0)
    got = {k: got[k] for k in OUT}
    failed = first_blank(got)
    assert nfail == int((failed > 0).sum()), (nfail, failed.nonzero())
    return got, failed


# ---- host restatements (tests/test_knot_reference.py, the fp32 expansion reference) ---------------------------

def rn(x: Fraction) -> float:
    """The exact rational rounded to nearest-even float64 (CPython's Fraction -> float division is correctly
    rounded, gradual underflow and overflow to inf included)."""
    try:
        return x.numerator / x.denominator
    except OverflowError:
        return float("inf") if x > 0 else float("-inf")


def fma(a: float, b: float, c: float) -> float:
    """RN(a * b + c) with one rounding, finite operands.  An exact zero takes the sign IEEE gives it under
    round-to-nearest: -0.0 only where the product and the addend are both negative zeros."""
    x = Fraction(a) * Fraction(b) + Fraction(c)
    if x == 0:
        pneg = (np.signbit(a) != np.signbit(b))
        if a * b == 0.0 and c == 0.0:
            return -0.0 if (pneg and np.signbit(c)) else 0.0
        return 0.0  # exact cancellation of non-zero terms
    return rn(x)


def div_u(a: float, b: float, rb: float) -> float:
    """rs_math.hpp rs_div_u: q0 = a * rb; rem = fma(-b, q0, a); fma(rem, rb, q0) - finite a."""
    q0 = a * rb
    rem = fma(-b, q0, a)
    return fma(rem, rb, q0)


# |k1 - k0| inside [DV_MIN, DV_MAX), or zero, and a k0 that is not -0.0: the knot interval takes the division by
# reciprocal (rs_kernels.hip knot_interval_fast); tests/test_knot_reference.py derives the two edges
DV_MIN = 2.0 ** -1015
DV_MAX = 2.0 ** 1017


def lerp_f32(k0: np.ndarray, k1: np.ndarray, r: np.ndarray, spk: int) -> np.ndarray:
    """The fp32 kernels' rule (rs_kernels_f32.hip rs32_lerp_knot): ONE fused multiply-add in single precision,
    fma(w, float(k1 - k0), float(k0)) with w = float(r) * float(1 / spk) - at r = 0 too, except where the
    difference is not finite in single precision: there 0 * inf would be NaN and the value is the knot's.
    Evaluated in float64 - the product of two floats is exact there, the sum is rounded once to float64 and once
    more to float32; `lerp_f32_exact` settles an element on which that double rounding could matter."""
    with np.errstate(invalid="ignore", over="ignore"):
        w = (np.float32(r) * np.float32(1.0 / spk)).astype(np.float64)
        v0 = np.float32(k0).astype(np.float64)
        dv = np.float32(k1 - k0).astype(np.float64)
        v = (w * dv + v0).astype(np.float32)
    return np.where((r == 0) & ~np.isfinite(dv), np.float32(k0), v)


def lerp_f32_exact(k0: float, k1: float, r: int, spk: int) -> np.float32:
    """One element of lerp_f32 with exact rationals: a single rounding to float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        w = float(np.float32(r) * np.float32(1.0 / spk))
        v0, dv = float(np.float32(k0)), float(np.float32(k1 - k0))
        if not (np.isfinite(v0) and np.isfinite(dv)):
            return np.float32(v0) if (r == 0 and not np.isfinite(dv)) else np.float32(w * dv + v0)
    x = Fraction(w) * Fraction(dv) + Fraction(v0)
    if x == 0:
        return np.float32(w * dv + v0)  # the sign of an exact zero: float64 has fma's rule for it
    lo = np.float32(rn(x))  # the doubly rounded candidate and its two neighbours: the nearest, ties to even
    cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - x) if np.isfinite(c) else Fraction(10) ** 400,
                                     int(np.float32(c).view(np.uint32)) & 1))
    return np.float32(best)


def expand_f32(K: dict, simlen: int, spk: int) -> dict:
    """The fp32 windows' seven interpolated streams [n][simlen] by lerp_f32, with the operands kept for
    lerp_f32_exact: (values, k0, k1, r)."""
    t = np.arange(simlen)
    k = t // spk
    r = t - k * spk
    out = {}
    for name in gh.KNOT_FIELDS:
        A = np.asarray(K[name], np.float64)
        k0, k1 = A[:, k], A[:, np.minimum(k + 1, A.shape[1] - 1)]
        out[name] = (lerp_f32(k0, k1, r[None, :], spk), k0, k1, r)
    return out


# CheckValues' forcing limits as the double-precision kernels compare them (src/InputOutput.f90:55-66: REAL(4)
# literals) - strict tests: a value ON a limit passes
F4 = lambda x: float(np.float32(x))
LIMITS = {"tair": (-90.0, 100.0), "vz": (-1.0, 100.0), "rhz": (F4(-0.1), 120.0), "prec": (F4(-0.1), 500.0),
          "sw": (F4(-0.1), 4000.0), "lw": (F4(-0.1), 1000.0), "tdew": (-90.0, 100.0)}


def predict_failure(f: dict, full: bool) -> np.ndarray:
    """The 1-based index at which CheckValues fails each point on its forcing, from the numpy series alone: the
    first index below SimLen (the last is not checked) with a value strictly outside a limit - VZ after its floor
    of 0.4 at index 1 (Initialization.f90:121-123), Tdew only with the FULL feature set.  0: never.  A NaN
    compares false everywhere: it fails nothing."""
    n, L = f["tair"].shape
    bad = np.zeros((n, L), bool)
    with np.errstate(invalid="ignore"):
        for name, (lo, hi) in LIMITS.items():
            if name == "tdew" and not full:
                continue
            v = f[name].copy()
            if name == "vz":
                v[:, 0] = np.where(v[:, 0] < 0.4, 0.4, v[:, 0])
            bad |= (v < lo) | (v > hi)
    bad[:, L - 1] = False
    return np.where(bad.any(axis=1), bad.argmax(axis=1) + 1, 0).astype(np.int32)


def same_bits(a: np.ndarray, b: np.ndarray, nan_equal: bool = False) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {8: np.int64, 4: np.int32}[a.itemsize]
    eq = a.view(it) == b.view(it)
    if nan_equal and a.dtype.kind == "f":
        eq |= np.isnan(a) & np.isnan(b)
    return bool(eq.all())
