"""Parameter sets off the reference's defaults, and the knots and locals they are run on, for
tests/test_param_sets_reference.py (CPU) and tests/test_hip_param_sets.py (a plain module: no fixture, no pytest
setting, no GPU at import).

``draw`` moves every parameter tests/test_hip_param_fuzz.py moves - its tables, imported, and its rules for the
derived limits - and the thirteen no test moved before.  ``GUARD_OFF`` holds the five single edits that switch the
kernels' wave-uniform shortcuts off (rs_consts_dev.h: bareFastOk, precFastOk): a negative upper storage limit, a
negative MinPrecmm.  The reference is finite and fails no point on any of them (tests/test_param_sets_reference.py).
"""
from __future__ import annotations

import numpy as np

import golden_helpers as gh
from roadsurf_amd import abi, synth
# The tables are imported, not copied: one set of bands.  test_hip_param_fuzz is a gpu-marked test module, and this
# module is imported by a CPU test file: that module must keep doing nothing at import that needs a GPU or the
# product library (today it defines tables and functions only).
from test_hip_param_fuzz import _SCALED, _SHIFTED

# (name, low, high): multiplicative band around the default.  The bands keep log(ZRefW / ZMom) and
# log(ZRefT / ZHeat) positive over test_hip_param_fuzz's ZMom and ZHeat bands (ZRefW >= 5 > ZMom <= 0.8,
# ZRefT >= 1 > ZHeat <= 0.01), the displacement height below both reference heights, and AlbDry below one
EXTRA_SCALED = [("Grav", 0.9, 1.1), ("SB_Const", 0.9, 1.1), ("VK_Const", 0.8, 1.2), ("Omega", 0.8, 1.2),
                ("ZRefW", 0.5, 2.0), ("ZRefT", 0.5, 2.0), ("AlbDry", 0.5, 2.0),
                ("MinPrecmm", 0.0, 3.0), ("MinWatmms", 0.0, 3.0), ("MinSnowmms", 0.0, 3.0),
                ("MinDepmms", 0.0, 3.0), ("MinIcemms", 0.0, 3.0)]
ZERO_DISP = (0.0, 0.5)  # uniform, not a factor: the default is 0


def draw(seed: int, dt: float = 30.0) -> abi.InputParameters:
    """One parameter set: every band drawn independently from RandomState(4000 + seed)."""
    rs = np.random.RandomState(4000 + seed)
    p = abi.default_parameters(dt)
    for name, lo, hi in _SCALED:
        setattr(p, name, getattr(p, name) * rs.uniform(lo, hi))
    for name, lo, hi in _SHIFTED:
        setattr(p, name, getattr(p, name) + rs.uniform(lo, hi))
    p.PLimSnow = rs.uniform(0.1, 0.45)
    p.PLimRain = rs.uniform(0.55, 0.9)
    # the derived limits follow the reference driver's expressions (InputParameters.cpp:13-21)
    p.MaxWatmms = p.MaxPormms + p.MaxExtmms
    p.WDampLim = 0.1 * p.MaxPormms; p.WWetLim = 0.9 * p.MaxPormms; p.WWearLim = 0.1 * p.MaxPormms
    for name, lo, hi in EXTRA_SCALED:
        setattr(p, name, getattr(p, name) * rs.uniform(lo, hi))
    p.ZeroDisp = rs.uniform(*ZERO_DISP)
    return p


def _edited(name, value):
    def make(dt: float = 30.0) -> abi.InputParameters:
        p = abi.default_parameters(dt)
        setattr(p, name, value)
        return p
    return make


#: name -> maker of the default set with ONE member edited; the first switches precFastOk off, the others bareFastOk
GUARD_OFF = {"MinPrecmm": _edited("MinPrecmm", -1e-3), "MaxDepmms": _edited("MaxDepmms", -0.5),
             "MaxIcemms": _edited("MaxIcemms", -0.5), "MaxSnowmms": _edited("MaxSnowmms", -0.5),
             "MaxWatmms": _edited("MaxWatmms", -0.5)}


def members(p: abi.InputParameters) -> dict:
    return {k: getattr(p, k) for k in abi.INPUT_PARAMETER_NAMES}


def knots(n: int, hours: int, spk: int, seed: int, start_hour: int = 0) -> dict:
    """Generator weather at the knots (tests/test_hip_time_bookkeeping.py's _knots): K[field][n, hours + 1],
    phase [n, hours + 1], tsurf0 [n]."""
    f = synth.synth_forcing(n, hours * spk + 1, seed=seed, steps_per_knot=spk, start_hour=start_hour)
    K = {k: np.ascontiguousarray(f[k][:, ::spk]) for k in gh.KNOT_FIELDS}
    K["phase"] = np.ascontiguousarray(f["precphase"][:, ::spk])
    K["tsurf0"] = f["tsurfobs"][:, 0].copy()
    return K


def dry_first_wavefront(K: dict, k0: int, k1: int, points: int = 64) -> dict:
    """A copy of K without precipitation at knots k0..k1 for points 0-63: in natural order the first wavefront
    has prec == 0 in every lane at every index of the intervals between those knots.  points = 128: the second
    fp64 wavefront too - the two are the one wavefront of the fp32 kernel, whose lanes own two points each."""
    D = {k: v.copy() for k, v in K.items()}
    D["prec"][:points, k0:k1 + 1] = 0.0
    return D


def lean_locals(n: int) -> list:
    ls = []
    for _ in range(n):
        li = abi.default_local(); li.InitLenI = 1
        ls.append(li)
    return ls


def full_locals(K: dict, n: int, spk: int) -> list:
    """tests/test_hip_time_bookkeeping.py's _locals: relaxation behind an initialization phase that ends on index
    1, one behind a knot, on a knot, or deep in the series (eleven knots in, or one knot before the last where the
    series is shorter); one target in five invalid."""
    deep = min(11, K["tair"].shape[1] - 2)
    ls = []
    for i in range(n):
        li = abi.default_local()
        li.InitLenI = (1, spk + 2, 3 * spk + 1, deep * spk + 5)[i % 4]
        li.tair_relax = float(K["tair"][i, 1]) + 1.5
        li.VZ_relax = 3.0; li.RH_relax = 85.0
        if i % 5 == 4:
            li.tair_relax = -9999.0
        ls.append(li)
    return ls
