"""The rules of roadsurf_amd/legs.py that need no GPU: which feature set a run needs, how a coupled run is staged, and
the host tables of sky view.  The expected stages are written out by hand from the rule (include/roadsurf.h,
rs_hip_step_cpl), not computed by a second copy of it."""
import numpy as np
import pytest

from roadsurf_amd import abi, legs

LAST = 241


def _settings(coupled=True, dtsecs=30.0, minutes=60):
    s = abi.default_settings(LAST, dtsecs)
    s.use_coupling = 1 if coupled else 0
    s.DTSecs = dtsecs
    s.coupling_minutes = minutes  # 60 min of 30 s: a coupling window of 120 indices
    return s


def _points(*pairs):
    ls = []
    for ci, ct in pairs:
        l = abi.default_local(); l.couplingIndexI = ci; l.couplingTsurf = ct
        ls.append(l)
    return ls


STAGES = [
    ("uncoupled", _settings(False), _points((100, -1.0)), True, [("step", 1, 241)]),
    ("one-launch", _settings(), _points((100, -1.0)), False, [("step", 1, 241)]),
    ("no-observation", _settings(), _points((100, -9999.0)), True, [("step_cpl", 1, 241)]),
    ("no-index", _settings(), _points((0, -1.0)), True, [("step_cpl", 1, 241)]),
    # the window would begin before index 1: it begins there
    ("short", _settings(), _points((100, -1.0)), True,
     [("step_cpl", 1, 100), ("cpl_replay", 1, 101), ("step_cpl", 101, 241)]),
    # windows [30, 150] and [80, 200]; the point that is off has no say in any bound
    ("two", _settings(), _points((150, -1.0), (10, -9999.0), (200, 2.0), (230, -101.0)), True,
     [("step_cpl", 1, 200), ("cpl_replay", 30, 201), ("step_cpl", 151, 241)]),
    ("at-last", _settings(), _points((241, -1.0)), True,
     [("step_cpl", 1, 241), ("cpl_replay", 121, 241), ("step_cpl", 242, 241)]),
    ("beyond-last", _settings(), _points((246, -1.0)), True,
     [("step_cpl", 1, 241), ("cpl_replay", 126, 241), ("step_cpl", 247, 241)]),
    # a window of 60 / 45 = 1.33 indices is one index long: index 1 is inside it, index 2 begins at 2 - 1
    ("fraction-1", _settings(True, 45.0, 1), _points((1, -1.0)), True,
     [("step_cpl", 1, 1), ("cpl_replay", 1, 2), ("step_cpl", 2, 241)]),
    ("fraction-2", _settings(True, 45.0, 1), _points((2, -1.0)), True,
     [("step_cpl", 1, 2), ("cpl_replay", 1, 3), ("step_cpl", 3, 241)]),
]


@pytest.mark.parametrize("settings,points,chunked,want", [c[1:] for c in STAGES], ids=[c[0] for c in STAGES])
def test_coupling_stages(settings, points, chunked, want):
    assert legs.coupling_stages(settings, points, LAST, chunked) == want


def _lean():
    s = abi.default_settings(LAST)
    l = abi.default_local(); l.InitLenI = 1
    f = {"depth": np.full((2, LAST), -9999.9), "tdew": np.zeros((2, LAST))}
    return s, [l, abi.default_local()], f


def test_feature_set_lean():
    s, ls, f = _lean()
    f["tdew"][0, 0], f["tdew"][1, 5] = -90.0, 100.0   # the limits themselves pass the Tdew check
    ls[0].sky_view, ls[1].sky_view = 1.0, -0.01       # neither is a sky view
    assert legs.feature_set(s, ls, [f]) == (False, False)
    assert legs.feature_set(s, ls, [f, f]) == (False, False)
    assert legs.feature_set(s, ls, [f], lean_if_possible=False) == (True, False)


def _initlen(s, ls, f): ls[1].InitLenI = 2
def _force(s, ls, f): s.force_tsurf = 1
def _relax(s, ls, f): s.use_relaxation = 1
def _coupling(s, ls, f): s.use_coupling = 1
def _outdepth(s, ls, f): s.tsurfOutputDepth = 0.0
def _depth(s, ls, f): f["depth"][1, 7] = 0.0
def _tdew_low(s, ls, f): f["tdew"][1, 7] = -90.5
def _tdew_high(s, ls, f): f["tdew"][0, 0] = 100.5


@pytest.mark.parametrize("switch", [_initlen, _force, _relax, _coupling, _outdepth, _depth, _tdew_low, _tdew_high],
                         ids=lambda fn: fn.__name__[1:])
def test_feature_set_full(switch):
    s, ls, f = _lean()
    switch(s, ls, f)
    assert legs.feature_set(s, ls, [f]) == (True, False)
    if switch in (_depth, _tdew_low, _tdew_high):  # in any of the forcings
        assert legs.feature_set(s, ls, [_lean()[2], f]) == (True, False)


@pytest.mark.parametrize("sky_view", [0.0, 0.5, 0.99])
def test_feature_set_sky_view(sky_view):
    s, ls, f = _lean()
    ls[1].sky_view = sky_view
    assert legs.feature_set(s, ls, [f]) == (True, True)


def test_sky_tables_are_the_host_library_tables():
    from test_host_logic import sun_case   # (held to the oracle's solar position there)
    axes, ls, tab, geo = sun_case()
    for i, l in enumerate(ls):
        l.sky_view = i / len(ls)
    got = legs.sky_tables(dict(zip(legs.AXES, axes)), ls)
    want = (tab, np.array([l.sky_view for l in ls]), *geo)
    assert len(got) == 5 and all(a.dtype == np.float64 and np.array_equal(a, b) for a, b in zip(got, want))
