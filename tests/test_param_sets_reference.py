"""CPU: the parameter sets of tests/param_helpers.py on the reference itself, before any kernel is held to them
(tests/test_hip_param_sets.py).

The recorded scenarios' knots (tests/golden/e2e_scenarios.npz: eight points, every precipitation phase) expanded
by the plain numpy rule over 24 h.  On every drawn set and on every single edit that switches a kernel shortcut
off, the C restatement and the reference's own Fortran agree bit for bit and fail no point - so either may stand
as the reference of the GPU tests - and every such edit changes the reference's outputs at more than one
point-step in a hundred: a kernel that ignored the edit could not pass there.
"""
import functools

import numpy as np
import pytest

import golden_helpers as gh
import knot_helpers as kh
import oracle_helpers as oh
import param_helpers as ph
from roadsurf_amd import abi

SPK, HOURS = 120, 24
L = HOURS * SPK + 1
OUT = oh.F64_OUT


@functools.lru_cache(None)
def _forcing():
    z = gh.load("e2e_scenarios.npz")
    K = {k[5:]: z[k] for k in z.files if k.startswith("knot_")}
    assert K["tair"].shape[0] == 8 and K["tair"].shape[1] >= HOURS + 1
    return kh.expand(K, L, SPK)


@functools.lru_cache(None)
def _run(kind, name):
    """name: "default", "draw<seed>" or a key of GUARD_OFF."""
    if name == "default":
        p = abi.default_parameters()
    elif name.startswith("draw"):
        p = ph.draw(int(name[4:]))
    else:
        p = ph.GUARD_OFF[name]()
    f = _forcing()
    out, _, _ = oh.run_oracle(kind, f, abi.default_settings(L), p, ph.lean_locals(f["tair"].shape[0]))
    return out


# draws 8 and 9 stand in for draws 4 and 0 in tests/test_hip_param_sets.py
SETS = [f"draw{seed}" for seed in range(10)] + list(ph.GUARD_OFF)


def test_the_sets_are_what_they_are_meant_to_be():
    d = ph.members(abi.default_parameters())
    for name, make in ph.GUARD_OFF.items():
        m = ph.members(make())
        assert [k for k in d if m[k] != d[k]] == [name] and m[name] < 0.0
    moved = set()
    for seed in range(10):
        m = ph.members(ph.draw(seed))
        moved |= {k for k in d if m[k] != d[k]}
        assert m["MaxWatmms"] == m["MaxPormms"] + m["MaxExtmms"] and m["PLimSnow"] < m["PLimRain"]
        assert m["NightOn"] != round(m["NightOn"]) and m["NightOff"] != round(m["NightOff"])
        assert 0.0 <= m["ZeroDisp"] <= 0.5 and m["ZRefW"] > m["ZMom"] and m["ZRefT"] > m["ZHeat"]
        assert all(m[k] >= 0.0 for k in ("MinPrecmm", "MinWatmms", "MinSnowmms", "MinDepmms", "MinIcemms"))
    for k in ("Grav", "SB_Const", "VK_Const", "ZRefW", "ZRefT", "ZeroDisp", "AlbDry", "Omega", "MinPrecmm",
              "MinSnowmms", "MinDepmms", "MinIcemms", "MinWatmms", "NightOn", "NightOff"):
        assert k in moved, k
    assert ph.members(ph.draw(3)) == ph.members(ph.draw(3)) != ph.members(ph.draw(4))


@pytest.mark.parametrize("name", SETS)
def test_no_point_fails_in_the_restatement(name):
    port = _run("port", name)
    for k in OUT:
        assert np.isfinite(port[k]).all(), (name, k)
    assert not kh.first_blank(port).any() and (port["tsurf"] > -100.0).all(), name


@pytest.mark.skipif(not oh.have_ref(), reason="reference build not available")
@pytest.mark.parametrize("name", SETS)
def test_restatement_and_reference_agree_bit_for_bit(name):
    port, ref = _run("port", name), _run("ref", name)
    for k in OUT:
        assert kh.same_bits(port[k], ref[k]), (name, k, int((port[k] != ref[k]).sum()))
    assert not kh.first_blank(ref).any() and (ref["tsurf"] > -100.0).all(), name


@pytest.mark.parametrize("name", list(ph.GUARD_OFF))
def test_every_guard_edit_changes_the_reference(name):
    kind = "ref" if oh.have_ref() else "port"
    base, got = _run(kind, "default"), _run(kind, name)
    frac = {k: float((got[k] != base[k]).mean()) for k in OUT}
    print(name, {k: round(v, 4) for k, v in frac.items()})
    assert max(frac.values()) > 0.01, (name, frac)
