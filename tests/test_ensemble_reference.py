"""CPU: the premise of the ensemble fan-out, held on the reference itself, and the numpy definition.

roadsurf_amd/ensemble.py steps the analysis that the members of a station share once and branches the members from its
carried state.  That is the run of the replicated input only if the outputs at indices <= B do not depend on forcing
or relaxation targets that differ behind B: checked here on the oracle (the reference's own Fortran where it is built,
the C restatement otherwise), together with the converse that makes the runner refuse its input."""
import os
import re

import numpy as np
import pytest

import ensemble_helpers as eh
import oracle_helpers as oh
from roadsurf_amd import abi, ensemble, lib


def test_parents_and_replicate_on_a_toy_case():
    assert np.array_equal(ensemble.parents(3, 2), [0, 0, 1, 1, 2, 2])
    assert ensemble.parents(3, 2).dtype == np.int32
    S, L, B = 3, 7, 4
    st = {"tair": np.arange(S * L, dtype=np.float64).reshape(S, L), "precphase": np.ones((S, L), np.int32),
          "hour": np.arange(L, dtype=np.int32)}
    parent = np.array([2, 0, 0, 1, 2], np.int32)
    tl = {"tair": 100.0 + np.arange(5 * (L - B), dtype=np.float64).reshape(5, L - B),
          "precphase": np.zeros((5, L - B), np.int32), "hour": np.array([40, 50, 60], np.int32)}
    rep = ensemble.replicate(st, tl, parent, B)
    assert set(rep) == {"tair", "precphase", "hour"}
    assert rep["tair"].shape == (5, L) and rep["tair"].dtype == np.float64 and rep["tair"].flags.c_contiguous
    assert rep["precphase"].dtype == np.int32 and rep["hour"].dtype == np.int32
    assert np.array_equal(rep["tair"][:, :B], st["tair"][parent, :B])
    assert np.array_equal(rep["tair"][:, B:], tl["tair"])
    assert np.array_equal(rep["precphase"], np.concatenate([np.ones((5, B)), np.zeros((5, L - B))], axis=1))
    assert np.array_equal(rep["hour"], [0, 1, 2, 3, 40, 50, 60])
    with pytest.raises(ValueError, match="tair"):
        ensemble.replicate(st, dict(tl, tair=tl["tair"][:4]), parent, B)


def _members_differ(out, S, M, row):
    """stations whose members do not all have the same Tsurf at ``row``"""
    t = out["tsurf"][:, row].reshape(S, M)
    return int((t.max(1) != t.min(1)).sum())


def test_premise_on_the_reference_uncoupled():
    c = eh.lean_case()
    S, M, L, B, parent = c["S"], c["M"], c["L"], c["B"], c["parent"]
    rep = eh.lean_oracle()
    alone = oh.run_oracle(eh.lean_kind(), c["stations"], c["settings"], c["params"], c["local"])[0]
    for k in oh.F64_OUT:
        assert np.array_equal(rep[k][:, :B], alone[k][parent, :B]), k
        assert not (rep[k] == -9999.0).any(), k
    assert _members_differ(rep, S, M, B) == S
    assert _members_differ(rep, S, M, L - 1) == S


def test_premise_on_the_reference_coupled_and_relaxed():
    c = eh.coupled_case()
    S, M, L, B, parent = c["S"], c["M"], c["L"], c["B"], c["parent"]
    rep = eh.coupled_oracle()
    # the stations alone: their own forcing to the end (anything behind B), their own targets
    alone = oh.run_oracle(eh.cpl_kind(), c["stations"], c["settings"], c["params"], c["station_local"])[0]
    for k in oh.F64_OUT:
        assert np.array_equal(rep[k][:, :B], alone[k][parent, :B]), k
        assert not (rep[k] == -9999.0).any(), k
    for row in (B, B + 1, L - 1):
        assert _members_differ(rep, S, M, row) == S, row
    # the members' own targets act: the same members with their stations' targets give other values
    same = [eh.copy_local(c["station_local"][q]) for q in parent]
    plain = oh.run_oracle(eh.cpl_kind(), c["rep"], c["settings"], c["params"], same)[0]
    depend = int((np.abs(plain["tsurf"][:, B:] - rep["tsurf"][:, B:]).max(1) > 0).sum())
    print("points that depend on their own targets:", depend)
    assert depend >= S * (M - 1)


def test_converse_targets_of_their_own_before_b_are_refused_and_not_shared():
    """InitLenI = 700 < B = 760: the members' targets act from index 701 on, so the rows <= B are NOT shared - on the
    reference - and the runner refuses the input."""
    c = eh.coupled_case(initlen=700, B=760)
    S, M, B, parent = c["S"], c["M"], c["B"], c["parent"]
    rep = eh.coupled_oracle(initlen=700, B=760)
    differ = [k for k in oh.F64_OUT if (rep[k][:, :B].reshape(S, M, B).max(1) != rep[k][:, :B].reshape(S, M, B).min(1)).any()]
    print("not shared at rows <= B:", differ)
    assert "tsurf" in differ and len(differ) >= 3
    with pytest.raises(ValueError, match=r"InitLenI = 700 < B = 760"):
        ensemble.run_ensemble(c["stations"], c["tails"], B, c["settings"], c["params"], c["station_local"],
                              c["member_local"], chunk=128)
    # the same targets are fine once nothing of theirs acts before B
    ok = eh.coupled_case()
    ensemble.check(ok["S"], ok["L"], ok["B"], ok["settings"], ok["station_local"], ok["member_local"], ok["parent"])


def test_runner_refusals_need_no_device():
    c = eh.lean_case()
    for B in (0, c["L"]):
        with pytest.raises(ValueError, match="outside"):
            ensemble.check(c["S"], c["L"], B, c["settings"], [c["local"]] * c["S"], None, c["parent"])


def test_library_exports_the_fanout_and_the_header_declares_it():
    assert "rs_hip_state_fanout" in lib.EXPORTS
    L = lib.load()
    assert hasattr(L, "rs_hip_state_fanout")
    header = open(os.path.join(oh.ROOT, "include", "roadsurf.h")).read()
    assert re.search(r"int\s+rs_hip_state_fanout\(RsPlan \*dst, RsPlan \*src, const int32_t \*parent\);", header)
    assert L.rs_abi_version() == int(re.search(r"#define RS_ABI_VERSION (\d+)", header).group(1))
