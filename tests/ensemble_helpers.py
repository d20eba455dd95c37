"""The ensemble cases that tests/test_ensemble_reference.py (CPU, the reference) and tests/test_hip_ensemble.py (GPU)
share: inputs, and the oracle's results for the replicated input, each made once."""
from __future__ import annotations

import functools
import os

import numpy as np

import oracle_helpers as oh
from roadsurf_amd import abi, ensemble

MISSING_OBS = -9999.9
OFFSETS = [0.0, 0.05, 0.5, -0.5, 2.0, -2.0, 6.0, -6.0, 15.0, -15.0]  # tests/test_hip_coupling.py


def lean_kind():
    return "ref" if oh.have_ref() else "port"


def cpl_kind():
    return "ref_cpl" if os.path.exists(oh.REF_CPL_SO) else "port"


def tails(n, L, B, seed):
    f = oh.synth_forcing(n, L, seed=seed, point_offset=1000)
    return {k: np.ascontiguousarray(v[..., B:]) for k, v in f.items()}


def copy_local(l):
    c = abi.LocalParameters()
    for name, _ in abi.LocalParameters._fields_:
        setattr(c, name, getattr(l, name))
    return c


@functools.lru_cache(maxsize=None)
def lean_case():
    """S, M, L, B = 70, 5, 721, 433; default settings and parameters, InitLenI = 1."""
    S, M, L, B = 70, 5, 721, 433
    st = oh.synth_forcing(S, L, seed=11)
    tl = tails(S * M, L, B, 12)
    s = abi.default_settings(L); p = abi.default_parameters(); l = abi.default_local(); l.InitLenI = 1
    parent = ensemble.parents(S, M)
    rep = ensemble.replicate(st, tl, parent, B)
    return dict(S=S, M=M, L=L, B=B, stations=st, tails=tl, settings=s, params=p, local=l, parent=parent, rep=rep)


@functools.lru_cache(maxsize=None)
def lean_oracle():
    c = lean_case()
    return oh.run_oracle(lean_kind(), c["rep"], c["settings"], c["params"], c["local"])[0]


@functools.lru_cache(maxsize=None)
def coupled_case(initlen=None, B=701):
    """L, ci = 1441, 700, coupled and relaxed: the stations' observations are the uncoupled Tsurf + 0.3 up to B and
    missing behind, InitLenI = B (or ``initlen``), every 50th station without a coupling observation; member m of a
    station relaxes towards tair(B + 1) + 0.5 m, 3 + 0.2 m, 80 - m."""
    S, M, L, ci = 70, 5, 1441, 700
    st = oh.synth_forcing(S, L, seed=21)
    tl = tails(S * M, L, B, 22)
    s0 = abi.default_settings(L); p = abi.default_parameters(); l0 = abi.default_local(); l0.InitLenI = 1
    base = oh.run_oracle("port", st, s0, p, l0)[0]
    st["tsurfobs"][:, :B] = base["tsurf"][:, :B] + 0.3
    st["tsurfobs"][:, B:] = MISSING_OBS
    tl["tsurfobs"][:] = MISSING_OBS
    s = abi.default_settings(L); s.use_coupling = 1; s.use_relaxation = 1
    rs = np.random.RandomState(21)
    sl = []
    for i in range(S):
        li = abi.default_local()
        li.InitLenI = B if initlen is None else initlen
        li.couplingIndexI = ci
        li.couplingTsurf = float(base["tsurf"][i, ci - 1] + rs.choice(OFFSETS))
        if i % 50 == 0:
            li.couplingTsurf = -9999.0
        li.tair_relax = float(st["tair"][i, B]); li.VZ_relax = 3.0; li.RH_relax = 80.0
        sl.append(li)
    parent = ensemble.parents(S, M)
    ml = []
    for q, pt in enumerate(parent):
        m = q % M
        li = copy_local(sl[pt])
        li.tair_relax = float(tl["tair"][q, 0]) + 0.5 * m; li.VZ_relax = 3.0 + 0.2 * m; li.RH_relax = 80.0 - m
        ml.append(li)
    rep = ensemble.replicate(st, tl, parent, B)
    return dict(S=S, M=M, L=L, B=B, stations=st, tails=tl, settings=s, params=p, station_local=sl, member_local=ml,
                parent=parent, rep=rep)


@functools.lru_cache(maxsize=None)
def coupled_oracle(initlen=None, B=701):
    c = coupled_case(initlen, B)
    return oh.run_oracle(cpl_kind(), c["rep"], c["settings"], c["params"], c["member_local"])[0]
