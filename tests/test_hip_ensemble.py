"""GPU: the fan-out of the carried state (rs_hip_state_fanout) and the ensemble runner built on it
(roadsurf_amd/ensemble.py).  Every comparison is bit equality, fp32 included: both sides run the same kernels on the
same values - the runner against ``device.run_points`` of the replicated input (``ensemble.replicate``, the
definition), and that against the oracle."""
import ctypes as C

import numpy as np
import pytest

import ensemble_helpers as eh
import oracle_helpers as oh
from roadsurf_amd import abi, ensemble, groups, legs, lib
from test_hip_parity import _compare

pytestmark = pytest.mark.gpu

NL = 15                                   # NLayers of the default settings
NAMED = list(range(abi.RS_MAX_LAYERS, abi.RS_MAX_LAYERS + 17))            # RS_ST_TNW1 .. RS_ST_BLSCORE
CPL = list(range(abi.RS_MAX_LAYERS + 17, abi.RS_MAX_LAYERS + 17 + 15))    # RS_ST_CPL_ITER .. RS_ST_CPL_RESUME
SAVE = list(range(abi.RS_MAX_LAYERS + 32, abi.RS_MAX_LAYERS + 38))        # RS_ST_CPL_SAVE_TSURF .. _ALBEDO
SAVE_TMP0 = abi.RS_MAX_LAYERS + 38
STALE_TMP0 = SAVE_TMP0 + abi.RS_MAX_LAYERS


def _live_rows(coupling, closed):
    rows = list(range(NL)) + NAMED
    if coupling:
        rows += CPL
        if not closed:
            rows += SAVE + list(range(SAVE_TMP0, SAVE_TMP0 + NL)) + list(range(STALE_TMP0, STALE_TMP0 + NL))
    return rows


def _bits(plan, f32):
    """the state block as integers [RS_NSTATE, np_pad]: of an fp32 plan the floats it keeps at the block's start"""
    t = plan.state().numpy()
    if not f32:
        return t.view(np.uint64).copy()
    return t.view(np.uint32).reshape(-1)[:t.shape[0] * t.shape[1]].reshape(t.shape).copy()


def _expect(dst0, src0, order_dst, order_src, parent, rows):
    n = len(parent)
    slot_src = np.empty(len(order_src), np.int64)
    slot_src[order_src] = np.arange(len(order_src))
    want = dst0.copy()
    frm = slot_src[parent[order_dst[:n]]]
    for r in rows:
        want[r, :n] = src0[r, frm]
    return want


# a permutation with repeats that is not np.repeat: members of a station far apart, station 69 without a member
PARENT = ((np.arange(350) * 37 + 11) % 69).astype(np.int32)


@pytest.mark.parametrize("precision", [64, 32], ids=["fp64", "fp32"])
def test_the_copy_itself_between_two_resorted_plans(precision):
    """70 stations stepped to index 200 and 350 points stepped on weather of their own, both re-sorted behind every
    launch: after fanout_from every live row of dst at the slot of point p is src's at the slot of parent[p]; dst's
    padding columns, its other rows and its order row, and all of src, are what they were."""
    f32 = precision == 32
    c = eh.lean_case()
    s, p, date = c["settings"], c["params"], (2024, 1, 10)
    own = oh.synth_forcing(350, 150, seed=13, point_offset=5000)
    kw = dict(need_full=False, precision=precision, recluster=True, tbottom_date=date)
    src = legs.Leg({k: v[..., :200] for k, v in c["stations"].items()}, s, p, c["local"], **kw)
    dst = legs.Leg(own, s, p, c["local"], **kw)
    src.init(); src.chunks(1, 200, 100)
    dst.init(); dst.chunks(1, 150, 75)
    src.plan.sync(); dst.plan.sync()
    order_src = src.plan.order().cpu().numpy().copy()
    order_dst = dst.plan.order().cpu().numpy().copy()
    assert not np.array_equal(order_src[:70], np.arange(70)) and not np.array_equal(order_dst[:350], np.arange(350))
    assert np.array_equal(np.sort(order_src[:70]), np.arange(70))
    assert len(set(PARENT.tolist())) == 69 and 69 not in PARENT and not np.array_equal(PARENT, np.sort(PARENT))
    src0, dst0 = _bits(src.plan, f32), _bits(dst.plan, f32)
    dst.plan.fanout_from(src.plan, PARENT)
    dst.plan.sync()
    want = _expect(dst0, src0, order_dst, order_src, PARENT, _live_rows(False, False))
    got = _bits(dst.plan, f32)
    assert not np.array_equal(got, dst0)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(_bits(src.plan, f32), src0)
    assert np.array_equal(dst.plan.order().cpu().numpy(), order_dst)
    src.plan.close(); dst.plan.close()


@pytest.mark.parametrize("closed", [False, True], ids=["open", "closed"])
def test_coupling_rows_and_two_streams(closed):
    """Every cell of both blocks is a number of its own, src lives on a stream of its own: with use_coupling the
    coupling scalars travel, and the saved and stale profiles only while src's coupling windows are open; dst takes
    src's flag.  Nothing else of dst changes, whatever parent says (here: an irregular one, identity orders)."""
    import torch
    from roadsurf_amd import device
    s = abi.default_settings(241); s.use_coupling = 1
    p = abi.default_parameters()
    side = torch.cuda.Stream()
    src = device.Plan(70, s, p, 0, stream=side)
    dst = device.Plan(350, s, p, 0)
    nst = lib.RS_NSTATE
    a = torch.arange(nst * src.np_pad, dtype=torch.float64).reshape(nst, src.np_pad) + 0.25
    b = -torch.arange(nst * dst.np_pad, dtype=torch.float64).reshape(nst, dst.np_pad) - 0.5
    src.load_state(a); dst.load_state(b)
    if closed:
        src.coupling_windows_closed(True)
    dst.fanout_from(src, PARENT)
    dst.sync(); src.sync()
    want = b.numpy().copy()
    for r in _live_rows(True, closed):
        want[r, :350] = a.numpy()[r, PARENT]
    assert np.array_equal(dst.state().numpy(), want)
    assert np.array_equal(src.state().numpy(), a.numpy())
    src.close(); dst.close()


def _ens(c, **kw):
    return ensemble.run_ensemble(c["stations"], c["tails"], c["B"], c["settings"], c["params"],
                                 c.get("station_local", c.get("local")), c.get("member_local"), parent=c["parent"], **kw)


def _same(res, rep, c, tag):
    """the runner's rows against the rows of the replicated run: members behind B, stations up to it"""
    B, parent = c["B"], np.asarray(c["parent"])
    first = {int(q): i for i, q in reversed(list(enumerate(parent)))}   # a member of every station that has one
    have = sorted(first)
    for k in oh.F64_OUT:
        assert res["members"][k].shape == (len(parent), c["L"] - B)
        assert np.array_equal(res["members"][k], rep[k][:, B:]), (tag, k)
        assert np.array_equal(res["stations"][k][have], rep[k][[first[q] for q in have], :B]), (tag, k)


_REP = {}


def _lean_rep(variant):
    from roadsurf_amd import device
    if variant not in _REP:
        c = eh.lean_case()
        _REP[variant] = device.run_points(c["rep"], c["settings"], c["params"], c["local"], chunk=97, variant=variant)
    return _REP[variant]


@pytest.mark.parametrize("variant,recluster", [(1, False), (2, False), (3, False), (0, True)],
                         ids=["reg", "lds", "duo", "auto-recluster"])
def test_lean_end_to_end(variant, recluster):
    c = eh.lean_case()
    rep, nfail = _lean_rep(variant)
    res = _ens(c, chunk=97, variant=variant, recluster=recluster)
    assert res["failed"] == (0, 0) and nfail == 0
    _same(res, rep, c, f"lean-{variant}")
    if variant == 2:
        ora = eh.lean_oracle()
        B = c["B"]
        _compare({k: res["members"][k] for k in oh.F64_OUT}, {k: ora[k][:, B:] for k in oh.F64_OUT}, "ensemble-members")
        _compare({k: res["stations"][k] for k in oh.F64_OUT}, {k: ora[k][::c["M"], :B] for k in oh.F64_OUT},
                 "ensemble-stations")


def _small_case(S, M, L, B, seed=31):
    st = oh.synth_forcing(S, L, seed=seed)
    tl = eh.tails(S * M, L, B, seed + 1)
    s = abi.default_settings(L); p = abi.default_parameters(); l = abi.default_local(); l.InitLenI = 1
    parent = ensemble.parents(S, M)
    return dict(S=S, M=M, L=L, B=B, stations=st, tails=tl, settings=s, params=p, local=l, parent=parent)


@pytest.mark.parametrize("S,M,B", [(1, 1, 120), (3, 100, 120), (257, 1, 120), (5, 3, 1), (5, 3, 240)],
                         ids=["one", "members-pass-a-workgroup", "stations-pass-a-workgroup", "B1", "B-last"])
def test_shapes_at_the_edges(S, M, B):
    from roadsurf_amd import device
    c = _small_case(S, M, 241, B)
    rep, _ = device.run_points(ensemble.replicate(c["stations"], c["tails"], c["parent"], B), c["settings"], c["params"],
                               c["local"], chunk=64)
    res = _ens(c, chunk=64)
    assert res["failed"] == (0, 0)
    _same(res, rep, c, f"edge-{S}-{M}-{B}")


def test_a_failed_station_fails_its_members():
    from roadsurf_amd import device
    S, M, L, B = 6, 4, 241, 120
    c = _small_case(S, M, L, B, seed=41)
    c["stations"]["tair"][2, 99] = 250.0       # index 100 < B: station 2 and all its members
    c["tails"]["tair"][4 * M + 1, 30] = 250.0  # index B + 31: that member alone
    rep, nfail = device.run_points(ensemble.replicate(c["stations"], c["tails"], c["parent"], B), c["settings"],
                                   c["params"], c["local"], chunk=64)
    res = _ens(c, chunk=64)
    assert nfail == M + 1 and res["failed"] == (1, M + 1)
    _same(res, rep, c, "failed")
    for k in oh.F64_OUT:
        assert (res["members"][k][2 * M:3 * M] == -9999.0).all()
        assert (res["members"][k][4 * M + 1, 31:] == -9999.0).all() and res["members"][k][4 * M + 1, 30] != -9999.0
        others = np.ones(S * M, bool); others[2 * M:3 * M] = False; others[4 * M + 1] = False
        assert not (res["members"][k][others] == -9999.0).any()


@pytest.mark.parametrize("precision", [64, 32], ids=["fp64", "fp32"])
def test_full_features(precision):
    """Observation forcing up to InitLenI = B, relaxation towards targets of the members' own."""
    from roadsurf_amd import device
    S, M, L, B = 20, 4, 481, 240
    c = _small_case(S, M, L, B, seed=51)
    c["stations"]["tsurfobs"][:, :B] = c["stations"]["tair"][:, :B] - 0.7
    c["stations"]["tsurfobs"][::3, 100:140] = eh.MISSING_OBS
    c["tails"]["tsurfobs"][:] = eh.MISSING_OBS
    c["settings"].use_relaxation = 1
    sl, ml = [], []
    for i in range(S):
        li = abi.default_local(); li.InitLenI = B
        li.tair_relax = float(c["stations"]["tair"][i, B - 1]) + 1.5; li.VZ_relax = 3.0; li.RH_relax = 85.0
        sl.append(li)
    for q, pt in enumerate(c["parent"]):
        m = q % M
        li = eh.copy_local(sl[pt])
        li.tair_relax = float(c["tails"]["tair"][q, 0]) + 0.5 * m; li.VZ_relax = 3.0 + 0.2 * m; li.RH_relax = 80.0 - m
        if q % 7 == 0:
            li.tair_relax = -9999.0
        ml.append(li)
    c["station_local"], c["member_local"] = sl, ml
    rep, _ = device.run_points(ensemble.replicate(c["stations"], c["tails"], c["parent"], B), c["settings"], c["params"],
                               ml, chunk=100, precision=precision)
    res = _ens(c, chunk=100, precision=precision)
    _same(res, rep, c, f"full-{precision}")
    t = res["members"]["tsurf"].reshape(S, M, L - B)
    assert ((t.max(1) != t.min(1)).any(1)).all()   # the members of every station part ways


def _sky_case():
    """a morning in June at 59-70 N: stations with sky views 0 .. 1 and local horizons, members with their own weather"""
    S, M, L, B = 12, 4, 481, 240
    rs = np.random.RandomState(71)
    st = oh.synth_forcing(S, L, seed=71, start_hour=8)
    tl_full = oh.synth_forcing(S * M, L, seed=72, point_offset=1000, start_hour=8)
    for f in (st, tl_full):
        f.update(oh.time_axis(L, 30.0, (2024, 6, 20, 8, 0, 0)))
        n = f["tair"].shape[0]
        f["sw"] *= 2.0
        f["sw_dir"] = np.ascontiguousarray(f["sw"] * rs.uniform(0.2, 1.2, (n, 1)))  # some SW_dir > SW: the clamp
        f["lw_net"] = np.ascontiguousarray(-40.0 - 30 * rs.rand(n, L))
    hz = np.ascontiguousarray(np.round(rs.uniform(0, 25, (S, 360)), 1)); hz[::5] = 0.0
    st["local_horizons"] = hz
    tl = {k: np.ascontiguousarray(v[..., B:]) for k, v in tl_full.items()}
    sl = []
    for i in range(S):
        li = abi.default_local(); li.InitLenI = 1
        li.lat = float(rs.uniform(59, 70)); li.lon = float(rs.uniform(19, 31))
        li.sky_view = [0.0, 0.3, 0.75, 0.99, 1.0][i % 5]
        sl.append(li)
    s = abi.default_settings(L); p = abi.default_parameters()
    parent = ensemble.parents(S, M)
    rep = ensemble.replicate(st, tl, parent, B)
    return dict(S=S, M=M, L=L, B=B, stations=st, tails=tl, settings=s, params=p, station_local=sl,
                member_local=None, parent=parent, rep=rep, rep_local=[eh.copy_local(sl[q]) for q in parent])


@pytest.mark.parametrize("recluster", [False, True], ids=["natural", "recluster"])
def test_sky_view_is_the_stations(recluster):
    """A member has its station's sky view, position and local horizons (re-sorted: read through the order row)."""
    from roadsurf_amd import device
    c = _sky_case()
    rep, _ = device.run_points(c["rep"], c["settings"], c["params"], c["rep_local"], chunk=100)
    res = _ens(c, chunk=100, recluster=recluster)
    _same(res, rep, c, f"sky-{recluster}")
    ora = oh.run_oracle(eh.lean_kind(), c["rep"], c["settings"], c["params"], c["rep_local"])[0]
    B = c["B"]
    _compare({k: res["members"][k] for k in oh.F64_OUT}, {k: ora[k][:, B:] for k in oh.F64_OUT}, "sky-members")
    plain = oh.run_oracle("port", c["rep"], c["settings"], c["params"], abi.default_local())[0]
    assert np.abs(plain["tsurf"][:, B:] - ora["tsurf"][:, B:]).max() > 0.5   # the sky view acts behind B


def test_coupled_fp64():
    from roadsurf_amd import device
    c = eh.coupled_case()
    B = c["B"]
    rep, nfail = device.run_points(c["rep"], c["settings"], c["params"], c["member_local"], chunk=128)
    res = _ens(c, chunk=128)
    assert res["failed"] == (0, 0) and nfail == 0
    _same(res, rep, c, "coupled")
    ora = eh.coupled_oracle()
    _compare({k: res["members"][k] for k in oh.F64_OUT}, {k: ora[k][:, B:] for k in oh.F64_OUT}, "coupled-members")
    _compare({k: res["stations"][k] for k in oh.F64_OUT}, {k: ora[k][::c["M"], :B] for k in oh.F64_OUT},
             "coupled-stations")


def test_groups_of_the_member_rows():
    from roadsurf_amd import device
    S, M, L, B = 8, 6, 241, 120
    c = _small_case(S, M, L, B, seed=61)
    spec = groups.GroupSpec(ngroups=S, edges=(-5.0, 0.0, 5.0))
    rep, _ = device.run_points(ensemble.replicate(c["stations"], c["tails"], c["parent"], B), c["settings"], c["params"],
                               c["local"], chunk=64)
    res = _ens(c, chunk=64, groups=(spec, c["parent"]))
    want = groups.reduce_groups(*[rep[k][:, B:] for k in oh.F64_OUT], c["parent"], spec)
    assert res["groups"].shape == (L - B, S, groups.cols(spec))
    assert np.array_equal(res["groups"], want)
    assert (want[:, :, groups.COUNT] == M).all()


def test_refusals_name_their_reason_and_launch_nothing():
    """Every refusal of rs_hip_state_fanout and every ValueError of the runner.  (Two devices: only where two are
    visible.)"""
    import torch
    from roadsurf_amd import device
    s = abi.default_settings(241); p = abi.default_parameters()
    a, b = device.Plan(10, s, p, 0), device.Plan(30, s, p, 0)
    L = a.L
    par = np.zeros(30, np.int32)
    before = b.state().numpy().copy()

    def refused(dst, src, parent, word):
        ptr = None if parent is None else C.c_void_p(parent.ctypes.data)
        assert L.rs_hip_state_fanout(dst, src, ptr) != 0
        assert word in lib.last_error(), lib.last_error()

    refused(None, a._h, par, "null")
    refused(b._h, None, par, "null")
    refused(b._h, a._h, None, "null")
    refused(b._h, b._h, par, "same plan")
    bad = par.copy(); bad[17] = 10; bad[20] = -1
    refused(b._h, a._h, bad, "parent[17] = 10")
    bad[3] = -2
    refused(b._h, a._h, bad, "parent[3] = -2")
    with pytest.raises(RuntimeError, match=r"parent\[3\] = -2"):
        b.fanout_from(a, bad)
    with pytest.raises(ValueError, match="30 integers"):
        b.fanout_from(a, par[:29])
    b.set_precision(32)
    refused(b._h, a._h, par, "precision")
    b.set_precision(64)
    s2 = abi.default_settings(242)
    d = device.Plan(30, s2, p, 0)
    refused(d._h, a._h, par, "RsConstants differ")
    d.close()
    lib.check(L.rs_hip_set_diagnostics(b._h, 1), "rs_hip_set_diagnostics")
    refused(b._h, a._h, par, "diagnostics")
    lib.check(L.rs_hip_set_diagnostics(b._h, 0), "rs_hip_set_diagnostics")
    lib.check(L.rs_hip_set_diagnostics(a._h, 1), "rs_hip_set_diagnostics")
    refused(b._h, a._h, par, "diagnostics")
    lib.check(L.rs_hip_set_diagnostics(a._h, 0), "rs_hip_set_diagnostics")
    if torch.cuda.device_count() > 1:
        e = device.Plan(30, s, p, 1)
        refused(e._h, a._h, par, "different devices")
        e.close()
    assert np.array_equal(b.state().numpy(), before)
    a.close(); b.close()

    # the runner: ValueError before any device work
    c = eh.lean_case()
    for B in (0, c["L"]):
        with pytest.raises(ValueError, match="outside"):
            ensemble.run_ensemble(c["stations"], c["tails"], B, c["settings"], c["params"], c["local"])
    cc = eh.coupled_case()
    late = [eh.copy_local(l) for l in cc["station_local"]]
    late[5].couplingIndexI = cc["B"]
    with pytest.raises(ValueError, match=r"station 5: couplingIndexI \+ 1 = 702 > B = 701"):
        ensemble.run_ensemble(cc["stations"], cc["tails"], cc["B"], cc["settings"], cc["params"], late, None, chunk=128)
    early = [eh.copy_local(l) for l in cc["station_local"]]
    for l in early:
        l.InitLenI = 700
    members = [eh.copy_local(l) for l in cc["member_local"]]
    for l in members:
        l.InitLenI = 700
    with pytest.raises(ValueError, match=r"InitLenI = 700 < B = 701"):
        ensemble.run_ensemble(cc["stations"], cc["tails"], cc["B"], cc["settings"], cc["params"], early, members)
    with pytest.raises(ValueError, match="fp64 only"):
        ensemble.run_ensemble(cc["stations"], cc["tails"], cc["B"], cc["settings"], cc["params"], cc["station_local"],
                              cc["member_local"], precision=32)
