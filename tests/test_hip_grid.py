"""GPU: gridded forcing sources - the gather kernel (rs_hip_gather_nodes) against its definition
(roadsurf_amd/grid.py gather_nodes), and rs_driver_run_grid / rs_driver_expand_grid against the same calls fed per
point with grid.to_raw_source and against the CPU checker.  Everything is compared bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import driver_helpers as dh
import grid_helpers as gh
import oracle_helpers as oh
from roadsurf_amd import abi, device, driver, grid, groups, lib, summary

pytestmark = pytest.mark.gpu
M = -9999.9
GUARD = 777.25
LP_FIELDS = ("tair_relax", "VZ_relax", "RH_relax", "couplingIndexI", "couplingTsurf", "InitLenI")


def _kind(coupled):
    if coupled:
        return "ref_cpl" if os.path.exists(oh.REF_CPL_SO) else "port"
    return "ref" if os.path.exists(oh.REF_SO) else "port"


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _kernel_case(rs, n, st, n_nodes, nrows):
    """fields with NaN, inf, -0.0 and a missing value among the nodes; stencils with exact zeros - some of them on
    bad nodes and on indices out of range - single-node stencils of weight 1.0, and ONE node out of range under a
    non-zero weight (the node just behind the field: the guard column, were it read)"""
    src = rs.uniform(-50.0, 50.0, (nrows, n_nodes))
    special = (np.nan, np.inf, -0.0, M)
    for j, v in enumerate(special):
        if n_nodes > 1 + j:
            src[(j + nrows - 1) % nrows, 1 + j] = v
    node = rs.randint(0, n_nodes, (n, st)).astype(np.int32)
    weight = rs.uniform(0.0, 1.0, (n, st))
    weight[rs.rand(n, st) < 0.3] = 0.0
    for p in range(0, n, 5):                       # weight 1.0 on one node: its bits, whatever they are
        weight[p] = 0.0
        weight[p, p % st] = 1.0
        node[p, p % st] = (p // 5) % n_nodes
    for p in range(2, n, 7):                       # no weight on a node out of range / on the NaN node
        k = p % st
        weight[p, k] = 0.0
        node[p, k] = (n_nodes + 1000, -3, min(1, n_nodes - 1))[(p // 7) % 3]
    if n > 3:
        weight[3] = 0.0                            # no term exists
    q = n // 2
    node[q, q % st] = n_nodes
    weight[q, q % st] = 0.5
    return src, node, weight


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_gather_kernel_equals_the_definition(n):
    s = abi.default_settings(121); p = abi.default_parameters()
    plan = device.Plan(n, s, p, 0)
    dev = plan.device
    rs = np.random.RandomState(1000 + n)
    perm = rs.permutation(n).astype(np.int32)
    order = torch.from_numpy(perm).to(dev)
    side = torch.cuda.Stream(device=dev)
    for st in (1, 2, 4):
        for n_nodes in (1, 7, 12):
            for nrows in (1, 3):
                src, node, weight = _kernel_case(rs, n, st, n_nodes, nrows)
                want = grid.gather_nodes(src, node, weight, -100.0)
                # the case holds what it is there for (on the definition's result)
                assert (want[:, n // 2] == M).all()
                if n >= 63 and n_nodes >= 7:
                    assert (want == M).any() and (want != M).any()
                src_stride, dst_stride = n_nodes + 3, n + 9
                hs = np.full((nrows, src_stride), GUARD); hs[:, :n_nodes] = src
                d_src = torch.from_numpy(hs).to(dev)
                d_node, d_w = torch.from_numpy(node).to(dev), torch.from_numpy(weight).to(dev)
                for how in ("plan order", "kept order", "kept order, side stream"):
                    d_dst = torch.full((nrows, dst_stride), GUARD, dtype=torch.float64, device=dev)
                    if how == "plan order":        # a plan that was never re-sorted: slot = point
                        plan.gather_nodes(d_src, d_node, d_w, d_dst, -100.0, n_nodes=n_nodes)
                        plan.sync()
                        exp = want
                    else:
                        stream = side if how.endswith("side stream") else None
                        if stream is not None:
                            side.wait_stream(torch.cuda.current_stream(dev))
                        plan.gather_nodes(d_src, d_node, d_w, d_dst, -100.0, n_nodes=n_nodes, order=order, stream=stream)
                        plan.sync(); side.synchronize()
                        exp = want[:, perm]
                    got = d_dst.cpu().numpy()
                    assert _same_bits(got[:, :n], exp), (how, st, n_nodes, nrows, np.argwhere(_bits(got[:, :n]) != _bits(exp))[:5])
                    assert (got[:, n:] == GUARD).all(), (how, st, n_nodes, nrows)      # columns >= n unchanged
                assert _same_bits(d_src.cpu().numpy(), hs)
                # the caller's threshold and missing value
                d_dst = torch.full((nrows, dst_stride), GUARD, dtype=torch.float64, device=dev)
                plan.gather_nodes(d_src, d_node, d_w, d_dst, -1e300, missing=-1.0, n_nodes=n_nodes)
                plan.sync()
                assert _same_bits(d_dst.cpu().numpy()[:, :n], grid.gather_nodes(src, node, weight, -1e300, missing=-1.0))
    # refused calls write nothing
    d_dst = torch.full((1, n + 9), GUARD, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="kept one"):
        plan.gather_nodes(d_src[:1], d_node, d_w, d_dst, -100.0, n_nodes=n_nodes, stream=side)
    assert plan.L.rs_hip_gather_nodes(plan._h, C.c_void_p(d_src.data_ptr()), 1, 12, 12, C.c_void_p(d_node.data_ptr()),
                                      C.c_void_p(d_w.data_ptr()), 5, None, -100.0, M, C.c_void_p(d_dst.data_ptr()), n + 9,
                                      None) != 0
    assert "stencil" in lib.last_error()
    assert plan.L.rs_hip_gather_nodes(plan._h, C.c_void_p(d_src.data_ptr()), 1, 12, 11, C.c_void_p(d_node.data_ptr()),
                                      C.c_void_p(d_w.data_ptr()), 4, None, -100.0, M, C.c_void_p(d_dst.data_ptr()), n + 9,
                                      None) != 0
    assert "src_stride" in lib.last_error()
    if n > 1:
        assert plan.L.rs_hip_gather_nodes(plan._h, C.c_void_p(d_src.data_ptr()), 1, 12, 15, C.c_void_p(d_node.data_ptr()),
                                          C.c_void_p(d_w.data_ptr()), 4, None, -100.0, M, C.c_void_p(d_dst.data_ptr()),
                                          n - 1, None) != 0
        assert "dst_stride" in lib.last_error()
    plan.sync()
    assert (d_dst.cpu().numpy() == GUARD).all()
    assert plan.L.rs_hip_grid_max_stencil() == grid.MAX_STENCIL == 4
    plan.close()


def _compare_read_input(g, o, n):
    assert np.array_equal(g["status"], o["status"])
    assert np.array_equal(g["missing_index"], o["missing_index"])
    for k in driver.MERGED_FIELDS:
        assert _same_bits(g["merged"][k], o["merged"][k]), k
    for p in range(n):
        for f in LP_FIELDS:
            assert getattr(g["local"][p], f) == getattr(o["local"][p], f), (p, f)


def test_read_input_with_a_gridded_forecast():
    """The forecast on a 6 x 7 grid (bilinear, a few points nearest-neighbour, a few node values missing) beside
    per-point observations with gaps: what read_input returns - merged series, status, missing index, local
    decisions - equals the checker's and the device's own on grid.to_raw_source of it."""
    n = 150
    src, L, t0, tf = gh.grid_scenario(n, hours=12, seed=23)
    raw = [grid.to_raw_source(src[0]), src[1]]
    for kw in (dict(), dict(use_relaxation=1, use_coupling=1)):
        s = abi.default_settings(L)
        for k, v in kw.items():
            setattr(s, k, v)
        g = driver.read_input(src, s, t0, tf)
        o = dh.oracle_read_input(raw, s, t0, tf)
        r = driver.read_input(raw, s, t0, tf)
        _compare_read_input(g, o, n)
        _compare_read_input(g, r, n)
    rejected = o["status"] != 0
    assert 0 < rejected.sum() < n // 2
    assert rejected[gh.touches(src[0], gh.HOLES[0][2])].all()
    assert (o["merged"]["rhz"] > -100).all(axis=1).sum() > n // 2      # RH completed from the gathered Tdew
    # a gridded observation source too, alone (every source gridded: the points are the stencils')
    obs = grid.GridSource(src[0].times, {k: src[0].fields[k] for k in ("tair", "tdew", "vz", "prec", "sw", "lw")},
                          src[0].node, src[0].weight, True)
    s = abi.default_settings(L); s.use_relaxation = 1
    _compare_read_input(driver.read_input([obs], s, t0, tf), dh.oracle_read_input([grid.to_raw_source(obs)], s, t0, tf), n)


MODES = {"plain": dict(), "relaxation": dict(use_relaxation=1), "coupling": dict(use_relaxation=1, use_coupling=1),
         "skyview": dict(use_relaxation=1)}


@pytest.mark.parametrize("mode", list(MODES))
def test_run_with_a_gridded_forecast(mode, monkeypatch):
    """rs_driver_run_grid: outputs bit-equal to the checker's and to the per-point call on grid.to_raw_source, stepped
    the same way (tiles, raw-series launches); identical in two tiles, from the fan-out and with summaries and groups
    asked for."""
    n = 384
    src, L, t0, tf = gh.grid_scenario(n, hours=12, seed=23)
    raw = [grid.to_raw_source(src[0]), src[1]]
    s = abi.default_settings(L); s.outputStep = 20
    for k, v in MODES[mode].items():
        setattr(s, k, v)
    p = abi.default_parameters()
    local, hz = None, None
    if mode == "skyview":
        rs = np.random.RandomState(3)
        local = []
        for i in range(n):
            lp = abi.default_local()
            lp.lat, lp.lon = 60.0 + rs.uniform(0, 8), 21.0 + rs.uniform(0, 8)
            lp.sky_view = float(rs.uniform(0.3, 1.0)) if i % 3 else 1.0
            local.append(lp)
        hz = rs.uniform(0, 25, (n, 360))
    L_ = driver._bind(lib.load())
    o = dh.oracle_run(_kind(mode == "coupling"), raw, s, p, t0, tf, local=local, horizons=hz)
    r = driver.run(raw, s, p, t0, tf, local=local, horizons=hz)
    how_raw = (L_.rs_driver_last_tiles(), L_.rs_driver_last_raw_launches())
    g = driver.run(src, s, p, t0, tf, local=local, horizons=hz)
    assert (L_.rs_driver_last_tiles(), L_.rs_driver_last_raw_launches()) == how_raw
    rejected = o["status"] != 0
    assert 0 < rejected.sum() < n // 2 and rejected[gh.touches(src[0], gh.HOLES[0][2])].all()

    def same(a, what):
        assert np.array_equal(a["status"], o["status"]) and np.array_equal(a["missing_index"], o["missing_index"]), what
        for k in driver.OUT_FIELDS:
            assert _same_bits(a[k], o[k]) and _same_bits(a[k], r[k]), (what, k)
        for q in range(n):
            for f in LP_FIELDS:
                assert getattr(a["local"][q], f) == getattr(o["local"][q], f) == getattr(r["local"][q], f), (what, q, f)
    same(g, "one tile")
    assert (g["tsurf"][rejected] == -9999.0).all() and (g["tsurf"][~rejected] > -100).all()

    same(driver.run(src, s, p, t0, tf, local=local, horizons=hz, device=-1), "fan-out")

    monkeypatch.setenv("ROADSURF_HIP_TILE_POINTS", "200")
    same(driver.run(src, s, p, t0, tf, local=local, horizons=hz), "two tiles")
    assert L_.rs_driver_last_tiles() == 2
    monkeypatch.delenv("ROADSURF_HIP_TILE_POINTS")

    first, last = driver.forecast_rows(s, t0, tf)
    th = summary.SummarySpec(0.0, (0.0,) * 5)
    gspec = groups.GroupSpec(th, 4, (-2.0, 0.0, 2.0))
    gid = np.random.RandomState(4).randint(0, 4, n).astype(np.int32)
    kw = dict(summary=th, summary_rows=(first, last), groups=gspec, group_of=gid, group_rows=(first, last))
    both = driver.run(src, s, p, t0, tf, local=local, horizons=hz, **kw)
    same(both, "with summaries and groups")
    per_point = driver.run(raw, s, p, t0, tf, local=local, horizons=hz, **kw)
    assert _same_bits(both["summary"], per_point["summary"]) and _same_bits(both["groups"], per_point["groups"])
    only = driver.run(src, s, p, t0, tf, local=local, horizons=hz, series=False, **kw)
    assert "tsurf" not in only and _same_bits(only["summary"], both["summary"]) and _same_bits(only["groups"], both["groups"])


def test_refusals(monkeypatch):
    """What a gridded source must be: refused with a message before anything is launched or uploaded."""
    n = 150
    src, L, t0, tf = gh.grid_scenario(n, hours=12, seed=23)
    gs = src[0]
    s = abi.default_settings(L); s.outputStep = 20
    p = abi.default_parameters()
    L_ = driver._bind(lib.load())
    step, n_out = driver.output_rows(s)
    cal = driver.calendar(t0, L, int(s.DTSecs))

    def call(inp, grids):
        """(rc of rs_driver_run_grid, its message, rc of rs_driver_expand_grid, its message); the outputs untouched"""
        out = driver.RsDriverOutput(); out.n_out = n_out
        st = np.full(n, 77, np.int32); mi = np.full(n, 77, np.int32)
        ts = np.full((n, n_out), GUARD)
        out.tsurf = ts.ctypes.data_as(abi.c_double_p)
        out.status = st.ctypes.data_as(abi.c_int32_p); out.missing_index = mi.ctypes.data_as(abi.c_int32_p)
        rc = L_.rs_driver_run_grid(C.byref(inp), grids, C.byref(s), C.byref(p), driver._locals(n, None), C.byref(out),
                                   None, None, 0)
        msg = lib.last_error()
        merged = np.full((len(driver.MERGED_FIELDS), n, L), GUARD)
        rc2 = L_.rs_driver_expand_grid(C.byref(inp), grids, C.byref(s), driver._locals(n, None),
                                       merged.ctypes.data_as(abi.c_double_p), st.ctypes.data_as(abi.c_int32_p),
                                       mi.ctypes.data_as(abi.c_int32_p), 0)
        assert (st == 77).all() and (mi == 77).all() and (ts == GUARD).all() and (merged == GUARD).all()
        return rc, msg, rc2, lib.last_error()

    def refused(inp, grids, word):
        rc, msg, rc2, msg2 = call(inp, grids)
        assert rc != 0 and word in msg, msg
        assert rc2 != 0 and word in msg2, msg2

    # the scenario as it stands is accepted through the same path
    inp, grids, keep = driver.make_grid_input(src, t0, tf, cal)
    # a gridded source with per-point time axes
    tpp = np.ascontiguousarray(np.tile(gs.times, (n, 1)))
    inp.sources[0].times = tpp.ctypes.data_as(driver.c_int64_p)
    inp.sources[0].times_per_point = 1
    refused(inp, grids, "shared")
    # ... with a field pointer in its RsRawSource
    inp, grids, keep = driver.make_grid_input(src, t0, tf, cal)
    stray = np.zeros((n, len(gs.times)))
    inp.sources[0].vz = stray.ctypes.data_as(abi.c_double_p)
    refused(inp, grids, "must be NULL")
    # stencil 0 or 5
    for st in (0, 5):
        inp, grids, keep = driver.make_grid_input(src, t0, tf, cal)
        grids[0].contents.stencil = st
        refused(inp, grids, "stencil %d outside" % st)
    # a weight that is not finite: the first offending point is named
    for bad in (np.nan, np.inf):
        w = gs.weight.copy()
        w[97, 2] = bad
        w[120, 0] = bad
        inp, grids, keep = driver.make_grid_input([grid.GridSource(gs.times, gs.fields, gs.node, w), src[1]], t0, tf, cal)
        refused(inp, grids, "weight 2 of point 97 is not finite")
    # a node out of range under a non-zero weight (on either side); under a zero weight it is none of the library's business
    for node_value in (gs.n_nodes, -1):
        nd = gs.node.copy()
        assert gs.weight[41, 1] != 0.0
        nd[41, 1] = node_value
        nd[99, 0] = node_value
        inp, grids, keep = driver.make_grid_input([grid.GridSource(gs.times, gs.fields, nd, gs.weight), src[1]], t0, tf, cal)
        refused(inp, grids, "node 1 of point 41")
    with pytest.raises(RuntimeError, match="node 1 of point 41"):
        driver.run([grid.GridSource(gs.times, gs.fields, nd, gs.weight), src[1]], s, p, t0, tf)
    # grids NULL, or all entries NULL: rs_driver_run_groups
    raw = [grid.to_raw_source(gs), src[1]]
    inp, keep = driver.make_input(raw, t0, tf, cal)
    ref = driver.run(raw, s, p, t0, tf)
    for grids in (None, (C.POINTER(driver.RsGridSource) * 2)()):
        out = driver.RsDriverOutput(); out.n_out = n_out
        st = np.empty(n, np.int32); mi = np.empty(n, np.int32); ts = np.empty((n, n_out))
        out.tsurf = ts.ctypes.data_as(abi.c_double_p)
        out.status = st.ctypes.data_as(abi.c_int32_p); out.missing_index = mi.ctypes.data_as(abi.c_int32_p)
        assert L_.rs_driver_run_grid(C.byref(inp), grids, C.byref(s), C.byref(p), driver._locals(n, None), C.byref(out),
                                     None, None, 0) == 0, lib.last_error()
        assert _same_bits(ts, ref["tsurf"]) and np.array_equal(st, ref["status"])
