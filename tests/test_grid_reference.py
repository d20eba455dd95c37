"""CPU: the definition of gridded sources (roadsurf_amd/grid.py) - gather_nodes by hand on a 3 x 4 grid, the
stencil makers, the presence thresholds, to_raw_source through the checker - and the conditions of the scenario the
GPU tests (tests/test_hip_grid.py) compare on."""
import math

import numpy as np
import pytest

import driver_helpers as dh
import grid_helpers as gh
from roadsurf_amd import abi, driver, grid

M = -9999.9
NX, NY = 4, 3


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _field():
    """two rows of a 3 x 4 grid: node k holds 10 + k (row 0) and 100 + k (row 1), but node 5 NaN, node 6 missing,
    node 7 -0.0 and node 8 inf in row 0"""
    a = np.stack([10.0 + np.arange(12), 100.0 + np.arange(12)])
    a[0, 5], a[0, 6], a[0, 7], a[0, 8] = np.nan, M, -0.0, np.inf
    return a


def test_gather_nodes_by_hand():
    a = _field()
    node = np.array([[0, 1], [2, 3], [1, 5], [1, 6], [1, 12], [1, -1], [5, 6]], np.int32)
    weight = np.array([[0.25, 0.75], [0.5, 0.5], [1.0, 0.0], [1.0, 0.0], [1.0, 0.0], [1.0, 0.0], [0.0, 0.0]])
    got = grid.gather_nodes(a, node, weight, -100.0)
    assert got.shape == (2, 7)
    # plain sums, every product and sum rounded on its own
    assert got[0, 0] == 0.25 * 10.0 + 0.75 * 11.0 and got[1, 0] == 0.25 * 100.0 + 0.75 * 101.0
    assert got[0, 1] == 0.5 * 12.0 + 0.5 * 13.0
    # a zero weight hides a NaN node, a missing node and nodes out of range on either side
    assert (got[:, 2:6] == a[:, [1]]).all()
    # no term exists
    assert (got[:, 6] == M).all()
    # a non-zero weight on each of them gives missing - in the row where the node is bad, for a node out of range in all
    weight[2:6, 1] = 1e-300
    got = grid.gather_nodes(a, node, weight, -100.0)
    assert got[0, 2] == M and got[0, 3] == M and (got[:, 4] == M).all() and (got[:, 5] == M).all()
    assert got[1, 2] == 101.0 + 1e-300 * 105.0 and got[1, 3] == 101.0 + 1e-300 * 106.0
    # the caller's missing value
    assert (grid.gather_nodes(a, node, weight, -100.0, missing=-1.0)[:, 4] == -1.0).all()


def test_rounding_is_per_operation():
    """no fused multiply-add: w0*a0 is rounded before w1*a1 is added (an FMA would keep the exact product)"""
    w0, a0 = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30          # exact product 1 + 2^-29 + 2^-60: the last term is lost
    src = np.array([[a0, -1.0]])
    got = grid.gather_nodes(src, np.array([[1, 0]], np.int32), np.array([[1.0 + 2.0 ** -29, w0]]), -100.0)
    assert got[0, 0] == -(1.0 + 2.0 ** -29) + (w0 * a0) == 0.0           # fused: 2^-60


def test_nearest_stencil_returns_node_bits():
    a = _field()
    x = np.array([0.0, 1.4, 2.5, 3.0, 0.2])            # nodes 0, 5 (row 1), 7 (row 1), 7, 8 (row 2)
    y = np.array([0.0, 1.0, 0.6, 1.2, 1.6])
    node, weight = grid.nearest_stencil(x, y, NX, NY)
    assert node.dtype == np.int32 and node[:, 0].tolist() == [0, 5, 7, 7, 8] and (weight == 1.0).all()
    got = grid.gather_nodes(a, node, weight, -100.0)
    assert _bits(got[0, 2]) == _bits(-0.0) and _bits(got[0, 3]) == _bits(-0.0)      # -0.0 stays -0.0
    assert got[0, 4] == np.inf and got[0, 1] == M                                   # inf is a value, NaN absent
    assert np.array_equal(_bits(got[1]), _bits(a[1, node[:, 0]]))


def test_bilinear_stencil():
    rs = np.random.RandomState(5)
    x = np.concatenate([rs.uniform(0, NX - 1, 500), [0.0, NX - 1, NX - 1, 1.0, 2.0 - 2.0 ** -52]])
    y = np.concatenate([rs.uniform(0, NY - 1, 500), [0.0, NY - 1, 0.5, NY - 1, 1.0]])
    node, weight = grid.bilinear_stencil(x, y, NX, NY)
    assert node.shape == weight.shape == (505, 4) and node.dtype == np.int32
    # last row and column stay in range, and what would lie outside has no weight
    assert node.min() >= 0 and node.max() < NX * NY
    assert (weight[x == NX - 1][:, [1, 3]] == 0.0).all() and (weight[y == NY - 1][:, [2, 3]] == 0.0).all()
    assert (weight >= 0.0).all()
    # The weights sum to 1 within 1 ulp.  The sum itself is formed exactly (fsum, one rounding), so what is bounded
    # is the weights' own error: 1 - f is exact or off by at most 2^-54 (f in [0, 1)), so (gx + fx)(gy + fy) lies
    # within 2^-53 of 1; each product is off by at most half an ulp of itself, <= 2^-53 times itself, and the four
    # add up to ~1: together at most 2^-52 = 1 ulp of 1.0, which the one rounding of the sum cannot pass.
    for w in weight:
        assert abs(math.fsum(w) - 1.0) <= 2.0 ** -52, w
    # on nodes it reproduces node values exactly
    a = _field()[1]
    jx, jy = np.meshgrid(np.arange(NX), np.arange(NY))
    node, weight = grid.bilinear_stencil(jx.ravel().astype(float), jy.ravel().astype(float), NX, NY)
    assert np.array_equal(_bits(grid.gather_nodes(a[None, :], node, weight, -100.0)[0]), _bits(a))
    # the four corners in the documented order, row-major [ny][nx]
    node, weight = grid.bilinear_stencil([1.25], [0.5], NX, NY)
    assert node[0].tolist() == [1, 2, 5, 6] and weight[0].tolist() == [0.375, 0.125, 0.375, 0.125]
    with pytest.raises(ValueError):
        grid.bilinear_stencil([NX - 0.5], [0.0], NX, NY)


def test_presence_thresholds_of_to_raw_source():
    """a value at or below the threshold is missing; lw_net has its own"""
    assert grid.present_above("lw_net") == -1000.0
    assert all(grid.present_above(k) == -100.0 for k in driver.RAW_FIELDS if k != "lw_net")
    times = np.array([0, 3600], np.int64)
    vals = np.array([[-100.0, np.nextafter(-100.0, 0.0), -500.0, -1000.0, np.nextafter(-1000.0, 0.0)]] * 2)
    node, weight = np.arange(5, dtype=np.int32)[:, None], np.ones((5, 1))
    raw = grid.to_raw_source(grid.GridSource(times, {"tair": vals, "lw_net": vals}, node, weight))
    assert raw.fields["tair"][:, 0].tolist() == [M, vals[0, 1], M, M, M]
    assert raw.fields["lw_net"][:, 0].tolist() == [-100.0, vals[0, 1], -500.0, M, vals[0, 4]]
    assert raw.fields["tair"].shape == (5, 2) and raw.fields["tair"].flags.c_contiguous


def test_grid_source_takes_fields_as_the_model_delivers_them():
    t = np.array([0, 3600, 7200], np.int64)
    f3 = np.arange(3 * NY * NX, dtype=np.float64).reshape(3, NY, NX)
    node, weight = grid.nearest_stencil([3.0, 0.0], [2.0, 1.0], NX, NY)
    gs = grid.GridSource(t, {"tair": f3}, node, weight)
    assert gs.n_nodes == 12 and gs.n_points == 2 and gs.fields["tair"].shape == (3, 12)
    assert grid.to_raw_source(gs).fields["tair"].tolist() == [[11.0, 23.0, 35.0], [4.0, 16.0, 28.0]]
    with pytest.raises(ValueError):
        grid.GridSource(np.zeros((2, 3), np.int64), {}, node, weight)          # per-point time axes
    with pytest.raises(ValueError):
        grid.GridSource(t, {"tair": f3}, np.zeros((2, 5), np.int32), np.zeros((2, 5)))


def test_scenario_through_the_checker():
    """to_raw_source through the existing checker (its shape and layout), and the conditions that keep the GPU
    comparison from passing vacuously: some points rejected, fewer than half, some because a node is missing."""
    n = 150
    src, L, t0, tf = gh.grid_scenario(n, hours=12, seed=23)
    gs = src[0]
    raw = grid.to_raw_source(gs)
    assert isinstance(raw, driver.RawSource) and set(raw.fields) == set(gs.fields)
    for k, a in raw.fields.items():
        assert a.shape == (n, len(gs.times)) and a.dtype == np.float64 and a.flags.c_contiguous, k
    s = abi.default_settings(L); s.use_relaxation = 1
    o = dh.oracle_read_input([raw, src[1]], s, t0, tf)
    rejected = o["status"] != 0
    assert 0 < rejected.sum() < n // 2
    # sw is in no observation: the forecast's raw times inside the simulation are copied (JsonSource.cpp:86-91)
    inside = [k for k, t in enumerate(gs.times) if t0 <= t < t0 + L * 30]
    assert len(inside) == 13
    for k in inside:
        assert np.array_equal(_bits(o["merged"]["sw"][:, (gs.times[k] - t0) // 30]), _bits(raw.fields["sw"][:, k]))
    # the missing nodes reject exactly the points that reach them with a weight
    for name, rows, node in gh.HOLES:
        hit = gh.touches(gs, node)
        assert hit.any() and not hit.all() and rejected[hit].all(), name
        assert (raw.fields[name][hit][:, list(rows)] == M).all() and (raw.fields[name][~hit] > -100).all()
    status_of = {"sw": 4, "lw": 5, "tair": 1}
    assert {int(x) for x in o["status"][gh.touches(gs, gh.HOLES[0][2])]} <= {status_of[h[0]] for h in gh.HOLES}
    # nearest-neighbour points, points on the last row and column
    assert all((gs.weight[p] == (1.0, 0.0, 0.0, 0.0)).all() for p in gh.NEAREST)
    assert gs.node[list(gh.NEAREST), 1:].min() < 0 and gs.node[list(gh.NEAREST), 1:].max() >= gs.n_nodes
    assert (gs.weight[[1, 2, 4]] == 0.0).any(axis=1).all()
    # the driver binding: a gridded source's RsRawSource carries the time axis alone
    inp, grids, keep = driver.make_grid_input(src, t0, tf)
    assert inp.n_points == n and inp.n_sources == 2 and bool(grids[0]) and not bool(grids[1])
    assert inp.sources[0].n_times == len(gs.times) and not inp.sources[0].tair and not inp.sources[0].times_per_point
    g0 = grids[0].contents
    assert (g0.n_nodes, g0.stencil) == (42, 4) and bool(g0.tair) and not bool(g0.rhz)
    plain, none, _ = driver.make_grid_input([raw, src[1]], t0, tf)
    assert none is None and plain.n_points == n
