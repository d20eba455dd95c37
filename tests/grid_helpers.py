"""The gridded-source scenario shared by tests/test_grid_reference.py (CPU: its conditions, with the checker alone)
and tests/test_hip_grid.py (GPU): driver_helpers.scenario's two sources with the forecast delivered as fields."""
from __future__ import annotations

import numpy as np

import driver_helpers as dh
import oracle_helpers as oh
from roadsurf_amd import grid

NX, NY = 7, 6
#: (field, raw time indices, node): values the model did not deliver.  sw and lw are mandatory and in no
#: observation; the air temperature's hole lies behind the last observation
HOLES = (("sw", (4, 5), 16), ("lw", (9,), 30), ("tair", (10,), 3))
NEAREST = (0, 7, 20)          # points that take the nearest node instead of the bilinear four


def grid_scenario(n, hours=12, seed=7, obs_hours=6):
    """(sources, L, start, forecast_time): sources[0] the hourly forecast on a 6 x 7 grid (no RH: Tdew only) with
    the points scattered over it - bilinear stencils, a few points nearest-neighbour, a few exactly on nodes and on
    the last row and column - and a few node values missing; sources[1] the per-point observations with gaps of
    driver_helpers.scenario."""
    src, L, t0, tf = dh.scenario(n, hours=hours, seed=seed, obs_hours=obs_hours)
    fc_t = np.asarray(src[0].times, np.int64)
    f = oh.synth_forcing(NX * NY, (hours + 2) * 120 + 1, seed=seed + 100)
    fc_idx = np.arange(0, (hours + 2) * 120 + 1, 120)
    fields = {k: np.ascontiguousarray(f[k][:, fc_idx].T).reshape(len(fc_idx), NY, NX)
              for k in ("tair", "tdew", "vz", "prec", "sw", "lw", "sw_dir", "lw_net")}
    for name, rows, node in HOLES:
        for r in rows:
            fields[name].reshape(len(fc_idx), -1)[r, node] = -9999.9
    rs = np.random.RandomState(seed)
    x, y = rs.uniform(0, NX - 1, n), rs.uniform(0, NY - 1, n)
    x[1], y[2] = NX - 1, NY - 1            # last column, last row
    x[3], y[3] = 2.0, 3.0                  # on a node
    x[4], y[4] = NX - 1, NY - 1            # the last node
    node, weight = grid.bilinear_stencil(x, y, NX, NY)
    nn, _ = grid.nearest_stencil(x, y, NX, NY)
    for p in NEAREST:
        node[p] = (nn[p, 0], -5, NX * NY, 0)     # the three terms without weight name no usable node
        weight[p] = (1.0, 0.0, 0.0, 0.0)
    gs = grid.GridSource(fc_t, fields, node, weight, False)
    return [gs, src[1]], L, t0, tf


def touches(gs, node):
    """points whose stencil reaches `node` with a non-zero weight"""
    return ((gs.node == node) & (gs.weight != 0.0)).any(axis=1)
