"""Gridded forcing sources: the definition (numpy only, no GPU, no library).

A weather model delivers fields ``[time][y][x]``; the driver path reads one raw series per road point.  What lies
between is a *stencil* per point - up to four nodes of the (flattened) field with one weight each - and
``gather_nodes``, the rule by which a row of node values becomes a row of point values.  Projections stay the
caller's business: the library takes stencils, which also covers masks and unstructured meshes;
``bilinear_stencil`` and ``nearest_stencil`` make them for fractional coordinates of a regular grid.

``GridSource`` is a data source in that form and ``to_raw_source`` the equivalent per-point ``driver.RawSource``: the
device side (``rs_hip_gather_nodes``, ``rs_driver_run_grid``: include/roadsurf.h, roadsurf_amd/csrc/rs_grid.hip) is
held to it bit for bit by the tests.
"""
from __future__ import annotations

import dataclasses

import numpy as np

MAX_STENCIL = 4
MISSING = -9999.9


def present_above(name: str) -> float:
    """The reference's test for "this raw value is there" (rs_raw.hpp raw_threshold; JsonSource.cpp:92-111,
    323-345): ``> -100.0``, for ``lw_net`` ``> -1000.0``."""
    return -1000.0 if name == "lw_net" else -100.0


def _stencil(node, weight):
    node = np.asarray(node, np.int32)
    weight = np.asarray(weight, np.float64)
    if node.ndim == 1:
        node, weight = node[:, None], weight[:, None]
    if node.ndim != 2 or node.shape != weight.shape or not 1 <= node.shape[1] <= MAX_STENCIL:
        raise ValueError(f"node and weight: [n_points][stencil] with 1 <= stencil <= {MAX_STENCIL}")
    return node, weight


def gather_nodes(src, node, weight, present_above: float, missing: float = MISSING) -> np.ndarray:
    """``src`` [nrows][n_nodes] float64, ``node`` / ``weight`` [n_points][stencil] -> [nrows][n_points].

    Per point and row: a term whose weight is exactly 0.0 does not exist - its node is not looked at, whatever it
    holds (NaN, a missing value, an index out of range).  A term's value is present iff it is ``> present_above``
    (NaN is absent).  If any existing term is absent, or its node lies outside [0, n_nodes), or no term exists,
    the result is ``missing``; else ``acc = w0*a0; acc = acc + w1*a1; ...`` over the existing terms in stencil
    order, every product and every sum rounded on its own (no fused multiply-add): one node with weight 1.0 gives
    the node's bits, -0.0 included."""
    src = np.asarray(src, np.float64)
    if src.ndim != 2:
        raise ValueError("src: [nrows][n_nodes]")
    node, weight = _stencil(node, weight)
    nrows, n_nodes = src.shape
    n, st = node.shape
    exists = weight != 0.0
    inside = (node >= 0) & (node < n_nodes)
    bad = (exists & ~inside).any(axis=1) | ~exists.any(axis=1)
    ok = np.broadcast_to(~bad, (nrows, n)).copy()
    acc = np.zeros((nrows, n))
    started = np.zeros(n, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(st):
            use = exists[:, k] & ~bad
            if not use.any():
                continue
            a = src[:, np.where(use, node[:, k], 0)]  # (a point that does not use the term reads node 0: ignored)
            ok &= ~use[None, :] | (a > present_above)
            term = weight[None, :, k] * a
            first = use & ~started
            acc = np.where(first[None, :], term, np.where((use & started)[None, :], acc + term, acc))
            started |= use
    return np.where(ok, acc, missing)


def _cell(x, nx, what):
    x = np.asarray(x, np.float64)
    if x.size and not (np.all(x >= 0.0) and np.all(x <= nx - 1)):
        raise ValueError(f"{what}: fractional grid coordinates in [0, {nx - 1}]")
    i = np.minimum(np.floor(x), nx - 1).astype(np.int64)
    return i, x - i, np.minimum(i + 1, nx - 1)


def bilinear_stencil(x, y, nx: int, ny: int):
    """Fractional grid coordinates ``x`` in [0, nx-1], ``y`` in [0, ny-1] of a row-major ``[ny][nx]`` grid ->
    ``(node [n][4] int32, weight [n][4] float64)``: the four corners of the cell with the weights
    ``(1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx*fy``.  A coordinate on the last row or column has fx (fy) = 0: the
    far corners get weight 0 and are named by the near ones, not by nodes outside the grid."""
    ix, fx, ix1 = _cell(x, nx, "x")
    iy, fy, iy1 = _cell(y, ny, "y")
    node = np.stack([iy * nx + ix, iy * nx + ix1, iy1 * nx + ix, iy1 * nx + ix1], axis=-1).astype(np.int32)
    gx, gy = 1.0 - fx, 1.0 - fy
    weight = np.stack([gx * gy, fx * gy, gx * fy, fx * fy], axis=-1)
    return node.reshape(-1, 4), weight.reshape(-1, 4)


def nearest_stencil(x, y, nx: int, ny: int):
    """The nearest node (halves go up) with weight 1.0: ``(node [n][1], weight [n][1])``."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    ix = np.clip(np.floor(x + 0.5), 0, nx - 1).astype(np.int64)
    iy = np.clip(np.floor(y + 0.5), 0, ny - 1).astype(np.int64)
    node = (iy * nx + ix).astype(np.int32).reshape(-1, 1)
    return node, np.ones(node.shape)


@dataclasses.dataclass
class GridSource:
    """One data source as fields: ``times`` [n_times] epoch seconds shared by all points, ``fields`` name ->
    [n_times][n_nodes] float64 (or [n_times][ny][nx], flattened row-major; absent name = variable not in the
    source), and every point's stencil ``node`` / ``weight`` [n_points][stencil]."""
    times: np.ndarray
    fields: dict
    node: np.ndarray
    weight: np.ndarray
    is_observation: bool = False

    def __post_init__(self):
        self.times = np.ascontiguousarray(self.times, np.int64)
        if self.times.ndim != 1:
            raise ValueError("a gridded source has one time axis shared by all points")
        node, weight = _stencil(self.node, self.weight)
        self.node, self.weight = np.ascontiguousarray(node), np.ascontiguousarray(weight)
        flat = {}
        for name, a in self.fields.items():
            a = np.asarray(a, np.float64)
            if a.ndim < 2 or a.shape[0] != self.times.shape[0]:
                raise ValueError(f"{name}: expected [{self.times.shape[0]}][n_nodes], got {a.shape}")
            flat[name] = np.ascontiguousarray(a.reshape(a.shape[0], -1))
        if len({a.shape[1] for a in flat.values()}) > 1:
            raise ValueError("all fields of a gridded source share its nodes")
        self.fields = flat

    @property
    def n_points(self) -> int:
        return self.node.shape[0]

    @property
    def n_nodes(self) -> int:
        return next(iter(self.fields.values())).shape[1] if self.fields else 0


def to_raw_source(gs: GridSource):
    """The per-point ``driver.RawSource`` a gridded source stands for: every field gathered with the reference's
    presence rule and laid out [n_points][n_times]."""
    from . import driver

    fields = {name: np.ascontiguousarray(gather_nodes(a, gs.node, gs.weight, present_above(name)).T)
              for name, a in gs.fields.items()}
    return driver.RawSource(gs.times, fields, gs.is_observation)
