"""Device-resident driver of the HIP path (layer 1 of ``include/roadsurf.h``).

PyTorch is plumbing here: it owns the HBM buffers (``torch.empty`` on the
``cuda`` device), the stream and, in ``bench.py``, ``torch.distributed``.  All
arithmetic happens in ``libroadsurf_hip.so``; tensors cross the boundary as raw
device pointers.

Layouts (points are the fastest axis, see ``include/roadsurf.h``)::

    forcing / outputs   tensor[t, p]   shape [nsteps, npoints_padded]
    per-point params    tensor[p]
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import torch

from . import abi, lib

F64_FORCING = ("tair", "tdew", "vz", "rhz", "prec", "sw", "lw", "tsurfobs", "depth")
OUT_FIELDS = ("tsurf", "snow", "water", "ice", "deposit", "ice2")


def _ptr(t):  # a tensor's device pointer; None (an optional array, the plan's own order row) stays None
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream_ptr(stream):  # a stream of the caller's; None: the plan's
    return None if stream is None else C.c_void_p(stream.cuda_stream)


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise RuntimeError("roadsurf_amd needs a HIP device (torch.cuda.is_available() is False); "
                           "there is no CPU path")


@dataclass
class ForcingWindow:
    """Step-resolution forcing for ``nsteps`` consecutive time indices on the device."""
    nsteps: int
    t_stride: int
    tensors: dict = field(default_factory=dict)  # name -> torch tensor or None
    hour_per_point: bool = False

    @classmethod
    def empty(cls, nsteps: int, np_pad: int, device, optional=("tdew", "tsurfobs", "depth"),
              dtype=torch.float64):
        t = {}
        for n in F64_FORCING:
            if n in ("tdew", "tsurfobs", "depth") and n not in optional:
                t[n] = None
            else:
                t[n] = torch.empty((nsteps, np_pad), dtype=dtype, device=device)
        t["precphase"] = torch.empty((nsteps, np_pad), dtype=torch.int32, device=device)
        t["hour"] = torch.empty((nsteps,), dtype=torch.int32, device=device)
        return cls(nsteps, np_pad, t)

    def struct(self, row: int = 0) -> lib.RsForcing:
        f = lib.RsForcing()
        for n in F64_FORCING + ("precphase",):
            t = self.tensors.get(n)
            setattr(f, n, None if t is None else C.c_void_p(t[row].data_ptr()))
        h = self.tensors["hour"]
        f.hour = C.c_void_p(h[row].data_ptr())
        f.t_stride = self.t_stride
        f.hour_pstride = 1 if self.hour_per_point else 0
        for n in ("sw_dir", "lw_net"):
            t = self.tensors.get(n)
            setattr(f, n, None if t is None else C.c_void_p(t[row].data_ptr()))
        sun = self.tensors.get("sun")  # [nsteps, RS_SUN_COLS = 6]
        f.sun = None if sun is None else C.c_void_p(sun[row].data_ptr())
        return f


@dataclass
class OutputWindow:
    nrows: int
    t_stride: int
    tensors: dict
    decimate: int = 1

    @classmethod
    def empty(cls, nrows: int, np_pad: int, device, decimate: int = 1, dtype=torch.float64):
        # rows the simulation never saves read -9999.0, as in the reference (OutputData.cpp:5-13)
        t = {n: torch.full((nrows, np_pad), -9999.0, dtype=dtype, device=device) for n in OUT_FIELDS}
        return cls(nrows, np_pad, t, decimate)

    def struct(self, row0: int) -> lib.RsOutputs:
        o = lib.RsOutputs()
        for n in OUT_FIELDS:
            setattr(o, n, C.c_void_p(self.tensors[n].data_ptr()))
        o.t_stride = self.t_stride
        o.decimate = self.decimate
        o.row0 = row0
        return o

    def struct_at(self, t0: int, out_row0: int | None = None) -> lib.RsOutputs:
        """For a launch at time index ``t0``: its first output row is the window's row 0, unless ``out_row0`` says
        which absolute row that is."""
        return self.struct((t0 - 1 + self.decimate - 1) // self.decimate if out_row0 is None else out_row0)

    def struct_from(self, row: int) -> lib.RsOutputs:
        """The window from its row ``row`` on (what the consumers of output rows read)."""
        o = self.struct(0)
        for n in OUT_FIELDS:
            setattr(o, n, C.c_void_p(self.tensors[n][row].data_ptr()))
        return o


class Plan:
    """RAII wrapper of ``RsPlan``: one shard of points on one GPU, one stream."""

    def __init__(self, npoints: int, settings: abi.InputSettings, params: abi.InputParameters,
                 device: int | None = None, stream: torch.cuda.Stream | None = None):
        require_gpu()
        self.L = lib.load()
        self.device_index = torch.cuda.current_device() if device is None else device
        self.device = torch.device("cuda", self.device_index)
        self.stream = stream or torch.cuda.current_stream(self.device)
        self.settings, self.params = settings, params
        self.consts = lib.build_constants(settings, params)
        self.npoints = npoints
        self._h = self.L.rs_hip_plan_create(self.device_index, npoints, C.byref(self.consts),
                                            C.c_void_p(self.stream.cuda_stream))
        if not self._h:
            raise RuntimeError("rs_hip_plan_create failed: " + lib.last_error())
        self.np_pad = int(self.L.rs_hip_plan_npoints_padded(self._h))
        self._pp_keep = None

    def close(self):
        if getattr(self, "_h", None):
            self.L.rs_hip_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    # -- per-point parameters -------------------------------------------------
    def point_params(self, tbottom, initlen=None, tair_relax=None, vz_relax=None, rh_relax=None,
                     coupling_index=None, coupling_tsurf=None, sky=None):
        """tbottom: float (uniform) or tensor[np_pad]; others tensors or None."""
        if not torch.is_tensor(tbottom):
            tbottom = torch.full((self.np_pad,), float(tbottom), dtype=torch.float64,
                                 device=self.device)
        keep = (tbottom, initlen, tair_relax, vz_relax, rh_relax, coupling_index, coupling_tsurf)
        pp = lib.RsPointParams()
        pp.tbottom = _ptr(tbottom)
        pp.initlen = _ptr(initlen)
        pp.tair_relax = _ptr(tair_relax)
        pp.vz_relax = _ptr(vz_relax)
        pp.rh_relax = _ptr(rh_relax)
        pp.coupling_index = _ptr(coupling_index)
        pp.coupling_tsurf = _ptr(coupling_tsurf)
        if sky is not None:  # dict: sky_view, sin_lat, cos_lat, lon_rad, horizons (tensors)
            pp.sky_view = _ptr(sky["sky_view"]); pp.sin_lat = _ptr(sky["sin_lat"])
            pp.cos_lat = _ptr(sky["cos_lat"]); pp.lon_rad = _ptr(sky["lon_rad"])
            pp.horizons = _ptr(sky.get("horizons"))
            pp.horizon_index = _ptr(sky.get("horizon_index"))  # int32[np_pad]: column of slot s (plan order)
            pp.albedo_surroundings = float(self.params.Albedo_surroundings)
            keep = keep + (sky,)
        self._pp_keep = keep
        return pp

    def uniform_tbottom(self, year=2024, month=1, day=10) -> float:
        return lib.bottom_temperature(self.params, self.consts, year, month, day)

    # -- kernels ----------------------------------------------------------------
    def init_state(self, window: ForcingWindow, pp) -> None:
        f = window.struct(0)
        lib.check(self.L.rs_hip_init_state(self._h, C.byref(f), C.byref(pp)), "rs_hip_init_state")

    def step(self, window: ForcingWindow, out: OutputWindow, pp, t0: int, nsteps: int,
             window_row: int = 0, out_row0: int | None = None) -> None:
        f = window.struct(window_row)
        o = out.struct_at(t0, out_row0)
        lib.check(self.L.rs_hip_step(self._h, C.byref(f), C.byref(o), C.byref(pp), t0, nsteps),
                  "rs_hip_step")

    def step_knots(self, spec, knots: torch.Tensor, out: OutputWindow, pp, t0: int, nsteps: int,
                   out_row0: int | None = None) -> None:
        """expand_ordered + step in one launch without a forcing window (rs_hip_step_knots: the
        two-wavefront flavour's ground wave interpolates the forcing from the knots)."""
        o = out.struct_at(t0, out_row0)
        lib.check(self.L.rs_hip_step_knots(self._h, C.byref(spec), C.c_void_p(knots.data_ptr()), 0, knots.shape[0],
                                           C.byref(o), C.byref(pp), t0, nsteps), "rs_hip_step_knots")

    def step_cpl(self, window: ForcingWindow, out: OutputWindow, pp, t0: int, nsteps: int,
                 window_row: int = 0, out_row0: int | None = None) -> None:
        """A chunk of a coupled run in lock step (rs_hip_step_cpl): no replays, points park."""
        f = window.struct(window_row)
        o = out.struct_at(t0, out_row0)
        lib.check(self.L.rs_hip_step_cpl(self._h, C.byref(f), C.byref(o), C.byref(pp), t0, nsteps),
                  "rs_hip_step_cpl")

    def cpl_replay(self, window: ForcingWindow, out: OutputWindow, pp, t0: int, nsteps: int,
                   window_row: int = 0, out_row0: int | None = None) -> int:
        """The replay rounds of the parked points over [t0, t0+nsteps) (rs_hip_cpl_replay)."""
        f = window.struct(window_row)
        o = out.struct_at(t0, out_row0)
        rounds = C.c_int32(0)
        lib.check(self.L.rs_hip_cpl_replay(self._h, C.byref(f), C.byref(o), C.byref(pp), t0, nsteps,
                                           C.byref(rounds)), "rs_hip_cpl_replay")
        return int(rounds.value)

    def set_precision(self, bits: int) -> None:
        """32: fp32 flavour (LEAN features, float windows); 64: the parity path."""
        lib.check(self.L.rs_hip_set_precision(self._h, bits), "rs_hip_set_precision")

    def set_history_score(self, on: bool) -> None:
        lib.check(self.L.rs_hip_set_history_score(self._h, 1 if on else 0), "rs_hip_set_history_score")

    def coupling_windows_closed(self, closed: bool = True) -> None:
        """Every coupling window (replays included) is behind the plan: re-sorts move the coupling
        scalars only (rs_hip_coupling_windows_closed)."""
        lib.check(self.L.rs_hip_coupling_windows_closed(self._h, 1 if closed else 0),
                  "rs_hip_coupling_windows_closed")

    def set_variant(self, v: int) -> None:
        lib.check(self.L.rs_hip_set_variant(self._h, v), "rs_hip_set_variant")
        self.variant = v

    def sync(self) -> None:
        lib.check(self.L.rs_hip_sync(self._h), "rs_hip_sync")

    def failed_count(self) -> int:
        return int(self.L.rs_hip_failed_count(self._h))

    def first_failed_index(self):
        """numpy int32[npoints]: 0, or the 1-based index at which the point's run was failed."""
        import numpy as np
        out = np.zeros(self.npoints, np.int32)
        lib.check(self.L.rs_hip_first_failed_index(self._h, C.c_void_p(out.ctypes.data)),
                  "rs_hip_first_failed_index")
        return out

    def timing_reset(self) -> None:
        self.L.rs_hip_timing_reset(self._h)

    def timing_step_ms(self):
        n = C.c_int32(0)
        ms = self.L.rs_hip_timing_step_ms(self._h, C.byref(n))
        return float(ms), int(n.value)

    def timing_intervals(self, ref_event: torch.cuda.Event):
        """[(start_ms, stop_ms)] of the step launches since timing_reset(), after ref_event."""
        import numpy as np
        cap = 65536
        a = np.zeros(cap); b = np.zeros(cap)
        n = self.L.rs_hip_timing_intervals(self._h, C.c_void_p(ref_event.cuda_event), C.c_void_p(a.ctypes.data),
                                           C.c_void_p(b.ctypes.data), cap)
        if n < 0:
            raise RuntimeError("rs_hip_timing_intervals failed: " + lib.last_error())
        return list(zip(a[:n].tolist(), b[:n].tolist()))

    def state(self) -> torch.Tensor:
        """Carried state block as a host tensor [RS_NSTATE, np_pad]."""
        nb = self.L.rs_hip_plan_state_bytes(self._h)
        t = torch.empty((nb // 8 // self.np_pad, self.np_pad), dtype=torch.float64)
        lib.check(self.L.rs_hip_state_download(self._h, C.c_void_p(t.data_ptr()), nb),
                  "rs_hip_state_download")
        return t

    def load_state(self, t: torch.Tensor) -> None:
        t = t.contiguous()
        lib.check(self.L.rs_hip_state_upload(self._h, C.c_void_p(t.data_ptr()), t.numel() * 8),
                  "rs_hip_state_upload")

    def fanout_from(self, src: "Plan", parent) -> None:
        """Point p of this plan takes the carried state of point ``parent[p]`` of ``src``, on the device, whatever
        order the slots of either plan are in (rs_hip_state_fanout; roadsurf_amd/ensemble.py is the definition).
        ``parent``: int32 numpy array or CPU tensor of ``npoints`` entries, every one a point of ``src`` - the
        library checks them before anything is launched.  Asynchronous: on this plan's stream, behind ``src``'s."""
        import numpy as np
        if not hasattr(self.L, "rs_hip_state_fanout"):
            raise RuntimeError("this libroadsurf_hip.so has no state fan-out (rs_hip_state_fanout)")
        if not isinstance(src, Plan) or not src._h or not self._h:
            raise RuntimeError("rs_hip_state_fanout: null argument (dst, src and parent are required)")
        if parent is None:
            raise RuntimeError("rs_hip_state_fanout: null argument (dst, src and parent are required)")
        if torch.is_tensor(parent):
            if parent.is_cuda:
                raise ValueError("fanout_from: parent is a HOST array (numpy or a CPU tensor)")
            parent = parent.numpy()
        par = np.asarray(parent)
        if par.dtype.kind not in "iu" or par.shape != (self.npoints,):
            raise ValueError(f"fanout_from: parent must be {self.npoints} integers, one per point of this plan")
        if par.size and (par.min() < -2**31 or par.max() >= 2**31):
            raise ValueError("fanout_from: parent does not fit int32")
        par = np.ascontiguousarray(par, dtype=np.int32)
        lib.check(self.L.rs_hip_state_fanout(self._h, src._h, C.c_void_p(par.ctypes.data)), "rs_hip_state_fanout")

    # -- synthetic workload -----------------------------------------------------
    def synth_knots(self, seed: int, nknots: int, point_offset: int = 0, steps_per_knot: int = 120,
                    start_hour: int = 0):
        spec = lib.RsSynthSpec(seed, point_offset, steps_per_knot, start_hour)
        knots = torch.empty((nknots, lib.RS_KNOT_FIELDS, self.np_pad), dtype=torch.float64,
                            device=self.device)
        lib.check(self.L.rs_hip_synth_knots(self._h, C.byref(spec), C.c_void_p(knots.data_ptr()),
                                            0, nknots), "rs_hip_synth_knots")
        return spec, knots

    # -- plan order (rs_hip_recluster) ---------------------------------------------
    def order(self) -> torch.Tensor:
        """Zero-copy view of the plan's slot -> local point array (int32 [np_pad]).  Valid until
        the next recluster(): clone it to keep the order a window was produced in."""
        ptr = self.L.rs_hip_plan_order(self._h)
        if not ptr:
            raise RuntimeError("rs_hip_plan_order failed: " + lib.last_error())

        class _View:
            __cuda_array_interface__ = {"shape": (self.np_pad,), "typestr": "<i4",
                                        "data": (int(ptr), False), "version": 2}
        return torch.as_tensor(_View(), device=self.device)

    def copy_order_to(self, dst: torch.Tensor) -> None:
        """Keep the order the last launch was stepped in: dst int32[np_pad] on this device
        (asynchronous on the plan's stream; call before recluster())."""
        assert dst.dtype == torch.int32 and dst.numel() == self.np_pad and dst.is_contiguous()
        lib.check(self.L.rs_hip_plan_order_copy(self._h, C.c_void_p(dst.data_ptr())),
                  "rs_hip_plan_order_copy")

    def outputs_by_point(self, out: "OutputWindow", nrows: int, dst: dict, dst_row0: int = 0, order=None,
                         stream: torch.cuda.Stream | None = None) -> None:
        """The first ``nrows`` rows of the output window, [row][slot], into point-major tensors
        ``dst[name][npoints, dst_rows]`` at columns ``dst_row0 ...`` (rs_hip_outputs_by_point); ``order``: a kept
        order row, default the plan's current order (call between the launch and the next re-sort)."""
        o = out.struct(0)
        rows = next(iter(dst.values())).shape[1]
        ptrs = (C.c_void_p * 6)(*[dst[n].data_ptr() for n in OUT_FIELDS])
        lib.check(self.L.rs_hip_outputs_by_point(self._h, C.byref(o), int(nrows), _ptr(order), ptrs, C.c_int64(rows),
                                                 C.c_int64(dst_row0), _stream_ptr(stream)), "rs_hip_outputs_by_point")

    def summary_reset(self, acc: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """The empty summary into every column of ``acc``, float64 [RS_SUM_COLS, np_pad] on this device (made
        here if None) - what ``outputs_summary`` accumulates into (rs_hip_summary_reset)."""
        if acc is None:
            acc = torch.empty((lib.RS_SUM_COLS, self.np_pad), dtype=torch.float64, device=self.device)
        assert acc.dtype == torch.float64 and acc.shape == (lib.RS_SUM_COLS, self.np_pad) and acc.is_contiguous()
        lib.check(self.L.rs_hip_summary_reset(self._h, C.c_void_p(acc.data_ptr()), _stream_ptr(stream)),
                  "rs_hip_summary_reset")
        return acc

    def outputs_summary(self, out: "OutputWindow", nrows: int, index0: int, index_step: int, spec, acc: torch.Tensor,
                        order=None, stream: torch.cuda.Stream | None = None, row: int = 0) -> None:
        """Rows ``row .. row + nrows - 1`` of the output window, [row][slot], merged into the per-point summaries
        ``acc`` [RS_SUM_COLS, np_pad] in POINT order (rs_hip_outputs_summary; roadsurf_amd/summary.py defines the
        columns).  The first of these rows is the absolute 1-based time index ``index0``, the next ``index0 +
        index_step``; ``spec``: summary.SummarySpec; ``order`` and ``stream`` as for ``outputs_by_point``."""
        assert acc.dtype == torch.float64 and acc.shape == (lib.RS_SUM_COLS, self.np_pad) and acc.is_contiguous()
        o = out.struct_from(row)
        sp = lib.summary_spec(spec)
        lib.check(self.L.rs_hip_outputs_summary(self._h, C.byref(o), int(nrows), int(index0), int(index_step), _ptr(order),
                                                C.byref(sp), C.c_void_p(acc.data_ptr()), _stream_ptr(stream)),
                  "rs_hip_outputs_summary")

    def summary(self, acc: torch.Tensor):
        """``acc`` as the numpy array [npoints, RS_SUM_COLS] that summary.reduce_series returns (synchronises)."""
        return acc[:, :self.npoints].T.contiguous().cpu().numpy()

    def _period_acc(self, spec, acc):
        sp, cols = lib.period_spec(spec), lib.period_cols()
        lib.check(self.L.rs_hip_period_check(C.byref(sp)), "rs_hip_period_check")  # (the spec sizes the accumulator)
        shape = (int(sp.nperiods), cols, self.np_pad)
        if acc is None:
            acc = torch.empty(shape, dtype=torch.float64, device=self.device)
        assert acc.dtype == torch.float64 and acc.shape == shape and acc.is_contiguous()
        return sp, acc

    def periods_reset(self, spec, acc: torch.Tensor | None = None,
                      stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """The cell of no rows into every column of every period of ``acc``, float64 [nperiods, RS_PER_COLS, np_pad]
        on this device (made here if None) - what ``outputs_periods`` continues (rs_hip_periods_reset); ``spec``:
        periods.PeriodSpec."""
        sp, acc = self._period_acc(spec, acc)
        lib.check(self.L.rs_hip_periods_reset(self._h, C.byref(sp), C.c_void_p(acc.data_ptr()), _stream_ptr(stream)),
                  "rs_hip_periods_reset")
        return acc

    def outputs_periods(self, out: "OutputWindow", nrows: int, index0: int, index_step: int, spec, acc: torch.Tensor,
                        order=None, stream: torch.cuda.Stream | None = None, row: int = 0) -> None:
        """Rows ``row .. row + nrows - 1`` of the output window, [row][slot], fed IN TIME ORDER into the per-point
        cells of the output periods ``acc`` [nperiods, RS_PER_COLS, np_pad] in POINT order (rs_hip_outputs_periods;
        roadsurf_amd/periods.py defines the columns and the feed contract).  The first of these rows is the absolute
        1-based time index ``index0``, the next ``index0 + index_step``; rows outside the spec's periods are ignored;
        ``spec``: periods.PeriodSpec; ``order`` and ``stream`` as for ``outputs_by_point``."""
        sp, acc = self._period_acc(spec, acc)
        o = out.struct_from(row)
        lib.check(self.L.rs_hip_outputs_periods(self._h, C.byref(o), int(nrows), int(index0), int(index_step), _ptr(order),
                                                C.byref(sp), C.c_void_p(acc.data_ptr()), _stream_ptr(stream)),
                  "rs_hip_outputs_periods")

    def periods(self, acc: torch.Tensor, spec=None):
        """``acc`` as the numpy array [npoints, nperiods, RS_PER_COLS] that periods.reduce_series returns
        (synchronises)."""
        a = acc[:, :, :self.npoints].permute(2, 0, 1).contiguous().cpu().numpy()
        assert spec is None or a.shape[1:] == (int(spec.nperiods), lib.period_cols())
        return a

    def _episode_acc(self, spec, acc):
        if not hasattr(self.L, "rs_hip_episode_cols"):
            raise RuntimeError("this libroadsurf_hip.so has no threshold episodes (rs_hip_episode_cols)")
        sp = lib.episode_spec(spec)
        cols = lib.episode_cols(sp)
        if acc is None:
            acc = torch.empty((cols, self.np_pad), dtype=torch.float64, device=self.device)
        assert acc.dtype == torch.float64 and acc.shape == (cols, self.np_pad) and acc.is_contiguous()
        return sp, acc

    def episodes_reset(self, spec, acc: torch.Tensor | None = None,
                       stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """The accumulator of no rows into every column of ``acc``, float64 [cols, np_pad] on this device (made here
        if None) - what ``outputs_episodes`` feeds (rs_hip_episodes_reset); ``spec``: episodes.EpisodeSpec."""
        sp, acc = self._episode_acc(spec, acc)
        lib.check(self.L.rs_hip_episodes_reset(self._h, C.byref(sp), C.c_void_p(acc.data_ptr()), _stream_ptr(stream)),
                  "rs_hip_episodes_reset")
        return acc

    def outputs_episodes(self, out: "OutputWindow", nrows: int, index0: int, index_step: int, spec, acc: torch.Tensor,
                         deficit: torch.Tensor | None = None, order=None, stream: torch.cuda.Stream | None = None,
                         row: int = 0) -> None:
        """Rows ``row .. row + nrows - 1`` of the output window, [row][slot], fed IN ORDER into the per-point
        episodes ``acc`` [cols, np_pad] in POINT order (rs_hip_outputs_episodes; roadsurf_amd/episodes.py defines
        the automaton).  The first of these rows is the absolute 1-based time index ``index0``, the next ``index0 +
        index_step``; ``deficit``: the dew-point deficit of the same rows in the window's layout and type
        ([rows, t_stride]; its row ``row`` is the first one read), required iff the spec tests it or keeps its peak;
        ``order`` and ``stream`` as for ``outputs_by_point``."""
        sp, acc = self._episode_acc(spec, acc)
        o = out.struct_from(row)
        d = None
        if deficit is not None:
            assert deficit.dtype == out.tensors["tsurf"].dtype and deficit.dim() == 2 and deficit.stride(1) == 1
            assert deficit.stride(0) == out.t_stride and deficit.shape[0] >= row + nrows
            d = C.c_void_p(deficit[row].data_ptr())
        lib.check(self.L.rs_hip_outputs_episodes(self._h, C.byref(o), d, int(nrows), int(index0), int(index_step),
                                                 _ptr(order), C.byref(sp), C.c_void_p(acc.data_ptr()),
                                                 _stream_ptr(stream)), "rs_hip_outputs_episodes")

    def episodes_finish(self, spec, acc: torch.Tensor, stream: torch.cuda.Stream | None = None) -> None:
        """Close every point's open run (rs_hip_episodes_finish): what a consumer reads.  Idempotent."""
        sp, acc = self._episode_acc(spec, acc)
        lib.check(self.L.rs_hip_episodes_finish(self._h, C.byref(sp), C.c_void_p(acc.data_ptr()), _stream_ptr(stream)),
                  "rs_hip_episodes_finish")

    def episodes(self, acc: torch.Tensor):
        """``acc`` as the numpy array [npoints, cols] that episodes.reduce_series returns (synchronises)."""
        return acc[:, :self.npoints].T.contiguous().cpu().numpy()

    def groups_reset(self, nrows: int, spec, acc: torch.Tensor | None = None,
                     stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """The empty cell into every cell of ``acc``, float64 [nrows, ngroups, cols] on this device (made here if
        None) - what ``outputs_groups`` accumulates into (rs_hip_group_reset); ``spec``: groups.GroupSpec."""
        sp = lib.group_spec(spec)
        shape = (int(nrows), int(sp.ngroups), lib.group_cols(sp))
        if acc is None:
            acc = torch.empty(shape, dtype=torch.float64, device=self.device)
        assert acc.dtype == torch.float64 and acc.shape == shape and acc.is_contiguous()
        lib.check(self.L.rs_hip_group_reset(self._h, C.c_void_p(acc.data_ptr()), int(nrows), C.byref(sp),
                                            _stream_ptr(stream)), "rs_hip_group_reset")
        return acc

    def outputs_groups(self, out: "OutputWindow", nrows: int, group: torch.Tensor, spec, acc: torch.Tensor,
                       acc_row0: int, order=None, stream: torch.cuda.Stream | None = None, row: int = 0) -> None:
        """Rows ``row .. row + nrows - 1`` of the output window, [row][slot], merged into rows ``acc_row0 ..`` of the
        per-group series ``acc`` [rows, ngroups, cols] (rs_hip_outputs_groups; roadsurf_amd/groups.py defines the
        cells).  ``group``: int32 [npoints] on this device, every point's group in POINT order; ``spec``:
        groups.GroupSpec; ``order`` and ``stream`` as for ``outputs_by_point``."""
        assert acc.dtype == torch.float64 and acc.dim() == 3 and acc.is_contiguous()
        assert group.dtype == torch.int32 and group.numel() >= self.npoints and group.is_contiguous()
        o = out.struct_from(row)
        sp = lib.group_spec(spec)
        lib.check(self.L.rs_hip_outputs_groups(self._h, C.byref(o), int(nrows), C.c_void_p(group.data_ptr()), _ptr(order),
                                               C.byref(sp), C.c_void_p(acc.data_ptr()), int(acc.shape[0]), int(acc_row0),
                                               _stream_ptr(stream)), "rs_hip_outputs_groups")

    def groups(self, acc: torch.Tensor, spec=None):
        """``acc`` as the numpy array [rows, ngroups, cols] that groups.reduce_groups returns (synchronises)."""
        a = acc.cpu().numpy()
        assert spec is None or a.shape[1:] == (int(spec.ngroups), lib.group_cols(spec))
        return a

    def _ens_spec(self, spec):
        if not hasattr(self.L, "rs_hip_ens_cols"):
            raise RuntimeError("this libroadsurf_hip.so has no ensemble statistics (rs_hip_ens_cols)")
        sp = lib.ens_spec(spec)
        return sp, lib.ens_cols(sp)

    def ens_table(self, group, spec) -> torch.Tensor:
        """The member table of ``group`` - int32 [npoints] on the HOST (numpy or a CPU tensor), every point's station
        in POINT order - built by the library (rs_ens_member_table; roadsurf_amd/ensstats.py, member_table, defines
        it) and uploaded: int32 [ngroups + 1 + npoints] on this device, what ``outputs_ens`` reads.  A station with
        more than ``spec.max_members`` members is refused.  Also makes the plan's work row for ``outputs_ens``.
        ``spec``: an ensstats.EnsSpec, or an ensprob.ProbSpec - ``ngroups`` and ``max_members`` alone make the table,
        which serves ``outputs_prob`` too."""
        import numpy as np
        sp, _ = self._ens_spec(spec)
        if torch.is_tensor(group):
            if group.is_cuda:
                raise ValueError("ens_table: group is a HOST array (numpy or a CPU tensor)")
            group = group.numpy()
        gid = np.asarray(group)
        if gid.dtype.kind not in "iu" or gid.shape != (self.npoints,):
            raise ValueError(f"ens_table: group must be {self.npoints} integers, one per point of this plan")
        gid = np.ascontiguousarray(np.clip(gid, -1, 2**31 - 1), dtype=np.int32)   # (beyond int32: no station either)
        table = np.empty(int(self.L.rs_ens_table_ints(self.npoints, C.byref(sp))), np.int32)
        lib.check(self.L.rs_ens_member_table(self.npoints, C.c_void_p(gid.ctypes.data), C.byref(sp),
                                             C.c_void_p(table.ctypes.data)), "rs_ens_member_table")
        if getattr(self, "_ens_work", None) is None:
            self._ens_work = torch.empty((self.np_pad,), dtype=torch.int32, device=self.device)
        return torch.from_numpy(table).to(self.device)

    def outputs_ens(self, out: "OutputWindow", nrows: int, table: torch.Tensor, spec, acc: torch.Tensor,
                    acc_row0: int, order=None, stream: torch.cuda.Stream | None = None, row: int = 0,
                    work: torch.Tensor | None = None) -> None:
        """Rows ``row .. row + nrows - 1`` of the output window, [row][slot], reduced per station and WRITTEN to rows
        ``acc_row0 ..`` of ``acc`` [rows, ngroups, cols] (rs_hip_outputs_ens; roadsurf_amd/ensstats.py defines the
        cells).  ``table``: what ``ens_table`` returned; ``spec``: ensstats.EnsSpec; ``order`` and ``stream`` as for
        ``outputs_by_point``.  ``work``: int32 [np_pad] scratch on this device, default the plan's own row (made by
        ``ens_table``) - calls on different streams need a row each."""
        sp, cols = self._ens_spec(spec)
        assert acc.dtype == torch.float64 and acc.dim() == 3 and acc.is_contiguous()
        assert acc.shape[1:] == (int(sp.ngroups), cols)
        assert table.dtype == torch.int32 and table.is_contiguous()
        assert table.numel() >= int(sp.ngroups) + 1 + self.npoints
        if work is None:
            if getattr(self, "_ens_work", None) is None:
                self._ens_work = torch.empty((self.np_pad,), dtype=torch.int32, device=self.device)
            work = self._ens_work
        assert work.dtype == torch.int32 and work.numel() >= self.np_pad and work.is_contiguous()
        o = out.struct_from(row)
        lib.check(self.L.rs_hip_outputs_ens(self._h, C.byref(o), int(nrows), C.c_void_p(table.data_ptr()), _ptr(order),
                                            C.byref(sp), C.c_void_p(acc.data_ptr()), int(acc.shape[0]), int(acc_row0),
                                            C.c_void_p(work.data_ptr()), _stream_ptr(stream)), "rs_hip_outputs_ens")

    def ens(self, acc: torch.Tensor, spec=None):
        """``acc`` as the numpy array [rows, ngroups, cols] that ensstats.reduce_members returns (synchronises)."""
        if not hasattr(self.L, "rs_hip_ens_cols"):
            raise RuntimeError("this libroadsurf_hip.so has no ensemble statistics (rs_hip_ens_cols)")
        a = acc.cpu().numpy()
        assert spec is None or a.shape[1:] == (int(spec.ngroups), lib.ens_cols(spec))
        return a

    def _prob_spec(self, spec):
        if not hasattr(self.L, "rs_hip_prob_cols"):
            raise RuntimeError("this libroadsurf_hip.so has no probabilities over the members (rs_hip_prob_cols)")
        sp = lib.prob_spec(spec)
        return sp, lib.prob_cols(sp)

    def prob_work_ints(self, nrows: int) -> int:
        """int32s of scratch one ``outputs_prob`` over ``nrows`` rows needs (rs_hip_prob_work_ints)."""
        if not hasattr(self.L, "rs_hip_prob_cols"):
            raise RuntimeError("this libroadsurf_hip.so has no probabilities over the members (rs_hip_prob_cols)")
        n = int(self.L.rs_hip_prob_work_ints(self._h, int(nrows)))
        if n < 0:
            raise ValueError("prob_work_ints: nrows >= 1")
        return n

    def prob_reset(self, ever: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Zero into every entry of the carry ``ever``, int32 [np_pad] on this device in POINT order (made here if
        None) - what ``outputs_prob`` reads and updates (rs_hip_prob_reset): no condition has held yet."""
        if not hasattr(self.L, "rs_hip_prob_cols"):
            raise RuntimeError("this libroadsurf_hip.so has no probabilities over the members (rs_hip_prob_cols)")
        if ever is None:
            ever = torch.empty((self.np_pad,), dtype=torch.int32, device=self.device)
        assert ever.dtype == torch.int32 and ever.shape == (self.np_pad,) and ever.is_contiguous()
        lib.check(self.L.rs_hip_prob_reset(self._h, C.c_void_p(ever.data_ptr()), _stream_ptr(stream)),
                  "rs_hip_prob_reset")
        return ever

    def outputs_prob(self, out: "OutputWindow", nrows: int, table: torch.Tensor, spec, ever: torch.Tensor,
                     acc: torch.Tensor, acc_row0: int, deficit: torch.Tensor | None = None, order=None,
                     stream: torch.cuda.Stream | None = None, row: int = 0, work: torch.Tensor | None = None) -> None:
        """Rows ``row .. row + nrows - 1`` of the output window, [row][slot], fed IN ORDER: per station the members
        under each condition now and by now, WRITTEN to rows ``acc_row0 ..`` of ``acc`` [rows, ngroups, cols], and the
        carry ``ever`` [np_pad] updated (rs_hip_outputs_prob; roadsurf_amd/ensprob.py defines the cells).  ``table``:
        what ``ens_table`` returned for the same stations; ``spec``: ensprob.ProbSpec; ``deficit`` as for
        ``outputs_episodes``, required iff a condition tests it; ``order`` and ``stream`` as for
        ``outputs_by_point``.  ``work``: int32 scratch on this device of at least ``prob_work_ints(nrows)`` entries,
        default the plan's own, grown as needed - a call on a stream of the caller's needs its own."""
        sp, cols = self._prob_spec(spec)
        assert acc.dtype == torch.float64 and acc.dim() == 3 and acc.is_contiguous()
        assert acc.shape[1:] == (int(sp.ngroups), cols)
        assert table.dtype == torch.int32 and table.is_contiguous()
        assert table.numel() >= int(sp.ngroups) + 1 + self.npoints
        assert ever.dtype == torch.int32 and ever.numel() >= self.np_pad and ever.is_contiguous()
        if work is None:
            if stream is not None:
                raise ValueError("outputs_prob: a call on a stream of the caller's needs a work of the caller's")
            need = self.prob_work_ints(nrows)
            if getattr(self, "_prob_work", None) is None or self._prob_work.numel() < need:
                self._prob_work = torch.empty((need,), dtype=torch.int32, device=self.device)
            work = self._prob_work
        assert work.dtype == torch.int32 and work.dim() == 1 and work.is_contiguous()
        o = out.struct_from(row)
        d = None
        if deficit is not None:
            assert deficit.dtype == out.tensors["tsurf"].dtype and deficit.dim() == 2 and deficit.stride(1) == 1
            assert deficit.stride(0) == out.t_stride and deficit.shape[0] >= row + nrows
            d = C.c_void_p(deficit[row].data_ptr())
        lib.check(self.L.rs_hip_outputs_prob(self._h, C.byref(o), d, int(nrows), C.c_void_p(table.data_ptr()),
                                             _ptr(order), C.byref(sp), C.c_void_p(ever.data_ptr()),
                                             C.c_void_p(acc.data_ptr()), int(acc.shape[0]), int(acc_row0),
                                             C.c_void_p(work.data_ptr()), int(work.numel()), _stream_ptr(stream)),
                  "rs_hip_outputs_prob")

    def prob(self, acc: torch.Tensor, spec=None):
        """``acc`` as the numpy array [rows, ngroups, cols] that ensprob.reduce_members_prob returns (synchronises)."""
        if not hasattr(self.L, "rs_hip_prob_cols"):
            raise RuntimeError("this libroadsurf_hip.so has no probabilities over the members (rs_hip_prob_cols)")
        a = acc.cpu().numpy()
        assert spec is None or a.shape[1:] == (int(spec.ngroups), lib.prob_cols(spec))
        return a

    def gather_nodes(self, src: torch.Tensor, node: torch.Tensor, weight: torch.Tensor, dst: torch.Tensor,
                     present_above: float, missing: float = -9999.9, n_nodes: int | None = None, order=None,
                     stream: torch.cuda.Stream | None = None) -> None:
        """Fields gathered to this plan's points (rs_hip_gather_nodes; roadsurf_amd/grid.py gather_nodes defines the
        values): ``src`` float64 [nrows, src_stride] holding ``n_nodes`` (default all) nodes per row, ``node`` int32 /
        ``weight`` float64 [>= npoints, stencil], ``dst`` float64 [nrows, dst_stride >= npoints] whose columns
        [0, npoints) are written in slot order; ``order`` and ``stream`` as for ``outputs_by_point``."""
        if not hasattr(self.L, "rs_hip_grid_max_stencil"):
            raise RuntimeError("this libroadsurf_hip.so has no gridded sources (rs_hip_grid_max_stencil)")
        assert src.dtype == torch.float64 and src.dim() == 2 and src.stride(1) == 1
        assert dst.dtype == torch.float64 and dst.dim() == 2 and dst.stride(1) == 1 and dst.shape[0] == src.shape[0]
        assert node.dtype == torch.int32 and weight.dtype == torch.float64 and node.dim() == 2
        assert node.shape == weight.shape and node.shape[0] >= self.npoints and node.is_contiguous() and weight.is_contiguous()
        lib.check(self.L.rs_hip_gather_nodes(self._h, C.c_void_p(src.data_ptr()), int(src.shape[0]),
                                             int(src.shape[1] if n_nodes is None else n_nodes), int(src.stride(0)),
                                             C.c_void_p(node.data_ptr()), C.c_void_p(weight.data_ptr()),
                                             int(node.shape[1]), _ptr(order), float(present_above), float(missing),
                                             C.c_void_p(dst.data_ptr()), int(dst.stride(0)), _stream_ptr(stream)),
                  "rs_hip_gather_nodes")

    def reset_order(self) -> None:
        lib.check(self.L.rs_hip_plan_reset_order(self._h), "rs_hip_plan_reset_order")

    def recluster_forecast(self, tair_rows, vz_rows, hours, tair_now, alpha: float = 0.5,
                           mode: int = 1, point_order: bool = False, prec_rows=None, between=None) -> None:
        """Sort the slots by a forecast of the next launch (rs_hip_recluster_forecast): rows are
        tensors [np_pad] at the preview times, hours the hour of day.  Rows in the CURRENT slot order,
        or - ``point_order`` - in point order, read through the plan's order row.  ``between``: per preview
        (tair_b, vz_b, w) - the preview lies between its row and that one (RsPreview::tair_b); tair_now may
        then be None."""
        pv = lib.RsPreview()
        if between is not None:
            for q, (tb, vb, w) in enumerate(between):
                pv.tair_b[q] = tb.data_ptr(); pv.vz_b[q] = vb.data_ptr(); pv.w[q] = float(w)
        pv.index = self.L.rs_hip_plan_order(self._h) if point_order else None
        pv.n = len(tair_rows)
        for q, (ta, vz, h) in enumerate(zip(tair_rows, vz_rows, hours)):
            pv.tair[q] = ta.data_ptr(); pv.vz[q] = vz.data_ptr(); pv.hour[q] = int(h)
        if prec_rows is not None:  # one more key bit: precipitation somewhere in the next window
            for q, pr in enumerate(prec_rows):
                pv.prec[q] = pr.data_ptr()
        pv.tair_now = tair_now.data_ptr() if tair_now is not None else None
        pv.alpha = alpha
        pv.mode = mode
        lib.check(self.L.rs_hip_recluster_forecast(self._h, C.byref(pv)), "rs_hip_recluster_forecast")

    def recluster(self) -> None:
        """Sort the slots by the boundary-layer passes of the last launch; later windows,
        per-point parameters and outputs are in the new slot order."""
        lib.check(self.L.rs_hip_recluster(self._h), "rs_hip_recluster")

    def synth_knots_range(self, spec, knots: torch.Tensor, k0: int, nknots: int, ordered: bool):
        """Knots k0..k0+nknots-1 into the first rows of ``knots``; with ``ordered`` column p
        belongs to point order()[p]."""
        spec.order = self.L.rs_hip_plan_order(self._h) if ordered else None
        lib.check(self.L.rs_hip_synth_knots(self._h, C.byref(spec), C.c_void_p(knots.data_ptr()),
                                            k0, nknots), "rs_hip_synth_knots")

    def expand_range(self, spec, knots: torch.Tensor, k0: int, nknots: int, window: ForcingWindow,
                     t0: int, nsteps: int) -> None:
        f = window.struct(0)
        lib.check(self.L.rs_hip_expand_forcing(self._h, C.byref(spec), C.c_void_p(knots.data_ptr()),
                                               k0, nknots, C.byref(f), t0, nsteps),
                  "rs_hip_expand_forcing")

    def expand_ordered(self, spec, knots: torch.Tensor, window: ForcingWindow, t0: int, nsteps: int) -> None:
        """Knots [nknots][9][np_pad] in POINT order (all of the series, knot 0 first) -> the window in
        the plan's current slot order (rs_hip_expand_forcing_ordered)."""
        f = window.struct(0)
        lib.check(self.L.rs_hip_expand_forcing_ordered(self._h, C.byref(spec), C.c_void_p(knots.data_ptr()),
                                                       0, knots.shape[0], C.byref(f), t0, nsteps),
                  "rs_hip_expand_forcing_ordered")

    def expand(self, spec, knots, window: ForcingWindow, t0: int, nsteps: int,
               stream: torch.cuda.Stream | None = None) -> None:
        f = window.struct(0)
        st = (stream or self.stream).cuda_stream
        lib.check(self.L.rs_hip_expand_forcing_on(self._h, C.byref(spec),
                                                  C.c_void_p(knots.data_ptr()), 0, knots.shape[0],
                                                  C.byref(f), t0, nsteps, C.c_void_p(st)),
                  "rs_hip_expand_forcing_on")


def run_points(forcing: dict, settings: abi.InputSettings, params: abi.InputParameters,
               local, chunk: int = 0, variant: int = 0, device: int = 0,
               lean_if_possible: bool = True, year_month_day=None, history_score: bool | None = None,
               precision: int = 64, horizon_index=None, summary=None, groups=None, episodes=None, probs=None,
               periods=None):
    """Run host arrays ``forcing[name][n, SimLen]`` (numpy, reference layout) through the
    device-resident API and return outputs ``[n, SimLen]`` as numpy.  Test/bench helper:
    transposes with torch on the device, windows of ``chunk`` steps (0 = whole series).
    ``summary``: a summary.SummarySpec - every launch's rows are also reduced on the device
    (``Plan.outputs_summary``) and the result has ``summary`` [n, RS_SUM_COLS]; not with coupling,
    whose replays rewrite rows that earlier launches wrote.  ``groups``: (groups.GroupSpec, group ids int32 [n]) -
    every launch's rows are also reduced over the points of each group (``Plan.outputs_groups``) and the result
    has ``groups`` [SimLen, ngroups, cols], row r being time index r + 1; not with coupling either.
    ``episodes``: an episodes.EpisodeSpec that does not need the deficit - every launch's rows are also fed to the
    per-point episodes (``Plan.outputs_episodes``) and the result has ``episodes`` [n, cols], finished; not with
    coupling either.  ``probs``: (ensprob.ProbSpec that does not need the deficit, stations int32 [n]) - every
    launch's rows are also counted per station and condition (``Plan.outputs_prob``) and the result has ``probs``
    [SimLen, ngroups, cols], row r being time index r + 1; not with coupling either.  ``periods``: a
    periods.PeriodSpec - every launch's rows are also fed, by absolute time index and in time order, to the per-point
    aggregates over output periods (``Plan.outputs_periods``) and the result has ``periods`` [n, nperiods,
    RS_PER_COLS]; not with coupling either."""
    from . import ensprob, legs  # (legs imports this module when a Leg is made)
    from . import periods as periods_

    require_gpu()
    n, L = forcing["tair"].shape
    assert L == settings.SimLen
    if isinstance(local, abi.LocalParameters):
        local = [local] * n
    coupled = settings.use_coupling == 1
    for name, spec in (("summary", summary), ("groups", groups), ("episodes", episodes), ("probs", probs),
                       ("periods", periods)):
        if spec is not None and coupled:  # (the reducers are for the launches of an uncoupled run)
            raise ValueError(f"run_points: no {name} with coupling")
    if probs is not None and ensprob.needs_deficit(probs[0]):
        raise ValueError("run_points: probs: a condition uses the deficit, and the runner has no deficit rows")
    if periods is not None:
        periods_.check_spec(periods)
    if year_month_day is None:
        year_month_day = (int(forcing["year"][0]), int(forcing["month"][0]), int(forcing["day"][0]))
    need_full, sky_on = legs.feature_set(settings, local, [forcing], lean_if_possible)
    leg = legs.Leg(forcing, settings, params, local, need_full=need_full, sky_on=sky_on, tbottom_date=year_month_day,
                   precision=precision, variant=variant, history_score=history_score, horizon_index=horizon_index,
                   device=device, summary=summary, groups=groups, episodes=episodes, probs=probs,
                   periods=periods)
    leg.init()
    leg.run(legs.coupling_stages(settings, local, L, chunked=bool(chunk)), chunk)
    res = leg.results()
    res.update(leg.reduced())
    nfail = leg.plan.failed_count()
    leg.plan.close()
    return res, nfail
