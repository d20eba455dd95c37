"""ctypes binding of ``roadsurf_amd/lib/libroadsurf_hip.so`` (``include/roadsurf.h``).

The library holds the HIP kernels, the C-ABI shim and the Fortran host
orchestration.  There is no CPU implementation behind this binding: if the
shared object is missing, ``load()`` raises; if no GPU is visible, every
compute entry point returns an error that the wrappers turn into
``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ROADSURF_HIP_LIB") or os.path.join(_HERE, "lib", "libroadsurf_hip.so")

RS_MAX_LAYERS = abi.RS_MAX_LAYERS
RS_KNOT_FIELDS = 9
RS_NSTATE = RS_MAX_LAYERS + 17 + 21 + 2 * RS_MAX_LAYERS

_tbl = C.c_double * (RS_MAX_LAYERS + 2)


class RsConstants(C.Structure):
    _fields_ = (
        [("NLayers", C.c_int32), ("SimLen", C.c_int32), ("use_relaxation", C.c_int32),
         ("force_tsurf", C.c_int32), ("use_coupling", C.c_int32), ("cplLenI", C.c_int32),
         ("cplLenR", C.c_double), ("cplReduction", C.c_double),
         ("DTSecs", C.c_double), ("Tph", C.c_double), ("tsurfOutputDepth", C.c_double),
         ("twoDT", C.c_double),
         ("ZDpth", _tbl), ("DyC", _tbl), ("condDZ", _tbl), ("WCont", _tbl), ("dryCap", _tbl)]
        + [(n, C.c_double) for n in (
            "HSfac1", "logMom", "logHeat", "logCond", "logUstar",
            "VK_Const", "ZRefT", "Grav", "LVap", "LFus",
            "Emiss", "SB_Const", "Albedo0",
            "NightOn", "NightOff", "CalmLimDay", "CalmLimNgt", "TrfFricNgt", "TrFfricDay",
            "MaxPormms", "MissValI", "MinPrecmm", "MinWatmms", "MinSnowmms", "MinDepmms",
            "MinIcemms", "MaxSnowmms", "MaxDepmms", "MaxIcemms", "MaxWatmms", "AlbDry", "AlbSnow",
            "WatDens", "WatMHeat", "PorEvaF", "DampWearF", "TLimFreeze", "TLimMeltSnow",
            "TLimMeltIce", "TLimMeltDep", "TLimDew", "TLimColdH", "TLimColdL", "WetSnowFormR",
            "WetSnowMeltR", "PLimSnow", "PLimRain", "WWetLim", "WWearLim", "T4Melt0",
            "wSnowTran", "wSnow2Ice", "wIce", "wIce2", "wDep", "wWat",
        )]
    )


class RsForcing(C.Structure):
    _fields_ = (
        [(n, C.c_void_p) for n in ("tair", "tdew", "vz", "rhz", "prec", "sw", "lw",
                                   "tsurfobs", "depth", "precphase", "hour")]
        + [("t_stride", C.c_int64), ("hour_pstride", C.c_int32)]
        + [(n, C.c_void_p) for n in ("sw_dir", "lw_net", "sun")]
    )


class RsOutputs(C.Structure):
    _fields_ = (
        [(n, C.c_void_p) for n in ("tsurf", "snow", "water", "ice", "deposit", "ice2")]
        + [("t_stride", C.c_int64), ("decimate", C.c_int32), ("row0", C.c_int64)]
    )


class RsPointParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("tbottom", "initlen", "tair_relax", "vz_relax", "rh_relax",
                                          "coupling_index", "coupling_tsurf", "sky_view",
                                          "sin_lat", "cos_lat", "lon_rad", "horizons")] + \
               [("albedo_surroundings", C.c_double), ("horizon_index", C.c_void_p), ("horizons_by_point", C.c_int32)]


class RsHostExtras(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("sun", "sin_lat", "cos_lat", "lon_rad")] + \
               [("albedo_surroundings", C.c_double), ("first_failed", C.c_void_p), ("writeback", C.c_int32),
                ("diagnostics", C.c_void_p)]


RS_PREVIEW_MAX = 8


class RsPreview(C.Structure):
    _fields_ = [("n", C.c_int32), ("tair", C.c_void_p * RS_PREVIEW_MAX), ("vz", C.c_void_p * RS_PREVIEW_MAX),
                ("hour", C.c_int32 * RS_PREVIEW_MAX), ("tair_now", C.c_void_p), ("alpha", C.c_double),
                ("mode", C.c_int32), ("index", C.c_void_p), ("prec", C.c_void_p * RS_PREVIEW_MAX),
                ("tair_b", C.c_void_p * RS_PREVIEW_MAX), ("vz_b", C.c_void_p * RS_PREVIEW_MAX),
                ("w", C.c_double * RS_PREVIEW_MAX)]


RS_SUM_COLS = 17


class RsSummarySpec(C.Structure):
    _fields_ = [("tsurf_below", C.c_double), ("storage_above", C.c_double * 5)]


RS_GRP_COLS = 14
RS_GRP_MAX_EDGES = 31


class RsGroupSpec(C.Structure):
    _fields_ = [("thresholds", RsSummarySpec), ("ngroups", C.c_int32), ("nedges", C.c_int32),
                ("edges", C.c_double * RS_GRP_MAX_EDGES)]


RS_ENS_MAX_MEMBERS = 64
RS_ENS_MAX_QUANT = 8
RS_ENS_COLS = 9


class RsEnsSpec(C.Structure):
    _fields_ = [("ngroups", C.c_int32), ("max_members", C.c_int32), ("nquant", C.c_int32),
                ("quant", C.c_double * RS_ENS_MAX_QUANT)]


RS_EPI_VARS = 7
RS_EPI_MAX = 8
RS_EPI_HEAD = 10
RS_EPI_REC = 6


class RsEpisodeSpec(C.Structure):
    _fields_ = [("use", C.c_int32), ("peak", C.c_int32), ("min_rows", C.c_int32), ("max_episodes", C.c_int32),
                ("above", C.c_double * RS_EPI_VARS), ("below", C.c_double * RS_EPI_VARS)]


RS_PROB_MAX_CONDS = 8


class RsProbCond(C.Structure):
    _fields_ = [("use", C.c_int32), ("reserved", C.c_int32),
                ("above", C.c_double * RS_EPI_VARS), ("below", C.c_double * RS_EPI_VARS)]


class RsProbSpec(C.Structure):
    _fields_ = [("ngroups", C.c_int32), ("max_members", C.c_int32), ("nconds", C.c_int32), ("reserved", C.c_int32),
                ("cond", RsProbCond * RS_PROB_MAX_CONDS)]


RS_PER_COLS = 17


class RsPeriodSpec(C.Structure):
    _fields_ = [("first_index", C.c_int32), ("length", C.c_int32), ("nperiods", C.c_int32), ("reserved", C.c_int32),
                ("th", RsSummarySpec)]


class RsSynthSpec(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("point_offset", C.c_int64),
                ("steps_per_knot", C.c_int32), ("start_hour", C.c_int32), ("order", C.c_void_p)]


#: every symbol ``include/roadsurf.h`` declares
EXPORTS = (
    "rs_default_parameters", "rs_default_settings", "rs_default_local",
    "runsimulation", "runsimulation_batch", "runsimulation_batch_ex", "rs_coalesce_run", "rs_coalesce_stats", "rs_runsimulation_gathered", "rs_synth_fill_points", "rs_build_sha16", "rs_build_constants", "rs_bottom_temperature",
    "rs_sun_table", "rs_point_geometry",
    "rs_last_error", "rs_hip_device_count", "rs_hip_plan_create", "rs_hip_plan_destroy",
    "rs_hip_plan_npoints", "rs_hip_plan_npoints_padded", "rs_hip_plan_state_bytes",
    "rs_hip_init_state", "rs_hip_step", "rs_hip_step_cpl", "rs_hip_cpl_replay", "rs_hip_set_output_by_point", "rs_hip_state_download", "rs_hip_state_upload", "rs_hip_state_fanout",
    "rs_hip_failed_count", "rs_hip_clock_probe", "rs_hip_first_failed_index", "rs_hip_set_diagnostics", "rs_hip_diagnostics", "rs_hip_sync", "rs_hip_synth_knots", "rs_hip_expand_forcing", "rs_hip_expand_forcing_ordered", "rs_hip_step_knots", "rs_hip_expand_forcing_on",
    "rs_hip_plan_order", "rs_hip_recluster", "rs_hip_recluster_forecast", "rs_hip_set_history_score", "rs_hip_coupling_windows_closed", "rs_hip_set_writeback", "rs_hip_plan_order_copy", "rs_hip_outputs_by_point", "rs_hip_summary_cols", "rs_hip_summary_reset", "rs_hip_outputs_summary", "rs_hip_group_cols", "rs_hip_group_path", "rs_hip_group_reset", "rs_hip_outputs_groups", "rs_hip_ens_cols", "rs_ens_table_ints", "rs_ens_member_table", "rs_hip_outputs_ens", "rs_hip_episode_cols", "rs_hip_episodes_reset", "rs_hip_outputs_episodes", "rs_hip_episodes_finish", "rs_hip_prob_cols", "rs_hip_prob_needs_deficit", "rs_hip_prob_spec_bytes", "rs_hip_prob_work_ints", "rs_hip_prob_reset", "rs_hip_outputs_prob", "rs_hip_period_cols", "rs_hip_period_spec_bytes", "rs_hip_period_check", "rs_hip_periods_reset", "rs_hip_outputs_periods", "rs_hip_grid_max_stencil", "rs_hip_gather_nodes", "rs_hip_plan_reset_order", "rs_hip_set_variant", "rs_hip_set_precision", "rs_hip_test_math", "rs_hip_division_mode", "rs_hip_div_mismatch_count", "rs_hip_div_special_count", "rs_hip_div_samples", "rs_hip_timing_reset", "rs_hip_timing_step_ms", "rs_hip_timing_intervals",
    "rs_host_run_batch", "rs_last_fanout", "rs_driver_run_request", "rs_driver_run", "rs_driver_run_summary", "rs_driver_run_groups", "rs_driver_run_grid", "rs_driver_expand_grid", "rs_driver_run_kept", "rs_driver_kept_fields", "rs_driver_run_episodes", "rs_driver_ensemble_bytes", "rs_driver_run_ensemble", "rs_driver_last_tiles", "rs_driver_last_raw_launches", "rs_hip_bl_stats", "rs_compat_begin", "rs_compat_step", "rs_compat_replay", "rs_compat_failed_index", "rs_compat_last_state", "rs_compat_outputs", "rs_compat_end", "rs_driver_expand", "rs_driver_release_cache", "rs_abi_version", "rs_abi_sizeof", "rs_fortran_sizeof",
)

_lib = None


def load() -> C.CDLL:
    """Load the HIP library or raise: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm wheels bundle their own libamdhip64.so; two HIP runtimes in one
    # process do not share the device.  Import torch FIRST so that our library's
    # DT_NEEDED libamdhip64.so.7 resolves to the copy torch has already mapped.
    # (A pure C/C++/Fortran host, e.g. the reference's roadrunner, simply gets
    # /opt/rocm/lib/libamdhip64.so.7 via the rpath.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing - build it with `make -C roadsurf_amd` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "roadsurf_amd has no CPU implementation."
        )
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    L.rs_last_error.restype = C.c_char_p
    L.rs_abi_version.restype = C.c_int
    L.rs_hip_device_count.restype = C.c_int
    L.rs_default_parameters.argtypes = [P(abi.InputParameters), C.c_double]
    L.rs_default_settings.argtypes = [P(abi.InputSettings), C.c_int32]
    L.rs_default_local.argtypes = [P(abi.LocalParameters)]
    L.rs_build_constants.argtypes = [P(abi.InputSettings), P(abi.InputParameters), P(RsConstants),
                                     P(C.c_int32)]
    L.rs_build_constants.restype = None
    L.rs_bottom_temperature.argtypes = [P(abi.InputParameters), P(RsConstants), C.c_int32,
                                        C.c_int32, C.c_int32]
    L.rs_bottom_temperature.restype = C.c_double
    L.runsimulation.argtypes = [P(abi.OutputPointers), P(abi.InputPointers), P(abi.InputSettings),
                                P(abi.InputParameters), P(abi.LocalParameters)]
    L.runsimulation.restype = None
    L.runsimulation_batch.argtypes = [C.c_int32, P(abi.OutputPointers), P(abi.InputPointers),
                                      P(abi.InputSettings), P(abi.InputParameters),
                                      P(abi.LocalParameters), P(C.c_int32)]
    L.runsimulation_batch.restype = None
    L.runsimulation_batch_ex.argtypes = [C.c_int32, P(abi.OutputPointers), P(abi.InputPointers),
                                         P(abi.InputSettings), P(abi.InputParameters),
                                         P(abi.LocalParameters), P(C.c_int32), C.c_void_p]
    L.runsimulation_batch_ex.restype = None
    L.rs_hip_plan_create.argtypes = [C.c_int32, C.c_int64, P(RsConstants), C.c_void_p]
    L.rs_hip_plan_create.restype = C.c_void_p
    L.rs_hip_plan_destroy.argtypes = [C.c_void_p]
    L.rs_hip_plan_destroy.restype = None
    for n in ("rs_hip_plan_npoints", "rs_hip_plan_npoints_padded", "rs_hip_failed_count"):
        getattr(L, n).argtypes = [C.c_void_p]
        getattr(L, n).restype = C.c_int64
    L.rs_hip_clock_probe.argtypes = [C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.rs_hip_plan_state_bytes.argtypes = [C.c_void_p]
    L.rs_hip_plan_state_bytes.restype = C.c_size_t
    L.rs_hip_init_state.argtypes = [C.c_void_p, P(RsForcing), P(RsPointParams)]
    L.rs_hip_step.argtypes = [C.c_void_p, P(RsForcing), P(RsOutputs), P(RsPointParams),
                              C.c_int32, C.c_int32]
    L.rs_hip_step_cpl.argtypes = [C.c_void_p, P(RsForcing), P(RsOutputs), P(RsPointParams),
                                  C.c_int32, C.c_int32]
    L.rs_hip_set_output_by_point.argtypes = [C.c_void_p, C.c_int32]
    L.rs_hip_cpl_replay.argtypes = [C.c_void_p, P(RsForcing), P(RsOutputs), P(RsPointParams),
                                    C.c_int32, C.c_int32, P(C.c_int32)]
    L.rs_hip_state_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.rs_hip_state_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.rs_hip_sync.argtypes = [C.c_void_p]
    L.rs_hip_first_failed_index.argtypes = [C.c_void_p, C.c_void_p]
    L.rs_hip_set_diagnostics.argtypes = [C.c_void_p, C.c_int32]
    L.rs_hip_diagnostics.argtypes = [C.c_void_p, C.c_void_p]
    L.rs_hip_synth_knots.argtypes = [C.c_void_p, P(RsSynthSpec), C.c_void_p, C.c_int32, C.c_int32]
    L.rs_hip_expand_forcing.argtypes = [C.c_void_p, P(RsSynthSpec), C.c_void_p, C.c_int32,
                                        C.c_int32, P(RsForcing), C.c_int32, C.c_int32]
    L.rs_hip_expand_forcing_ordered.argtypes = L.rs_hip_expand_forcing.argtypes
    L.rs_hip_expand_forcing_on.argtypes = [C.c_void_p, P(RsSynthSpec), C.c_void_p, C.c_int32,
                                           C.c_int32, P(RsForcing), C.c_int32, C.c_int32, C.c_void_p]
    L.rs_hip_step_knots.argtypes = [C.c_void_p, P(RsSynthSpec), C.c_void_p, C.c_int32, C.c_int32, P(RsOutputs),
                                    P(RsPointParams), C.c_int32, C.c_int32]
    L.rs_hip_plan_order.argtypes = [C.c_void_p]
    L.rs_hip_plan_order.restype = C.c_void_p
    L.rs_hip_recluster.argtypes = [C.c_void_p]
    L.rs_hip_recluster_forecast.argtypes = [C.c_void_p, P(RsPreview)]
    L.rs_hip_set_history_score.argtypes = [C.c_void_p, C.c_int32]
    L.rs_hip_coupling_windows_closed.argtypes = [C.c_void_p, C.c_int32]
    L.rs_hip_set_writeback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.rs_hip_plan_order_copy.argtypes = [C.c_void_p, C.c_void_p]
    L.rs_hip_outputs_by_point.argtypes = [C.c_void_p, P(RsOutputs), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    if hasattr(L, "rs_hip_summary_cols"):  # the ABI number did not move for the summaries: a library has them or not
        L.rs_hip_summary_cols.restype = C.c_int32
        L.rs_hip_summary_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rs_hip_outputs_summary.argtypes = [C.c_void_p, P(RsOutputs), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                             P(RsSummarySpec), C.c_void_p, C.c_void_p]
    if hasattr(L, "rs_hip_group_cols"):  # ... nor for the group series
        L.rs_hip_group_cols.restype = C.c_int32
        L.rs_hip_group_cols.argtypes = [P(RsGroupSpec)]
        L.rs_hip_group_path.restype = C.c_int32
        L.rs_hip_group_path.argtypes = [P(RsGroupSpec)]
        L.rs_hip_group_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, P(RsGroupSpec), C.c_void_p]
        L.rs_hip_outputs_groups.argtypes = [C.c_void_p, P(RsOutputs), C.c_int32, C.c_void_p, C.c_void_p, P(RsGroupSpec),
                                            C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    if hasattr(L, "rs_hip_ens_cols"):  # ... nor for the ensemble statistics
        L.rs_hip_ens_cols.restype = C.c_int32
        L.rs_hip_ens_cols.argtypes = [P(RsEnsSpec)]
        L.rs_ens_table_ints.restype = C.c_int64
        L.rs_ens_table_ints.argtypes = [C.c_int32, P(RsEnsSpec)]
        L.rs_ens_member_table.argtypes = [C.c_int32, C.c_void_p, P(RsEnsSpec), C.c_void_p]
        L.rs_hip_outputs_ens.argtypes = [C.c_void_p, P(RsOutputs), C.c_int32, C.c_void_p, C.c_void_p, P(RsEnsSpec),
                                         C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    if hasattr(L, "rs_hip_grid_max_stencil"):  # ... nor for the gridded sources
        L.rs_hip_grid_max_stencil.restype = C.c_int32
        L.rs_hip_gather_nodes.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_int64, C.c_void_p]
    if hasattr(L, "rs_hip_episode_cols"):  # ... nor for the threshold episodes
        L.rs_hip_episode_cols.restype = C.c_int32
        L.rs_hip_episode_cols.argtypes = [P(RsEpisodeSpec)]
        L.rs_hip_episodes_reset.argtypes = [C.c_void_p, P(RsEpisodeSpec), C.c_void_p, C.c_void_p]
        L.rs_hip_outputs_episodes.argtypes = [C.c_void_p, P(RsOutputs), C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_void_p, P(RsEpisodeSpec), C.c_void_p, C.c_void_p]
        L.rs_hip_episodes_finish.argtypes = [C.c_void_p, P(RsEpisodeSpec), C.c_void_p, C.c_void_p]
    if hasattr(L, "rs_hip_prob_cols"):  # ... nor for the probabilities of conditions over the members
        L.rs_hip_prob_cols.restype = C.c_int32
        L.rs_hip_prob_cols.argtypes = [P(RsProbSpec)]
        L.rs_hip_prob_needs_deficit.restype = C.c_int32
        L.rs_hip_prob_needs_deficit.argtypes = [P(RsProbSpec)]
        L.rs_hip_prob_spec_bytes.restype = C.c_int64
        L.rs_hip_prob_spec_bytes.argtypes = []
        if L.rs_hip_prob_spec_bytes() != C.sizeof(RsProbSpec):
            raise RuntimeError(f"{LIB_PATH}: RsProbSpec has {L.rs_hip_prob_spec_bytes()} bytes, this binding assumes "
                               f"{C.sizeof(RsProbSpec)}")
        L.rs_hip_prob_work_ints.restype = C.c_int64
        L.rs_hip_prob_work_ints.argtypes = [C.c_void_p, C.c_int32]
        L.rs_hip_prob_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rs_hip_outputs_prob.argtypes = [C.c_void_p, P(RsOutputs), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                          P(RsProbSpec), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                          C.c_int64, C.c_void_p]
    if hasattr(L, "rs_hip_period_cols"):  # ... nor for the aggregates over output periods
        L.rs_hip_period_cols.restype = C.c_int32
        L.rs_hip_period_cols.argtypes = []
        L.rs_hip_period_spec_bytes.restype = C.c_int64
        L.rs_hip_period_spec_bytes.argtypes = []
        if L.rs_hip_period_spec_bytes() != C.sizeof(RsPeriodSpec):
            raise RuntimeError(f"{LIB_PATH}: RsPeriodSpec has {L.rs_hip_period_spec_bytes()} bytes, this binding "
                               f"assumes {C.sizeof(RsPeriodSpec)}")
        L.rs_hip_period_check.argtypes = [P(RsPeriodSpec)]
        L.rs_hip_periods_reset.argtypes = [C.c_void_p, P(RsPeriodSpec), C.c_void_p, C.c_void_p]
        L.rs_hip_outputs_periods.argtypes = [C.c_void_p, P(RsOutputs), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                             P(RsPeriodSpec), C.c_void_p, C.c_void_p]
    if hasattr(L, "rs_hip_state_fanout"):  # ... nor for the fan-out of the carried state
        L.rs_hip_state_fanout.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rs_hip_plan_reset_order.argtypes = [C.c_void_p]
    L.rs_hip_set_variant.argtypes = [C.c_void_p, C.c_int32]
    L.rs_hip_set_precision.argtypes = [C.c_void_p, C.c_int32]
    L.rs_hip_div_mismatch_count.argtypes = [C.c_void_p]
    L.rs_hip_div_mismatch_count.restype = C.c_int64
    L.rs_hip_div_special_count.argtypes = [C.c_void_p]
    L.rs_hip_div_special_count.restype = C.c_int64
    L.rs_hip_div_samples.argtypes = [C.c_void_p, C.c_void_p]
    L.rs_hip_test_math.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.rs_hip_timing_reset.argtypes = [C.c_void_p]
    L.rs_hip_timing_step_ms.argtypes = [C.c_void_p, P(C.c_int32)]
    L.rs_hip_timing_step_ms.restype = C.c_double
    L.rs_hip_timing_intervals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    L.rs_hip_timing_intervals.restype = C.c_int32
    L.rs_host_run_batch.argtypes = [C.c_int32, P(abi.OutputPointers), P(abi.InputPointers),
                                    P(RsConstants), P(abi.LocalParameters), P(C.c_double),
                                    P(RsHostExtras), C.c_int32]
    L.rs_sun_table.argtypes = [C.c_int32] + [C.c_void_p] * 7
    L.rs_sun_table.restype = None
    L.rs_point_geometry.argtypes = [C.c_int32, P(abi.LocalParameters)] + [C.c_void_p] * 3
    L.rs_point_geometry.restype = None
    for n in ("rs_abi_sizeof", "rs_fortran_sizeof"):
        getattr(L, n).argtypes = [C.c_int]
        getattr(L, n).restype = C.c_int64
    _lib = L
    return L


def summary_spec(spec) -> RsSummarySpec:
    """RsSummarySpec of anything with ``tsurf_below`` and ``storage_above[5]`` (summary.SummarySpec)."""
    if isinstance(spec, RsSummarySpec):
        return spec
    above = [float(x) for x in spec.storage_above]
    if len(above) != 5:
        raise ValueError("storage_above: five thresholds (snow, water, ice, deposit, ice2)")
    return RsSummarySpec(float(spec.tsurf_below), (C.c_double * 5)(*above))


def group_spec(spec) -> RsGroupSpec:
    """RsGroupSpec of anything with ``thresholds``, ``ngroups`` and ``edges`` (groups.GroupSpec).  More edges than
    the struct holds are cut to that many and their number kept: the library refuses the spec."""
    if isinstance(spec, RsGroupSpec):
        return spec
    edges = [float(x) for x in spec.edges]
    g = RsGroupSpec()
    g.thresholds = summary_spec(spec.thresholds)
    g.ngroups = int(spec.ngroups)
    g.nedges = len(edges)
    for i, e in enumerate(edges[:RS_GRP_MAX_EDGES]):
        g.edges[i] = e
    return g


def group_cols(spec) -> int:
    """Numbers per cell of this spec as the library counts them (rs_hip_group_cols); raises on a spec it refuses."""
    L = load()
    if not hasattr(L, "rs_hip_group_cols"):
        raise RuntimeError("this libroadsurf_hip.so has no group series (rs_hip_group_cols)")
    n = L.rs_hip_group_cols(C.byref(group_spec(spec)))
    if n < 0:
        raise RuntimeError("rs_hip_group_cols: bad spec (ngroups >= 1, at most RS_GRP_MAX_EDGES edges, strictly increasing)")
    return n


def group_path(spec) -> str:
    """Which kernel the host chooses for this spec (rs_hip_group_path): "lds" or "global"."""
    group_cols(spec)
    return {1: "lds", 2: "global"}[load().rs_hip_group_path(C.byref(group_spec(spec)))]


def ens_spec(spec) -> RsEnsSpec:
    """RsEnsSpec of anything with ``ngroups``, ``max_members`` and ``quantiles`` (ensstats.EnsSpec).  More quantiles
    than the struct holds are cut to that many and their number kept: the library refuses the spec."""
    if isinstance(spec, RsEnsSpec):
        return spec
    quant = [float(x) for x in getattr(spec, "quantiles", ())]  # (none: the table of an ensprob.ProbSpec)
    e = RsEnsSpec()
    e.ngroups = int(spec.ngroups)
    e.max_members = int(spec.max_members)
    e.nquant = len(quant)
    for i, q in enumerate(quant[:RS_ENS_MAX_QUANT]):
        e.quant[i] = q
    return e


def ens_cols(spec) -> int:
    """Numbers per cell of this spec as the library counts them (rs_hip_ens_cols); raises on a spec it refuses."""
    L = load()
    if not hasattr(L, "rs_hip_ens_cols"):
        raise RuntimeError("this libroadsurf_hip.so has no ensemble statistics (rs_hip_ens_cols)")
    n = L.rs_hip_ens_cols(C.byref(ens_spec(spec)))
    if n < 0:
        raise RuntimeError("rs_hip_ens_cols: bad spec (ngroups >= 1, 1 <= max_members <= RS_ENS_MAX_MEMBERS, at most "
                           "RS_ENS_MAX_QUANT quantiles in [0, 1], strictly increasing)")
    return n


def episode_spec(spec) -> RsEpisodeSpec:
    """RsEpisodeSpec of anything with ``use``, ``above[7]``, ``below[7]``, ``peak``, ``min_rows`` and
    ``max_episodes`` (episodes.EpisodeSpec).  Nothing is judged here: the library refuses a bad spec."""
    if isinstance(spec, RsEpisodeSpec):
        return spec
    above, below = [float(x) for x in spec.above], [float(x) for x in spec.below]
    if len(above) != RS_EPI_VARS or len(below) != RS_EPI_VARS:
        raise ValueError("above, below: seven bounds (tsurf, snow, water, ice, deposit, ice2, deficit)")
    return RsEpisodeSpec(int(spec.use), int(spec.peak), int(spec.min_rows), int(spec.max_episodes),
                         (C.c_double * RS_EPI_VARS)(*above), (C.c_double * RS_EPI_VARS)(*below))


def episode_cols(spec) -> int:
    """Numbers per point of this spec as the library counts them (rs_hip_episode_cols); raises on a spec it
    refuses."""
    L = load()
    if not hasattr(L, "rs_hip_episode_cols"):
        raise RuntimeError("this libroadsurf_hip.so has no threshold episodes (rs_hip_episode_cols)")
    n = L.rs_hip_episode_cols(C.byref(episode_spec(spec)))
    if n < 0:
        raise RuntimeError("rs_hip_episode_cols: bad spec (use: bits 0..6, at least one; no NaN bound; peak 0..6; "
                           "min_rows >= 1; max_episodes 1..RS_EPI_MAX)")
    return n


def prob_spec(spec) -> RsProbSpec:
    """RsProbSpec of anything with ``ngroups``, ``max_members`` and ``conditions``, each with ``use``, ``above[7]`` and
    ``below[7]`` (ensprob.ProbSpec).  More conditions than the struct holds are cut to that many and their number
    kept; nothing else is judged here: the library refuses a bad spec."""
    if isinstance(spec, RsProbSpec):
        return spec
    s = RsProbSpec()
    s.ngroups = int(spec.ngroups)
    s.max_members = int(spec.max_members)
    s.nconds = len(spec.conditions)
    for i, c in enumerate(list(spec.conditions)[:RS_PROB_MAX_CONDS]):
        above, below = [float(x) for x in c.above], [float(x) for x in c.below]
        if len(above) != RS_EPI_VARS or len(below) != RS_EPI_VARS:
            raise ValueError("above, below: seven bounds (tsurf, snow, water, ice, deposit, ice2, deficit)")
        s.cond[i].use = int(c.use)
        for k in range(RS_EPI_VARS):
            s.cond[i].above[k], s.cond[i].below[k] = above[k], below[k]
    return s


def prob_cols(spec) -> int:
    """Numbers per cell of this spec as the library counts them (rs_hip_prob_cols); raises on a spec it refuses."""
    L = load()
    if not hasattr(L, "rs_hip_prob_cols"):
        raise RuntimeError("this libroadsurf_hip.so has no probabilities over the members (rs_hip_prob_cols)")
    n = L.rs_hip_prob_cols(C.byref(prob_spec(spec)))
    if n < 0:
        raise RuntimeError("rs_hip_prob_cols: bad spec (ngroups >= 1, 1 <= max_members <= RS_ENS_MAX_MEMBERS, 1 .. "
                           "RS_PROB_MAX_CONDS conditions; use: bits 0..6, at least one; no NaN bound)")
    return n


def period_spec(spec) -> RsPeriodSpec:
    """RsPeriodSpec of anything with ``first_index``, ``length``, ``nperiods``, ``tsurf_below`` and
    ``storage_above[5]`` (periods.PeriodSpec).  An integer that does not fit the struct's int32 is a ValueError (ctypes
    would wrap it); nothing else is judged here: the library refuses a bad spec."""
    if isinstance(spec, RsPeriodSpec):
        return spec
    ints = [int(x) for x in (spec.first_index, spec.length, spec.nperiods)]
    if any(not -2**31 <= x < 2**31 for x in ints):
        raise ValueError("first_index, length, nperiods: int32")
    return RsPeriodSpec(*ints, 0, summary_spec(spec))


def period_cols() -> int:
    """Numbers per point and period as the library counts them (rs_hip_period_cols)."""
    L = load()
    if not hasattr(L, "rs_hip_period_cols"):
        raise RuntimeError("this libroadsurf_hip.so has no aggregates over output periods (rs_hip_period_cols)")
    return int(L.rs_hip_period_cols())


def last_error() -> str:
    return (load().rs_last_error() or b"").decode()


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error()}")


def build_constants(settings: abi.InputSettings, params: abi.InputParameters) -> RsConstants:
    """Host-side (Fortran) constants table; needs no GPU."""
    c = RsConstants()
    st = C.c_int32(0)
    load().rs_build_constants(C.byref(settings), C.byref(params), C.byref(c), C.byref(st))
    if st.value != 0:
        raise ValueError("rs_build_constants rejected the settings (NLayers in 5..32, SimLen>=1, DTSecs>0)")
    return c


def bottom_temperature(params: abi.InputParameters, consts: RsConstants, year: int, month: int,
                       day: int) -> float:
    return float(load().rs_bottom_temperature(C.byref(params), C.byref(consts), year, month, day))
