/*
 * oracle/driver_ref_harness.cpp — TEST INFRASTRUCTURE, our own code.
 *
 * A C surface over the reference's own example driver (the .cpp files of examples/example1/src), linked
 * with those twelve files into oracle/_ref/libroadrunner_ref.so by oracle/build_ref.sh.
 * roadrunner.cpp is compiled with -Dmain=roadrunner_ref_main, so read_input, get_times,
 * parse_options and the global `options` are linkable; <json/json.h> and <fmt/format.h> are
 * the stand-ins of oracle/shim.  The harness follows main() and run_locations_sync
 * (roadrunner.cpp) up to the call of runsimulation and copies out what the reference holds
 * there; it decides nothing itself.  No C++ exception leaves it: each call returns 0 or -1
 * and rr_ref_error() has the message.
 */
#include "DataHandler.h"
#include "InputData.h"
#include "InputParameters.h"
#include "InputSettings.h"
#include "JsonTools.h"
#include "LocalParameters.h"
#include "OutputData.h"
#include "SkyView.h"

#include <unistd.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

/* roadrunner.cpp */
extern Options options;
bool parse_options(int argc, char* argv[]);
std::vector<time_t> get_times(const InputSettings& pSettings);
InputData read_input(InputSettings& pSettings, const std::vector<time_t> pTimes, const DataHandler& pDataHandler,
                     const InputParameters& parameters, LocalParameters& lParameters, SkyView& skyview, int pointID,
                     bool& success);
extern "C" void runsimulation(OutputPointers* pOutputPointers, const InputPointers* pInputPointers,
                              const InputSettings* pSettings, const InputParameters* pInputParams,
                              const LocalParameters* lParameters);

namespace {

struct Handle {
  Json::Value json;
  std::unique_ptr<InputSettings> settings;
  DataHandler data;
  std::unique_ptr<InputParameters> params;
  std::unique_ptr<SkyView> sky;
  std::vector<time_t> times;
  std::vector<int> ids;
  std::vector<LocalParameters> locations;
};

thread_local std::string g_error;

template <class F>
int guarded(F&& f) {
  try {
    g_error.clear();
    f();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
  } catch (...) {
    g_error = "unknown C++ exception";
  }
  return -1;
}

void copy_local(const LocalParameters& lp, double* d, int32_t* i) {
  d[0] = lp.tair_relax;
  d[1] = lp.VZ_relax;
  d[2] = lp.RH_relax;
  d[3] = lp.couplingTsurf;
  d[4] = lp.lat;
  d[5] = lp.lon;
  d[6] = lp.sky_view;
  i[0] = lp.couplingIndexI;
  i[1] = lp.InitLenI;
}

/* series [10][SimLen] in the order tair tdew VZ Rhz prec SW LW SW_dir LW_net TSurfObs;
 * calendar [7][SimLen] in the order year month day hour minute second, then PrecPhase */
void copy_input(const InputData& in, int L, double* series, int32_t* cal, double* horizons, int32_t* n_horizons) {
  const std::vector<double>* s[10] = {&in.tair, &in.tdew, &in.VZ,     &in.Rhz,    &in.prec,
                                      &in.SW,   &in.LW,   &in.SW_dir, &in.LW_net, &in.TSurfObs};
  const std::vector<int>* c[7] = {&in.year, &in.month, &in.day, &in.hour, &in.minute, &in.second, &in.PrecPhase};
  for (int f = 0; f < 10; ++f)
    for (int i = 0; i < L; ++i) series[(size_t)f * L + i] = s[f]->at(i);
  for (int f = 0; f < 7; ++f)
    for (int i = 0; i < L; ++i) cal[(size_t)f * L + i] = c[f]->at(i);
  *n_horizons = static_cast<int32_t>(in.local_horizons.size());
  for (size_t i = 0; i < in.local_horizons.size() && i < 360; ++i) horizons[i] = in.local_horizons[i];
}

}  // namespace

extern "C" {

const char* rr_ref_error(void) { return g_error.c_str(); }

/* roadrunner.cpp's own reading of `-t TEXT -c CONFIG`: options.time, or -1 */
int64_t rr_ref_cli_time(const char* text, const char* config) {
  int64_t t = -1;
  guarded([&] {
    std::string a0 = "roadrunner", a1 = "-t", a2 = text, a3 = "-c", a4 = config;
    char* argv[] = {&a0[0], &a1[0], &a2[0], &a3[0], &a4[0], nullptr};
    optind = 1;
    options = Options();
    options.time = 0;
    parse_options(5, argv);
    t = static_cast<int64_t>(options.time);
  });
  return t;
}

/* main() up to run(), then run_locations_sync up to its loop.  cli_time: what -t gives, 0 = not given */
void* rr_ref_open(const char* config_path, int64_t cli_time) {
  Handle* h = nullptr;
  int rc = guarded([&] {
    std::unique_ptr<Handle> u(new Handle);
    options = Options();
    options.configfile = config_path;
    options.time = static_cast<time_t>(cli_time);
    u->json = read_json(options.configfile);
    u->settings.reset(new InputSettings{u->json, options});
    InputSettings& s = *u->settings;
    u->data.init(s.forecast_time, s.start_time, s.end_time, u->json, s.SimLen, s.DTSecs);
    Json::Value nulljson;
    u->params.reset(new InputParameters{s, u->json.get("parameters", nulljson)});
    u->sky.reset(new SkyView(u->json.get("parameters", nulljson)));
    u->times = get_times(s);
    u->locations = u->data.GetLocations();
    u->ids = u->data.GetPointIDs();
    h = u.release();
  });
  return rc == 0 ? h : nullptr;
}

void rr_ref_close(void* handle) { delete static_cast<Handle*>(handle); }

/* ints: SimLen use_coupling use_relaxation NLayers coupling_minutes outputStep
 * reals: DTSecs tsurfOutputDepth couplingEffectReduction;  times: forecast start end */
void rr_ref_settings(void* handle, int32_t* ints, double* reals, int64_t* times) {
  const InputSettings& s = *static_cast<Handle*>(handle)->settings;
  ints[0] = s.SimLen;
  ints[1] = s.use_coupling;
  ints[2] = s.use_relaxation;
  ints[3] = s.NLayers;
  ints[4] = s.coupling_minutes;
  ints[5] = s.outputStep;
  reals[0] = s.DTSecs;
  reals[1] = s.tsurfOutputDepth;
  reals[2] = s.couplingEffectReduction;
  times[0] = static_cast<int64_t>(s.forecast_time);
  times[1] = static_cast<int64_t>(s.start_time);
  times[2] = static_cast<int64_t>(s.end_time);
}

/* the members of InputParameters in the order of InputParameters.h; returns their number */
int32_t rr_ref_parameters(void* handle, double* out, int32_t capacity) {
  const InputParameters& p = *static_cast<Handle*>(handle)->params;
  const double v[] = {
      p.NightOn, p.NightOff, p.CalmLimDay, p.CalmLimNgt, p.TrfFricNgt, p.TrFfricDay,
      p.Grav, p.SB_Const, p.VK_Const, p.LVap, p.LFus, p.WatDens, p.SnowDens, p.IceDens, p.DepDens, p.WatMHeat,
      p.PorEvaF,
      p.ZRefW, p.ZRefT, p.ZeroDisp, p.ZMom, p.ZHeat, p.Emiss, p.Albedo, p.Albedo_surroundings, p.MaxPormms,
      p.TClimG, p.DampDpth, p.Omega, p.AZ, p.DampWearF, p.AlbDry, p.AlbSnow, p.vsh1, p.vsh2, p.Poro1, p.Poro2,
      p.RhoB1, p.RhoB2, p.Silt1, p.Silt2,
      p.freezing_limit_normal, p.snow_melting_limit_normal, p.ice_melting_limit_normal,
      p.frost_melting_limit_normal, p.frost_formation_limit_normal, p.T4Melt_normal,
      p.TLimColdH, p.TLimColdL, p.WetSnowFormR, p.WetSnowMeltR,
      p.PLimSnow, p.PLimRain, p.MaxSnowmms, p.MaxDepmms, p.MaxIcemms, p.MaxExtmms,
      p.MissValI, p.MissValR,
      p.Snow2IceFac,
      p.MinPrecmm, p.MinWatmms, p.MinSnowmms, p.MaxWatmms, p.WDampLim, p.WWetLim, p.WWearLim, p.MinDepmms,
      p.MinIcemms};
  const int32_t n = static_cast<int32_t>(sizeof v / sizeof v[0]);
  for (int32_t i = 0; i < n && i < capacity; ++i) out[i] = v[i];
  return n;
}

int32_t rr_ref_n_stations(void* handle) { return static_cast<int32_t>(static_cast<Handle*>(handle)->ids.size()); }

/* GetPointIDs() and GetLocations() */
void rr_ref_stations(void* handle, int32_t* ids, double* lat, double* lon) {
  const Handle& h = *static_cast<Handle*>(handle);
  for (size_t k = 0; k < h.ids.size(); ++k) {
    ids[k] = h.ids[k];
    lat[k] = h.locations[k].lat;
    lon[k] = h.locations[k].lon;
  }
}

/* read_input for station k as run_locations_sync calls it.
 * local_d: tair_relax VZ_relax RH_relax couplingTsurf lat lon sky_view;  local_i: couplingIndexI InitLenI */
int32_t rr_ref_read_input(void* handle, int32_t k, double* series, int32_t* cal, double* horizons,
                          int32_t* n_horizons, double* local_d, int32_t* local_i, int32_t* success) {
  Handle& h = *static_cast<Handle*>(handle);
  return guarded([&] {
    LocalParameters lp = h.locations.at(k);
    bool ok = false;
    const InputData in = read_input(*h.settings, h.times, h.data, *h.params, lp, *h.sky, h.ids.at(k), ok);
    copy_input(in, h.settings->SimLen, series, cal, horizons, n_horizons);
    copy_local(lp, local_d, local_i);
    *success = ok ? 1 : 0;
  });
}

/* read_input + runsimulation for station k; out [6][SimLen] in the order
 * TsurfOut SnowOut WaterOut IceOut DepositOut Ice2Out (untouched -9999.0 where read_input refuses) */
int32_t rr_ref_run(void* handle, int32_t k, double* out, int32_t* success) {
  Handle& h = *static_cast<Handle*>(handle);
  return guarded([&] {
    LocalParameters lp = h.locations.at(k);
    bool ok = false;
    const InputData in = read_input(*h.settings, h.times, h.data, *h.params, lp, *h.sky, h.ids.at(k), ok);
    const int L = h.settings->SimLen;
    OutputData o(L);
    if (ok) {
      auto outPointers = o.pointers();
      auto inPointers = in.pointers();
      runsimulation(&outPointers, &inPointers, h.settings.get(), h.params.get(), &lp);
    }
    const std::vector<double>* s[6] = {&o.TsurfOut, &o.SnowOut, &o.WaterOut, &o.IceOut, &o.DepositOut, &o.Ice2Out};
    for (int f = 0; f < 6; ++f)
      for (int i = 0; i < L; ++i) out[(size_t)f * L + i] = s[f]->at(i);
    *success = ok ? 1 : 0;
  });
}

}  // extern "C"
