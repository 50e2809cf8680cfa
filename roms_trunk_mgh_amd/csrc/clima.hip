// clima.hip -- climatology nudging (mod_clima.F:190-261), LnudgeM2CLM / LnudgeM3CLM / LnudgeTCLM: the eight device
// copies of CLIMA(ng) (RomsClima, roms_dev.h), each with its guard bands, roms_hip_set_clima and roms_hip_get_clima.
// Host code only: the kernels that nudge are the step kernels.
#include "roms_dev.h"
#include <algorithm>

namespace {
enum { CL_M2nudgcof = 0, CL_ubarclm, CL_vbarclm, CL_M3nudgcof, CL_uclm, CL_vclm, CL_Tnudgcof, CL_tclm, CL_COUNT };
const char *const k_clima_name[CL_COUNT] = {"M2nudgcof", "ubarclm", "vbarclm", "M3nudgcof", "uclm", "vclm", "Tnudgcof", "tclm"};
Guarded g_clima[CL_COUNT];
}  // namespace

// (roms_hip_set_bounds: the climatology has the old extents)
void clima_release()
{
  for (int q = 0; q < CL_COUNT; q++) guarded_free(&g_clima[q]);
  g_ctx.hostc.clima = RomsClima{};
  g_ctx.devc_dirty = true;
}

extern "C" int roms_hip_set_clima(int LnudgeM2CLM, const double *M2nudgcof, const double *ubarclm, const double *vbarclm,
                                  int LnudgeM3CLM, const double *M3nudgcof, const double *uclm, const double *vclm,
                                  const int *LnudgeTCLM, const double *Tnudgcof, const double *tclm, double obcfac)
{
  const char *me = "roms_hip_set_clima";
  if (int rc = roms_setup_check(me)) return rc;
  if (!(obcfac >= 0.0)) return roms_fail(me, "climatology: obcfac < 0");
  const roms_bounds_t &b = g_ctx.b;
  const long nij = (long)(b.UBi - b.LBi + 1) * (long)(b.UBj - b.LBj + 1);
  RomsClima want{};
  want.m2 = LnudgeM2CLM != 0;
  want.m3 = LnudgeM3CLM != 0;
  want.obcfac = obcfac;
  for (int it = 0; it < b.NT; it++)
    if (LnudgeTCLM && LnudgeTCLM[it]) {
      want.itrc[want.nt] = it + 1;
      want.ic[it] = ++want.nt;
    }
  const RomsClima &have = g_ctx.hostc.clima;
  if (!want.m2 && !want.m3 && !want.nt) {              // all flags zero: release everything
    if (have.m2 || have.m3 || have.nt) {
      HIP_TRY(hipStreamSynchronize(g_ctx.stream));
      step2d_graphs_release();
      clima_release();
    }
    return 0;
  }
  const bool same = want.m2 == have.m2 && want.m3 == have.m3 && std::equal(want.ic, want.ic + ROMS_MAXNT, have.ic);
  const double *host[CL_COUNT] = {M2nudgcof, ubarclm, vbarclm, M3nudgcof, uclm, vclm, Tnudgcof, tclm};
  const long n[CL_COUNT] = {nij, nij, nij, nij * b.N, nij * b.N, nij * b.N, nij * b.N * want.nt, nij * b.N * want.nt};
  const bool on[CL_COUNT] = {want.m2 != 0, want.m2 != 0, want.m2 != 0, want.m3 != 0, want.m3 != 0, want.m3 != 0,
                             want.nt != 0, want.nt != 0};
  // a NULL array = "keep the copy you have": only with the flags of the call that gave it.  Nothing is touched
  // before every argument has been looked at, so that a refused call leaves the library as it was.
  for (int q = 0; q < CL_COUNT; q++)
    if (on[q] && !host[q] && !(same && g_clima[q].dev)) {
      const std::string m = std::string("climatology: the switch of ") + k_clima_name[q] + " is set but the array was never "
                            "given (NULL keeps an earlier copy only after a call with the same switches that brought one)";
      return roms_fail(me, m.c_str());
    }
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  // the boundary-condition launches inside the captured LOOP_2D graphs hold the coefficient address and obcfac
  if (!same || want.obcfac != have.obcfac) step2d_graphs_release();
  if (!same) clima_release();
  for (int q = 0; q < CL_COUNT; q++) {
    if (!on[q] || !host[q]) continue;
    if (!g_clima[q].dev) {
      int rc = guarded_alloc(&g_clima[q], k_clima_name[q], -1, n[q]);
      if (rc) { clima_release(); return rc; }
    }
    HIP_TRY(hipMemcpyAsync(g_clima[q].dev, host[q], sizeof(double) * n[q], hipMemcpyHostToDevice, g_ctx.stream));
  }
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  want.M2nudgcof = g_clima[CL_M2nudgcof].dev; want.ubarclm = g_clima[CL_ubarclm].dev; want.vbarclm = g_clima[CL_vbarclm].dev;
  want.M3nudgcof = g_clima[CL_M3nudgcof].dev; want.uclm = g_clima[CL_uclm].dev; want.vclm = g_clima[CL_vclm].dev;
  want.Tnudgcof = g_clima[CL_Tnudgcof].dev; want.tclm = g_clima[CL_tclm].dev;
  g_ctx.hostc.clima = want;
  g_ctx.devc_dirty = true;
  return 0;
}

// One of the eight device copies back to the host (tests; a host that writes the interpolated climatology out).
extern "C" int roms_hip_get_clima(const char *name, double *host, long n_doubles)
{
  const char *me = "roms_hip_get_clima";
  if (!g_ctx.inited) return roms_fail(me, "library not initialised");
  if (!name || !host) return roms_fail(me, "climatology: null argument");
  for (int q = 0; q < CL_COUNT; q++) {
    if (strcmp(name, k_clima_name[q])) continue;
    if (!g_clima[q].dev) return roms_fail(me, (std::string("climatology: the library has no copy of ") + name + " (roms_hip_set_clima)").c_str());
    return roms_copy_out(me, "climatology", name, g_clima[q].dev, g_clima[q].count, host, n_doubles);
  }
  return roms_fail(me, (std::string("climatology: unknown array ") + name).c_str());
}
