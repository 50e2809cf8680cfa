// k_set_diags.hip -- tracer budget diagnostics, DIAGNOSTICS_TS: set_diags(ng,tile), ROMS/Utility/set_diags.F:28
// (main3d.F:490-492), the rate-of-change statement at the end of step3d_t_tile (step3d_t.F:1598-1611), and the
// library-owned arrays DiaTwrk, DiaTrc, avgzeta and rmask_dia (mod_diags.F, mod_grid.F).
//
// The other DiaTwrk statements sit inside the fused tracer kernels, in their DIA instantiations: k_pre_t
// (pre_step3d.F:894-904), k_t3dmix_s (t3dmix2_s.h:293-296), k_step3d_t_pipe (step3d_t.F:868-871, :1199-1205,
// :1417-1427, :1475-1500).  DiaTwrk and DiaTrc take no halo exchange: a tile owns its IstrR:IendR, JstrR:JendR.
//
// Both kernels here are pure streaming, one thread per point, consecutive lanes along i, blockIdx.z over level x plane
// (as k_avg): per point k_dia_rate reads two doubles and writes one, k_set_diags reads one or two and writes one.
#include "roms_dev.h"
#include <algorithm>

namespace {

struct DiaStore {
  int nDIA = 0, ntsDIA = 0, ntstart = 0, nrrec = 0;
  int ndt = 0, NT = 0, N = 0;
  long nij = 0;
  Guarded wrk, trc, zeta, cnt;                       // DiaTwrk, DiaTrc, avgzeta, rmask_dia (wet_dry)
} g_dia;

const int k_dia_group[DIA_COUNT] = {
#define ROMS_DIA(name, group, what) group,
#define ROMS_DIA_RESERVED(name, what)
#include "roms_dia.def"
#undef ROMS_DIA
#undef ROMS_DIA_RESERVED
};
const char *const k_dia_name[DIA_END] = {
#define ROMS_DIA(name, group, what) #name,
#define ROMS_DIA_RESERVED(name, what)
#include "roms_dia.def"
#undef ROMS_DIA
#undef ROMS_DIA_RESERVED
  "NDT",
#define ROMS_DIA(name, group, what)
#define ROMS_DIA_RESERVED(name, what) #name,
#include "roms_dia.def"
#undef ROMS_DIA
#undef ROMS_DIA_RESERVED
};

// step3d_t.F:1598-1611: DiaTwrk(iTrate) = t(nnew) - DiaTwrk(iTrate) on IstrR:IendR, JstrR:JendR, after t3dbc_tile, the
// nudging and the land/sea mask.  At the interior points DiaTwrk(iTrate) holds Hz*t(nstp)*oHz of this step; at the
// points of a physical boundary nothing has written it since the last step, so the statement as written leaves
// t(nnew) minus the previous step's value there (zero before the first step: the allocation).
// grid: x, y over the R ranges, z = level + N * (itrc - 1)
__global__ void __launch_bounds__(BLK_X *BLK_Y) k_dia_rate(const RomsDev *__restrict__ c, int nnew)
{
  DEV_PROLOGUE(c)
  const int i = b.IstrR + blockIdx.x * BLK_X + threadIdx.x, j = b.JstrR + blockIdx.y * BLK_Y + threadIdx.y;
  if (i > b.IendR || j > b.JendR) return;
  const int k = blockIdx.z % N + 1, itrc = blockIdx.z / N + 1;
  const long q = I3(i, j, k);
  const gcd_t t = (gcd_t)(c->F.t + ((long)(nnew - 1) + 3L * (itrc - 1)) * n3r);
  const gd_t rate = DIA_PLANE(c, DIA_iTrate, itrc, n3r);
  rate[q] = t[q] - rate[q];
}

// set_diags.F:164-190 (INIT) and :288-317: DiaTrc = [rmask_full *] DiaTwrk or DiaTrc + [rmask_full *] DiaTwrk over every
// plane (z < nplanes: level + N * (tracer + NT * term)), avgzeta from zeta(:,:,kout) (z = nplanes; INIT: avgzeta = zeta,
// then avgzeta * rmask_full), and under WET_DRY the counter rmask_dia (z = nplanes + 1; :139-145, :260-267).
struct DiaArgs {
  const double *wrk, *zeta, *full;
  double *trc, *avgzeta, *cnt;
  long ni, nij;
  int nplanes, LBi, LBj, i0, i1, j0, j1;
};
// blockIdx.z of the two kernels: at most NDT * NT * N + 2 with NDT <= DIA_COUNT; roms_hip_set_bounds refuses more
// tracers or levels than these limits
static_assert((long)DIA_COUNT * ROMS_MAXNT * ROMS_MAXN + 2 <= 65535, "level x plane no longer fits gridDim.z: fold planes into blockIdx.y");
template <bool INIT, bool WET>
__global__ void __launch_bounds__(BLK_X *BLK_Y) k_set_diags(const DiaArgs a)
{
  const int i = a.i0 + (int)(blockIdx.x * BLK_X + threadIdx.x), j = a.j0 + (int)(blockIdx.y * BLK_Y + threadIdx.y);
  if (i > a.i1 || j > a.j1) return;
  const long q2 = (long)(i - a.LBi) + (long)(j - a.LBj) * a.ni;
  const int z = blockIdx.z;
  const double m = WET ? ((gcd_t)a.full)[q2] : 1.0;
  if (z < a.nplanes) {
    const long q = q2 + (long)z * a.nij;
    const double w = ((gcd_t)a.wrk)[q];
    const gd_t trc = (gd_t)a.trc;
    if (INIT) trc[q] = WET ? m * w : w;
    else trc[q] = WET ? trc[q] + m * w : trc[q] + w;
  } else if (z == a.nplanes) {
    const double zt = ((gcd_t)a.zeta)[q2];
    const gd_t az = (gd_t)a.avgzeta;
    if (INIT) az[q2] = WET ? zt * m : zt;
    else az[q2] = WET ? az[q2] + m * zt : az[q2] + zt;
  } else if (WET) {
    const double wet = fmax(0.0, fmin(m, 1.0));
    const gd_t cnt = (gd_t)a.cnt;
    cnt[q2] = INIT ? wet : cnt[q2] + wet;
  }
}

bool rotated_mixing(const roms_params_t &p) { return p.ts_dif2 && (p.mix_geo_ts || p.mix_iso_ts); }

// what the diagnostics are not built with; the text names the option
const char *dia_refusal(const roms_bounds_t &b, const roms_params_t &p)
{
  for (int it = 0; it < b.NT; it++) {
    if (p.Hadv[it] == ADV_MPDATA || p.Vadv[it] == ADV_MPDATA) return "diagnostics: MPDATA tracers are not built with DIAGNOSTICS_TS";
    if (p.Hadv[it] == ADV_HSIMT || p.Vadv[it] == ADV_HSIMT) return "diagnostics: HSIMT tracers are not built with DIAGNOSTICS_TS";
  }
  if (p.ts_dif4) return "diagnostics: TS_DIF4 is not built with DIAGNOSTICS_TS";
  if (rotated_mixing(p))
    return "diagnostics: rotated mixing (MIX_GEO_TS / MIX_ISO_TS, iTsdif) is not built with DIAGNOSTICS_TS";
  if (p.point_sources & 3) return "diagnostics: point sources (LuvSrc / LwSrc / LtracerSrc) are not built with DIAGNOSTICS_TS";
  return nullptr;
}

}  // namespace

// The reference's idiag of a term (mod_scalars.F:4027-4043): 1 + the number of present terms before it; NDT for
// dia_id = DIA_COUNT (mod_param.F:1380-1389).  0: the term is not present.
extern "C" int roms_hip_dia_index(int dia_id, int hdif, int rotated)
{
  if (dia_id < 0 || dia_id > DIA_COUNT) return 0;
  auto present = [&](int id) {
    return k_dia_group[id] == DIA_ALWAYS || (k_dia_group[id] == DIA_HDIF && hdif) || (k_dia_group[id] == DIA_ROT && hdif && rotated);
  };
  if (dia_id < DIA_COUNT && !present(dia_id)) return 0;
  int n = 0;
  for (int id = 0; id < dia_id; id++) n += present(id);
  return dia_id < DIA_COUNT ? n + 1 : n;
}

// (roms_hip_set_bounds: the tracer diagnostics have the old extents)
void dia_release()
{
  for (Guarded *a : {&g_dia.wrk, &g_dia.trc, &g_dia.zeta, &g_dia.cnt}) guarded_free(a);
  g_dia = DiaStore{};
  if (g_ctx.hostc.dia.wrk) {
    memset(&g_ctx.hostc.dia, 0, sizeof g_ctx.hostc.dia);
    g_ctx.devc_dirty = true;
  }
}

bool dia_on() { return g_dia.wrk.dev != nullptr; }

int dia_check(const char *where)
{
  if (!dia_on()) return 0;
  const roms_bounds_t &b = g_ctx.b;
  const roms_params_t &p = g_ctx.p;
  if (const char *why = dia_refusal(b, p)) return roms_fail(where, why);
  if (g_dia.ndt != roms_hip_dia_index(DIA_COUNT, p.ts_dif2, 0))
    return roms_fail(where, "diagnostics: ts_dif2 changed after roms_hip_set_diagnostics (NDT differs); call it again");
  if (b.N > ROMS_MAXN) return roms_fail(where, "N > 64 not instantiated");
  return 0;
}

int dia_rate(int nnew)
{
  const roms_bounds_t &b = g_ctx.b;
  ScopedTimer tm("step3d_t_diags");
  const dim3 grid((b.IendR - b.IstrR + BLK_X) / BLK_X, (b.JendR - b.JstrR + BLK_Y) / BLK_Y, b.N * b.NT);
  hipLaunchKernelGGL(k_dia_rate, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, nnew);
  KERNEL_CHECK("k_dia_rate");
  return 0;
}

extern "C" int roms_hip_set_diagnostics(int nDIA, int ntsDIA, int ntstart, int nrrec)
{
  const char *me = "roms_hip_set_diagnostics";
  if (int rc = roms_setup_check(me)) return rc;
  if (nDIA < 0) return roms_fail(me, "diagnostics: nDIA < 0");
  if (nDIA == 0) {                                        // set_diags.F:113
    if (dia_on()) HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    dia_release();
    return 0;
  }
  const roms_bounds_t &b = g_ctx.b;
  const roms_params_t &p = g_ctx.p;
  if (const char *why = dia_refusal(b, p)) return roms_fail(me, why);
  if (b.N > ROMS_MAXN) return roms_fail(me, "N > 64 not instantiated");
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  dia_release();
  const long nij = (long)(b.UBi - b.LBi + 1) * (long)(b.UBj - b.LBj + 1);
  g_dia.nDIA = nDIA; g_dia.ntsDIA = ntsDIA; g_dia.ntstart = ntstart; g_dia.nrrec = nrrec;
  g_dia.ndt = roms_hip_dia_index(DIA_COUNT, p.ts_dif2, 0);
  g_dia.NT = b.NT; g_dia.N = b.N; g_dia.nij = nij;
  const long n4 = nij * b.N * b.NT * g_dia.ndt;
  int rc = guarded_alloc(&g_dia.wrk, "DiaTwrk", -1, n4);      // zeroed, as mod_diags.F allocates them
  if (!rc) rc = guarded_alloc(&g_dia.trc, "DiaTrc", -1, n4);
  if (!rc) rc = guarded_alloc(&g_dia.zeta, "avgzeta (diagnostics)", -1, nij);
  if (!rc && p.wet_dry) rc = guarded_alloc(&g_dia.cnt, "rmask_dia", -1, nij);
  if (rc) { dia_release(); return rc; }
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  RomsDia &d = g_ctx.hostc.dia;
  d.wrk = g_dia.wrk.dev;
  d.ndt = g_dia.ndt;
  for (int id = 0; id < DIA_COUNT; id++) d.ix[id] = roms_hip_dia_index(id, p.ts_dif2, 0) - 1;
  g_ctx.devc_dirty = true;
  return 0;
}

extern "C" int roms_hip_set_diags(const roms_step_idx_t *s)
{
  const char *me = "roms_hip_set_diags";
  if (!g_ctx.inited) return roms_fail(me, "library not initialised");
  if (!dia_on()) return 0;                                 // no roms_hip_set_diagnostics, or nDIA = 0: set_diags.F:113
  int rc = roms_entry_check(me);
  if (rc) return rc;
  if (!s) return roms_fail(me, "null argument");
  if ((rc = dia_check(me))) return rc;
  // set_diags.F:121-124 and :244 = the initialise / accumulate part of the averages' schedule
  const int phase = roms_hip_avg_phase(s->iic, g_dia.nDIA, g_dia.ntsDIA, g_dia.ntstart, g_dia.nrrec);
  if (!(phase & (AVP_SET | AVP_ADD))) return 0;
  if (s->kstp < 1 || s->kstp > 3) return roms_fail(me, "diagnostics: kstp outside 1..3");
  const roms_bounds_t &b = g_ctx.b;
  const bool wet = g_ctx.p.wet_dry != 0;
  const long ni = b.UBi - b.LBi + 1, nij = ni * (long)(b.UBj - b.LBj + 1);
  if (nij != g_dia.nij || b.N != g_dia.N || b.NT != g_dia.NT) return roms_fail(me, "diagnostics: the arrays have other extents than the bounds");
  if (wet && !g_dia.cnt.dev) return roms_fail(me, "diagnostics: wet_dry was switched on after roms_hip_set_diagnostics; call it again");
  if (!g_ctx.field[FID_zeta].dev) return roms_fail(me, "diagnostics: zeta is not registered");
  if (wet && !g_ctx.field[FID_rmask_full].dev) return roms_fail(me, "diagnostics: rmask_full is not registered");
  ScopedTimer tm("set_diags");
  DiaArgs a;
  a.wrk = g_dia.wrk.dev; a.trc = g_dia.trc.dev; a.avgzeta = g_dia.zeta.dev; a.cnt = g_dia.cnt.dev;
  a.zeta = g_ctx.field[FID_zeta].dev + (long)(s->kstp - 1) * nij;          // KOUT = kstp
  a.full = wet ? g_ctx.field[FID_rmask_full].dev : nullptr;
  a.ni = ni; a.nij = nij; a.LBi = b.LBi; a.LBj = b.LBj;
  a.nplanes = g_dia.ndt * b.NT * b.N;
  // never outside the allocation, whatever the bounds say
  a.i0 = std::max(b.IstrR, b.LBi); a.i1 = std::min(b.IendR, b.UBi);
  a.j0 = std::max(b.JstrR, b.LBj); a.j1 = std::min(b.JendR, b.UBj);
  dim3 grid = grid2d(a.i1 - a.i0 + 1, a.j1 - a.j0 + 1);
  grid.z = (unsigned)(a.nplanes + (wet ? 2 : 1));
  const bool init = (phase & AVP_SET) != 0;
  if (wet) {
    if (init) hipLaunchKernelGGL((k_set_diags<true, true>), grid, block2d(), 0, g_ctx.stream, a);
    else hipLaunchKernelGGL((k_set_diags<false, true>), grid, block2d(), 0, g_ctx.stream, a);
  } else {
    if (init) hipLaunchKernelGGL((k_set_diags<true, false>), grid, block2d(), 0, g_ctx.stream, a);
    else hipLaunchKernelGGL((k_set_diags<false, false>), grid, block2d(), 0, g_ctx.stream, a);
  }
  KERNEL_CHECK("k_set_diags");
  return 0;
}

extern "C" int roms_hip_get_diagnostic(int dia_id, int itrc, int accumulated, double *host, long n_doubles)
{
  const char *me = "roms_hip_get_diagnostic";
  if (!g_ctx.inited) return roms_fail(me, "library not initialised");
  if (dia_id < 0 || dia_id >= DIA_END || dia_id == DIA_COUNT) return roms_fail(me, "diagnostics: bad id");
  if (!dia_on()) return roms_fail(me, "diagnostics: not switched on (roms_hip_set_diagnostics)");
  const double *src;
  long n;
  if (dia_id == DIA_avgzeta) { src = g_dia.zeta.dev; n = g_dia.nij; }
  else if (dia_id == DIA_rmask_dia) {
    if (!g_dia.cnt.dev) return roms_fail(me, "diagnostics: rmask_dia exists with wet_dry only");
    src = g_dia.cnt.dev; n = g_dia.nij;
  } else {
    const int ix = g_ctx.hostc.dia.ix[dia_id];
    if (ix < 0) {
      const std::string m = std::string("diagnostics: ") + k_dia_name[dia_id] + " is not a term of this configuration (NDT = " +
                            std::to_string(g_dia.ndt) + ")";
      return roms_fail(me, m.c_str());
    }
    if (itrc < 1 || itrc > g_dia.NT) return roms_fail(me, "diagnostics: itrc outside 1..NT");
    n = g_dia.nij * g_dia.N;
    src = (accumulated ? g_dia.trc : g_dia.wrk).dev + ((long)ix * g_dia.NT + (itrc - 1)) * n;
  }
  if (!host) return roms_fail(me, "diagnostics: host array is NULL");
  return roms_copy_out(me, "diagnostics", k_dia_name[dia_id], src, n, host, n_doubles);
}
