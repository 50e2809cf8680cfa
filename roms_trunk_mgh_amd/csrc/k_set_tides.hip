// k_set_tides.hip -- tidal forcing of the open boundaries: set_tides_tile (ROMS/Nonlinear/set_tides.F:116-643) with
// SSH_TIDES and / or UV_TIDES, with or without MASKING, RAMP_TIDES, ADD_FSOBC, ADD_M2OBC.  Not built: AVERAGES_DETIDE,
// TIDE_GENERATING_FORCES, the CLIMA(ng)%ssh / ubarclm / vbarclm additions of the two ADD options (:301-319, :480-507).
//
// roms_hip_set_tides (configuration) gathers, per edge, the two lines of rho-points the edge loads read into edge-major
// strips (RomsTides, roms_dev.h), one constituent plane at a time; roms_hip_tides (per step) evaluates the harmonics on
// those strips and writes zeta_bry, ubar_bry, vbar_bry at the points the *_bry convention gives the reference's edge
// vectors (roms_fields.def: the value of a boundary point sits AT that point), in ONE launch: one thread per boundary
// point, blockIdx.y = edge x variable, the constituent loop in registers.  Latency-bound by construction.
//
// No exchange: every value comes from harmonic constants at the tile's own points plus one ghost point (Uwrk(Istr-1,j),
// Vwrk(i,Jstr-1) on a tile that is not on the western / southern edge; the periodic image with E-W periodicity), which
// the host supplies filled, as the reference's TIDES(ng) arrays are after their read and exchange.
//
// The four corner rho-points.  The reference keeps four zeta vectors; zeta_west(Jstr-1) and zeta_south(Istr-1) are two
// numbers (means over different pairs of points) that the *_bry layout maps to the one point (Istr-1,Jstr-1).  No
// condition reads either of them: the edge loops of zetabc, u2dbc and v2dbc run over Jstr:Jend / Istr:Iend and the
// corner values are the means of their two neighbours (zetabc.F:699-731).  The four points are therefore left
// untouched.  The ubar / vbar vectors agree where they overlap (ubar_west(Jstr-1) = Utide(Istr,Jstr-1) =
// ubar_south(Istr) ...): both edges store the same bits.
#include "roms_dev.h"
#include <vector>

namespace {
enum { TS_amp = 0, TS_eph, TS_ang, TS_uph, TS_maj, TS_mnr, TS_angler, TS_rmask, TS_umask, TS_vmask, TS_zbase, TS_ubase,
       TS_vbase, TS_COUNT };
struct TidesStore {
  double *dev[TS_COUNT] = {nullptr};
} g_tides;
}  // namespace

// (roms_hip_set_bounds: the tidal strips have the old extents)
void tides_release()
{
  for (int q = 0; q < TS_COUNT; q++) {
    if (g_tides.dev[q]) (void)hipFree(g_tides.dev[q]);
    g_tides.dev[q] = nullptr;
  }
  g_ctx.hostc.tides = RomsTides{};
  g_ctx.devc_dirty = true;
}

// boundary data of variable v are "acquired" on side sd (inp_decode.F:1621-1655, no FSOBC_REDUCED): Cla, Fla, Shc, RadNud
// set it; Fla / Shc on ubar or vbar set the free surface's too
static bool tides_acquire(int sd, int v)
{
  const roms_params_t &p = g_ctx.p;
  auto own = [&](int w) {
    const int c = lbc_code(p, sd, w);
    return c == LBC_CLAMPED || c == LBC_FLATHER || c == LBC_SHCHEPETKIN || c == LBC_RADIATION_NUDGING;
  };
  auto fs = [&](int w) {
    const int c = lbc_code(p, sd, w);
    return c == LBC_FLATHER || c == LBC_SHCHEPETKIN;
  };
  if (v == LBV_ZETA) return own(LBV_ZETA) || fs(LBV_UBAR) || fs(LBV_VBAR);
  return own(v);
}

// Uwrk / Vwrk of one constituent at strip element s (set_tides.F:443-452); omega = cff / Tperiod(itide)
template <bool V>
__device__ __forceinline__ double tide_wrk(const RomsTides &T, long s, long q, double omega)
{
  const double angle = T.ang[q] - T.angler[s];
  const double Cangle = cos(angle), Sangle = sin(angle);
  const double phase = omega - T.uph[q];
  const double Cphase = cos(phase), Sphase = sin(phase);
  return V ? T.maj[q] * Sangle * Cphase + T.mnr[q] * Cangle * Sphase
           : T.maj[q] * Cangle * Cphase - T.mnr[q] * Sangle * Sphase;
}

// grid: x = position along the edge, y = 3 * edge + variable (0 zeta, 1 ubar, 2 vbar).  zmask / uvmask: bit sd set = the
// reference's IF of that side holds (:332-334 ..., :512-513 ...).  cff = 2 pi (time - tide_start * day2sec).
__global__ void __launch_bounds__(64) k_set_tides(const RomsDev *__restrict__ c, double cff, double ramp, int zmask, int uvmask)
{
  DEV_PROLOGUE(c)
  const RomsTides &T = c->tides;
  const int e = blockIdx.y / 3, var = blockIdx.y % 3;
  const bool we = e <= LBS_EAST, hi = e == LBS_EAST || e == LBS_NORTH;
  if (!(e == LBS_WEST ? b.west_edge : e == LBS_EAST ? b.east_edge : e == LBS_SOUTH ? b.south_edge : b.north_edge)) return;
  if (we ? b.EWperiodic : b.NSperiodic) return;
  if (var == 0 ? !(T.ssh && ((zmask >> e) & 1)) : !(T.uv && ((uvmask >> e) & 1))) return;
  const int a = T.lb[e] + blockIdx.x * blockDim.x + threadIdx.x;
  // the reference's ranges: zeta JstrR:JendR / IstrR:IendR; ubar JstrR:JendR / Istr:IendR; vbar Jstr:JendR / IstrR:IendR
  int a0, a1;
  if (we) { a0 = var == 2 ? b.Jstr : b.JstrR; a1 = b.JendR; }
  else { a0 = var == 1 ? b.Istr : b.IstrR; a1 = b.IendR; }
  if (a < a0 || a > a1) return;
  const long s0 = T.off[e] + (a - T.lb[e]), s1 = s0 + T.len[e];        // outside line, inside line
  const long sm = T.off[e] / 2 + (a - T.lb[e]);                        // umask / vmask line
  const long tot = T.tot;
  int bi, bj;                                                          // the point of *_bry
  double x = 0.0;
  if (var == 0) {
    // the four corner rho-points are left alone (see the header)
    if (we ? ((a == b.Jstr - 1 && b.south_edge) || (a == b.Jend + 1 && b.north_edge))
           : ((a == b.Istr - 1 && b.west_edge) || (a == b.Iend + 1 && b.east_edge))) return;
    double E0 = 0.0, E1 = 0.0;                                         // Etide outside / inside (:279-295)
    for (int it = 0; it < T.ntc; it++) {
      if (!(T.Tperiod[it] > 0.0)) continue;
      const double omega = cff / T.Tperiod[it];
      const long q = (long)it * tot;
      E0 = E0 + ramp * T.amp[q + s0] * cos(omega - T.eph[q + s0]);
      E1 = E1 + ramp * T.amp[q + s1] * cos(omega - T.eph[q + s1]);
      if (T.rmask) { E0 = E0 * T.rmask[s0]; E1 = E1 * T.rmask[s1]; }
    }
    x = hi ? 0.5 * (E1 + E0) : 0.5 * (E0 + E1);                        // :339-341, :363-365, :387-389, :411-413
    bi = we ? (hi ? b.Iend + 1 : b.Istr - 1) : a;
    bj = we ? a : (hi ? b.Jend + 1 : b.Jstr - 1);
  } else {
    // the two rho-points a u- / v-point averages, lower index first (:455-472)
    long p0, p1;
    const bool vt = var == 2;
    if (we == !vt) { p0 = hi ? s1 : s0; p1 = hi ? s0 : s1; }           // across the edge: ubar on W / E, vbar on S / N
    else { p0 = s0 - 1; p1 = s0; }                                     // along the outside line
    double acc = 0.0;
    const double *M = vt ? T.vmask : T.umask;
    for (int it = 0; it < T.ntc; it++) {
      if (!(T.Tperiod[it] > 0.0)) continue;
      const double omega = cff / T.Tperiod[it];
      const long q = (long)it * tot;
      const double w0 = vt ? tide_wrk<true>(T, p0, q + p0, omega) : tide_wrk<false>(T, p0, q + p0, omega);
      const double w1 = vt ? tide_wrk<true>(T, p1, q + p1, omega) : tide_wrk<false>(T, p1, q + p1, omega);
      acc = acc + ramp * 0.5 * (w0 + w1);
      if (T.rmask) acc = acc * M[sm];
    }
    x = acc;
    // ubar_west = Utide(Istr,j), ubar_east = Utide(Iend+1,j), ubar_south = Utide(i,Jstr-1), ubar_north = Utide(i,Jend+1);
    // vbar_west = Vtide(Istr-1,j), vbar_east = Vtide(Iend+1,j), vbar_south = Vtide(i,Jstr), vbar_north = Vtide(i,Jend+1)
    if (we) { bi = hi ? b.Iend + 1 : (vt ? b.Istr - 1 : b.Istr); bj = a; }
    else { bi = a; bj = hi ? b.Jend + 1 : (vt ? b.Jstr : b.Jstr - 1); }
  }
  const long B = I2(bi, bj);
  // ADD_FSOBC / ADD_M2OBC: the sub-tidal value + the tide, from the library's copy of the base (never += on the output)
  if (var == 0) GF(zeta_bry)[B] = T.add_fs ? T.zeta_base[B] + x : x;
  else if (var == 1) GF(ubar_bry)[B] = T.add_m2 ? T.ubar_base[B] + x : x;
  else GF(vbar_bry)[B] = T.add_m2 ? T.vbar_base[B] + x : x;
}

// ------------------------------------------------------------------------------------------- configuration --
// the strip element of rho-/u-/v-point line `line` of edge e at along-edge position a, as an index into a host plane
static inline long strip_src(const roms_bounds_t &b, int e, int fixed, int a)
{
  const long ni = b.UBi - b.LBi + 1;
  return e <= LBS_EAST ? (long)(fixed - b.LBi) + (long)(a - b.LBj) * ni : (long)(a - b.LBi) + (long)(fixed - b.LBj) * ni;
}

extern "C" int roms_hip_set_tides(int NTC, int MTC, const double *Tperiod, const double *SSH_Tamp, const double *SSH_Tphase,
                                  const double *UV_Tangle, const double *UV_Tphase, const double *UV_Tmajor,
                                  const double *UV_Tminor, const double *angler, double tide_start, int ramp_tides,
                                  double dstart, int add_fsobc, const double *zeta_base, int add_m2obc,
                                  const double *ubar_base, const double *vbar_base)
{
  const char *me = "roms_hip_set_tides";
  if (int rc = roms_setup_check(me)) return rc;
  if (NTC < 0) return roms_fail(me, "tides: NTC < 0");
  if (NTC > MTC) return roms_fail(me, "tides: NTC > MTC");
  if (NTC > ROMS_MAXTC) return roms_fail(me, "tides: NTC > ROMS_MAXTC constituents");
  const RomsTides &have = g_ctx.hostc.tides;
  const bool any_ssh = SSH_Tamp || SSH_Tphase, any_uv = UV_Tangle || UV_Tphase || UV_Tmajor || UV_Tminor;
  if (NTC == 0) {
    if (any_ssh || any_uv) return roms_fail(me, "tides: NTC = 0 with harmonic arrays");
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    if (have.ssh_only) step2d_graphs_release();
    tides_release();
    return 0;
  }
  if (!Tperiod) return roms_fail(me, "tides: Tperiod is NULL");
  if (any_ssh && !(SSH_Tamp && SSH_Tphase)) return roms_fail(me, "tides: SSH_Tamp and SSH_Tphase come together (SSH_TIDES)");
  if (any_uv && !(UV_Tangle && UV_Tphase && UV_Tmajor && UV_Tminor))
    return roms_fail(me, "tides: UV_Tangle, UV_Tphase, UV_Tmajor and UV_Tminor come together (UV_TIDES)");
  if (!any_ssh && !any_uv) return roms_fail(me, "tides: NTC > 0 needs the arrays of SSH_TIDES or UV_TIDES");
  const bool keep = have.ntc > 0;                  // an earlier configuration: a NULL base keeps its copy
  if (add_fsobc && !any_ssh) return roms_fail(me, "tides: add_fsobc needs SSH_TIDES");
  if (add_m2obc && !any_uv) return roms_fail(me, "tides: add_m2obc needs UV_TIDES");
  if (add_fsobc && !zeta_base && !(keep && g_tides.dev[TS_zbase]))
    return roms_fail(me, "tides: add_fsobc without zeta_base");
  if (add_m2obc && !((ubar_base || (keep && g_tides.dev[TS_ubase])) && (vbar_base || (keep && g_tides.dev[TS_vbase]))))
    return roms_fail(me, "tides: add_m2obc without ubar_base and vbar_base");
  if (add_m2obc && g_ctx.hostc.clima.m2)
    return roms_fail(me, "tides: add_m2obc with LnudgeM2CLM is not built (set_tides.F:476-508 moves ubarclm / vbarclm as well)");
  const roms_bounds_t &b = g_ctx.b;
  if (b.NSperiodic) return roms_fail(me, "tides: N-S periodic grids are not implemented on this path");
  const bool masked = g_ctx.p.masking != 0;
  if (masked && !(g_ctx.field[FID_rmask].dev && g_ctx.field[FID_umask].dev && g_ctx.field[FID_vmask].dev))
    return roms_fail(me, "tides: masking = 1 but rmask, umask, vmask are not registered yet");
  const long ni = b.UBi - b.LBi + 1, nj = b.UBj - b.LBj + 1, nij = ni * nj;

  RomsTides want{};
  want.ntc = NTC;
  want.ssh = any_ssh; want.uv = any_uv; want.ssh_only = any_ssh && !any_uv;
  want.ramp = ramp_tides != 0; want.add_fs = add_fsobc != 0; want.add_m2 = add_m2obc != 0;
  want.tide_start = tide_start; want.dstart = dstart;
  for (int it = 0; it < NTC; it++) want.Tperiod[it] = Tperiod[it];
  long tot = 0;
  for (int e = 0; e < 4; e++) {
    want.lb[e] = e <= LBS_EAST ? b.LBj : b.LBi;
    want.len[e] = (int)(e <= LBS_EAST ? nj : ni);
    want.off[e] = tot;
    tot += 2L * want.len[e];
  }
  want.tot = tot;
  // the fixed index of the strip lines: rho lines 0 / 1, the u-point line, the v-point line
  const int rho0[4] = {b.Istr - 1, b.Iend + 1, b.Jstr - 1, b.Jend + 1}, rho1[4] = {b.Istr, b.Iend, b.Jstr, b.Jend};
  const int ul[4] = {b.Istr, b.Iend + 1, b.Jstr - 1, b.Jend + 1}, vl[4] = {b.Istr - 1, b.Iend + 1, b.Jstr, b.Jend + 1};
  for (int e = 0; e < 4; e++)
    for (int f : {rho0[e], rho1[e], ul[e], vl[e]})
      if (f < (e <= LBS_EAST ? b.LBi : b.LBj) || f > (e <= LBS_EAST ? b.UBi : b.UBj))
        return roms_fail(me, "tides: the bounds leave no ghost point beside an edge");

  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  if (want.ssh_only != have.ssh_only) step2d_graphs_release();   // the boundary launches of the captured loops hold the switch
  // the bases outlive a reconfiguration (NULL = keep); everything else is built again
  double *zb = g_tides.dev[TS_zbase], *ub = g_tides.dev[TS_ubase], *vb = g_tides.dev[TS_vbase];
  g_tides.dev[TS_zbase] = g_tides.dev[TS_ubase] = g_tides.dev[TS_vbase] = nullptr;
  tides_release();
  g_tides.dev[TS_zbase] = zb; g_tides.dev[TS_ubase] = ub; g_tides.dev[TS_vbase] = vb;

  auto fail = [&](int rc) { tides_release(); return rc; };
#define TIDES_TRY(expr)                                                              \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess) return fail(roms_fail(#expr, hipGetErrorString(e_)));      \
  } while (0)
  std::vector<double> stage((size_t)tot);
  // gather one host plane into the strip layout: rho lines (both) or one u- / v-line (first half of the stage)
  auto gather_rho = [&](const double *plane) {
    for (int e = 0; e < 4; e++)
      for (int line = 0; line < 2; line++)
        for (int k = 0; k < want.len[e]; k++)
          stage[want.off[e] + (long)line * want.len[e] + k] =
              plane ? plane[strip_src(b, e, line ? rho1[e] : rho0[e], want.lb[e] + k)] : 0.0;
  };
  auto gather_line = [&](const double *plane, const int *fixed) {
    for (int e = 0; e < 4; e++)
      for (int k = 0; k < want.len[e]; k++) stage[want.off[e] / 2 + k] = plane[strip_src(b, e, fixed[e], want.lb[e] + k)];
  };
  const double *harm[6] = {SSH_Tamp, SSH_Tphase, UV_Tangle, UV_Tphase, UV_Tmajor, UV_Tminor};
  for (int q = 0; q < 6; q++) {
    if (!harm[q]) continue;
    TIDES_TRY(hipMalloc(&g_tides.dev[TS_amp + q], sizeof(double) * tot * NTC));
    for (int it = 0; it < NTC; it++) {             // one constituent plane at a time through the stage
      gather_rho(harm[q] + (size_t)it * nij);
      TIDES_TRY(hipMemcpy(g_tides.dev[TS_amp + q] + (size_t)it * tot, stage.data(), sizeof(double) * tot, hipMemcpyHostToDevice));
    }
  }
  if (any_uv) {                                    // angler: NULL = zero
    TIDES_TRY(hipMalloc(&g_tides.dev[TS_angler], sizeof(double) * tot));
    gather_rho(angler);
    TIDES_TRY(hipMemcpy(g_tides.dev[TS_angler], stage.data(), sizeof(double) * tot, hipMemcpyHostToDevice));
  }
  if (masked) {                                    // the masks as the device holds them now
    std::vector<double> plane((size_t)nij);
    const int fid[3] = {FID_rmask, FID_umask, FID_vmask};
    for (int q = 0; q < 3; q++) {
      TIDES_TRY(hipMemcpy(plane.data(), g_ctx.field[fid[q]].dev, sizeof(double) * nij, hipMemcpyDeviceToHost));
      const long n = q == 0 ? tot : tot / 2;
      if (q == 0) gather_rho(plane.data());
      else gather_line(plane.data(), q == 1 ? ul : vl);
      TIDES_TRY(hipMalloc(&g_tides.dev[TS_rmask + q], sizeof(double) * n));
      TIDES_TRY(hipMemcpy(g_tides.dev[TS_rmask + q], stage.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    }
  }
  const double *base[3] = {zeta_base, ubar_base, vbar_base};
  const bool base_on[3] = {want.add_fs != 0, want.add_m2 != 0, want.add_m2 != 0};
  for (int q = 0; q < 3; q++) {
    if (!base_on[q]) {
      if (g_tides.dev[TS_zbase + q]) (void)hipFree(g_tides.dev[TS_zbase + q]);
      g_tides.dev[TS_zbase + q] = nullptr;
      continue;
    }
    if (!g_tides.dev[TS_zbase + q]) TIDES_TRY(hipMalloc(&g_tides.dev[TS_zbase + q], sizeof(double) * nij));
    if (base[q]) TIDES_TRY(hipMemcpy(g_tides.dev[TS_zbase + q], base[q], sizeof(double) * nij, hipMemcpyHostToDevice));
  }
#undef TIDES_TRY
  want.amp = g_tides.dev[TS_amp]; want.eph = g_tides.dev[TS_eph];
  want.ang = g_tides.dev[TS_ang]; want.uph = g_tides.dev[TS_uph]; want.maj = g_tides.dev[TS_maj]; want.mnr = g_tides.dev[TS_mnr];
  want.angler = g_tides.dev[TS_angler];
  want.rmask = g_tides.dev[TS_rmask]; want.umask = g_tides.dev[TS_umask]; want.vmask = g_tides.dev[TS_vmask];
  want.zeta_base = g_tides.dev[TS_zbase]; want.ubar_base = g_tides.dev[TS_ubase]; want.vbar_base = g_tides.dev[TS_vbase];
  g_ctx.hostc.tides = want;
  g_ctx.devc_dirty = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------ per step --
extern "C" int roms_hip_tides(double time)
{
  const char *me = "roms_hip_tides";
  int rc = roms_entry_check(me);
  if (rc) return rc;
  const RomsTides &T = g_ctx.hostc.tides;
  if (T.ntc == 0) return 0;
  if ((rc = check_lbc())) return rc;
  if (T.add_m2 && g_ctx.hostc.clima.m2)
    return roms_fail(me, "tides: add_m2obc with LnudgeM2CLM is not built (set_tides.F:476-508 moves ubarclm / vbarclm as well)");
  const roms_bounds_t &b = g_ctx.b;
  if (T.len[LBS_WEST] != b.UBj - b.LBj + 1 || T.len[LBS_SOUTH] != b.UBi - b.LBi + 1)
    return roms_fail(me, "tides: the strips were gathered under other bounds");
  ScopedTimer tm("set_tides");
  const double pi = 3.14159265358979323846, day2sec = 86400.0;
  const double ramp = T.ramp ? tanh((time / 86400.0 - T.dstart) / 1.0) : 1.0;      // :249-253
  const double cff = 2.0 * pi * (time - T.tide_start * day2sec);                  // :280, :437
  int zmask = 0, uvmask = 0;
  for (int sd = 0; sd < 4; sd++) {
    if (tides_acquire(sd, LBV_ZETA) || tides_acquire(sd, LBV_UBAR) || tides_acquire(sd, LBV_VBAR)) zmask |= 1 << sd;
    if (tides_acquire(sd, LBV_UBAR) && tides_acquire(sd, LBV_VBAR)) uvmask |= 1 << sd;
  }
  const int nmax = T.len[LBS_WEST] > T.len[LBS_SOUTH] ? T.len[LBS_WEST] : T.len[LBS_SOUTH];
  hipLaunchKernelGGL(k_set_tides, dim3((nmax + 63) / 64, 12), dim3(64), 0, g_ctx.stream, g_ctx.devc, cff, ramp, zmask, uvmask);
  KERNEL_CHECK("k_set_tides");
  return 0;
}
