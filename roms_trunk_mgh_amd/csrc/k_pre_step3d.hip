// k_pre_step3d.hip -- predictor step, pre_step3d_tile
// (ROMS/Nonlinear/pre_step3d.F:123-1156).
//
//   k_pre_t   one thread per water column and tracer, one upward sweep:
//             horizontal + vertical advective fluxes of t(nstp), artificial
//             continuity, t(n+1/2) -> t(:,:,:,3,itrc)  (:342-915), and the
//             start of the corrector t(:,:,:,nnew,itrc) = Hz*t(nstp) + explicit
//             vertical flux divergence incl. KPP non-local and solar terms
//             (:917-1010, lmd_swfrac.F:6).  A thread reads t(nnew) only in its
//             own column before overwriting it, so the fusion is hazard-free.
//   k_pre_uv  one thread per column: start of u,v(nnew) with the AB3 terms
//             5/12 ru(nrhs) - 16/12 ru(3-nrhs) and surface/bottom stress
//             (:1012-1120).
// Algorithmic traffic (BENCHMARK, NT=2), the entry on its own: per tracer read t(nstp), t(nnew), Akt,
// ghats; write t(3), t(nnew) = 48 B; shared Huon,Hvom,W,Hz,z_r,z_w = 48 B, read once per tracer; momentum
// part reads u,v(nstp), ru,rv x2, Akv, writes u,v(nnew) = 72 B.
// Inside roms_hip_rhs3d with rotated mixing (DEFER, NTR = 2): per tracer read t(nstp), t(nnew), write t(3) = 24 B;
// shared Huon,Hvom,W,Hz = 32 B read once per pair of tracers; Akt, ghats, z_w and the write of t(nnew) are k_t3dmix_geo's.
#include "roms_dev.h"
#include "advect.h"

namespace {

// MASK: MASKING applications, first differences times umask / vmask of their face (pre_step3d.F:398, :463)
// DIA (DIAGNOSTICS_TS, pre_step3d.F:899-902): the two summands of the corrector's start go to DiaTwrk(iTrate) and
// DiaTwrk(iTvdif) (m Tunits; k_step3d_t_pipe turns them into Tunits).  Instantiated at NMAX = ROMS_MAXN only.
// DEFER (inside roms_hip_rhs3d, rhs3d_fuses_tstart()): the start of the corrector is left to k_t3dmix_geo<0, ISO, false,
// true>, which stores it together with its own term -- t(nnew) is read here (the cff2 term of t(3)) and not written; Akt,
// ghats, z_w and the surface / bottom fluxes are not read.  Both loops cover Istr:Iend, Jstr:Jend on every tile
// (pre_step3d.F:837-898, t3dmix2_geo.h:401-408), and t3dbc_tile / the exchanges at the end of the predictor work on
// level 3 alone (pre_step3d.F:1131-1149).
// NTR = 2: the thread carries the tracers itrc and itrc + 1 of one column; Huon, Hvom, W, Hz of a level are loaded and
// the artificial-continuity reciprocal DC is formed once for both.  For the schemes without whole-column arrays.
template <int HADV, int VADV, int NMAX, bool MASK, bool DIA = false, bool DEFER = false, int NTR = 1>
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_pre_t(const RomsDev *__restrict__ c, int nstp, int nnew, int first_step, int itrc0, int ntr)
{
  static_assert(NTR == 1 || (VADV != ADV_A4 && VADV != ADV_SPLINES && !DIA), "pairs: no whole-column arrays, no diagnostics");
  static_assert(!(DIA && DEFER), "diagnostics keep the two kernels");
  DEV_PROLOGUE(c)
  const TileCol tc = tile_column(b, itrc0, ntr);
  if (!tc.valid) return;
  const int i = tc.i, j = tc.j;
  const int itrc1 = itrc0 + NTR * (tc.itrc - itrc0);       // the first tracer of the thread
  const roms_params_t &p = c->p;
  const double dt = p.dt;
  const ColFields f = column_fields(c);
  const long c0 = I2(i, j);
  const Walls wl = column_walls(c, i, j);
  // time-stepping weights, pre_step3d.F:586-600
  // (upstream predictors -- MPDATA, HSIMT -- use Gamma = 1/2; the horizontal part takes the weight of the horizontal
  // scheme, :557-563, the vertical part that of the vertical scheme, :793-799: they differ for "HSIMT vertically with
  // another scheme horizontally")
  const double Gamma = (HADV == ADV_MPDATA) ? 0.5 : 1.0 / 6.0;
  const double GammaV = (VADV == ADV_MPDATA) ? 0.5 : 1.0 / 6.0;
  double cff, cff1, cff2;
  if (first_step) { cff = 0.5 * dt; cff1 = 1.0; cff2 = 0.0; }
  else { cff = (1.0 - Gamma) * dt; cff1 = 0.5 + Gamma; cff2 = 0.5 - Gamma; }
  const double cpp = cff * GF(pm)[c0] * GF(pn)[c0];
  const double cppv = (first_step ? 0.5 * dt : (1.0 - GammaV) * dt) * GF(pm)[c0] * GF(pn)[c0];

  // per tracer: the three time levels, the explicit vertical flux of the corrector's start (advect.h) and the k-window
  gcd_t ts[NTR];
  gd_t t3[NTR], tn[NTR];
  VStart vs[NTR];
  double zr_k[NTR], FDprev[NTR];                              // z_r(k) of the explicit flux; diffusive FC(k-1)
  double tkm1[NTR], tk[NTR], tkp1[NTR], tkp2[NTR];
  double FCprev[NTR];                                         // advective FC(k-1)
  // vertical schemes that need the whole column first
  double a4cf[(VADV == ADV_A4) ? NMAX + 2 : 1];
  double spl[(VADV == ADV_SPLINES) ? NMAX + 1 : 1];
#pragma unroll
  for (int q = 0; q < NTR; q++) {
    ts[q] = (gcd_t)tracer_level(c, nstp, itrc1 + q, n3r);
    t3[q] = (gd_t)tracer_level(c, 3, itrc1 + q, n3r);
    tn[q] = (gd_t)tracer_level(c, nnew, itrc1 + q, n3r);
    if constexpr (!DEFER) {
      vs[q] = vstart_column(c, itrc1 + q, c0, nij, n3w);
      FDprev[q] = vstart_bottom(c, vs[q], c0, nij);
      zr_k[q] = (vs[q].cff3 != 0.0) ? vs[q].z_r[c0] : 0.0;
    }
    tkm1[q] = 0.0; tk[q] = ts[q][c0]; tkp1[q] = (N >= 2) ? ts[q][c0 + nij] : 0.0;
    FCprev[q] = 0.0;
  }
  if constexpr (VADV == ADV_A4) a4_slopes<NMAX>(ts[0], c0, nij, N, a4cf);
  if constexpr (VADV == ADV_SPLINES) spline_w<true, NMAX>(ts[0], f.Hz, f.W, c0, nij, N, spl);

  const bool src_cell = c->src.n > 0 && src_cell_any(c, c0, ni);      // LuvSrc: a face of this cell is a source face
  double w_km1 = f.W[c0];
  for (int k = 1; k <= N; k++) {
    const long ck = c0 + (long)(k - 1) * nij;
    // ---- the loads of the level: with two tracers both tracers' before the first store.  (The tracer-independent
    // loads and t(nnew) of a single tracer stay where the one-tracer kernel has always had them, in the first pass of
    // the loop below: issued up here they cost it 24 VGPRs and a wave.) ----
    HStencil s[NTR];
    double tnn[NTR];
#pragma unroll
    for (int q = 0; q < NTR; q++) {
      const gcd_t t = ts[q];
      tkp2[q] = (k + 2 <= N) ? t[ck + 2 * nij] : 0.0;
      s[q].xm1 = t[ck - 1]; s[q].xp1 = t[ck + 1];
      s[q].xm2 = wl.w ? 0.0 : t[ck - 2];
      s[q].xp2 = wl.e ? 0.0 : t[ck + 2];
      s[q].ym1 = t[ck - ni]; s[q].yp1 = t[ck + ni];
      s[q].ym2 = wl.s ? 0.0 : t[ck - 2 * ni];
      s[q].yp2 = wl.n ? 0.0 : t[ck + 2 * ni];
      if constexpr (NTR > 1) tnn[q] = tn[q][ck];
    }
    const double hu0 = f.Huon[ck], hu1 = f.Huon[ck + 1], hv0 = f.Hvom[ck], hv1 = f.Hvom[ck + ni];
    double hz, w_k, DCk;
#pragma unroll
    for (int q = 0; q < NTR; q++) {
      const int itrc = itrc1 + q;
      // ---- horizontal fluxes of t(nstp) ----
      s[q].hu0 = hu0; s[q].hu1 = hu1; s[q].hv0 = hv0; s[q].hv1 = hv1;
      Faces fx = cell_faces<HADV, MASK>(tk[q], s[q], wl, c, c0, ni);
      if (src_cell)                                    // LuvSrc, pre_step3d.F:530-553
        src_cell_fluxes<true>(c, c0, ck, ni, k, itrc, nullptr, fx.FXi, fx.FXip1, fx.FEj, fx.FEjp1);
      if (q == 0) hz = f.Hz[ck];
      if constexpr (NTR == 1) tnn[q] = tn[q][ck];
      double t3v = hz * (cff1 * tk[q] + cff2 * tnn[q]) - cpp * (fx.FXip1 - fx.FXi + fx.FEjp1 - fx.FEj);
      // ---- vertical advective flux through the top face ----
      if (q == 0) w_k = f.W[ck + nij];
      const double FCk = vflux_level<VADV>(k, N, w_k, tkm1[q], tk[q], tkp1[q], tkp2[q], spl, a4cf);
      // ---- artificial continuity, pre_step3d.F:893-915 ----
      if (q == 0) DCk = 1.0 / (hz - cppv * (hu1 - hu0 + hv1 - hv0 + (w_k - w_km1)));
      t3v = DCk * (t3v - cppv * (FCk - FCprev[q]));
      t3[q][ck] = t3v;
      // ---- start of the corrector: explicit vertical flux, pre_step3d.F:837-898 ----
      if constexpr (!DEFER) {
        const VStartIn in = (k < N) ? vstart_load(vs[q], ck + nij) : VStartIn{0.0, 0.0, 0.0};
        const double FDk = vstart_flux<true>(c, vs[q], k, N, c0, nij, ck + nij, in, tk[q], tkp1[q], zr_k[q]);
        const double hzt = hz * tk[q], dFD = FDk - FDprev[q];
        tn[q][ck] = hzt + dFD;
        if constexpr (DIA) {
          DIA_PLANE(c, DIA_iTrate, itrc, n3r)[ck] = hzt;
          DIA_PLANE(c, DIA_iTvdif, itrc, n3r)[ck] = dFD;
        }
        FDprev[q] = FDk;
      }
      FCprev[q] = FCk;
      tkm1[q] = tk[q]; tk[q] = tkp1[q]; tkp1[q] = tkp2[q];
    }
    w_km1 = w_k;
  }
}

__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_pre_uv(const RomsDev *__restrict__ c, int nstp, int nnew, int nrhs, int stage)
{
  // stage: 0 = first step (forward Euler), 1 = second step (AB2), 2 = AB3
  DEV_PROLOGUE(c)
  const Blk XB = xcd_block();
  const int i = b.Istr + XB.x * BLK_X + threadIdx.x;
  const int j = b.Jstr + XB.y * BLK_Y + threadIdx.y;
  if (i > b.Iend || j > b.Jend) return;
  const roms_params_t &p = c->p;
  const double dt = p.dt;
  const double cff3 = dt * (1.0 - p.lambda);
  const gcd_t z_r = (gcd_t)(c->F.z_r);
  const gcd_t Hz = (gcd_t)(c->F.Hz);
  const gcd_t Akv = (gcd_t)(c->F.Akv);
  const gcd_t pm = (gcd_t)(c->F.pm);
  const gcd_t pn = (gcd_t)(c->F.pn);
  const long c0 = I2(i, j);
  const int indx = 3 - nrhs;
#pragma unroll
  for (int comp = 0; comp < 2; comp++) {
    if (comp == 0 && i < b.IstrU) continue;
    if (comp == 1 && j < b.JstrV) continue;
    const long off = comp == 0 ? 1 : ni;          // neighbour at i-1 or j-1
    const gcd_t vel = (gcd_t)((comp == 0 ? c->F.u : c->F.v) + (long)(nstp - 1) * n3r);
    const gd_t vnew = (gd_t)((comp == 0 ? c->F.u : c->F.v) + (long)(nnew - 1) * n3r);
    const gcd_t r1 = (gcd_t)((comp == 0 ? c->F.ru : c->F.rv) + (long)(nrhs - 1) * n3w);
    const gcd_t r2 = (gcd_t)((comp == 0 ? c->F.ru : c->F.rv) + (long)(indx - 1) * n3w);
    const double bstr = (comp == 0 ? c->F.bustr : c->F.bvstr)[c0];
    const double sstr = (comp == 0 ? c->F.sustr : c->F.svstr)[c0];
    const double cq = dt * 0.25;
    const double DC0 = cq * (pm[c0] + pm[c0 - off]) * (pn[c0] + pn[c0 - off]);
    double FCprev = dt * bstr;
    double vk = vel[c0];
    double zsum_k = 0.0;   // unused placeholder for clarity
    (void)zsum_k;
    for (int k = 1; k <= N; k++) {
      const long ck = c0 + (long)(k - 1) * nij;
      double FCk, vk1 = 0.0;
      if (k == N) FCk = dt * sstr;
      else {
        vk1 = vel[ck + nij];
        if (cff3 != 0.0) {
          const double cz = 1.0 / (z_r[ck + nij] + z_r[ck + nij - off] - z_r[ck] - z_r[ck - off]);
          FCk = cff3 * cz * (vk1 - vk) * (Akv[ck + nij] + Akv[ck + nij - off]);
        } else {
          // lambda = 1 (fully implicit vertical viscosity, every shipped application): the explicit flux is
          // cff3 * (...) = +-0; z_r and Akv need not be read (a zero of either sign gives the same sums)
          FCk = 0.0;
        }
      }
      const double hzs = Hz[ck] + Hz[ck - off];
      const double d = FCk - FCprev;
      vnew[ck] = uv_start(stage, vk, hzs, DC0, r1, r2, ck + nij, d);
      FCprev = FCk;
      vk = vk1;
    }
  }
}

// One launch of k_pre_t<HADV, VADV, ., ., ., DEFER, NTR> over nthr tracers (NTR = 1) or pairs of tracers (NTR = 2)
// from tracer itrc0 on
template <int HADV, int VADV, bool DEFER, int NTR>
int launch_pre_t_n(const roms_step_idx_t *s, int itrc0, int nthr)
{
  typedef void (*PreKernel)(const RomsDev *, int, int, int, int, int);
  const roms_bounds_t &b = g_ctx.b;
  const dim3 grid = grid_tile_tracer(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1, nthr);
  const int first = s->iic == s->ntfirst;
  if (b.N > ROMS_MAXN) return roms_fail("roms_hip_pre_step3d", "N > 64 not instantiated");
  PreKernel kernel;
  if constexpr (NTR == 2) {                              // no whole-column arrays: NMAX is not used
    kernel = k_pre_t<HADV, VADV, ROMS_MAXN, false, false, DEFER, 2>;
    if constexpr (HADV != ADV_MPDATA)
      if (g_ctx.p.masking) kernel = k_pre_t<HADV, VADV, ROMS_MAXN, true, false, DEFER, 2>;
  } else {
    kernel = kernel_for_n(b.N, [](auto nm) -> PreKernel { return k_pre_t<HADV, VADV, nm.value, false, false, DEFER>; });
    if constexpr (HADV != ADV_MPDATA)                    // the upstream predictor of MPDATA / HSIMT has no mask
      if (g_ctx.p.masking)
        kernel = kernel_for_n(b.N, [](auto nm) -> PreKernel { return k_pre_t<HADV, VADV, nm.value, true, false, DEFER>; });
    if constexpr (HADV != ADV_MPDATA && VADV != ADV_MPDATA && !DEFER)   // (dia_check has refused the upstream predictors)
      if (dia_on())
        kernel = g_ctx.p.masking ? k_pre_t<HADV, VADV, ROMS_MAXN, true, true> : k_pre_t<HADV, VADV, ROMS_MAXN, false, true>;
  }
  hipLaunchKernelGGL(kernel, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, s->nstp, s->nnew, first, itrc0, nthr);
  KERNEL_CHECK("k_pre_t");
  return 0;
}

// the scheme pairs built with two tracers per thread
constexpr bool pre_t_pairs(int ha, int va)
{
  return (ha == ADV_U3 && va == ADV_C4) || (ha == ADV_C4 && va == ADV_C4) || (ha == ADV_C2 && va == ADV_C2) ||
         (ha == ADV_MPDATA && va == ADV_MPDATA);
}

// A run of ntr tracers of one scheme pair from tracer itrc0 on.  fused (see pre_step3d_entry()): pairs of tracers where
// the pair is built, one single-tracer launch for the rest.  Otherwise single tracers, as ever: with the corrector's
// start in the kernel a pair needs 210 VGPRs (U3 / C4: 2 waves per SIMD) and has not been measured.
template <int HADV, int VADV>
int launch_pre_t(const roms_step_idx_t *s, int itrc0, int ntr, bool fused)
{
  int rc = 0;
  if constexpr (pre_t_pairs(HADV, VADV))
    if (fused && ntr >= 2) {
      const int np = ntr / 2;
      rc = launch_pre_t_n<HADV, VADV, true, 2>(s, itrc0, np);
      if (rc) return rc;
      itrc0 += 2 * np;
      ntr -= 2 * np;
    }
  if (ntr == 0) return 0;
  return fused ? launch_pre_t_n<HADV, VADV, true, 1>(s, itrc0, ntr) : launch_pre_t_n<HADV, VADV, false, 1>(s, itrc0, ntr);
}

}  // namespace

// The tracer half of pre_step3d_tile (pre_step3d.F:342-915 and the tracer part of :917-1145): t(3), t(nnew),
// then t3dbc_tile(nout = 3) and the periodic wrap / mp_exchange4d of t(3).
static int pre_step3d_tracers(const roms_step_idx_t *s, bool fused)
{
  const roms_bounds_t &b = g_ctx.b;
  const roms_params_t &p = g_ctx.p;
  int rc = 0;
  {
    int it = 1;
    while (it <= b.NT) {
      const int n = adv_run_length(p, b.NT, it);
      switch (adv_pair(p.Hadv[it - 1], p.Vadv[it - 1])) {
      case ADV_U3 * 16 + ADV_C4:   rc = launch_pre_t<ADV_U3, ADV_C4>(s, it, n, fused); break;
      case ADV_A4 * 16 + ADV_A4:   rc = launch_pre_t<ADV_A4, ADV_A4>(s, it, n, fused); break;
      case ADV_C4 * 16 + ADV_C4:   rc = launch_pre_t<ADV_C4, ADV_C4>(s, it, n, fused); break;
      case ADV_C2 * 16 + ADV_C2:   rc = launch_pre_t<ADV_C2, ADV_C2>(s, it, n, fused); break;
      case ADV_U3 * 16 + ADV_SPLINES: rc = launch_pre_t<ADV_U3, ADV_SPLINES>(s, it, n, fused); break;
      case ADV_C4 * 16 + ADV_SPLINES: rc = launch_pre_t<ADV_C4, ADV_SPLINES>(s, it, n, fused); break;
      case ADV_A4 * 16 + ADV_SPLINES: rc = launch_pre_t<ADV_A4, ADV_SPLINES>(s, it, n, fused); break;
      case ADV_MPDATA * 16 + ADV_MPDATA: rc = launch_pre_t<ADV_MPDATA, ADV_MPDATA>(s, it, n, fused); break;
      // HSIMT: the predictor is the same first-order upstream step with Gamma = 1/2 (pre_step3d.F:364, :558, :730, :794)
      case ADV_HSIMT * 16 + ADV_HSIMT: rc = launch_pre_t<ADV_MPDATA, ADV_MPDATA>(s, it, n, fused); break;
      // HSIMT vertically with another scheme horizontally (the one working one-sided pair of the reference): the
      // vertical predictor is the upstream step (:729-748, Gamma = 1/2 :793-799), the horizontal one the scheme's own
      case ADV_U3 * 16 + ADV_HSIMT: rc = launch_pre_t<ADV_U3, ADV_MPDATA>(s, it, n, fused); break;
      case ADV_C4 * 16 + ADV_HSIMT: rc = launch_pre_t<ADV_C4, ADV_MPDATA>(s, it, n, fused); break;
      case ADV_A4 * 16 + ADV_HSIMT: rc = launch_pre_t<ADV_A4, ADV_MPDATA>(s, it, n, fused); break;
      case ADV_C2 * 16 + ADV_HSIMT: rc = launch_pre_t<ADV_C2, ADV_MPDATA>(s, it, n, fused); break;
      default:
        return roms_fail("roms_hip_pre_step3d", "advection scheme pair not implemented (MPDATA and HSIMT only as H+V pairs)");
      }
      if (rc) return rc;
      it += n;
    }
  }
  // t3dbc_tile(nout=3) + periodic wrap / mp_exchange4d, pre_step3d.F:1131-1145
  const long n3r = (long)(b.UBi - b.LBi + 1) * (b.UBj - b.LBj + 1) * b.N;
  for (int it = 1; it <= b.NT; it++)
    if ((rc = bc_t3d(3, it, s->nstp))) return rc;
  halo_batch_begin();
  for (int it = 1; it <= b.NT; it++) halo_exchange3d(GT_R, b.N, g_ctx.field[FID_t].dev + (2L + 3L * (it - 1)) * n3r);
  return halo_batch_end();
}

// The momentum half: u, v(nnew) of the predictor (pre_step3d.F:1012-1120)
static int pre_step3d_uv(const roms_step_idx_t *s)
{
  const roms_bounds_t &b = g_ctx.b;
  const int stage = (s->iic == s->ntfirst) ? 0 : (s->iic == s->ntfirst + 1 ? 1 : 2);
  hipLaunchKernelGGL(k_pre_uv, grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1), block2d(), 0, g_ctx.stream,
                     g_ctx.devc, s->nstp, s->nnew, s->nrhs, stage);
  KERNEL_CHECK("k_pre_uv");
  return 0;
}

// fused (roms_hip_rhs3d alone, roms_dev.h): t(nnew) is left to the mixing kernel that follows;
// uvstart: u, v(nnew) are left to the pressure-gradient kernel that follows
int pre_step3d_entry(const roms_step_idx_t *s, bool fused, bool uvstart)
{
  int rc = roms_entry_check("roms_hip_pre_step3d");
  if (rc) return rc;
  if ((rc = check_lbc())) return rc;
  if (g_ctx.b.N < 4) return roms_fail("roms_hip_pre_step3d", "needs N >= 4 levels (the vertical stencils of the column read k-1 .. k+2)");
  if ((rc = dia_check("roms_hip_pre_step3d"))) return rc;
  ScopedTimer tm("pre_step3d");
  // (the reference does the tracers first; the two halves share no output)
  if (!uvstart && (rc = pre_step3d_uv(s))) return rc;
  return pre_step3d_tracers(s, fused);
}

extern "C" int roms_hip_pre_step3d(const roms_step_idx_t *s) { return pre_step3d_entry(s, false, false); }
