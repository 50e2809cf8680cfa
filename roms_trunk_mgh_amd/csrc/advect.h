// advect.h -- the tracer column shared by the predictor k_pre_t (pre_step3d.F:342-915) and the correctors
// k_step3d_t_pipe / k_step3d_t_hsimt (step3d_t.F:363-1455): the reference writes the same C2 / U3 / A4 / C4 flux
// formulas, wall rules and whole-column reconstructions in both files; here each is stated once.
//   flux formulas     hflux<>, vflux<>
//   column frame      tile_column(), column_walls(), tracer_level(), column_fields(), tracer_akt()
//   whole column      a4_slopes<>(), spline_w<>()
//   one level         cell_faces<>(), vflux_level<>(), vstart_flux<>(), thomas_row()
//   host              adv_pair(), adv_run_length(), kernel_for_n()
// The device functions take loaded values: which load is issued when stays the kernel's business.
#pragma once
#include <type_traits>
#include "roms_dev.h"

template <int HADV>
__device__ __forceinline__ double hflux(double Hflx, double tm1, double t0, double dm1, double d0, double dp1)
{
  // flux through the face between cell "m1" and cell "0"; d* are first
  // differences centred on faces (dm1 = face-1, d0 = this face, dp1 = face+1).
  if constexpr (HADV == ADV_C2) {
    return Hflx * 0.5 * (tm1 + t0);
  } else if constexpr (HADV == ADV_MPDATA) {
    // first-order upstream (the MPDATA predictor, pre_step3d.F:364-386 / step3d_t.F:409-428)
    const double cff1 = fmax(Hflx, 0.0), cff2 = fmin(Hflx, 0.0);
    return cff1 * tm1 + cff2 * t0;
  } else if constexpr (HADV == ADV_U3) {
    const double curv_m1 = d0 - dm1;     // curv at cell m1
    const double curv_0 = dp1 - d0;      // curv at cell 0
    const double cff1 = 1.0 / 6.0;
    return Hflx * 0.5 * (tm1 + t0) -
           cff1 * (curv_m1 * fmax(Hflx, 0.0) + curv_0 * fmin(Hflx, 0.0));
  } else if constexpr (HADV == ADV_A4) {
    const double eps = 1.0E-16;
    double g_m1, g_0;
    double cff = 2.0 * d0 * dm1;
    g_m1 = (cff > eps) ? cff / (d0 + dm1) : 0.0;
    cff = 2.0 * dp1 * d0;
    g_0 = (cff > eps) ? cff / (dp1 + d0) : 0.0;
    const double cff2 = 1.0 / 3.0;
    return Hflx * 0.5 * (tm1 + t0 - cff2 * (g_0 - g_m1));
  } else {  // C4 / SU3
    const double g_m1 = 0.5 * (d0 + dm1);
    const double g_0 = 0.5 * (dp1 + d0);
    const double cff2 = 1.0 / 3.0;
    return Hflx * 0.5 * (tm1 + t0 - cff2 * (g_0 - g_m1));
  }
}

// Vertical flux FC(k), k = 1..N-1, for the non-spline schemes.
template <int VADV>
__device__ __forceinline__ double vflux(int k, int N, double Wk, double tkm1, double tk, double tkp1, double tkp2,
                                        double a4_cf_k, double a4_cf_kp1)
{
  if constexpr (VADV == ADV_C2) {
    return Wk * 0.5 * (tk + tkp1);
  } else if constexpr (VADV == ADV_MPDATA) {
    // first-order upstream, pre_step3d.F:729-748
    const double cff1 = fmax(Wk, 0.0), cff2 = fmin(Wk, 0.0);
    return cff1 * tk + cff2 * tkp1;
  } else if constexpr (VADV == ADV_A4) {
    const double cff1 = 1.0 / 3.0;
    return Wk * 0.5 * (tk + tkp1 - cff1 * (a4_cf_kp1 - a4_cf_k));
  } else {  // C4 / SU3, step3d_t.F:1094+
    const double cff1 = 0.5, cff2 = 7.0 / 12.0, cff3 = 1.0 / 12.0;
    if (k == 1) return Wk * (cff1 * tk + cff2 * tkp1 - cff3 * tkp2);
    if (k == N - 1) return Wk * (cff1 * tkp1 + cff2 * tk - cff3 * tkm1);
    return Wk * (cff2 * (tk + tkp1) - cff3 * (tkm1 + tkp2));
  }
}

// ---------------------------------------------------------------------------
// Column frame
// ---------------------------------------------------------------------------
// (i, j, tracer) of the calling thread in a launch over grid_tile_tracer(); !valid: the thread has no column.
// (Returned by value with the early exits of the kernels' former text: out-parameters cost two VGPRs here.)
struct TileCol { int i, j, itrc; bool valid; };
__device__ __forceinline__ TileCol tile_column(const roms_bounds_t &b, int itrc0, int ntr)
{
  const TileTr tt = decode_tile_tracer(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1, ntr);
  TileCol r;
  r.valid = false;
  if (!tt.valid) return r;
  r.i = b.Istr + tt.bx * BLK_X + threadIdx.x;
  r.j = b.Jstr + tt.by * BLK_Y + threadIdx.y;
  r.itrc = itrc0 + tt.itr;             // 1-based tracer index
  if (r.i > b.Iend || r.j > b.Jend) return r;
  r.valid = true;
  return r;
}
// The cell lies on a physical (closed, non-periodic) edge: the first difference outside the wall face is a copy of
// the wall face's, FX(Istr-1) = FX(Istr), FX(Iend+2) = FX(Iend+1) and likewise FE (step3d_t.F:700-715, :741-760;
// pre_step3d.F:401-412), so the outer stencil point of a wall row is not used -- what the caller loads in its place
// (a valid address, a literal 0) is the caller's business.
struct Walls { bool s, n, w, e; };
__device__ __forceinline__ Walls column_walls(const RomsDev *__restrict__ c, int i, int j)
{
  const roms_bounds_t &b = c->b;       // (through c, as the kernels read it: with a reference parameter the compiler
  Walls wl;                            // loads every member up front instead of short-circuiting)
  wl.s = b.south_edge && !b.NSperiodic && j == b.Jstr;
  wl.n = b.north_edge && !b.NSperiodic && j == b.Jend;
  wl.w = b.west_edge && !b.EWperiodic && i == b.Istr;
  wl.e = b.east_edge && !b.EWperiodic && i == b.Iend;
  return wl;
}
// t(:,:,:,lev,itrc), lev = nstp | 3 | nnew; n3r = points of a rho-array.  (Generic pointer: cast to gcd_t / gd_t.)
__device__ __forceinline__ double *tracer_level(const RomsDev *__restrict__ c, int lev, int itrc, long n3r)
{
  return c->F.t + ((long)(lev - 1) + 3L * (itrc - 1)) * n3r;
}
// the tracer-independent fields of the column sweep
struct ColFields { gcd_t Huon, Hvom, W, Hz; };
__device__ __forceinline__ ColFields column_fields(const RomsDev *__restrict__ c)
{
  ColFields f;
  f.Huon = (gcd_t)c->F.Huon;
  f.Hvom = (gcd_t)c->F.Hvom;
  f.W = (gcd_t)c->F.W;
  f.Hz = (gcd_t)c->F.Hz;
  return f;
}
// Akt(:,:,:,MIN(itrc,NAT)); n3w = points of a W-array
__device__ __forceinline__ gcd_t tracer_akt(const RomsDev *__restrict__ c, int itrc, long n3w)
{
  const int ltrc = itrc < c->b.NAT ? itrc : c->b.NAT;
  return (gcd_t)(c->F.Akt + (long)(ltrc - 1) * n3w);
}

// ---------------------------------------------------------------------------
// Vertical schemes that need the whole column first (c0 = index of (i,j,1), nij = level stride)
// ---------------------------------------------------------------------------
// A4: harmonic-mean slopes a4cf[1..N] of the vertical differences FC(k) = t(k+1)-t(k), FC(N) = FC(N-1), FC(0) = FC(1)
// (step3d_t.F:943-962, pre_step3d.F:671-690); t = t(nstp) in the predictor, t(3) in the corrector
template <int NMAX>
__device__ __forceinline__ void a4_slopes(gcd_t t, long c0, long nij, int N, double *a4cf)
{
  const double eps = 1.0E-16;
  double dprev = 0.0, tk = t[c0];
#pragma unroll
  for (int k = 1; k <= NMAX; k++) {
    if (k <= N) {
      double dk;
      if (k < N) { const double tk1 = t[c0 + (long)k * nij]; dk = tk1 - tk; tk = tk1; }
      else dk = dprev;
      if (k == 1) dprev = dk;
      const double cff = 2.0 * dk * dprev;
      a4cf[k] = (cff > eps) ? cff / (dk + dprev) : 0.0;
      dprev = dk;
    }
  }
}
// SPLINES: parabolic-spline reconstruction of t at W-points times W, spl[0..N] with zeroed ends.  The two files
// differ in the end conditions only: step3d_t.F:894-930 has 2 / 1 / 2 / 1 where pre_step3d.F:622-650 (PRED) has
// 1.5 / 0.5 / 3 / 2.
template <bool PRED, int NMAX>
__device__ __forceinline__ void spline_w(gcd_t t, gcd_t Hz, gcd_t W, long c0, long nij, int N, double *spl)
{
  constexpr double bot_t = PRED ? 1.5 : 2.0, bot_cf = PRED ? 0.5 : 1.0, top_t = PRED ? 3.0 : 2.0, top_cf = PRED ? 2.0 : 1.0;
  double cfs[NMAX + 1];
  spl[0] = bot_t * t[c0];
  cfs[1] = bot_cf;
#pragma unroll
  for (int k = 1; k < NMAX; k++) {
    if (k <= N - 1) {
      const double hk = Hz[c0 + (long)(k - 1) * nij], hk1 = Hz[c0 + (long)k * nij];
      const double cff = 1.0 / (2.0 * hk + hk1 * (2.0 - cfs[k]));
      cfs[k + 1] = cff * hk;
      spl[k] = cff * (3.0 * (hk * t[c0 + (long)k * nij] + hk1 * t[c0 + (long)(k - 1) * nij]) - hk1 * spl[k - 1]);
    }
  }
#pragma unroll
  for (int k = 1; k <= NMAX; k++)
    if (k == N) spl[k] = (top_t * t[c0 + (long)(N - 1) * nij] - spl[k - 1]) / (top_cf - cfs[k]);
#pragma unroll
  for (int k = NMAX - 1; k >= 0; k--) {
    if (k <= N - 1) {
      spl[k] = spl[k] - cfs[k + 1] * spl[k + 1];
      spl[k + 1] = W[c0 + (long)(k + 1) * nij] * spl[k + 1];
    }
  }
#pragma unroll
  for (int k = 0; k <= NMAX; k++) if (k == 0 || k == N) spl[k] = 0.0;
}

// ---------------------------------------------------------------------------
// One level of the column
// ---------------------------------------------------------------------------
// the eight horizontal neighbours of a cell (x = along i, y = along j) and the transports of its four faces
struct HStencil { double xm2, xm1, xp1, xp2, ym2, ym1, yp1, yp2, hu0, hu1, hv0, hv1; };
struct Faces { double FXi, FXip1, FEj, FEjp1; };
// Horizontal advective fluxes through the four faces of the cell with value tk (step3d_t.F:596-828 and the same
// text of pre_step3d.F).  MASK (MASKING): the first differences are multiplied by umask / vmask of their face (step3d_t.F:603,
// :667; pre_step3d.F:398, :463), the masks read per level at c0 (cache hits) rather than held in registers.
template <int HADV, bool MASK>
__device__ __forceinline__ Faces cell_faces(double tk, const HStencil &s, const Walls &wl, const RomsDev *__restrict__ c,
                                            long c0, long ni)
{
  double dxm1 = s.xm1 - s.xm2, dx0 = tk - s.xm1, dxp1 = s.xp1 - tk, dxp2 = s.xp2 - s.xp1;
  double dy0 = tk - s.ym1, dyp1 = s.yp1 - tk;
  double dym1 = s.ym1 - s.ym2, dyp2 = s.yp2 - s.yp1;
  if constexpr (MASK) {
    const gcd_t um = (gcd_t)c->F.umask, vm = (gcd_t)c->F.vmask;
    dxm1 = dxm1 * um[c0 + (wl.w ? 0 : -1)]; dx0 = dx0 * um[c0]; dxp1 = dxp1 * um[c0 + 1];
    dxp2 = dxp2 * um[c0 + (wl.e ? 1 : 2)];
    dy0 = dy0 * vm[c0]; dyp1 = dyp1 * vm[c0 + ni];
    dym1 = dym1 * vm[c0 + (wl.s ? 0 : -ni)]; dyp2 = dyp2 * vm[c0 + (wl.n ? ni : 2 * ni)];
  }
  if (wl.s) dym1 = dy0;
  if (wl.n) dyp2 = dyp1;
  if (wl.w) dxm1 = dx0;
  if (wl.e) dxp2 = dxp1;
  Faces f;
  f.FXi = hflux<HADV>(s.hu0, s.xm1, tk, dxm1, dx0, dxp1);
  f.FXip1 = hflux<HADV>(s.hu1, tk, s.xp1, dx0, dxp1, dxp2);
  f.FEj = hflux<HADV>(s.hv0, s.ym1, tk, dym1, dy0, dyp1);
  f.FEjp1 = hflux<HADV>(s.hv1, tk, s.yp1, dy0, dyp1, dyp2);
  return f;
}
// Vertical advective flux through the top face of level k = 1..N: zero at the surface, the spline value, or the
// stencil of the scheme (with the A4 slopes of the two levels).  spl / a4cf: the column of the scheme, unused otherwise.
template <int VADV>
__device__ __forceinline__ double vflux_level(int k, int N, double Wk, double tkm1, double tk, double tkp1, double tkp2,
                                              const double *spl, const double *a4cf)
{
  if (k == N) return 0.0;
  if constexpr (VADV == ADV_SPLINES) return spl[k];
  else {
    double cfk = 0.0, cfk1 = 0.0;
    if constexpr (VADV == ADV_A4) { cfk = a4cf[k]; cfk1 = a4cf[k + 1]; }
    return vflux<VADV>(k, N, Wk, tkm1, tk, tkp1, tkp2, cfk, cfk1);
  }
}
// The explicit vertical flux of the corrector's start, pre_step3d.F:837-890: FC(0) = dt*btflx, FC(N) = dt*stflx,
// between them cff3 * Akt * dt/dz (cff3 = dt*(1-lambda)), the KPP non-local term and the solar term (lmd_swfrac.F:6)
// with dt*srflx [*rmask_wet under WET_DRY, :876-878] formed first, left to right.  t(nnew) = Hz*t(nstp) + (FC(k) -
// FC(k-1)) (:894-898) is then the caller's: k_pre_t stores it, k_t3dmix_geo<0, ISO, false, true> adds its own term first.
struct VStart {
  double dt, cff3, dsrf, zwN, fac1, fac2, fac3;
  bool nonlocal, solar;
  gcd_t Akt, AktN, ghats, z_r, z_w;
  int itrc;
};
// the column's constants; c0 = index of (i,j,1)
__device__ __forceinline__ VStart vstart_column(const RomsDev *__restrict__ c, int itrc, long c0, long nij, long n3w)
{
  const roms_params_t &p = c->p;
  const roms_bounds_t &b = c->b;
  VStart v;
  v.dt = p.dt;
  v.cff3 = p.dt * (1.0 - p.lambda);
  v.nonlocal = p.lmd_nonlocal && itrc <= b.NAT;
  v.solar = p.solar_source && itrc == 1;
  v.Akt = tracer_akt(c, itrc, n3w);
  v.ghats = (gcd_t)(c->F.ghats + (long)((itrc <= b.NAT ? itrc : 1) - 1) * n3w);
  v.AktN = (gcd_t)(c->F.Akt + (long)((itrc <= b.NAT ? itrc : 1) - 1) * n3w);   // Akt(..,itrc) of the non-local term
  v.z_r = (gcd_t)(c->F.z_r);
  v.z_w = (gcd_t)(c->F.z_w);
  const double srf = GF(srflx)[c0];
  v.dsrf = p.wet_dry ? (p.dt * srf) * GF(rmask_wet)[c0] : p.dt * srf;
  v.zwN = v.z_w[c0 + (long)b.N * nij];
  v.fac1 = -1.0 / p.swfrac_mu1; v.fac2 = -1.0 / p.swfrac_mu2; v.fac3 = p.swfrac_r1;
  v.itrc = itrc;
  return v;
}
// what FC(k), k < N, reads at W-level k (cku = index of (i,j,k+1)): Akt and ghats of the non-local term, z_w of the
// solar term -- loaded values, so that a kernel may issue the loads a level ahead
struct VStartIn { double akn, gh, zwk; };
__device__ __forceinline__ VStartIn vstart_load(const VStart &v, long cku)
{
  VStartIn r{0.0, 0.0, 0.0};
  if (v.nonlocal) { r.akn = v.AktN[cku]; r.gh = v.ghats[cku]; }
  if (v.solar) r.zwk = v.z_w[cku];
  return r;
}
// FC(0), and FC(k), k = 1..N; cku = index of (i,j,k+1), in = vstart_load() of the level (unused at k = N), tk / tkp1 = t(nstp) of levels k and k+1, zr_k = z_r(k) carried by the
// caller (set to z_r(1) before the sweep when v.cff3 != 0).  EXPL = false: the caller has checked lambda = 1, where
// cff3 * (...) = +-0 -- z_r, the division and (without the non-local term) Akt are not read
__device__ __forceinline__ double vstart_bottom(const RomsDev *__restrict__ c, const VStart &v, long c0, long nij)
{
  return v.dt * GF(btflx)[c0 + (long)(v.itrc - 1) * nij];
}
template <bool EXPL>
__device__ __forceinline__ double vstart_flux(const RomsDev *__restrict__ c, const VStart &v, int k, int N, long c0, long nij,
                                              long cku, const VStartIn &in, double tk, double tkp1, double &zr_k)
{
  if (k == N) return v.dt * GF(stflx)[c0 + (long)(v.itrc - 1) * nij];
  double FDk = 0.0;
  if constexpr (EXPL) {
    if (v.cff3 != 0.0) {
      const double zr_k1 = v.z_r[cku];
      const double cz = 1.0 / (zr_k1 - zr_k);
      FDk = v.cff3 * cz * v.Akt[cku] * (tkp1 - tk);
      zr_k = zr_k1;
    }
  }
  if (v.nonlocal) FDk = FDk - v.dt * in.akn * in.gh;
  if (v.solar) {
    const double Z = v.zwN - in.zwk;
    const double swdk = exp(Z * v.fac1) * v.fac3 + exp(Z * v.fac2) * (1.0 - v.fac3);
    FDk = FDk + v.dsrf * swdk;
  }
  return FDk;
}

// Row k-1 of the forward elimination of the implicit vertical diffusion in spline form, step3d_t.F:1376-1410, formed
// while the upward sweep is at level k: *_m1 = level k-1, akt_m2 / akt_m1 / akt_0 = Akt(k-2) / Akt(k-1) / Akt(k),
// t_m1 / t_0 = the advected tracer of the two levels, CFm / DCm = CF(k-2) / DC(k-2); sets CF(k-1), DC(k-1).
__device__ __forceinline__ void thomas_row(double dt, double hz_m1, double ohz_m1, double hz, double ohz, double akt_m2,
                                           double akt_m1, double akt_0, double t_m1, double t_0, double CFm, double DCm,
                                           double &CF, double &DC)
{
  const double cff6 = 1.0 / 6.0, cff3r = 1.0 / 3.0;
  const double fc = cff6 * hz_m1 - dt * akt_m2 * ohz_m1;
  const double cf = cff6 * hz - dt * akt_0 * ohz;
  const double bc = cff3r * (hz_m1 + hz) + dt * akt_m1 * (ohz_m1 + ohz);
  const double cff = 1.0 / (bc - fc * CFm);
  CF = cff * cf;
  DC = cff * (t_0 - t_m1 - fc * DCm);
}

// ---------------------------------------------------------------------------
// Host side of the two entries (roms_hip_pre_step3d, roms_hip_step3d_t)
// ---------------------------------------------------------------------------
// Key Hadv * 16 + Vadv of a scheme pair for the switch over the built kernels.  SU3 runs the kernels of C4 (the
// "C4 / SU3" arms above) in the three pairs with SU3 that are built.
static inline int adv_pair(int ha, int va)
{
  const int hv = ha * 16 + va;
  switch (hv) {
  case ADV_U3 * 16 + ADV_SU3:    return ADV_U3 * 16 + ADV_C4;
  case ADV_SU3 * 16 + ADV_SU3:   return ADV_C4 * 16 + ADV_C4;
  case ADV_SU3 * 16 + ADV_HSIMT: return ADV_C4 * 16 + ADV_HSIMT;
  default:                       return hv;
  }
}
// length of the run of consecutive tracers it, it+1, ... (1-based, up to NT) that share tracer it's scheme pair: one
// launch per run (run-time selection per tracer, step3d_t.F:596+: one kernel per scheme, host dispatch)
static inline int adv_run_length(const roms_params_t &p, int NT, int it)
{
  const int ha = p.Hadv[it - 1], va = p.Vadv[it - 1];
  int n = 1;
  while (it + n <= NT && p.Hadv[it + n - 1] == ha && p.Vadv[it + n - 1] == va) n++;
  return n;
}
// The instantiation of a kernel template for columns of N levels: pick(NMAX) returns the kernel whose unrolled
// column arrays hold NMAX = 16 / 32 / (48, where the caller has that one) / ROMS_MAXN levels.
template <bool WITH48 = false, class Pick>
static inline auto kernel_for_n(int N, Pick pick)
{
  if (N <= 16) return pick(std::integral_constant<int, 16>{});
  if (N <= 32) return pick(std::integral_constant<int, 32>{});
  if constexpr (WITH48)
    if (N <= 48) return pick(std::integral_constant<int, 48>{});
  return pick(std::integral_constant<int, ROMS_MAXN>{});
}
