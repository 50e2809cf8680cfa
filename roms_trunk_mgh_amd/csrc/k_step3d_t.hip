// k_step3d_t.hip -- corrector time-step for tracers, step3d_t_tile
// (ROMS/Nonlinear/step3d_t.F:108-1682), as ONE fused kernel per tracer:
//
//   horizontal advection (C2/U3/A4/C4, :363-880) -> vertical advection
//   (C2/A4/C4/splines, :883-1210) -> t*oHz -> implicit vertical diffusion in
//   spline form (:1363-1455), per water column.
//
// Mapping: one thread per (i,j) water column, 64 consecutive i per wavefront,
// so every level of every field is read as contiguous 512-byte lines.  The
// column sweeps upward once (fluxes, advective update, Thomas forward
// elimination fused level by level) and downward once (back substitution +
// final update).  The column state the Thomas algorithm needs (post-advection
// tracer, modified super-diagonal CF, right-hand side DC) stays in VGPRs
// (fully unrolled, template on the maximum N), so t(:,:,:,nnew,itrc) is read
// once and written once.
//
// Algorithmic HBM traffic per cell and tracer: read t(..,3,itrc), read+write
// t(..,nnew,itrc), read Akt = 32 B, plus Huon,Hvom,W,Hz = 32 B shared by the
// tracers (8*(4*NT+4) B per cell).
//
// The arithmetic order inside every expression is the reference's (the build
// uses -ffp-contract=off), so results agree with the CPU restatement to the
// last bit except where a library function differs.
#include "roms_dev.h"
#include <cstdlib>

int roms_launch_step3d_t_mpdata(int nnew, int itrc0, int n);         // k_mpdata.hip

#include "advect.h"

namespace {

// ---------------------------------------------------------------------------
// HSIMT (Wu and Zhu, 2010) with the TVD limiter, step3d_t.F:430-590 (horizontal) and :1022-1090
// (vertical).  Evaluated straight from global memory by k_step3d_t_hsimt: an optional scheme that
// none of the five configurations uses, kept simple.  A face is named by the cell on its high side.
// ---------------------------------------------------------------------------
#define HS_EPS1 1.0E-12
__device__ __forceinline__ double hsimt_limited(double g0, double gn, double k0, double kn, double ok0)
{
  // cff of :473-489 for the upwind neighbour face (gn, kn): 0.5*MAX(0,MIN(2, 2 r rka, beta))*grad*Ka
  const double cc1 = 0.25, cc2 = 0.5, cc3 = 1.0 / 12.0;
  double r, rka;
  if (fabs(g0) <= HS_EPS1) { r = 0.0; rka = 0.0; }
  else { r = gn / g0; rka = kn * ok0; }
  const double a1 = cc1 * k0 + cc2 - cc3 * ok0;
  const double b1 = -cc1 * k0 + cc2 + cc3 * ok0;
  const double beta = a1 + b1 * r;
  return 0.5 * fmax(0.0, fmin(fmin(2.0, 2.0 * r * rka), beta)) * g0 * k0;
}
// horizontal face between cell (a - off) and cell a; off = 1 (xi, Huon) or ni (eta, Hvom).
// lo_zero / hi_zero: the wall rule of :451-464 / :527-540 applies to the neighbour face used.
// MASKING (fmask = umask / vmask of the direction, null without the option): the differences and Ka times the
// mask of their face (:448, :523) and the limited correction times rmask two cells upstream of the face,
// rmask(MAX(i-2,0)) or rmask(MIN(i+1,Lm+1)) (:487, :506, :562, :581); idx = the face's global i (j), idxmax = Lm+1 (Mm+1).
template <int DIR>
__device__ __forceinline__ double hsimt_hface(gcd_t t3, gcd_t H, gcd_t Hz, gcd_t pm, gcd_t pn, long a, long a2, long off,
                                              double dt, bool lo_zero, bool hi_zero, gcd_t fmask, gcd_t rmask, int idx,
                                              int idxmax)
{
  auto grad = [&](long x, long x2) {
    const double g = t3[x] - t3[x - off];
    return fmask ? g * fmask[x2] : g;
  };
  auto Ka = [&](long x, long x2) {
    double cff;
    if constexpr (DIR == 0) cff = 0.125 * (pm[x2 - off] + pm[x2]) * (pn[x2 - off] + pn[x2]) * dt;
    else cff = 0.125 * (pn[x2] + pn[x2 - off]) * (pm[x2] + pm[x2 - off]) * dt;
    double cff1;
    if constexpr (DIR == 0) cff1 = cff * (1.0 / Hz[x - off] + 1.0 / Hz[x]);
    else cff1 = cff * (1.0 / Hz[x] + 1.0 / Hz[x - off]);
    const double ka = 1.0 - fabs(H[x] * cff1);
    return fmask ? ka * fmask[x2] : ka;
  };
  const double Hf = H[a];
  const double g0 = grad(a, a2), k0 = Ka(a, a2);
  const double ok0 = (k0 <= HS_EPS1) ? 0.0 : 1.0 / fmax(k0, HS_EPS1);
  double sw;
  if (Hf >= 0.0) {
    const double gn = lo_zero ? 0.0 : grad(a - off, a2 - off), kn = lo_zero ? 0.0 : Ka(a - off, a2 - off);
    double cff = hsimt_limited(g0, gn, k0, kn, ok0);
    if (fmask) cff = cff * rmask[a2 + (long)((idx - 2 > 0 ? idx - 2 : 0) - idx) * off];
    sw = t3[a - off] + cff;
  } else {
    const double gn = hi_zero ? 0.0 : grad(a + off, a2 + off), kn = hi_zero ? 0.0 : Ka(a + off, a2 + off);
    double cff = hsimt_limited(g0, gn, k0, kn, ok0);
    if (fmask) cff = cff * rmask[a2 + (long)((idx + 1 < idxmax ? idx + 1 : idxmax) - idx) * off];
    sw = t3[a] - cff;
  }
  return sw * Hf;
}
// vertical flux through the top face of level k (W-level k), k = 1..N-1; a = index of (i,j,k) in rho arrays
__device__ __forceinline__ double hsimt_vface(gcd_t t3, gcd_t Wv, gcd_t z_r, long a, long nij, int k, int N, double cff)
{
  const double Wk = Wv[a + nij];
  if (k == 1 && Wk >= 0.0) return Wk * t3[a];
  if (k == N - 1 && Wk < 0.0) return Wk * t3[a + nij];
  // KaZ, gradZ at W-level q (1..N-1; zero at 0 and N), x = rho index of level q
  auto KaZ = [&](int q, long x) { return (q < 1 || q > N - 1) ? 0.0 : 1.0 - fabs(cff * Wv[x + nij] / (z_r[x + nij] - z_r[x])); };
  auto gradZ = [&](int q, long x) { return (q < 1 || q > N - 1) ? 0.0 : t3[x + nij] - t3[x]; };
  const double k0 = KaZ(k, a), g0 = gradZ(k, a);
  const double ok0 = 1.0 / k0;
  double sw;
  if (Wk >= 0) sw = t3[a] + hsimt_limited(g0, gradZ(k - 1, a - nij), k0, KaZ(k - 1, a - nij), ok0);
  else sw = t3[a + nij] - hsimt_limited(g0, gradZ(k + 1, a + nij), k0, KaZ(k + 1, a + nij), ok0);
  return Wk * sw;
}

// HSIMT in the vertical; in the horizontal HSIMT (three ghost points) or another scheme (two; not under MASKING).
// One thread per column, one upward sweep (fluxes, advective update, Thomas forward elimination) and one downward
// (back substitution), the column state in registers.
template <int HADV, int NMAX>
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_step3d_t_hsimt(const RomsDev *__restrict__ c, int nnew, int itrc0, int ntr)
{
  DEV_PROLOGUE(c)
  const TileCol tc = tile_column(b, itrc0, ntr);
  if (!tc.valid) return;
  const int i = tc.i, j = tc.j, itrc = tc.itrc;
  const double dt = c->p.dt;
  const gcd_t t3 = (gcd_t)tracer_level(c, 3, itrc, n3r);
  const gd_t tn_g = (gd_t)tracer_level(c, nnew, itrc, n3r);
  const ColFields f = column_fields(c);
  const gcd_t Akt = tracer_akt(c, itrc, n3w);
  const long c0 = I2(i, j);
  const double cffdt = dt * GF(pm)[c0] * GF(pn)[c0];
  const Walls wl = column_walls(c, i, j);
  // wall rows: the outer stencil point is not used; read a valid address instead
  const long oym2 = wl.s ? 0 : -2 * ni, oyp2 = wl.n ? 0 : 2 * ni;
  const long oxm2 = wl.w ? 0 : -2, oxp2 = wl.e ? 0 : 2;

  const bool src_cell = c->src.n > 0 && src_cell_any(c, c0, ni);      // LuvSrc: a face of this cell is a source face

  double tn[NMAX + 1], CF[NMAX + 1], DC[NMAX + 1];
  CF[0] = 0.0;
  DC[0] = 0.0;
  double FCprev = 0.0;
  double hz_m1 = 0.0, ohz_m1 = 0.0, akt_m2 = 0.0, akt_m1 = Akt[c0];   // Akt(k-1) for k=1 is Akt(0)

#pragma unroll
  for (int k = 1; k <= NMAX; k++) {
    if (k <= N) {
      const long ck = c0 + (long)(k - 1) * nij;
      const double hz = f.Hz[ck];
      double tv = tn_g[ck];
      const double akt_0 = Akt[ck + nij];          // Akt(i,j,k)
      const double tk = t3[ck];
      // ---- horizontal fluxes, step3d_t.F:430-590 or :596-828 ----
      Faces fx;
      if constexpr (HADV == ADV_HSIMT) {
        const gcd_t pmg = (gcd_t)c->F.pm, png = (gcd_t)c->F.pn;
        const bool mk = c->p.masking != 0;
        const gcd_t um = mk ? (gcd_t)c->F.umask : (gcd_t) nullptr, vm = mk ? (gcd_t)c->F.vmask : (gcd_t) nullptr;
        const gcd_t rm = (gcd_t)c->F.rmask;
        // physical edges: the face outside Istr / Jstr (Iend+1 / Jend+1) enters only through its zeroed gradient,
        // :451-464, :527-540
        fx.FXi = hsimt_hface<0>(t3, f.Huon, f.Hz, pmg, png, ck, c0, 1, dt, wl.w, false, um, rm, i, b.Lm + 1);
        fx.FXip1 = hsimt_hface<0>(t3, f.Huon, f.Hz, pmg, png, ck + 1, c0 + 1, 1, dt, false, wl.e, um, rm, i + 1, b.Lm + 1);
        fx.FEj = hsimt_hface<1>(t3, f.Hvom, f.Hz, pmg, png, ck, c0, ni, dt, wl.s, false, vm, rm, j, b.Mm + 1);
        fx.FEjp1 = hsimt_hface<1>(t3, f.Hvom, f.Hz, pmg, png, ck + ni, c0 + ni, ni, dt, false, wl.n, vm, rm, j + 1, b.Mm + 1);
      } else {
        HStencil s;
        s.xm2 = t3[ck + oxm2]; s.xm1 = t3[ck - 1]; s.xp1 = t3[ck + 1]; s.xp2 = t3[ck + oxp2];
        s.ym2 = t3[ck + oym2]; s.ym1 = t3[ck - ni]; s.yp1 = t3[ck + ni]; s.yp2 = t3[ck + oyp2];
        s.hu0 = f.Huon[ck]; s.hu1 = f.Huon[ck + 1];
        s.hv0 = f.Hvom[ck]; s.hv1 = f.Hvom[ck + ni];
        fx = cell_faces<HADV, false>(tk, s, wl, c, c0, ni);       // (the launcher refuses these pairs under MASKING)
      }
      if (src_cell)                                  // LuvSrc, step3d_t.F:734-799
        src_cell_fluxes<false>(c, c0, ck, ni, k, itrc, tracer_level(c, 3, itrc, n3r), fx.FXi, fx.FXip1, fx.FEj, fx.FEjp1);
      // ---- vertical flux through the top face of level k; cff = pm*pn*dt in this order, :1032 ----
      const double FCk = (k == N) ? 0.0 : hsimt_vface(t3, f.W, (gcd_t)c->F.z_r, ck, nij, k, N, GF(pm)[c0] * GF(pn)[c0] * dt);
      // ---- advective update, step3d_t.F:857-875 and :1168-1208 ----
      const double ohz = 1.0 / hz;
      {
        const double cff1 = cffdt * (fx.FXip1 - fx.FXi);
        const double cff2 = cffdt * (fx.FEjp1 - fx.FEj);
        const double cff3 = cff1 + cff2;
        tv = tv - cff3;
      }
      tv = tv - cffdt * (FCk - FCprev);
      tv = tv * ohz;
      if (src_cell) tv = src_w_tracer(c, c0, k, itrc, cffdt * ohz, tk, tv);       // LwSrc, step3d_t.F:1331-1360
      tn[k] = tv;
      FCprev = FCk;
      if (k >= 2)       // row k-1 of the forward elimination
        thomas_row(dt, hz_m1, ohz_m1, hz, ohz, akt_m2, akt_m1, akt_0, tn[k - 1], tn[k], CF[k - 2], DC[k - 2], CF[k - 1],
                   DC[k - 1]);
      hz_m1 = hz; ohz_m1 = ohz; akt_m2 = akt_m1; akt_m1 = akt_0;
    }
  }

  // ---- back substitution + final update, step3d_t.F:1411-1455 ----
  double dcA_up = 0.0;      // DC(N)*Akt(N) = 0
  double dc_up = 0.0;       // DC(N) = 0
#pragma unroll
  for (int kk = NMAX - 1; kk >= 0; kk--) {
    if (kk <= N - 1) {
      double dcA = 0.0;
      if (kk >= 1) {
        const double dc = DC[kk] - CF[kk] * dc_up;
        dc_up = dc;
        dcA = dc * Akt[c0 + (long)kk * nij];
      }
      const long ck = c0 + (long)kk * nij;        // level kk+1
      const double ohz = 1.0 / f.Hz[ck];
      const double cff1 = dt * ohz * (dcA_up - dcA);
      double tv = tn[kk + 1] + cff1;
      if constexpr (HADV == ADV_HSIMT)          // step3d_t.F:1586-1596
        if (c->p.masking) tv = tv * GF(rmask)[c0];
      tn_g[ck] = tv;
      dcA_up = dcA;
    }
  }
}

// ---------------------------------------------------------------------------
// The corrector of every other scheme pair, software-pipelined.  The post-advection tracer column tn()
// lives in LDS ([level][thread], conflict-free) rather than in ~60 VGPRs; those hold the 17 loads of level
// k+1, issued BEFORE level k is computed, so one memory round trip overlaps a whole level
// of arithmetic (and the other wave of the SIMD).  The downward sweep prefetches Akt and
// Hz two levels ahead.
//
// Tuning notes (MI355X, BENCHMARK3, profiles/r01c; measured on the kernel's unpipelined predecessor, which read every
// level straight from memory with tn() in registers): the sweep is bound by memory LATENCY per level, not by bytes --
// FETCH_SIZE barely moves the time.  Issuing every load of a level before the first use took 0.59 -> 0.53 ms.  Taller
// workgroups (64x8) changed neither traffic nor time (j-halo rows are L2 hits).  A compile-time N (no guards in the
// unrolled loop) let the scheduler hoist loads of many levels at once and was 2-3x SLOWER (occupancy 1 or scratch
// spills), so the run-time guards stay.  XCD strips (roms_dev.h) cut the fetch from 2.1 to 1.8 GB.
// ---------------------------------------------------------------------------
struct LevelIn {         // (members in the order of the loads: the copy cur = nxt follows it)
  double tkp2;
  HStencil s;
  double w, hz, tv, akt;
};

// MASK (MASKING applications, a second instantiation so that the unmasked kernel keeps its registers): the
// first differences are multiplied by umask / vmask of their face (step3d_t.F:603, :667) and the result by
// rmask (:1586-1596); the masks are read per level (cache hits) rather than held in registers.
// SRC (LuvSrc, point sources): the cells with a source face are a handful; the plain instantiation skips them (one
// look at the face maps per column, and only when there is a table) and the SRC instantiation -- the same text plus the
// replacement of the source faces' fluxes, step3d_t.F:734-799 -- runs over the list of those cells, grid =
// (cells / 256, tracers of the launch).  The threads of the kernel do not cooperate, so any cell-to-thread map will do.
// SPL = false (without SPLINES_VDIFF, step3d_t.F:1431-1501; 3 of the reference's 31 three-dimensional applications): the
// advected tracer stays thickness-weighted (:1196-1198 is not compiled) and the implicit vertical diffusion is a
// tridiagonal system for the tracer itself with the layer distances from z_r -- solved after the level loop from the
// column in LDS.  Instantiated at NMAX = 64 only (one kernel serves every N, not tuned).
// DIA (DIAGNOSTICS_TS; NMAX = 64 only, not tuned): per level the upward sweep writes DiaTwrk(iTxadv, iTyadv, iThadv,
// iTvadv) (step3d_t.F:868-871, :1199) and multiplies every term of the level by oHz (:1200-1203) -- those it has just
// formed in registers, and the planes iTrate, iTvdif and iT?dif that k_pre_t and k_t3dmix_s wrote earlier in the step,
// read, scaled and written back; the back substitution adds the implicit increment to iTvdif (:1421-1424, or
// :1482-1485 / :1495-1498 without SPLINES_VDIFF).  Six (nine with ts_dif2) planes per tracer, each store 64
// consecutive doubles per wavefront like the tracer's own.
template <int HADV, int VADV, int NMAX, bool MASK, bool SRC = false, bool SPL = true, bool DIA = false>
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_step3d_t_pipe(const RomsDev *__restrict__ c, int nnew, int itrc0, int ntr)
{
  DEV_PROLOGUE(c)
  constexpr int NTH = BLK_X * BLK_Y;
  __shared__ double s_tn[NMAX * NTH];
  const int tid = threadIdx.y * BLK_X + threadIdx.x;
  int i, j, itrc;
  if constexpr (SRC) {
    const int q = blockIdx.x * NTH + tid;
    if (q >= c->src.ncell) return;
    const int cell = c->src.cells[q];
    i = LBi + (int)(cell % ni);
    j = LBj + (int)(cell / ni);
    itrc = itrc0 + (int)blockIdx.y;
  } else {
    const TileCol tc = tile_column(b, itrc0, ntr);
    if (!tc.valid) return;
    i = tc.i; j = tc.j; itrc = tc.itrc;
    if (c->src.n > 0 && src_cell_any(c, I2(i, j), ni)) return;      // the SRC launch steps this column
  }
  const double dt = c->p.dt;
  const gcd_t t3 = (gcd_t)tracer_level(c, 3, itrc, n3r);
  const gd_t tn_g = (gd_t)tracer_level(c, nnew, itrc, n3r);
  const ColFields f = column_fields(c);
  const gcd_t Akt = tracer_akt(c, itrc, n3w);
  const long c0 = I2(i, j);
  const double cffdt = dt * GF(pm)[c0] * GF(pn)[c0];
  const Walls wl = column_walls(c, i, j);
  // wall rows: the outer stencil point is not used; read a valid address instead
  const long oym2 = wl.s ? 0 : -2 * ni, oyp2 = wl.n ? 0 : 2 * ni;
  const long oxm2 = wl.w ? 0 : -2, oxp2 = wl.e ? 0 : 2;
  static_assert(!(DIA && SRC), "point sources are refused together with the diagnostics");
  // the planes of the terms, found once per column (DIA = false: never set, never read)
  struct { gd_t xadv, yadv, hadv, vadv, rate, vdif, hdif, xdif, ydif; } dp{};
  bool dia_hdif = false;                                   // ts_dif2: the planes iThdif, iTxdif, iTydif exist
  if constexpr (DIA) {
    dp.xadv = DIA_PLANE(c, DIA_iTxadv, itrc, n3r); dp.yadv = DIA_PLANE(c, DIA_iTyadv, itrc, n3r);
    dp.hadv = DIA_PLANE(c, DIA_iThadv, itrc, n3r); dp.vadv = DIA_PLANE(c, DIA_iTvadv, itrc, n3r);
    dp.rate = DIA_PLANE(c, DIA_iTrate, itrc, n3r); dp.vdif = DIA_PLANE(c, DIA_iTvdif, itrc, n3r);
    dia_hdif = c->dia.ndt > 6;
    if (dia_hdif) {
      dp.hdif = DIA_PLANE(c, DIA_iThdif, itrc, n3r); dp.xdif = DIA_PLANE(c, DIA_iTxdif, itrc, n3r);
      dp.ydif = DIA_PLANE(c, DIA_iTydif, itrc, n3r);
    }
  }

  double CF[NMAX + 1], DC[NMAX + 1];
  CF[0] = 0.0;
  DC[0] = 0.0;

  // vertical schemes that need the whole column first
  double a4cf[(VADV == ADV_A4) ? NMAX + 2 : 1];
  double spl[(VADV == ADV_SPLINES) ? NMAX + 1 : 1];
  if constexpr (VADV == ADV_A4) a4_slopes<NMAX>(t3, c0, nij, N, a4cf);
  if constexpr (VADV == ADV_SPLINES) spline_w<false, NMAX>(t3, f.Hz, f.W, c0, nij, N, spl);

  auto load_level = [&](int k) {
    LevelIn L;
    const long ck = c0 + (long)(k - 1) * nij;
    L.hz = f.Hz[ck];
    L.tv = tn_g[ck];
    L.akt = Akt[ck + nij];
    L.w = f.W[ck + nij];
    L.tkp2 = (k + 2 <= N) ? t3[ck + 2 * nij] : 0.0;
    L.s.xm2 = t3[ck + oxm2]; L.s.xm1 = t3[ck - 1]; L.s.xp1 = t3[ck + 1]; L.s.xp2 = t3[ck + oxp2];
    L.s.ym1 = t3[ck - ni]; L.s.yp1 = t3[ck + ni];
    L.s.ym2 = t3[ck + oym2];
    L.s.yp2 = t3[ck + oyp2];
    L.s.hu0 = f.Huon[ck]; L.s.hu1 = f.Huon[ck + 1];
    L.s.hv0 = f.Hvom[ck]; L.s.hv1 = f.Hvom[ck + ni];
    return L;
  };

  double tkm1 = 0.0, tk = t3[c0], tkp1 = (N >= 2) ? t3[c0 + nij] : 0.0;
  double FCprev = 0.0, tn_prev = 0.0;
  double hz_m1 = 0.0, ohz_m1 = 0.0, akt_m2 = 0.0, akt_m1 = Akt[c0];
  LevelIn cur = load_level(1);

#pragma unroll
  for (int k = 1; k <= NMAX; k++) {
    if (k <= N) {
      LevelIn nxt;
      if (k + 1 <= N) nxt = load_level(k + 1);       // in flight while level k is computed
      const double tkp2 = cur.tkp2;
      Faces fx = cell_faces<HADV, MASK>(tk, cur.s, wl, c, c0, ni);
      if constexpr (SRC)                             // LuvSrc, step3d_t.F:734-799
        src_cell_fluxes<false>(c, c0, c0 + (long)(k - 1) * nij, ni, k, itrc, tracer_level(c, 3, itrc, n3r), fx.FXi, fx.FXip1,
                               fx.FEj, fx.FEjp1);
      const double FCk = vflux_level<VADV>(k, N, cur.w, tkm1, tk, tkp1, tkp2, spl, a4cf);
      const double hz = cur.hz;
      const double ohz = 1.0 / hz;
      double tv = cur.tv;
      const double cff1 = cffdt * (fx.FXip1 - fx.FXi);
      const double cff2 = cffdt * (fx.FEjp1 - fx.FEj);
      const double cff3 = cff1 + cff2;
      tv = tv - cff3;
      const double cffv = cffdt * (FCk - FCprev);
      tv = tv - cffv;
      if constexpr (SPL) tv = tv * ohz;
      if constexpr (DIA) {
        const long ck = c0 + (long)(k - 1) * nij;
        dp.xadv[ck] = -cff1 * ohz;
        dp.yadv[ck] = -cff2 * ohz;
        dp.hadv[ck] = -cff3 * ohz;
        dp.vadv[ck] = -cffv * ohz;
        dp.rate[ck] = dp.rate[ck] * ohz;
        dp.vdif[ck] = dp.vdif[ck] * ohz;
        if (dia_hdif) {
          dp.hdif[ck] = dp.hdif[ck] * ohz;
          dp.xdif[ck] = dp.xdif[ck] * ohz;
          dp.ydif[ck] = dp.ydif[ck] * ohz;
        }
      }
      if constexpr (SRC) tv = src_w_tracer(c, c0, k, itrc, SPL ? cffdt * ohz : cffdt, tk, tv);   // LwSrc, step3d_t.F:1331-1360
      s_tn[(k - 1) * NTH + tid] = tv;
      FCprev = FCk;
      const double akt_0 = cur.akt;
      if (SPL && k >= 2)       // row k-1 of the forward elimination
        thomas_row(dt, hz_m1, ohz_m1, hz, ohz, akt_m2, akt_m1, akt_0, tn_prev, tv, CF[k - 2], DC[k - 2], CF[k - 1], DC[k - 1]);
      tn_prev = tv;
      hz_m1 = hz; ohz_m1 = ohz; akt_m2 = akt_m1; akt_m1 = akt_0;
      tkm1 = tk; tk = tkp1; tkp1 = tkp2;
      cur = nxt;
    }
  }

  if constexpr (!SPL) {
    // the tridiagonal system of step3d_t.F:1431-1501: FC(k) = -dt lambda Akt(k) / (z_r(k+1) - z_r(k)),
    // BC(k) = Hz(k) - FC(k) - FC(k-1), right-hand side = the advected, thickness-weighted tracer
    const gcd_t z_r = (gcd_t)c->F.z_r;
    const double cfl = -dt * c->p.lambda;
    double fc_prev = 0.0;
#pragma unroll
    for (int k = 1; k <= NMAX; k++) {
      if (k <= N) {
        const long ck = c0 + (long)(k - 1) * nij;
        double fc = 0.0;
        if (k < N) {
          const double cff1 = 1.0 / (z_r[ck + nij] - z_r[ck]);
          fc = cfl * cff1 * Akt[ck + nij];
        }
        const double bc = f.Hz[ck] - fc - fc_prev;
        const double d = s_tn[(k - 1) * NTH + tid];
        if (k == 1) {
          const double cff = 1.0 / bc;
          CF[1] = cff * fc;
          DC[1] = cff * d;
        } else if (k < N) {
          const double cff = 1.0 / (bc - fc_prev * CF[k - 1]);
          CF[k] = cff * fc;
          DC[k] = cff * (d - fc_prev * DC[k - 1]);
        } else {
          DC[k] = (d - fc_prev * DC[k - 1]) / (bc - fc_prev * CF[k - 1]);
        }
        fc_prev = fc;
      }
    }
    double up = 0.0;
#pragma unroll
    for (int k = NMAX; k >= 1; k--) {
      if (k <= N) {
        const double v = (k == N) ? DC[k] : DC[k] - CF[k] * up;
        up = v;
        const long ck = c0 + (long)(k - 1) * nij;
        if constexpr (DIA) {                         // step3d_t.F:1476, :1482-1485 (k = N), :1490, :1495-1498
          const double cff1 = s_tn[(k - 1) * NTH + tid] * (1.0 / f.Hz[ck]);
          dp.vdif[ck] = dp.vdif[ck] + v - cff1;
        }
        if constexpr (MASK) tn_g[ck] = v * GF(rmask)[c0];
        else tn_g[ck] = v;
      }
    }
    return;
  }
  // ---- back substitution + final update; Akt(kk), Hz(kk+1) prefetched two levels ahead ----
  double dcA_up = 0.0, dc_up = 0.0;
  double akA = Akt[c0 + (long)(N - 1) * nij], hzA = f.Hz[c0 + (long)(N - 1) * nij];
  double akB = 0.0, hzB = 0.0;
  if (N >= 2) { akB = Akt[c0 + (long)(N - 2) * nij]; hzB = f.Hz[c0 + (long)(N - 2) * nij]; }
#pragma unroll
  for (int kk = NMAX - 1; kk >= 0; kk--) {
    if (kk <= N - 1) {
      double akC = 0.0, hzC = 0.0;
      if (kk >= 2) { akC = Akt[c0 + (long)(kk - 2) * nij]; hzC = f.Hz[c0 + (long)(kk - 2) * nij]; }
      double dcA = 0.0;
      if (kk >= 1) {
        const double dc = DC[kk] - CF[kk] * dc_up;
        dc_up = dc;
        dcA = dc * akA;
      }
      const long ck = c0 + (long)kk * nij;
      const double ohz = 1.0 / hzA;
      const double cff1 = dt * ohz * (dcA_up - dcA);
      if constexpr (MASK) tn_g[ck] = (s_tn[kk * NTH + tid] + cff1) * GF(rmask)[c0];
      else tn_g[ck] = s_tn[kk * NTH + tid] + cff1;
      if constexpr (DIA) {                           // step3d_t.F:1421-1424
        dp.vdif[ck] = dp.vdif[ck] + cff1;
      }
      dcA_up = dcA;
      akA = akB; hzA = hzB; akB = akC; hzB = hzC;
    }
  }
}

typedef void (*StepKernel)(const RomsDev *, int, int, int);

// HSIMT in the vertical, with HSIMT (HADV = ADV_HSIMT) or another scheme in the horizontal
template <int HADV>
int launch_hsimt(int nnew, int itrc0, int ntr)
{
  const roms_bounds_t &b = g_ctx.b;
  const dim3 grid = grid_tile_tracer(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1, ntr);
  if (b.N > ROMS_MAXN) return roms_fail("roms_hip_step3d_t", "N > 64 not instantiated");
  if (HADV != ADV_HSIMT && g_ctx.p.masking)
    return roms_fail("roms_hip_step3d_t", "MASKING is not built for the pair (other scheme, HSIMT)");
  const StepKernel kernel = kernel_for_n(b.N, [](auto nm) -> StepKernel { return k_step3d_t_hsimt<HADV, nm.value>; });
  hipLaunchKernelGGL(kernel, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, nnew, itrc0, ntr);
  KERNEL_CHECK("k_step3d_t");
  return 0;
}

// the software-pipelined kernel, then its SRC instantiation over the cells with a source face
template <int HADV, int VADV>
int launch_pipe(int nnew, int itrc0, int ntr)
{
  const roms_bounds_t &b = g_ctx.b;
  const dim3 grid = grid_tile_tracer(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1, ntr);
  if (b.N > ROMS_MAXN) return roms_fail("roms_hip_step3d_t", "N > 64 not instantiated");
  const bool mask = g_ctx.p.masking != 0, spl = g_ctx.p.splines_vdiff != 0;
  StepKernel kernel;
  if (dia_on())      // DIAGNOSTICS_TS: one instantiation for every N (dia_check has refused point sources)
    kernel = mask ? (spl ? k_step3d_t_pipe<HADV, VADV, ROMS_MAXN, true, false, true, true>
                         : k_step3d_t_pipe<HADV, VADV, ROMS_MAXN, true, false, false, true>)
                  : (spl ? k_step3d_t_pipe<HADV, VADV, ROMS_MAXN, false, false, true, true>
                         : k_step3d_t_pipe<HADV, VADV, ROMS_MAXN, false, false, false, true>);
  else if (!spl)     // without SPLINES_VDIFF: one instantiation for every N
    kernel = mask ? k_step3d_t_pipe<HADV, VADV, ROMS_MAXN, true, false, false>
                  : k_step3d_t_pipe<HADV, VADV, ROMS_MAXN, false, false, false>;
  else if (mask)     // land/sea masks applied
    kernel = kernel_for_n(b.N, [](auto nm) -> StepKernel { return k_step3d_t_pipe<HADV, VADV, nm.value, true>; });
  else               // NMAX = 48: the column arrays then spill into AGPRs (one wave per SIMD); slower per cell, same results
    kernel = kernel_for_n<true>(b.N, [](auto nm) -> StepKernel { return k_step3d_t_pipe<HADV, VADV, nm.value, false>; });
  hipLaunchKernelGGL(kernel, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, nnew, itrc0, ntr);
  KERNEL_CHECK("k_step3d_t");
  // LuvSrc: the cells with a source face (one instantiation serves every N: a handful of columns)
  const int ncell = g_ctx.hostc.src.ncell;
  if (ncell > 0) {
    const dim3 gs((ncell + BLK_X * BLK_Y - 1) / (BLK_X * BLK_Y), ntr);
    const StepKernel ks = mask ? (spl ? k_step3d_t_pipe<HADV, VADV, ROMS_MAXN, true, true>
                                      : k_step3d_t_pipe<HADV, VADV, ROMS_MAXN, true, true, false>)
                               : (spl ? k_step3d_t_pipe<HADV, VADV, ROMS_MAXN, false, true>
                                      : k_step3d_t_pipe<HADV, VADV, ROMS_MAXN, false, true, false>);
    hipLaunchKernelGGL(ks, gs, block2d(), 0, g_ctx.stream, g_ctx.devc, nnew, itrc0, ntr);
    KERNEL_CHECK("k_step3d_t (source cells)");
  }
  return 0;
}

// Nudging towards the tracer climatology, step3d_t.F:1572-1584, and the land/sea mask that follows it (:1590-1596):
//   t(nnew) = t(nnew) + dt * Tnudgcof(ic) * (tclm(ic) - t(nnew))      on IstrR:IendR, JstrR:JendR
// after t3dbc_tile (the radiation condition reads the un-nudged interior, and the boundary points are nudged too),
// before the exchange.  One thread per point, all nudged tracers in one launch (blockIdx.z = level + N * (ic-1)),
// consecutive lanes along i: three reads and one write of a double per point.  t(nnew) arrives masked (the advection
// kernel and t3dbc_tile end with the mask), so a land point stays a zero of either sign.
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_t_nudge(const RomsDev *__restrict__ c, int nnew)
{
  DEV_PROLOGUE(c)
  const RomsClima &C = c->clima;
  const int i = b.IstrR + blockIdx.x * BLK_X + threadIdx.x, j = b.JstrR + blockIdx.y * BLK_Y + threadIdx.y;
  if (i > b.IendR || j > b.JendR) return;
  const int k = blockIdx.z % N + 1, ic = blockIdx.z / N + 1;
  const int itrc = C.itrc[ic - 1];
  const long q2 = I2(i, j), q = q2 + (long)(k - 1) * nij;
  const gd_t t = (gd_t)(c->F.t + ((long)(nnew - 1) + 3L * (itrc - 1)) * n3r);
  const long qc = q + (long)(ic - 1) * n3r;
  const double t0 = t[q];
  double tn = t0 + c->p.dt * ((gcd_t)C.Tnudgcof)[qc] * (((gcd_t)C.tclm)[qc] - t0);
  if (c->p.masking) tn = tn * GF(rmask)[q2];
  t[q] = tn;
}

}  // namespace

extern "C" int roms_hip_step3d_t(const roms_step_idx_t *s)
{
  int rc = roms_entry_check("roms_hip_step3d_t");
  if (rc) return rc;
  if ((rc = check_lbc())) return rc;
  const roms_bounds_t &b = g_ctx.b;
  const roms_params_t &p = g_ctx.p;
  if (b.N < 4) return roms_fail("roms_hip_step3d_t", "needs N >= 4 levels (the vertical stencils of the column read k-1 .. k+2)");
  if ((rc = dia_check("roms_hip_step3d_t"))) return rc;
  if (!p.splines_vdiff)
    for (int it = 1; it <= b.NT; it++)
      if (p.Hadv[it - 1] == ADV_HSIMT || p.Vadv[it - 1] == ADV_HSIMT)
        return roms_fail("roms_hip_step3d_t", "HSIMT without SPLINES_VDIFF is not built (the straight-from-memory kernel "
                                              "carries the spline form of the vertical diffusion only)");
  {
    ScopedTimer tm("step3d_t");
    int it = 1;
    while (it <= b.NT) {
      const int n = adv_run_length(p, b.NT, it);
      switch (adv_pair(p.Hadv[it - 1], p.Vadv[it - 1])) {
      case ADV_U3 * 16 + ADV_C4:  rc = launch_pipe<ADV_U3, ADV_C4>(s->nnew, it, n); break;
      case ADV_A4 * 16 + ADV_A4:  rc = launch_pipe<ADV_A4, ADV_A4>(s->nnew, it, n); break;
      case ADV_C4 * 16 + ADV_C4:  rc = launch_pipe<ADV_C4, ADV_C4>(s->nnew, it, n); break;
      case ADV_C2 * 16 + ADV_C2:  rc = launch_pipe<ADV_C2, ADV_C2>(s->nnew, it, n); break;
      case ADV_U3 * 16 + ADV_SPLINES: rc = launch_pipe<ADV_U3, ADV_SPLINES>(s->nnew, it, n); break;
      case ADV_C4 * 16 + ADV_SPLINES: rc = launch_pipe<ADV_C4, ADV_SPLINES>(s->nnew, it, n); break;
      case ADV_A4 * 16 + ADV_SPLINES: rc = launch_pipe<ADV_A4, ADV_SPLINES>(s->nnew, it, n); break;
      case ADV_HSIMT * 16 + ADV_HSIMT: {
        // three-point footprint: refresh the ghost points of t(nnew) first (step3d_t.F:369-386)
        if (b.NghostPoints != 3) return roms_fail("roms_hip_step3d_t", "HSIMT needs NghostPoints = 3 (inp_par.F:266-278)");
        const long n3r_ = (long)(b.UBi - b.LBi + 1) * (b.UBj - b.LBj + 1) * b.N;
        halo_batch_begin();
        for (int q = 0; q < n; q++)
          halo_exchange3d(GT_R, b.N, g_ctx.field[FID_t].dev + ((long)(s->nnew - 1) + 3L * (it + q - 1)) * n3r_);
        if ((rc = halo_batch_end())) return rc;
        rc = launch_hsimt<ADV_HSIMT>(s->nnew, it, n);
        break;
      }
      // HSIMT vertically with another scheme horizontally (two ghost points suffice)
      case ADV_U3 * 16 + ADV_HSIMT: rc = launch_hsimt<ADV_U3>(s->nnew, it, n); break;
      case ADV_C4 * 16 + ADV_HSIMT: rc = launch_hsimt<ADV_C4>(s->nnew, it, n); break;
      case ADV_A4 * 16 + ADV_HSIMT: rc = launch_hsimt<ADV_A4>(s->nnew, it, n); break;
      case ADV_C2 * 16 + ADV_HSIMT: rc = launch_hsimt<ADV_C2>(s->nnew, it, n); break;
      case ADV_MPDATA * 16 + ADV_MPDATA:
        // multi-pass: upstream step, anti-diffusive velocities, FCT limiter, corrected step (k_mpdata.hip)
        rc = roms_launch_step3d_t_mpdata(s->nnew, it, n);
        break;
      default:
        return roms_fail("roms_hip_step3d_t", "advection scheme pair not implemented (MPDATA and HSIMT only as H+V pairs)");
      }
      if (rc) return rc;
      it += n;
    }
  }
  // t3dbc_tile + periodic wrap / mp_exchange4d, step3d_t.F:1564-1626
  for (int it = 1; it <= b.NT; it++)
    if ((rc = bc_t3d(s->nnew, it, s->nstp))) return rc;
  if (g_ctx.hostc.clima.nt > 0) {
    ScopedTimer tm("step3d_t_nudge");
    const dim3 grid((b.IendR - b.IstrR + BLK_X) / BLK_X, (b.JendR - b.JstrR + BLK_Y) / BLK_Y, b.N * g_ctx.hostc.clima.nt);
    hipLaunchKernelGGL(k_t_nudge, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, s->nnew);
    KERNEL_CHECK("k_t_nudge");
  }
  if (dia_on() && (rc = dia_rate(s->nnew))) return rc;     // step3d_t.F:1598-1611
  const long n3r = (long)(b.UBi - b.LBi + 1) * (b.UBj - b.LBj + 1) * b.N;
  halo_batch_begin();
  for (int it = 1; it <= b.NT; it++)
    halo_exchange3d(GT_R, b.N, g_ctx.field[FID_t].dev + ((long)(s->nnew - 1) + 3L * (it - 1)) * n3r);
  return halo_batch_end();
}
