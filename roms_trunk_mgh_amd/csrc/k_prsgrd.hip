// k_prsgrd.hip -- baroclinic pressure gradient, prsgrd32_tile
// (ROMS/Nonlinear/prsgrd32.h:106-423; DJ_GRADPS: density Jacobian with
// harmonic-mean limited cubic reconstruction, Shchepetkin & McWilliams 2003).
// First writer of ru,rv(:,:,1:N,nrhs).
//
// One kernel, k_prsgrd32: one thread per water column of a 64 x 4 tile, marching down from the surface.  Per level the
// thread advances the top-down recursion for the dynamic pressure P of its column (3-level sliding windows in
// registers; reads rho, z_r, z_w(N)), hands P(k) to its neighbours through LDS and evaluates the horizontal
// harmonic-mean slopes and the XI/ETA pressure-gradient terms of its point (reads rho, z_r, Hz with a 2-point i/j halo
// served by L1/L2; writes ru, rv).  P never reaches memory.
// Algorithmic traffic: rho, z_r, Hz read, ru, rv written = 5 field passes (40 B per cell); with the predictor's
// momentum start inside (roms_hip_rhs3d): + u, v(nstp), ru, rv of both levels read, u, v(nnew) written = 13 passes.
#include "roms_dev.h"

namespace {

__device__ __forceinline__ double harm(double a, double bq, double eps)
{
  // cff=2*a*b; cff>eps ? cff/(a+b) : 0  (prsgrd32.h:243-249)
  const double cff = 2.0 * a * bq;
  return (cff > eps) ? cff / (a + bq) : 0.0;
}
__device__ __forceinline__ double harm_inv(double a, double bq, double eps)
{
  // the horizontal form multiplies by a reciprocal (prsgrd32.h:306-320)
  const double cff = 2.0 * a * bq;
  if (cff > eps) { const double cff1 = 1.0 / (a + bq); return cff * cff1; }
  return 0.0;
}

// The P recursion of one water column (prsgrd32.h:215-290), top-down: the windows of rho, z_r and the limited slopes of
// the level above.  After P(k) has been formed, r_up, z_up are rho, z_r(k).  (The raw differences of the window are
// formed from it where they are used: the same subtraction of the same two values.)
struct PCol { double r_up, z_up, r_dn, z_dn, P_up, dR_up, dZ_up; };

// P(N) and the windows of level N
__device__ __forceinline__ double prsgrd32_P_top(const RomsDev *__restrict__ c, gcd_t rho, gcd_t z_r, long c0, int N,
                                                 long nij, PCol &q)
{
  const double eps = 1.0E-10;
  const double g = c->p.g, GRho = g / c->p.rho0;
  // raw differences: dRr(k)=rho(k+1)-rho(k), k=1..N-1; dRr(N)=dRr(N-1); dRr(0)=dRr(1)
  const double rho_k1 = rho[c0 + (long)(N - 1) * nij];      // rho(N)
  const double zr_k1 = z_r[c0 + (long)(N - 1) * nij];
  const double rho_k = rho[c0 + (long)(N - 2) * nij];       // rho(N-1)
  const double zr_k = z_r[c0 + (long)(N - 2) * nij];
  const double zwN = GF(z_w)[c0 + (long)N * nij];
  // surface level
  const double cff1 = 1.0 / (zr_k1 - zr_k);
  const double cff2 = 0.5 * (rho_k1 - rho_k) * (zwN - zr_k1) * cff1;
  double P;
  // ATM_PRESS (prsgrd32.h:229-232, :264-266): + (100 / rho0) (Pair - 1 atm), Pair in mb
  if (c->p.atm_press)
    P = g * zwN + (100.0 / c->p.rho0) * (GF(Pair)[c0] - 1013.25) + GRho * (rho_k1 + cff2) * (zwN - zr_k1);
  else
    P = g * zwN + GRho * (rho_k1 + cff2) * (zwN - zr_k1);
  // limited slopes at level N: harm(raw(N), raw(N-1)) with raw(N)=raw(N-1)
  const double rawR_k = rho_k1 - rho_k, rawZ_k = zr_k1 - zr_k;       // raw(N-1)
  q.r_up = rho_k1; q.z_up = zr_k1; q.r_dn = rho_k; q.z_dn = zr_k;
  q.dR_up = harm(rawR_k, rawR_k, eps);                                // dR(N)
  q.dZ_up = 2.0 * rawZ_k * rawZ_k / (rawZ_k + rawZ_k);                // dZ(N)
  q.P_up = P;
  return P;
}

// P(k) from the windows of level k+1, k = N-1 .. 1
__device__ __forceinline__ double prsgrd32_P_down(gcd_t rho, gcd_t z_r, long c0, int k, long nij, double HalfGRho, PCol &q)
{
  const double eps = 1.0E-10, OneFifth = 0.2, OneTwelfth = 1.0 / 12.0;
  const double rho_k1 = q.r_up, zr_k1 = q.z_up, rho_k = q.r_dn, zr_k = q.z_dn;
  const double rawR_k = rho_k1 - rho_k, rawZ_k = zr_k1 - zr_k, dR_k1 = q.dR_up, dZ_k1 = q.dZ_up;
  // raw(k-1): k-1 >= 1 -> rho(k)-rho(k-1); k-1 == 0 -> raw(1)
  double rawR_km1, rawZ_km1, rho_km1 = 0.0, zr_km1 = 0.0;
  if (k >= 2) {
    rho_km1 = rho[c0 + (long)(k - 2) * nij];
    zr_km1 = z_r[c0 + (long)(k - 2) * nij];
    rawR_km1 = rho_k - rho_km1;
    rawZ_km1 = zr_k - zr_km1;
  } else { rawR_km1 = rawR_k; rawZ_km1 = rawZ_k; }
  const double dR_k = harm(rawR_k, rawR_km1, eps);
  const double dZ_k = 2.0 * rawZ_k * rawZ_km1 / (rawZ_k + rawZ_km1);
  const double Pk = q.P_up +
      HalfGRho * ((rho_k1 + rho_k) * (zr_k1 - zr_k) -
                  OneFifth *
                  ((dR_k1 - dR_k) * (zr_k1 - zr_k - OneTwelfth * (dZ_k1 + dZ_k)) -
                   (dZ_k1 - dZ_k) * (rho_k1 - rho_k - OneTwelfth * (dR_k1 + dR_k))));
  q.P_up = Pk;
  q.r_up = rho_k; q.z_up = zr_k; q.r_dn = rho_km1; q.z_dn = zr_km1;
  q.dR_up = dR_k; q.dZ_up = dZ_k;
  return Pk;
}

// The horizontal level body of one face (off = 1: XI, prsgrd32.h:296-345; off = ni: ETA, :360-409): the density
// Jacobian between the cell ck (r0, z0) and its neighbour at ck - off, with the harmonic-mean limited slopes.
// mask: umask / vmask, read at the faces a2 - off, a2, a2 + off (MASKING, :300-306, :364-370).
__device__ __forceinline__ double prsgrd32_jac(gcd_t rho, gcd_t z_r, long ck, long off, double r0, double z0,
                                               bool masking, gcd_t mask, long a2, double HalfGRho)
{
  const double eps = 1.0E-10, OneFifth = 0.2, OneTwelfth = 1.0 / 12.0;
  const double rm2 = rho[ck - 2 * off], rm1 = rho[ck - off], rp1 = rho[ck + off];
  const double zm2 = z_r[ck - 2 * off], zm1 = z_r[ck - off], zp1 = z_r[ck + off];
  double aux_m1 = zm1 - zm2, aux_0 = z0 - zm1, aux_p1 = zp1 - z0;
  double FC_m1 = rm1 - rm2, FC_0 = r0 - rm1, FC_p1 = rp1 - r0;
  if (masking) {
    const double m_m1 = mask[a2 - off], m_0 = mask[a2], m_p1 = mask[a2 + off];
    aux_m1 = aux_m1 * m_m1; aux_0 = aux_0 * m_0; aux_p1 = aux_p1 * m_p1;
    FC_m1 = FC_m1 * m_m1; FC_0 = FC_0 * m_0; FC_p1 = FC_p1 * m_p1;
  }
  const double dZx0 = harm_inv(aux_0, aux_p1, eps), dZxm = harm_inv(aux_m1, aux_0, eps);
  const double dRx0 = harm_inv(FC_0, FC_p1, eps), dRxm = harm_inv(FC_m1, FC_0, eps);
  return HalfGRho * ((r0 + rm1) * (z0 - zm1) -
                     OneFifth * ((dRx0 - dRxm) * (z0 - zm1 - OneTwelfth * (dZx0 + dZxm)) -
                                 (dZx0 - dZxm) * (r0 - rm1 - OneTwelfth * (dRx0 + dRxm))));
}

// prsgrd32 in one launch.  One thread per water column of a 64 x 4 tile marches k from N down to 1: it advances the P
// recursion of its own column, publishes P(k) to an LDS plane of the (64+1) x (4+1) points the tile's u- and v-points
// read (own, i-1, j-1), and after one barrier evaluates ru(k), rv(k) of its point.  The 69 ring columns (i = first-1,
// j = first-1; where they exist, down to IstrU-1 / JstrV-1) are advanced by the first 69 threads as a second column
// each.  Two planes, so one barrier per level.  Everything of a level that does not need P -- the density Jacobians,
// the loads of the predictor -- is done ahead of the barrier.
// UVSTART (inside roms_hip_rhs3d, k_rhs3d.hip: rhs3d_fuses_uvstart()): the thread also forms the predictor's start of
// u, v(nnew) at its two points (k_pre_uv, pre_step3d.F:1012-1120) -- it reads the old ru, rv(nrhs) as the AB3 term
// before it stores the new one over it.  lambda = 1 there: the explicit viscous flux is zero, so level k needs level k
// alone (and bustr at k = 1, sustr at k = N) and the downward march gives the bits of the upward one.
template <bool UVSTART>
__global__ void __launch_bounds__(BLK_X *BLK_Y) __attribute__((amdgpu_waves_per_eu(4)))
k_prsgrd32(const RomsDev *__restrict__ c, int nrhs, int nstp, int nnew, int stage)
{
  DEV_PROLOGUE(c)
  const Blk XB = xcd_block();
  constexpr int PW = BLK_X + 1, PLANE = PW * (BLK_Y + 1);
  __shared__ double sP[2 * PLANE];
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * BLK_X + tx;
  const int i0 = b.Istr + XB.x * BLK_X, j0 = b.Jstr + XB.y * BLK_Y;
  const int i = i0 + tx, j = j0 + ty;
  const bool own = i <= b.Iend && j <= b.Jend;
  const bool do_u = own && i >= b.IstrU, do_v = own && j >= b.JstrV;
  // the ring column of this thread: row j0-1 (tid 0..64), then column i0-1 (tid 65..68)
  const int rli = tid < PW ? tid : 0, rlj = tid < PW ? 0 : tid - BLK_X;
  const int ri = i0 - 1 + rli, rj = j0 - 1 + rlj;
  const bool ring = tid < PW + BLK_Y && ri >= b.IstrU - 1 && ri <= b.Iend && rj >= b.JstrV - 1 && rj <= b.Jend;
  const int lo = (ty + 1) * PW + tx + 1, lr = rlj * PW + rli;       // plane slots of the two columns
  const gcd_t rho = (gcd_t)(c->F.rho);
  const gcd_t z_r = (gcd_t)(c->F.z_r);
  const gcd_t Hz = (gcd_t)(c->F.Hz);
  const double HalfGRho = 0.5 * (c->p.g / c->p.rho0);
  const bool masking = c->p.masking != 0, wet = c->p.wet_dry != 0;
  const long a2 = I2(own ? i : b.Iend, own ? j : b.Jend);           // clamped for address formation only
  const long ar = I2(ring ? ri : b.Iend, ring ? rj : b.Jend);
  const gd_t ru = (gd_t)(c->F.ru + (long)(nrhs - 1) * n3w), rv = (gd_t)(c->F.rv + (long)(nrhs - 1) * n3w);
  // per-thread constants of the two faces
  double onu = 0.0, omv = 0.0, uwet = 1.0, vwet = 1.0;
  if (do_u) {
    onu = GF(on_u)[a2];
    if (wet) uwet = GF(umask_wet)[a2];
  }
  if (do_v) {
    omv = GF(om_v)[a2];
    if (wet) vwet = GF(vmask_wet)[a2];
  }
  // the predictor's start (k_pre_uv): time levels and the per-point constants
  const double dt = c->p.dt;
  const gcd_t us = (gcd_t)(c->F.u + (long)(nstp - 1) * n3r), vs = (gcd_t)(c->F.v + (long)(nstp - 1) * n3r);
  const gd_t un = (gd_t)(c->F.u + (long)(nnew - 1) * n3r), vn = (gd_t)(c->F.v + (long)(nnew - 1) * n3r);
  const gcd_t ru2 = (gcd_t)(c->F.ru + (long)(3 - nrhs - 1) * n3w), rv2 = (gcd_t)(c->F.rv + (long)(3 - nrhs - 1) * n3w);
  double DCu = 0.0, DCv = 0.0;
  if constexpr (UVSTART) {
    const gcd_t pm = (gcd_t)(c->F.pm), pn = (gcd_t)(c->F.pn);
    const double cq = dt * 0.25;
    if (do_u) DCu = cq * (pm[a2] + pm[a2 - 1]) * (pn[a2] + pn[a2 - 1]);
    if (do_v) DCv = cq * (pm[a2] + pm[a2 - ni]) * (pn[a2] + pn[a2 - ni]);
  }

  PCol qo{}, qr{};
  double P0 = 0.0, Pr = 0.0;
  if (own) P0 = prsgrd32_P_top(c, rho, z_r, a2, N, nij, qo);
  if (ring) Pr = prsgrd32_P_top(c, rho, z_r, ar, N, nij, qr);
  for (int k = N; k >= 1; k--) {
    if (k < N) {
      if (own) P0 = prsgrd32_P_down(rho, z_r, a2, k, nij, HalfGRho, qo);
      if (ring) Pr = prsgrd32_P_down(rho, z_r, ar, k, nij, HalfGRho, qr);
    }
    double *pl = sP + (k & 1) * PLANE;
    if (own) pl[lo] = P0;
    if (ring) pl[lr] = Pr;
    // ---- ahead of the barrier: what does not need the neighbours' P ----
    const long ck = a2 + (long)(k - 1) * nij;
    const double r0 = qo.r_up, z0 = qo.z_up;                        // rho, z_r(i,j,k)
    double hz0 = 0.0, hsu = 0.0, hsv = 0.0, Ju = 0.0, Jv = 0.0, unew = 0.0, vnew = 0.0;
    if (own) hz0 = Hz[ck];
    if (do_u) {
      hsu = hz0 + Hz[ck - 1];
      Ju = prsgrd32_jac(rho, z_r, ck, 1, r0, z0, masking, (gcd_t)c->F.umask, a2, HalfGRho);
    }
    if (do_v) {
      hsv = hz0 + Hz[ck - ni];
      Jv = prsgrd32_jac(rho, z_r, ck, ni, r0, z0, masking, (gcd_t)c->F.vmask, a2, HalfGRho);
    }
    if constexpr (UVSTART) {
      // FC(k) - FC(k-1) of the vertical viscous flux with lambda = 1: the stresses at the two ends, zero between
      if (do_u) {
        const double FCk = (k == N) ? dt * GF(sustr)[a2] : 0.0, FCprev = (k == 1) ? dt * GF(bustr)[a2] : 0.0;
        unew = uv_start(stage, us[ck], hsu, DCu, (gcd_t)ru, ru2, ck + nij, FCk - FCprev);
      }
      if (do_v) {
        const double FCk = (k == N) ? dt * GF(svstr)[a2] : 0.0, FCprev = (k == 1) ? dt * GF(bvstr)[a2] : 0.0;
        vnew = uv_start(stage, vs[ck], hsv, DCv, (gcd_t)rv, rv2, ck + nij, FCk - FCprev);
      }
    }
    __syncthreads();
    if (do_u) {
      double r = onu * 0.5 * hsu * (pl[lo - 1] - P0 - Ju);
      if (wet) r = r * uwet;                                        // WET_DRY, prsgrd32.h:346-348
      if constexpr (UVSTART) un[ck] = unew;
      ru[ck + nij] = r;
    }
    if (do_v) {
      double r = omv * 0.5 * hsv * (pl[lo - PW] - P0 - Jv);
      if (wet) r = r * vwet;                                        // WET_DRY, prsgrd32.h:410-412
      if constexpr (UVSTART) vn[ck] = vnew;
      rv[ck + nij] = r;
    }
  }
}

// prsgrd31_tile (ROMS/Nonlinear/prsgrd31.h:97-364): the standard density Jacobian -- the reference's default when no
// pressure-gradient option is defined (prsgrd.F:24-25) -- and, WJ = true, the weighted Jacobian of Song 1998
// (WJ_GRADP).  One thread per column marches down from the surface with the two running sums phix, phie in
// registers and the (k+1) values of rho, z_r of its three columns kept from the previous level: every field is
// read once per point it is needed at, nothing goes through scratch (5 field passes: rho, z_r, Hz in; ru, rv out).
// RHO_SURF is always on (globaldefs.h:130); the routine has no MASKING blocks.
template <bool WJ>
__global__ void __launch_bounds__(BLK_X *BLK_Y) k_prsgrd31(const RomsDev *__restrict__ c, int nrhs)
{
  DEV_PROLOGUE(c)
  const Blk XB = xcd_block();
  const int i = b.Istr + XB.x * BLK_X + threadIdx.x, j = b.Jstr + XB.y * BLK_Y + threadIdx.y;
  if (i > b.Iend || j > b.Jend) return;
  const bool do_u = i >= b.IstrU, do_v = j >= b.JstrV;
  const gcd_t rho = (gcd_t)(c->F.rho), z_r = (gcd_t)(c->F.z_r), Hz = (gcd_t)(c->F.Hz);
  const gd_t ru = (gd_t)(c->F.ru + (long)(nrhs - 1) * n3w), rv = (gd_t)(c->F.rv + (long)(nrhs - 1) * n3w);
  const double g = c->p.g, rho0 = c->p.rho0;
  const double fac1 = 0.5 * g / rho0, fac2 = 1000.0 * g / rho0, fac3 = 0.25 * g / rho0;
  const long a = I2(i, j), aw = do_u ? a - 1 : a, as = do_v ? a - ni : a;   // neighbours only where they are used
  const double onu = GF(on_u)[a], omv = GF(om_v)[a];
  // WET_DRY: each stored term times the wet/dry mask of its face (prsgrd31.h:223, :269, :304, :350)
  const bool wet = c->p.wet_dry != 0;
  const double uw = wet ? (double)GF(umask_wet)[a] : 1.0, vw = wet ? (double)GF(vmask_wet)[a] : 1.0;
  // surface level, :196-226 and :276-306
  long q = a + (long)(N - 1) * nij, qw = aw + (long)(N - 1) * nij, qs = as + (long)(N - 1) * nij;
  double r1 = rho[q], z1 = z_r[q], r1w = rho[qw], z1w = z_r[qw], r1s = rho[qs], z1s = z_r[qs];
  const gcd_t zw = (gcd_t)(c->F.z_w);
  const double zw0 = zw[a + (long)N * nij], zww = zw[aw + (long)N * nij], zws = zw[as + (long)N * nij];
  double phix, phie;
  {
    const double cff1 = zw0 - z1 + zww - z1w;
    phix = fac1 * (r1 - r1w) * cff1;
    const bool atm = c->p.atm_press != 0;                       // ATM_PRESS, prsgrd31.h:213-215, :294-296
    const double fpa = 100.0 / rho0, pa0 = atm ? (double)GF(Pair)[a] : 0.0;
    if (atm) phix = phix + fpa * (pa0 - GF(Pair)[aw]);
    phix = phix + (fac2 + fac1 * (r1 + r1w)) * (zw0 - zww);
    const double cff1e = zw0 - z1 + zws - z1s;
    phie = fac1 * (r1 - r1s) * cff1e;
    if (atm) phie = phie + fpa * (pa0 - GF(Pair)[as]);
    phie = phie + (fac2 + fac1 * (r1 + r1s)) * (zw0 - zws);
    const double hz = Hz[q];
    if (do_u) { const double r = -0.5 * (hz + Hz[qw]) * phix * onu; ru[I3W(i, j, N)] = wet ? r * uw : r; }
    if (do_v) { const double r = -0.5 * (hz + Hz[qs]) * phie * omv; rv[I3W(i, j, N)] = wet ? r * vw : r; }
  }
  // interior: differentiate, then integrate downwards, :232-268 and :312-352
  auto jac = [&](double rk1, double rk1m, double rk, double rkm, double zk1, double zk1m, double zk, double zkm) {
    double cff1, cff2, cff3, cff4;
    if (WJ) {
      cff1 = 1.0 / ((zk1 - zk) * (zk1m - zkm));
      cff2 = zk - zkm + zk1 - zk1m;
      cff3 = zk1 - zk - zk1m + zkm;
      const double gamma = 0.125 * cff1 * cff2 * cff3;
      cff1 = (1.0 + gamma) * (rk1 - rk1m) + (1.0 - gamma) * (rk - rkm);
      cff2 = rk1 + rk1m - rk - rkm;
      cff3 = zk1 + zk1m - zk - zkm;
      cff4 = (1.0 + gamma) * (zk1 - zk1m) + (1.0 - gamma) * (zk - zkm);
    } else {
      cff1 = rk1 - rk1m + rk - rkm;
      cff2 = rk1 + rk1m - rk - rkm;
      cff3 = zk1 + zk1m - zk - zkm;
      cff4 = zk1 - zk1m + zk - zkm;
    }
    return fac3 * (cff1 * cff3 - cff2 * cff4);
  };
#pragma unroll 2
  for (int k = N - 1; k >= 1; k--) {
    q -= nij; qw -= nij; qs -= nij;
    const double r0 = rho[q], z0 = z_r[q], r0w = rho[qw], z0w = z_r[qw], r0s = rho[qs], z0s = z_r[qs];
    const double hz = Hz[q], hzw = Hz[qw], hzs = Hz[qs];
    phix = phix + jac(r1, r1w, r0, r0w, z1, z1w, z0, z0w);
    phie = phie + jac(r1, r1s, r0, r0s, z1, z1s, z0, z0s);
    if (do_u) { const double r = -0.5 * (hz + hzw) * phix * onu; ru[I3W(i, j, k)] = wet ? r * uw : r; }
    if (do_v) { const double r = -0.5 * (hz + hzs) * phie * omv; rv[I3W(i, j, k)] = wet ? r * vw : r; }
    r1 = r0; z1 = z0; r1w = r0w; z1w = z0w; r1s = r0s; z1s = z0s;
  }
}

// prsgrd40_tile (prsgrd40.h:170-268, PJ_GRADP): the hydrostatic pressure integral P of the own column and of the
// western / southern neighbour march downwards together in registers -- one launch, no scratch
__global__ void __launch_bounds__(BLK_X *BLK_Y) k_prsgrd40(const RomsDev *__restrict__ c, int nrhs)
{
  DEV_PROLOGUE(c)
  const Blk XB = xcd_block();
  const int i = b.Istr + XB.x * BLK_X + threadIdx.x, j = b.Jstr + XB.y * BLK_Y + threadIdx.y;
  if (i > b.Iend || j > b.Jend) return;
  const bool do_u = i >= b.IstrU, do_v = j >= b.JstrV;
  const gcd_t rho = (gcd_t)(c->F.rho), zw = (gcd_t)(c->F.z_w), Hz = (gcd_t)(c->F.Hz);
  const gd_t ru = (gd_t)(c->F.ru + (long)(nrhs - 1) * n3w), rv = (gd_t)(c->F.rv + (long)(nrhs - 1) * n3w);
  const double cff = 0.5 * c->p.g, cff1 = c->p.g / c->p.rho0;
  const long a = I2(i, j), aw = do_u ? a - 1 : a, as = do_v ? a - ni : a;
  const double onu = GF(on_u)[a], omv = GF(om_v)[a];
  const double dzx = zw[aw + (long)N * nij] - zw[a + (long)N * nij];      // z_w(i-1,j,N) - z_w(i,j,N)
  const double dze = zw[as + (long)N * nij] - zw[a + (long)N * nij];
  double P0 = 0.0, Pw = 0.0, Ps = 0.0;        // P(.,.,k) of the three columns
  if (c->p.atm_press) {                       // ATM_PRESS, prsgrd40.h:187-196: P(N) = (100 / g) (Pair - 1 atm)
    const double fpa = 100.0 / c->p.g;
    P0 = P0 + fpa * (GF(Pair)[a] - 1013.25); Pw = Pw + fpa * (GF(Pair)[aw] - 1013.25); Ps = Ps + fpa * (GF(Pair)[as] - 1013.25);
  }
  double FCx = 0.0, FCe = 0.0;                // FC(i,k) of the two components
  for (int k = N; k >= 1; k--) {
    const long q = a + (long)(k - 1) * nij, qw = aw + (long)(k - 1) * nij, qs = as + (long)(k - 1) * nij;
    const double h0 = Hz[q], hw = Hz[qw], hs = Hz[qs];
    const double P0m = P0 + h0 * rho[q], Pwm = Pw + hw * rho[qw], Psm = Ps + hs * rho[qs];    // P(k-1)
    const double FX0 = 0.5 * h0 * (P0 + P0m);
    if (do_u) {
      const double FXw = 0.5 * hw * (Pw + Pwm);
      const double dh = zw[q] - zw[qw];                                   // z_w(i,j,k-1) - z_w(i-1,j,k-1)
      const double FCm = 0.5 * dh * (P0m + Pwm);
      ru[I3W(i, j, k)] = (cff * (hw + h0) * dzx + cff1 * (FXw - FX0 + FCx - FCm)) * onu;
      FCx = FCm;
    }
    if (do_v) {
      const double FXs = 0.5 * hs * (Ps + Psm);
      const double dh = zw[q] - zw[qs];
      const double FCm = 0.5 * dh * (P0m + Psm);
      rv[I3W(i, j, k)] = (cff * (hs + h0) * dze + cff1 * (FXs - FX0 + FCe - FCm)) * omv;
      FCe = FCm;
    }
    P0 = P0m; Pw = Pwm; Ps = Psm;
  }
}

}  // namespace

// uvstart (roms_hip_rhs3d alone, roms_dev.h): prsgrd32 also forms the predictor's start of u, v(nnew)
int prsgrd_entry(const roms_step_idx_t *s, bool uvstart)
{
  int rc = roms_entry_check("roms_hip_prsgrd");
  if (rc) return rc;
  if ((rc = check_lbc())) return rc;
  ScopedTimer tm("prsgrd");
  const roms_bounds_t &b = g_ctx.b;
  if (g_ctx.p.pgf == PGF_PJ_GRADP) {
    // the reference does not compile PJ_GRADP with WET_DRY (prsgrd40.h:98-100 passes umask_wet, vmask_wet to a
    // routine that does not declare them): refused
    if (g_ctx.p.wet_dry) return roms_fail("roms_hip_prsgrd", "PJ_GRADP with WET_DRY does not exist in the reference");
    hipLaunchKernelGGL(k_prsgrd40, grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1), block2d(), 0, g_ctx.stream,
                       g_ctx.devc, s->nrhs);
    KERNEL_CHECK("k_prsgrd40");
    return 0;
  }
  if (g_ctx.p.pgf != PGF_DJ_GRADPS) {                   // prsgrd31.h: one launch, no scratch
    if (g_ctx.p.pgf != PGF_STANDARD && g_ctx.p.pgf != PGF_WJ_GRADP)
      return roms_fail("roms_hip_prsgrd", "unknown pressure-gradient algorithm (enum roms_pgf)");
    const dim3 grid = grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1);
    if (g_ctx.p.pgf == PGF_WJ_GRADP)
      hipLaunchKernelGGL(k_prsgrd31<true>, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, s->nrhs);
    else
      hipLaunchKernelGGL(k_prsgrd31<false>, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, s->nrhs);
    KERNEL_CHECK("k_prsgrd31");
    return 0;
  }
  if (b.N < 2) return roms_fail("roms_hip_prsgrd", "N < 2");
  const int stage = (s->iic == s->ntfirst) ? 0 : (s->iic == s->ntfirst + 1 ? 1 : 2);     // as pre_step3d_uv()
  hipLaunchKernelGGL(uvstart ? k_prsgrd32<true> : k_prsgrd32<false>, grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1),
                     block2d(), 0, g_ctx.stream, g_ctx.devc, s->nrhs, s->nstp, s->nnew, stage);
  KERNEL_CHECK("k_prsgrd32");
  return 0;
}

extern "C" int roms_hip_prsgrd(const roms_step_idx_t *s) { return prsgrd_entry(s, false); }
