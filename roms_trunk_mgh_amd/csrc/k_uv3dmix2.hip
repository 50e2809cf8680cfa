// k_uv3dmix2.hip -- harmonic horizontal viscosity along s-surfaces,
// uv3dmix2_s_tile (ROMS/Nonlinear/uv3dmix2_s.h:114-335); also accumulates
// rufrc, rvfrc.  Rotated to geopotentials (MIX_GEO_UV): k_uv3dmix2_geo below.  And the biharmonic one, uv3dmix4_s_tile (uv3dmix4_s.h:120-629): the first operator without the
// layer thickness (k_uv4_first -> LapU, LapV on a range one point wider), its rule outside physical edges and at the
// corners (k_uv4_edges, k_uv4_corners), then the harmonic kernel itself on LapU, LapV with visc4 and the sign reversed.
//
// One thread per (i,j) column sweeping k upward.  Each thread needs the stress
// at three rho-points (own, west, south) and three psi-points (own, north,
// east).  Their metric coefficients -- pmon/pnom and the four (pm+pm), (pn+pn)
// pairs per point -- do not depend on k, so they are formed once per column
// (RhoC / PsiC of visc.h, which states the stress and its divergence for every
// kernel here: 36 doubles in VGPRs) instead of ~50 L2 requests per level.  Per level the
// kernel then reads u, v (7 points each), Hz (8 points) and read-modify-writes
// u,v(nnew): the 7 algorithmic field passes plus cache-served neighbours.
#include "visc.h"
#include "uvgeo.h"

namespace {

// BIH = false: uv3dmix2_s.  BIH = true: the second operator of uv3dmix4_s (uv3dmix4_s.h:522-620) -- the same
// expressions on LapU, LapV (module extents, N levels) with visc4, subtracted.
template <bool BIH>
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_uv3dmix2_v2(const RomsDev *__restrict__ c, int nrhs, int nnew, const double *__restrict__ lapU,
              const double *__restrict__ lapV)
{
  DEV_PROLOGUE(c)
  const Blk XB = xcd_block();
  const int i = b.Istr + XB.x * BLK_X + threadIdx.x;
  const int j = b.Jstr + XB.y * BLK_Y + threadIdx.y;
  if (i > b.Iend || j > b.Jend) return;
  const bool do_u = i >= b.IstrU, do_v = j >= b.JstrV;
  const bool msk = c->p.masking != 0;
  const double dt = c->p.dt;
  // (u, v, Hz through the global address space: generic pointers made these flat loads, which tie up the LDS / scalar
  // counter as well and cannot be issued past it)
  const gcd_t u = (gcd_t)(BIH ? lapU : c->F.u + (long)(nrhs - 1) * n3r);
  const gcd_t v = (gcd_t)(BIH ? lapV : c->F.v + (long)(nrhs - 1) * n3r);
  const double *__restrict__ visc_r = BIH ? c->F.visc4_r : c->F.visc2_r;
  const double *__restrict__ visc_p = BIH ? c->F.visc4_p : c->F.visc2_p;
  const gcd_t Hz = (gcd_t)c->F.Hz;
  const gd_t un = (gd_t)(c->F.u + (long)(nnew - 1) * n3r);
  const gd_t vn = (gd_t)(c->F.v + (long)(nnew - 1) * n3r);
  const long a = I2(i, j);
  const double *pm = c->F.pm, *pn = c->F.pn;
  const double pm2u = pm[a - 1] + pm[a], pn2u = pn[a - 1] + pn[a], pm2v = pm[a - ni] + pm[a], pn2v = pn[a - ni] + pn[a];
  const double cu = dt * 0.25 * pm2u * pn2u, cv = dt * 0.25 * pm2v * pn2v;
  // the west / south stress points exist only where u / v is stepped: next to a closed wall
  // their stencil would reach below LBi / LBj (LBj = 0 on a closed southern edge)
  const RhoC r0 = rho_coef(c, a, ni, visc_r);
  const RhoC rw = do_u ? rho_coef(c, a - 1, ni, visc_r) : r0;
  const RhoC rs = do_v ? rho_coef(c, a - ni, ni, visc_r) : r0;
  const PsiC p0 = psi_coef(c, a, ni, visc_p), pN = psi_coef(c, a + ni, ni, visc_p), pE = psi_coef(c, a + 1, ni, visc_p);
  auto sr = [&](const RhoC &m, long q) { return Hz[q] * 0.5 * strain_r(m, u, v, q, ni); };      // uv3dmix2_s.h:205
  auto sp = [&](const PsiC &m, long q) {                                                        // :236
    return masked_p(0.125 * (Hz[q - 1] + Hz[q] + Hz[q - 1 - ni] + Hz[q - ni]) * strain_p(m, u, v, q, ni), m, msk);
  };
  double ruf = do_u ? c->F.rufrc[a] : 0.0, rvf = do_v ? c->F.rvfrc[a] : 0.0;
  // levels are independent apart from the two running sums: two at a time, so that the loads of the second
  // are in flight while the first is computed
#pragma unroll 2
  for (int k = 1; k <= N; k++) {
    const long ak = a + (long)(k - 1) * nij;
    const double sr0 = sr(r0, ak), sp0 = sp(p0, ak);
    if (do_u) {
      const Div2 d = div_flux(pn2u, pm2u, kx(r0) * sr0, kx(rw) * sr(rw, ak - 1), ke(pN) * sp(pN, ak + ni), ke(p0) * sp0);
      const double cff3 = cu * (d.cff1 + d.cff2);
      if constexpr (BIH) { ruf = ruf - d.cff1 - d.cff2; un[ak] = un[ak] - cff3; }
      else { ruf = ruf + d.cff1 + d.cff2; un[ak] = un[ak] + cff3; }
    }
    if (do_v) {
      const Div2 d = div_flux(pn2v, pm2v, kx(pE) * sp(pE, ak + 1), kx(p0) * sp0, ke(r0) * sr0, ke(rs) * sr(rs, ak - ni));
      const double cff3 = cv * (d.cff1 - d.cff2);
      if constexpr (BIH) { rvf = rvf - d.cff1 + d.cff2; vn[ak] = vn[ak] - cff3; }
      else { rvf = rvf + d.cff1 - d.cff2; vn[ak] = vn[ak] + cff3; }
    }
  }
  if (do_u) c->F.rufrc[a] = ruf;
  if (do_v) c->F.rvfrc[a] = rvf;
}

// ---- uv3dmix4_s: first operator (m s^-3/2), uv3dmix4_s.h:283-355 -> LapU, LapV on a range one point wider ----
struct Uv4 {
  double *lapU, *lapV;
  int iUa, iUb, jUa, jUb;        // IminU:ImaxU, JminU:JmaxU
  int iVa, iVb, jVa, jVb;        // IminV:ImaxV, JminV:JmaxV
  int cu[4], cv[4];              // the u / v condition on [LBS_WEST..LBS_NORTH] is "closed"
  double gamma2;
};
// the thread's point in a launch over the union of the two ranges, and which of LapU, LapV it owes there
struct Uv4Pt { int i, j; bool do_u, do_v; };
__device__ __forceinline__ Uv4Pt uv4_point(const Uv4 &A)
{
  Uv4Pt w;
  w.i = (A.iUa < A.iVa ? A.iUa : A.iVa) + blockIdx.x * BLK_X + threadIdx.x;
  w.j = (A.jUa < A.jVa ? A.jUa : A.jVa) + blockIdx.y * BLK_Y + threadIdx.y;
  w.do_u = w.i >= A.iUa && w.i <= A.iUb && w.j >= A.jUa && w.j <= A.jUb;
  w.do_v = w.i >= A.iVa && w.i <= A.iVb && w.j >= A.jVa && w.j <= A.jVb;
  return w;
}

__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_uv4_first(const RomsDev *__restrict__ c, int nrhs, Uv4 A)
{
  DEV_PROLOGUE(c)
  const Uv4Pt w = uv4_point(A);
  const bool do_u = w.do_u, do_v = w.do_v;
  if (!do_u && !do_v) return;
  const bool msk = c->p.masking != 0;
  const double *__restrict__ u = c->F.u + (long)(nrhs - 1) * n3r;
  const double *__restrict__ v = c->F.v + (long)(nrhs - 1) * n3r;
  const long a = I2(w.i, w.j);
  const double *pm = c->F.pm, *pn = c->F.pn;
  const RhoC r0 = rho_coef(c, a, ni, c->F.visc4_r);
  const RhoC rw = do_u ? rho_coef(c, a - 1, ni, c->F.visc4_r) : r0;
  const RhoC rs = do_v ? rho_coef(c, a - ni, ni, c->F.visc4_r) : r0;
  const PsiC p0 = psi_coef(c, a, ni, c->F.visc4_p);
  const PsiC pN = do_u ? psi_coef(c, a + ni, ni, c->F.visc4_p) : p0;
  const PsiC pE = do_v ? psi_coef(c, a + 1, ni, c->F.visc4_p) : p0;
  auto sr = [&](const RhoC &m, long q) { return 0.5 * strain_r(m, u, v, q, ni); };
  auto sp = [&](const PsiC &m, long q) { return masked_p(0.5 * strain_p(m, u, v, q, ni), m, msk); };
  const double mu = pm[a - 1] + pm[a], nu = pn[a - 1] + pn[a];          // :340-347
  const double mv = pm[a] + pm[a - ni], nv = pn[a] + pn[a - ni];
  for (int k = 1; k <= N; k++) {
    const long ak = a + (long)(k - 1) * nij;
    const double sr0 = sr(r0, ak), sp0 = sp(p0, ak);
    if (do_u)
      A.lapU[ak] = div_lap<false>(mu, nu, kx(r0) * sr0, kx(rw) * sr(rw, ak - 1), ke(pN) * sp(pN, ak + ni), ke(p0) * sp0);
    if (do_v)
      A.lapV[ak] = div_lap<true>(mv, nv, kx(pE) * sp(pE, ak + 1), kx(p0) * sp0, ke(r0) * sr0, ke(rs) * sr(rs, ak - ni));
  }
}

// the rule for LapU, LapV outside a physical edge, uv3dmix4_s.h:357-470: the normal component zero (closed) or a copy
// of the next one inside, the tangential one gamma2 times the first inside value (closed: the slipperiness) or zero.
// grid: x = positions along the edge, y = level, z = edge
__global__ void k_uv4_edges(const RomsDev *__restrict__ c, Uv4 A)      // gridDim.y = number of levels
{
  DEV_PROLOGUE(c)
  const int e = blockIdx.z, k = blockIdx.y + 1, q = blockIdx.x * blockDim.x + threadIdx.x;
  const long lev = (long)(k - 1) * nij;
  double *LU = A.lapU + lev, *LV = A.lapV + lev;
  if (e == LBS_WEST && b.west_edge && !b.EWperiodic) {
    const int ju = A.jUa + q, jv = A.jVa + q;
    if (ju <= A.jUb) LU[I2(b.Istr, ju)] = A.cu[e] ? 0.0 : LU[I2(b.Istr + 1, ju)];
    if (jv <= A.jVb) LV[I2(b.Istr - 1, jv)] = A.cv[e] ? A.gamma2 * LV[I2(b.Istr, jv)] : 0.0;
  } else if (e == LBS_EAST && b.east_edge && !b.EWperiodic) {
    const int ju = A.jUa + q, jv = A.jVa + q;
    if (ju <= A.jUb) LU[I2(b.Iend + 1, ju)] = A.cu[e] ? 0.0 : LU[I2(b.Iend, ju)];
    if (jv <= A.jVb) LV[I2(b.Iend + 1, jv)] = A.cv[e] ? A.gamma2 * LV[I2(b.Iend, jv)] : 0.0;
  } else if (e == LBS_SOUTH && b.south_edge && !b.NSperiodic) {
    const int iu = A.iUa + q, iv = A.iVa + q;
    if (iu <= A.iUb) LU[I2(iu, b.Jstr - 1)] = A.cu[e] ? A.gamma2 * LU[I2(iu, b.Jstr)] : 0.0;
    if (iv <= A.iVb) LV[I2(iv, b.Jstr)] = A.cv[e] ? 0.0 : LV[I2(iv, b.Jstr + 1)];
  } else if (e == LBS_NORTH && b.north_edge && !b.NSperiodic) {
    const int iu = A.iUa + q, iv = A.iVa + q;
    if (iu <= A.iUb) LU[I2(iu, b.Jend + 1)] = A.cu[e] ? A.gamma2 * LU[I2(iu, b.Jend)] : 0.0;
    if (iv <= A.iVb) LV[I2(iv, b.Jend + 1)] = A.cv[e] ? 0.0 : LV[I2(iv, b.Jend)];
  }
}

// corners, uv3dmix4_s.h:472-520 (after the edges); one thread per level
__global__ void k_uv4_corners(const RomsDev *__restrict__ c, Uv4 A, int nk)
{
  DEV_PROLOGUE(c)
  const int k = blockIdx.x * blockDim.x + threadIdx.x + 1;
  if (k > nk || b.EWperiodic || b.NSperiodic) return;
  const long lev = (long)(k - 1) * nij;
  double *LU = A.lapU + lev, *LV = A.lapV + lev;
  const int Is = b.Istr, Ie = b.Iend, Js = b.Jstr, Je = b.Jend;
  if (b.south_edge && b.west_edge) {
    LU[I2(Is, Js - 1)] = 0.5 * (LU[I2(Is + 1, Js - 1)] + LU[I2(Is, Js)]);
    LV[I2(Is - 1, Js)] = 0.5 * (LV[I2(Is - 1, Js + 1)] + LV[I2(Is, Js)]);
  }
  if (b.south_edge && b.east_edge) {
    LU[I2(Ie + 1, Js - 1)] = 0.5 * (LU[I2(Ie, Js - 1)] + LU[I2(Ie + 1, Js)]);
    LV[I2(Ie + 1, Js)] = 0.5 * (LV[I2(Ie, Js)] + LV[I2(Ie + 1, Js + 1)]);
  }
  if (b.north_edge && b.west_edge) {
    LU[I2(Is, Je + 1)] = 0.5 * (LU[I2(Is + 1, Je + 1)] + LU[I2(Is, Je)]);
    LV[I2(Is - 1, Je + 1)] = 0.5 * (LV[I2(Is, Je + 1)] + LV[I2(Is - 1, Je)]);
  }
  if (b.north_edge && b.east_edge) {
    LU[I2(Ie + 1, Je + 1)] = 0.5 * (LU[I2(Ie, Je + 1)] + LU[I2(Ie + 1, Je)]);
    LV[I2(Ie + 1, Je + 1)] = 0.5 * (LV[I2(Ie, Je + 1)] + LV[I2(Ie + 1, Je)]);
  }
}

// ---- the 2-D biharmonic viscosity of step2d, step2d_LF_AM3.h:1474-1740, as a pass of its own in front of the momentum
// kernel: the first operator on ubar, vbar(krhs) (no depth), the same edge / corner rule (with the conditions of ubar,
// vbar), the second operator with the total depth -> fac_u, fac_v, which k2d_mom_lds subtracts from rhs_ubar, rhs_vbar
// where the reference does.  The association of the products differs from the 3-D operator (visc4 multiplies first).
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k2d_visc4_first(const RomsDev *__restrict__ c, int krhs, Uv4 A)
{
  DEV_PROLOGUE(c)
  const Uv4Pt w = uv4_point(A);
  if (!w.do_u && !w.do_v) return;
  const bool msk = c->p.masking != 0;
  const double *__restrict__ u = c->F.ubar + (long)(krhs - 1) * nij;
  const double *__restrict__ v = c->F.vbar + (long)(krhs - 1) * nij;
  const double *pm = c->F.pm, *pn = c->F.pn;
  const long a = I2(w.i, w.j);
  auto sr = [&](const RhoC &m, long q) { return m.visc * 0.5 * strain_r(m, u, v, q, ni); };                 // :1474-1486
  auto sp = [&](const PsiC &m, long q) { return masked_p(m.visc * 0.5 * strain_p(m, u, v, q, ni), m, msk); };  // :1487-1505
  const RhoC r0 = rho_coef(c, a, ni, c->F.visc4_r);
  const PsiC p0 = psi_coef(c, a, ni, c->F.visc4_p);
  const double sr0 = sr(r0, a), sp0 = sp(p0, a);
  if (w.do_u) {
    const RhoC rw = rho_coef(c, a - 1, ni, c->F.visc4_r);
    const PsiC pN = psi_coef(c, a + ni, ni, c->F.visc4_p);
    A.lapU[a] = div_lap<false>(pm[a - 1] + pm[a], pn[a - 1] + pn[a], r0.on2 * sr0, rw.on2 * sr(rw, a - 1),
                               pN.om2 * sp(pN, a + ni), p0.om2 * sp0);
  }
  if (w.do_v) {
    const RhoC rs = rho_coef(c, a - ni, ni, c->F.visc4_r);
    const PsiC pE = psi_coef(c, a + 1, ni, c->F.visc4_p);
    A.lapV[a] = div_lap<true>(pm[a] + pm[a - ni], pn[a] + pn[a - ni], pE.on2 * sp(pE, a + 1), p0.on2 * sp0, r0.om2 * sr0,
                              rs.om2 * sr(rs, a - ni));
  }
}

__global__ void __launch_bounds__(BLK_X *BLK_Y)
k2d_visc4_second(const RomsDev *__restrict__ c, int krhs, Uv4 A, double *__restrict__ facu, double *__restrict__ facv)
{
  DEV_PROLOGUE(c)
  const int i = b.Istr + blockIdx.x * BLK_X + threadIdx.x;
  const int j = b.Jstr + blockIdx.y * BLK_Y + threadIdx.y;
  if (i > b.Iend || j > b.Jend) return;
  const bool do_u = i >= b.IstrU, do_v = j >= b.JstrV;
  const bool msk = c->p.masking != 0;
  const double *__restrict__ u = A.lapU, *__restrict__ v = A.lapV;
  const double *__restrict__ zeta = c->F.zeta + (long)(krhs - 1) * nij, *__restrict__ h = c->F.h;
  const double *pm = c->F.pm, *pn = c->F.pn;
  const long a = I2(i, j);
  auto D = [&](long q) { return zeta[q] + h[q]; };                       // Drhs, :700
  auto sr = [&](const RhoC &m, long q) { return m.visc * D(q) * 0.5 * strain_r(m, u, v, q, ni); };   // :1660-1672
  auto sp = [&](const PsiC &m, long q) {                                                             // :1673-1692
    const double Dp = 0.25 * (D(q) + D(q - 1) + D(q - ni) + D(q - 1 - ni));
    return masked_p(m.visc * Dp * 0.5 * strain_p(m, u, v, q, ni), m, msk);
  };
  const RhoC r0 = rho_coef(c, a, ni, c->F.visc4_r);
  const PsiC p0 = psi_coef(c, a, ni, c->F.visc4_p);
  const double sr0 = sr(r0, a), sp0 = sp(p0, a);
  if (do_u) {
    const RhoC rw = rho_coef(c, a - 1, ni, c->F.visc4_r);
    const PsiC pN = psi_coef(c, a + ni, ni, c->F.visc4_p);
    const Div2 d = div_flux(pn[a - 1] + pn[a], pm[a - 1] + pm[a], r0.on2 * sr0, rw.on2 * sr(rw, a - 1),
                            pN.om2 * sp(pN, a + ni), p0.om2 * sp0);
    facu[a] = d.cff1 + d.cff2;
  }
  if (do_v) {
    const RhoC rs = rho_coef(c, a - ni, ni, c->F.visc4_r);
    const PsiC pE = psi_coef(c, a + 1, ni, c->F.visc4_p);
    const Div2 d = div_flux(pn[a - ni] + pn[a], pm[a - ni] + pm[a], pE.on2 * sp(pE, a + 1), p0.on2 * sp0, r0.om2 * sr0,
                            rs.om2 * sr(rs, a - ni));
    facv[a] = d.cff1 - d.cff2;
  }
}

// ---- viscosity rotated to geopotential surfaces (MIX_GEO_UV; roms_params_t.uv_vis2 = 2, uv_vis4 = 2): the level body
// of uvgeo.h, instantiated for uv3dmix2_geo_tile (uv3dmix2_geo.h:116-756) on the tile itself and for the two passes of
// uv3dmix4_geo_tile (uv3dmix4_geo.h:262-1478): K_LOOP1 on the tile grown by one point -> LapU, LapV, and K_LOOP2 on
// LapU, LapV.  The rule for LapU, LapV outside the edges and at the corners between the passes (:806-976) is, statement
// for statement and range for range, the one of uv3dmix4_s.h: k_uv4_edges, k_uv4_corners above.
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_uv3dmix2_geo(const RomsDev *__restrict__ c, int nrhs, int nnew)
{
  const roms_bounds_t &b = c->b;
  const long n3r = (long)(b.UBi - b.LBi + 1) * (b.UBj - b.LBj + 1) * b.N;
  uvgeo_march<UVGEO_HARM>(c, GeoTile{b.Istr, b.IstrU, b.Iend, b.Jstr, b.JstrV, b.Jend},
                          (gcd_t)(c->F.u + (long)(nrhs - 1) * n3r), (gcd_t)(c->F.v + (long)(nrhs - 1) * n3r),
                          (gcd_t)c->F.visc2_r, (gcd_t)c->F.visc2_p,
                          (gd_t)(c->F.u + (long)(nnew - 1) * n3r), (gd_t)(c->F.v + (long)(nnew - 1) * n3r));
}

__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_uv4_geo_first(const RomsDev *__restrict__ c, int nrhs, GeoTile T, double *__restrict__ lapU, double *__restrict__ lapV)
{
  const roms_bounds_t &b = c->b;
  const long n3r = (long)(b.UBi - b.LBi + 1) * (b.UBj - b.LBj + 1) * b.N;
  uvgeo_march<UVGEO_FIRST>(c, T, (gcd_t)(c->F.u + (long)(nrhs - 1) * n3r), (gcd_t)(c->F.v + (long)(nrhs - 1) * n3r),
                           (gcd_t)c->F.visc4_r, (gcd_t)c->F.visc4_p, (gd_t)lapU, (gd_t)lapV);
}

__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_uv4_geo_second(const RomsDev *__restrict__ c, int nnew, const double *__restrict__ lapU, const double *__restrict__ lapV)
{
  const roms_bounds_t &b = c->b;
  const long n3r = (long)(b.UBi - b.LBi + 1) * (b.UBj - b.LBj + 1) * b.N;
  uvgeo_march<UVGEO_SECOND>(c, GeoTile{b.Istr, b.IstrU, b.Iend, b.Jstr, b.JstrV, b.Jend}, (gcd_t)lapU, (gcd_t)lapV,
                            (gcd_t)c->F.visc4_r, (gcd_t)c->F.visc4_p,
                            (gd_t)(c->F.u + (long)(nnew - 1) * n3r), (gd_t)(c->F.v + (long)(nnew - 1) * n3r));
}

}  // namespace

// the conditions of the pair (var_u, var_v) = (LBV_U, LBV_V) or (LBV_UBAR, LBV_VBAR) on the four sides
static void uv4_conditions(Uv4 &A, int var_u, int var_v)
{
  for (int sd = 0; sd < 4; sd++) {
    A.cu[sd] = lbc_code(g_ctx.p, sd, var_u) == LBC_CLOSED;
    A.cv[sd] = lbc_code(g_ctx.p, sd, var_v) == LBC_CLOSED;
  }
  A.gamma2 = g_ctx.p.gamma2;
}

// the rule for LapU, LapV of a filled Uv4 outside the edges and at the corners, on nk levels
static int uv4_rules(const Uv4 &A, int nk)
{
  const roms_bounds_t &b = g_ctx.b;
  auto mx = [](int x, int y) { return x > y ? x : y; };
  auto mn = [](int x, int y) { return x < y ? x : y; };
  const int nx = mx(A.iUb, A.iVb) - mn(A.iUa, A.iVa) + 1, ny = mx(A.jUb, A.jVb) - mn(A.jUa, A.jVa) + 1;
  if (!b.EWperiodic || !b.NSperiodic) {
    hipLaunchKernelGGL(k_uv4_edges, dim3((mx(nx, ny) + 63) / 64, nk, 4), dim3(64), 0, g_ctx.stream, g_ctx.devc, A);
    KERNEL_CHECK("k_uv4_edges");
  }
  if (!b.EWperiodic && !b.NSperiodic) {
    hipLaunchKernelGGL(k_uv4_corners, dim3((nk + 63) / 64), dim3(64), 0, g_ctx.stream, g_ctx.devc, A, nk);
    KERNEL_CHECK("k_uv4_corners");
  }
  return 0;
}

// LapU, LapV of a filled Uv4 on nk levels: the first operator (k_uv4_first on level index nrhs, k2d_visc4_first on
// krhs), then its rule outside the edges and at the corners
static int uv4_first_pass(void (*first)(const RomsDev *, int, Uv4), const Uv4 &A, int tindex, int nk)
{
  auto mx = [](int x, int y) { return x > y ? x : y; };
  auto mn = [](int x, int y) { return x < y ? x : y; };
  const int nx = mx(A.iUb, A.iVb) - mn(A.iUa, A.iVa) + 1, ny = mx(A.jUb, A.jVb) - mn(A.jUa, A.jVa) + 1;
  hipLaunchKernelGGL(first, grid2d(nx, ny), block2d(), 0, g_ctx.stream, g_ctx.devc, tindex, A);
  KERNEL_CHECK("k_uv4_first / k2d_visc4_first");
  return uv4_rules(A, nk);
}

// MIX_GEO_UV is one CPP switch for both operators (uv3dmix.F:21-34): a pair (uv_vis2, uv_vis4) of (1, 2) or (2, 1)
// is a model the reference cannot be compiled to
int roms_uv_mix_check(const char *where)
{
  const roms_params_t &p = g_ctx.p;
  if (p.uv_vis2 && p.uv_vis4 && (p.uv_vis2 == 2) != (p.uv_vis4 == 2))
    return roms_fail(where, "uv_vis2 and uv_vis4 disagree about MIX_GEO_UV: when both are set both are 1 (MIX_S_UV) "
                            "or both are 2 (MIX_GEO_UV), one CPP switch in the reference (uv3dmix.F:21-34)");
  return 0;
}

// called by step2d_impl (k_step2d.hip) in front of the momentum kernel when UV_VIS4 is set
int roms_launch_step2d_visc4(int krhs)
{
  const roms_bounds_t &b = g_ctx.b;
  if (b.NghostPoints != 3) return roms_fail("roms_hip_step2d", "UV_VIS4 needs NghostPoints = 3 (inp_par.F:268-270)");
  Uv4 A;
  A.lapU = g_ctx.hostc.ws2[20];
  A.lapV = g_ctx.hostc.ws2[21];
  A.iUa = b.IstrUm1; A.iUb = b.Iendp1; A.jUa = b.Jstrm1; A.jUb = b.Jendp1;      // :1506-1529
  A.iVa = b.Istrm1; A.iVb = b.Iendp1; A.jVa = b.JstrVm1; A.jVb = b.Jendp1;
  uv4_conditions(A, LBV_UBAR, LBV_VBAR);
  const int rc = uv4_first_pass(k2d_visc4_first, A, krhs, 1);
  if (rc) return rc;
  hipLaunchKernelGGL(k2d_visc4_second, grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1), block2d(), 0, g_ctx.stream,
                     g_ctx.devc, krhs, A, g_ctx.hostc.ws2[22], g_ctx.hostc.ws2[23]);
  KERNEL_CHECK("k2d_visc4_second");
  return 0;
}

extern "C" int roms_hip_uv3dmix2(const roms_step_idx_t *s)
{
  int rc = roms_entry_check("roms_hip_uv3dmix2");
  if (rc) return rc;
  if ((rc = roms_uv_mix_check("roms_hip_uv3dmix2"))) return rc;
  ScopedTimer tm("uv3dmix2");
  const roms_bounds_t &b = g_ctx.b;
  if (g_ctx.p.uv_vis2 == 2) {                                     // MIX_GEO_UV
    hipLaunchKernelGGL(k_uv3dmix2_geo, grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1), block2d(), 0, g_ctx.stream,
                       g_ctx.devc, s->nrhs, s->nnew);
    KERNEL_CHECK("k_uv3dmix2_geo");
    return 0;
  }
  hipLaunchKernelGGL(k_uv3dmix2_v2<false>, grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1), block2d(), 0, g_ctx.stream,
                     g_ctx.devc, s->nrhs, s->nnew, (const double *)nullptr, (const double *)nullptr);
  KERNEL_CHECK("k_uv3dmix2_v2");
  return 0;
}

extern "C" int roms_hip_uv3dmix4(const roms_step_idx_t *s)
{
  int rc = roms_entry_check("roms_hip_uv3dmix4");
  if (rc) return rc;
  const roms_bounds_t &b = g_ctx.b;
  const roms_params_t &p = g_ctx.p;
  if (!p.uv_vis4) return roms_fail("roms_hip_uv3dmix4", "UV_VIS4 is not set (roms_params_t.uv_vis4)");
  if ((rc = roms_uv_mix_check("roms_hip_uv3dmix4"))) return rc;
  if (b.NghostPoints != 3) return roms_fail("roms_hip_uv3dmix4", "UV_VIS4 needs NghostPoints = 3 (inp_par.F:268-270)");
  ScopedTimer tm("uv3dmix4");
  Uv4 A;
  A.lapU = g_ctx.hostc.ws3[1];
  A.lapV = g_ctx.hostc.ws3[2];
  auto mx = [](int x, int y) { return x > y ? x : y; };
  auto mn = [](int x, int y) { return x < y ? x : y; };
  if (b.EWperiodic) { A.iUa = b.Istr - 1; A.iUb = b.Iend + 1; A.iVa = b.Istr - 1; A.iVb = b.Iend + 1; }
  else { A.iUa = mx(2, b.IstrU - 1); A.iUb = mn(b.Iend + 1, b.Lm); A.iVa = mx(1, b.Istr - 1); A.iVb = mn(b.Iend + 1, b.Lm); }
  if (b.NSperiodic) { A.jUa = b.Jstr - 1; A.jUb = b.Jend + 1; A.jVa = b.Jstr - 1; A.jVb = b.Jend + 1; }
  else { A.jUa = mx(1, b.Jstr - 1); A.jUb = mn(b.Jend + 1, b.Mm); A.jVa = mx(2, b.JstrV - 1); A.jVb = mn(b.Jend + 1, b.Mm); }
  uv4_conditions(A, LBV_U, LBV_V);
  if (p.uv_vis4 == 2) {                                           // MIX_GEO_UV, uv3dmix4_geo.h
    // K_LOOP1 on the tile grown to the range of LapU, LapV (three ghost points carry it: no exchange between the
    // passes), the rule outside the edges, K_LOOP2 on the tile
    const GeoTile T{b.Istrm1, b.IstrUm1, b.Iendp1, b.Jstrm1, b.JstrVm1, b.Jendp1};
    if (T.IstrU != A.iUa || T.Iend != A.iUb || T.Jstr != A.jUa || T.Jend != A.jUb || T.Istr != A.iVa || T.JstrV != A.jVa)
      return roms_fail("roms_hip_uv3dmix4", "the bounds Istrm1 .. Jendp1 are not those of get_bounds.F for this tile");
    hipLaunchKernelGGL(k_uv4_geo_first, grid2d(T.Iend - T.Istr + 1, T.Jend - T.Jstr + 1), block2d(), 0, g_ctx.stream,
                       g_ctx.devc, s->nrhs, T, A.lapU, A.lapV);
    KERNEL_CHECK("k_uv4_geo_first");
    if ((rc = uv4_rules(A, b.N))) return rc;
    hipLaunchKernelGGL(k_uv4_geo_second, grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1), block2d(), 0, g_ctx.stream,
                       g_ctx.devc, s->nnew, (const double *)A.lapU, (const double *)A.lapV);
    KERNEL_CHECK("k_uv4_geo_second");
    return 0;
  }
  if ((rc = uv4_first_pass(k_uv4_first, A, s->nrhs, b.N))) return rc;
  hipLaunchKernelGGL(k_uv3dmix2_v2<true>, grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1), block2d(), 0, g_ctx.stream,
                     g_ctx.devc, s->nrhs, s->nnew, (const double *)A.lapU, (const double *)A.lapV);
  KERNEL_CHECK("k_uv3dmix2_v2<bih>");
  return 0;
}
