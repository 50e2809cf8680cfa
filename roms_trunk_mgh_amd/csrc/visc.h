// visc.h -- the lateral viscous stress along s-surfaces and its divergence, shared by the operators of
// k_uv3dmix2.hip: uv3dmix2_s.h:205-335, both operators of uv3dmix4_s.h and the two of the 2-D biharmonic pass of
// step2d (step2d_LF_AM3.h:1474-1740).  The reference writes the same two strain brackets, the same psi-point mask and
// the same two divergences in every one of them; here each is stated once.  (The harmonic viscosity of k2d_mom_lds,
// step2d_LF_AM3.h:1394-1471, is the same text on that kernel's row-table accessors and LDS tiles; see there.)
//   coefficients   RhoC, PsiC, rho_coef(), psi_coef(); kx(), ke()
//   strain         strain_r(), strain_p(): the brackets without a prefactor
//   mask           psi_mask(), masked_p()
//   divergence     div_flux(), div_lap<>()
// The copies differ in association only, and the caller keeps it: the prefactor (Hz*0.5, 0.5, visc*0.5, visc*D*0.5)
// multiplies the bracket from the left, and the weight of a stress is on2 * visc in the 3-D operators (uv3dmix2_s.h:
// 262) but on2 alone in the 2-D ones, whose prefactor holds visc already (step2d_LF_AM3.h:1416).
#pragma once
#include "roms_dev.h"

// One stress point: the two metric ratios, the four metric sums of its bracket, on^2 and om^2 there and the viscosity
// coefficient.  The 3-D kernels form it once per column (registers), the 2-D ones per point.
struct RhoC { double pmon, pnom, e1, e0, n1, n0, on2, om2, visc; };
struct PsiC { double pmon, pnom, a, b, c, d, on2, om2, visc, mask; };   // mask: psi_mask()
__device__ __forceinline__ double sqr(const double x) { return x * x; }
// the weight of a stress in the 3-D operators, on_r*on_r*visc / om_r*om_r*visc (rho or psi)
template <class C> __device__ __forceinline__ double kx(const C &m) { return m.on2 * m.visc; }
template <class C> __device__ __forceinline__ double ke(const C &m) { return m.om2 * m.visc; }
// MASKING: the stress at a psi-point is multiplied by pmask, under WET_DRY by pmask_wet as well (uv3dmix2_s.h:272-275,
// uv3dmix4_s.h:334, :560, step2d_LF_AM3.h:1433-1438, :1512, :1707)
__device__ __forceinline__ double psi_mask(const RomsDev *__restrict__ c, long q) { return c->p.masking ? pmaskw(c, q) : 1.0; }
__device__ __forceinline__ double masked_p(const double cff, const PsiC &m, const bool msk) { return msk ? cff * m.mask : cff; }
__device__ __forceinline__ RhoC rho_coef(const RomsDev *__restrict__ c, long q, long ni, const double *__restrict__ visc_r)
{
  const double *pm = c->F.pm, *pn = c->F.pn;
  return RhoC{c->F.pmon_r[q], c->F.pnom_r[q], pn[q] + pn[q + 1], pn[q - 1] + pn[q], pm[q] + pm[q + ni], pm[q - ni] + pm[q],
              sqr(c->F.on_r[q]), sqr(c->F.om_r[q]), visc_r[q]};
}
__device__ __forceinline__ PsiC psi_coef(const RomsDev *__restrict__ c, long q, long ni, const double *__restrict__ visc_p)
{
  const double *pm = c->F.pm, *pn = c->F.pn;
  return PsiC{c->F.pmon_p[q], c->F.pnom_p[q], pn[q - ni] + pn[q], pn[q - 1 - ni] + pn[q - 1], pm[q - 1] + pm[q],
              pm[q - 1 - ni] + pm[q - ni], sqr(c->F.on_p[q]), sqr(c->F.om_p[q]), visc_p[q], psi_mask(c, q)};
}

// The strain at rho-point q / psi-point q of the pair (u, v); sy = the stride of a row.  (Pointer type as the caller
// has it: generic pointers make flat loads, see k_uv3dmix2_v2.)
template <class P>
__device__ __forceinline__ double strain_r(const RhoC &m, const P u, const P v, const long q, const long sy)
{
  return m.pmon * (m.e1 * u[q + 1] - m.e0 * u[q]) - m.pnom * (m.n1 * v[q + sy] - m.n0 * v[q]);
}
template <class P>
__device__ __forceinline__ double strain_p(const PsiC &m, const P u, const P v, const long q, const long sy)
{
  return m.pmon * (m.a * v[q] - m.b * v[q - 1]) + m.pnom * (m.c * u[q] - m.d * u[q - sy]);
}

// The divergence of the weighted stresses at a u-point: X0, Xw = UFx at its own and its western rho-point, En, E0 =
// UFe at the northern and its own psi-point, pn2 = pn(i-1)+pn(i), pm2 likewise.  At a v-point the mirrored pair:
// (VFx east, own psi; VFe own, southern rho; pn(j-1)+pn(j)), combined as cff1 - cff2.
struct Div2 { double cff1, cff2; };
__device__ __forceinline__ Div2 div_flux(const double pn2, const double pm2, const double X0, const double Xw,
                                         const double En, const double E0)      // uv3dmix2_s.h:289-311
{
  return Div2{0.5 * pn2 * (X0 - Xw), 0.5 * pm2 * (En - E0)};
}
template <bool V>                                                                  // uv3dmix4_s.h:340-355
__device__ __forceinline__ double div_lap(const double pm2, const double pn2, const double X0, const double Xw,
                                          const double En, const double E0)
{
  if constexpr (V) return 0.125 * pm2 * pn2 * (pn2 * (X0 - Xw) - pm2 * (En - E0));
  else return 0.125 * pm2 * pn2 * (pn2 * (X0 - Xw) + pm2 * (En - E0));
}
