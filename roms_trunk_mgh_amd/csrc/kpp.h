// kpp.h -- the formulas the surface and the bottom boundary layer of K-profile mixing share (k_lmd_vmix, k_lmd_bkpp of
// k_lmd.hip; k_gls.hip uses the splines), each stated once.  The layers differ in what they pass: the stress pair, stflx
// or btflx, zwN - z or z - zw0, which of a pair is the reference value.  Every function keeps the operands and the
// association of the reference's expression: the build does not contract, so equal text is equal bits.
#pragma once
#include "roms_dev.h"

// ---- parabolic splines: one level of the forward recurrence and of the back-substitution ----
// the coefficient pair of W-level k from Hz of the rho-levels k (A) and k+1 (B) and FC(k-1)
struct SplineCoef { double cff, FC; };
__device__ __forceinline__ SplineCoef spline_coef(double HzA, double HzB, double FCm)
{
  const double cff = 1.0 / (2.0 * HzB + HzA * (2.0 - FCm));
  return SplineCoef{cff, cff * HzB};
}
// the forward value of one derivative; rhs is formed by the caller: 3.0*(uB - uA + u'B - u'A) or 6.0*(pdB - pdA)
__device__ __forceinline__ double spline_fwd(double cff, double rhs, double HzA, double dm) { return cff * (rhs - HzA * dm); }
// x(k) = x(k) - FC(k) x(k+1)
__device__ __forceinline__ double spline_back(double x, double FC, double xp) { return x - FC * xp; }

// ---- forcing of a boundary layer ----
__device__ __forceinline__ double swfrac(const roms_params_t &p, double Z)     // lmd_swfrac.F:60-75, Zscale = -1
{
  const double fac1 = -1.0 / p.swfrac_mu1, fac2 = -1.0 / p.swfrac_mu2, fac3 = p.swfrac_r1;
  return exp(Z * fac1) * fac3 + exp(Z * fac2) * (1.0 - fac3);
}

__device__ __forceinline__ void wscale(double Ustar, double sigma, double Bf, double &wm, double &ws)
{
  const double vonKar = 0.41, small = 1.0E-20;
  const double lmd_am = 1.257, lmd_as = -28.86, lmd_cm = 8.36, lmd_cs = 98.96, lmd_zetam = -0.2, lmd_zetas = -1.0;
  const double Ustar3 = Ustar * Ustar * Ustar;
  const double zetahat = vonKar * sigma * Bf;
  const double zetapar = zetahat / (Ustar3 + small);
  if (zetahat >= 0.0) {
    wm = vonKar * Ustar / (1.0 + 5.0 * zetapar);
    ws = wm;
  } else {
    // x**0.25, x**0.5, x**(1/3) of lmd_skpp.F:441-452 as sqrt(sqrt(x)), sqrt(x), cbrt(x): each within an
    // ulp of the reference's pow (whose device version is not bit-identical to the host's either) at a
    // fraction of the cost -- the kernel is bound by these calls, ~4 per level and sweep
    if (zetapar > lmd_zetam) wm = vonKar * Ustar * sqrt(sqrt(1.0 - 16.0 * zetapar));
    else wm = vonKar * cbrt(lmd_am * Ustar3 - lmd_cm * zetahat);
    if (zetapar > lmd_zetas) ws = vonKar * Ustar * sqrt(1.0 - 16.0 * zetapar);
    else ws = vonKar * cbrt(lmd_as * Ustar3 - lmd_cs * zetahat);
  }
}

// velocity scales of a level at distance depth from the layer's boundary; bl_dpth = lmd_epsilon * layer depth
__device__ __forceinline__ void kpp_wscale(double Ustar, double bf, double bl_dpth, double depth, double &wm, double &ws)
{
  const double sigma = (bf < 0.0) ? fmin(bl_dpth, depth) : depth;
  wscale(Ustar, sigma, bf, wm, ws);
}

// Ustar of a stress pair at the rho-point (the two u-faces, the two v-faces)
__device__ __forceinline__ double kpp_ustar(double su0, double su1, double sv0, double sv1, bool masking, double mr)
{
  const double b1 = 0.5 * (su0 + su1), b2 = 0.5 * (sv0 + sv1);
  const double Ustar = sqrt(sqrt(b1 * b1 + b2 * b2));
  return masking ? Ustar * mr : Ustar;
}
// buoyancy flux where the shortwave fraction is swd
__device__ __forceinline__ double kpp_bflux(double Bo, double Bosol, double swd, bool masking, double mr)
{
  const double bf = (Bo + Bosol * (1.0 - swd));
  return masking ? bf * mr : bf;
}
// ... at the layer depth zgrid: MASKING multiplies the depth too
__device__ __forceinline__ double kpp_bflux_at(const roms_params_t &p, double Bo, double Bosol, double zgrid, bool masking, double mr)
{
  return kpp_bflux(Bo, Bosol, swfrac(p, masking ? zgrid * mr : zgrid), masking, mr);
}
// velocity scales at the layer depth zbl, where the buoyancy flux is Bf; returns f1 of the shape functions' derivative
__device__ __forceinline__ double kpp_scales_at(double Ustar, double Bf, double zbl, double &wm, double &ws)
{
  const double vonKar = 0.41, eps = 1.0E-10, lmd_epsilon = 0.1;
  wscale(Ustar, ((Bf > 0.0) ? 1.0 : lmd_epsilon) * zbl, Bf, wm, ws);
  return 5.0 * fmax(0.0, Bf) * vonKar / (Ustar * Ustar * Ustar * Ustar + eps);
}

// ---- boundary-layer depth ----
// the critical function from the pairs whose differences A - B the layer compares (surface: reference - level, bottom:
// level - reference)
__device__ __forceinline__ double kpp_critical(double gorho0, double RA, double RB, double UA, double UB, double VA, double VB,
                                               double depth, double Vtc, double ws, double bvf)
{
  const double lmd_Ric = 0.3;
  const double Ritop = -gorho0 * (RA - RB) * depth;
  const double Ribot = (UA - UB) * (UA - UB) + (VA - VB) * (VA - VB) + Vtc * depth * ws * sqrt(fabs(bvf));
  return Ritop - lmd_Ric * Ribot;
}
// where the function crosses zero between the upper level (zU, FU) and the lower one (zL, FL)
__device__ __forceinline__ double kpp_crossing(double zU, double FU, double zL, double FL) { return (zU * FL - zL * FU) / (FL - FU); }

// ---- shape functions at the layer depth hbl between the W-levels k (zk) and k-1 (zm) ----
struct KppBracket { double cff, cff_dn, cff_up; };
__device__ __forceinline__ KppBracket kpp_bracket(double zk, double zm, double hbl)
{
  const double cff = 1.0 / (zk - zm);
  return KppBracket{cff, cff * (hbl - zm), cff * (zk - hbl)};
}
// G1 and dG1dS of one field from its value and its derivative at hbl.  The two layers are NOT the same arithmetic:
// -dK/(w+eps) - K*f1 at the surface, K*f1 - dK/(w+eps) at the bottom.
struct KppMatch { double G1, dG1dS; };
template <bool BOTTOM>
__device__ __forceinline__ KppMatch kpp_match(double K_bl, double dK_bl, double zbl, double w, double f1, bool masking, double mr)
{
  const double eps = 1.0E-10;
  double G1 = K_bl / (zbl * w + eps);
  if (masking) G1 = G1 * mr;
  return KppMatch{G1, BOTTOM ? fmin(0.0, K_bl * f1 - dK_bl / (w + eps)) : fmin(0.0, -dK_bl / (w + eps) - K_bl * f1)};
}
// ... from its values at the two levels (the bottom's derivative is -cff*(Kk - Km))
template <bool BOTTOM>
__device__ __forceinline__ KppMatch kpp_match(double Kk, double Km, KppBracket B, double zbl, double w, double f1, bool masking,
                                              double mr)
{
  const double K_bl = B.cff_dn * Kk + B.cff_up * Km;
  const double dK_bl = BOTTOM ? -B.cff * (Kk - Km) : B.cff * (Kk - Km);
  return kpp_match<BOTTOM>(K_bl, dK_bl, zbl, w, f1, masking, mr);
}
// the blended profile of momentum, temperature and salinity at sigma = depth / layer depth zbl (times the mask)
struct KppShape { KppMatch m, t, s; };
struct KppAk { double akv, akt, aks; };
__device__ __forceinline__ KppAk kpp_blend(double depth, double zbl, double wm, double ws, const KppShape &G, bool masking, double mr)
{
  const double s0 = depth / (zbl + 1.0E-10), sigma = masking ? s0 * mr : s0;
  const double a1 = sigma - 2.0, a2 = 3.0 - 2.0 * sigma, a3 = sigma - 1.0;
  const double Gm = a1 + a2 * G.m.G1 + a3 * G.m.dG1dS;
  const double Gt = a1 + a2 * G.t.G1 + a3 * G.t.dG1dS;
  const double Gs = a1 + a2 * G.s.G1 + a3 * G.s.dG1dS;
  return KppAk{depth * wm * (1.0 + sigma * Gm), depth * ws * (1.0 + sigma * Gt), depth * ws * (1.0 + sigma * Gs)};
}

// ---- lmd_finish: the convective increment where the stratification is unstable ----
__device__ __forceinline__ double kpp_convec(double bvf)
{
  const double lmd_bvfcon = -2.0E-5, lmd_nu0c = 0.01;
  double cff = fmax(bvf, lmd_bvfcon);
  cff = fmin(1.0, (lmd_bvfcon - cff) / lmd_bvfcon);
  double nu_sxc = 1.0 - cff * cff;
  nu_sxc = nu_sxc * nu_sxc * nu_sxc;
  return lmd_nu0c * nu_sxc;
}

// ---- bc_r2d_tile of a 2-D rho field the kernel owns: zero gradient at the closed walls of a channel ----
__device__ __forceinline__ void kpp_wall_rows(const roms_bounds_t &b, gd_t X, long a, long ni, int j, double x)
{
  if (!b.NSperiodic) {
    if (b.south_edge && j == b.Jstr) X[a - ni] = x;
    if (b.north_edge && j == b.Jend) X[a + ni] = x;
  }
}
