// gls.h -- the formulas the two equations (tke and gls) and the two steps (predictor and corrector) of the closure in
// k_gls.hip share, each stated once for one field:
//   horizontal   Grad<Y> (the masked face gradient and the edge rule, one direction), face_transport(),
//                flux_c4() (gls_prestep.F:176-263), flux_u3() (gls_corstep.F:444-640)
//   vertical     vface() (gls_prestep.F:322-352, gls_corstep.F:644-700)
//   implicit     diff_coef() (the off-diagonal -0.5*dt*(Ak+Ak)/Hz), thomas() (gls_corstep.F:864-960,
//                my25_corstep.F:649-692)
//   Dirichlet    stress_tke() (gls_corstep.F:806-830, my25_corstep.F:630-646)
// Every function keeps the operands and the association of the reference's expression: the build does not contract,
// so equal text is equal bits.  A factor that multiplies a bracket from the left (the transport, CF, cmu_fac3) is an
// argument or stays with the caller for that reason.
#pragma once
#include "roms_dev.h"

// Gradient of a field at a u-face (Y = false) or v-face (Y = true), with the MASKING multiply and the reference's rule
// for the face outside a physical edge (Istr-1 and Iend+2, or Jstr-1 and Jend+2): it takes the next face's value.
// s() = the stride of the direction.  The bounds are read through b where they are used, as uniform branches: copied
// into registers they become selects, every load of a level is then issued at once and k_gls_corstep needs 220
// VGPRs instead of 127.
template <bool Y> struct Grad {
  const roms_bounds_t &b; const double *mask; bool mk; long ni;
  __device__ __forceinline__ long s() const { return Y ? ni : 1; }
  // X: the level's plane, q: the 2-D index of face f, d: the face wanted is f + d
  __device__ __forceinline__ double operator()(const double *X, long q, int f, int d) const
  {
    int ff = f + d;
    if (!(Y ? b.NSperiodic : b.EWperiodic)) {
      if ((Y ? b.south_edge : b.west_edge) && ff == (Y ? b.Jstr : b.Istr) - 1) ff = (Y ? b.Jstr : b.Istr);
      if ((Y ? b.north_edge : b.east_edge) && ff == (Y ? b.Jend : b.Iend) + 2) ff = (Y ? b.Jend : b.Iend) + 1;
    }
    const long a = q + (long)(ff - f) * s();
    double g = (X[a] - X[a - s()]);
    if (mk) g = g * mask[a];
    return g;
  }
};
template <bool Y> __device__ __forceinline__ Grad<Y> grad_dir(const RomsDev *__restrict__ c, long ni)
{
  return Grad<Y>{c->b, Y ? c->F.vmask : c->F.umask, c->p.masking != 0, ni};
}

// transport through a face at W-level k: the average of the rho-levels k and k+1; r = the face at rho-level k
__device__ __forceinline__ double face_transport(const double *H, long r, long nij) { return 0.5 * (H[r] + H[r + nij]); }

// flux of X through face f with transport HF: centred fourth-order (predictor) ...
template <bool Y> __device__ __forceinline__ double flux_c4(const Grad<Y> &g, double HF, const double *X, long q, int f)
{
  return HF * 0.5 * (X[q - g.s()] + X[q] - 1.0 / 6.0 * (g(X, q, f, 1) - g(X, q, f, -1)));
}
// ... and third-order upstream-biased (corrector): the curvature at the point up = -1 (west / south of the face) or
// 0, the side the transport comes from.  The caller branches on the sign once for the two fields.
template <bool Y> __device__ __forceinline__ double flux_u3(const Grad<Y> &g, double HF, const double *X, long q, int f, int up)
{
  return HF * 0.5 * (X[q - g.s()] + X[q] - 1.0 / 3.0 * (g(X, q, f, up + 1) - g(X, q, f, up)));
}

// value of X (W-type) at the rho-level kk between the W-levels kk-1 and kk = w: fourth-order centred, one-sided at
// kk = 1 and kk = N.  The caller multiplies by CF = 0.5*(W(kk)+W(kk-1)).
__device__ __forceinline__ double vface(const double *X, long w, int kk, int N, long nij)
{
  if (kk == 1) return 1.0 / 3.0 * X[w - nij] + 5.0 / 6.0 * X[w] - 1.0 / 6.0 * X[w + nij];
  if (kk == N) return 1.0 / 3.0 * X[w] + 5.0 / 6.0 * X[w - nij] - 1.0 / 6.0 * X[w - 2 * nij];
  return 7.0 / 12.0 * (X[w - nij] + X[w]) - 1.0 / 12.0 * (X[w - 2 * nij] + X[w + nij]);
}

// off-diagonal of the implicit vertical diffusion at the rho-levels k0..k1 of column a2, stored at W-index k
__device__ __forceinline__ void diff_coef(double *FC, const double *Ak, const double *Hz, long a2, long nij, double dt, int k0, int k1)
{
  const double cff = -0.5 * dt;
  for (int k = k0; k <= k1; k++) {
    const long w = a2 + (long)k * nij;
    FC[w] = cff * (Ak[w] + Ak[w - nij]) / Hz[w - nij];
  }
}

// The tridiagonal system of one column, rows 1..N-1: diagonal BC, off-diagonal FC, X = right-hand side in, solution out;
// CF is scratch.  Elimination from the top, substitution from the bottom.  What differs between the systems:
//   top    the right-hand side of row N-1, boundary term included
//   fluxb  the bottom flux (GLS: X(1) is corrected by cff*fluxb, cff the reciprocal pivot of row 1)
//   k0     the first row of the substitution: 1 = from the Dirichlet value X(0) (MY25), 2 = from X(1) (GLS)
__device__ __forceinline__ void thomas(double *X, const double *BC, const double *FC, double *CF, long a2, long nij, int N,
                                       double top, double fluxb, int k0)
{
  const long wt = a2 + (long)(N - 1) * nij;
  double cff = 1.0 / BC[wt];
  double CFp = cff * FC[wt];
  CF[wt] = CFp;
  double Xp = cff * top;
  X[wt] = Xp;
  for (int k = N - 2; k >= 1; k--) {
    const long w = a2 + (long)k * nij;
    const double FC1 = FC[w + nij];
    cff = 1.0 / (BC[w] - CFp * FC1);
    CFp = cff * FC[w];
    CF[w] = CFp;
    Xp = cff * (X[w] - FC1 * Xp);
    X[w] = Xp;
  }
  if (k0 == 2) X[a2 + nij] = X[a2 + nij] - cff * fluxb;
  double Xm = X[a2 + (long)(k0 - 1) * nij];
  for (int k = k0; k <= N - 1; k++) {
    const long w = a2 + (long)k * nij;
    Xm = X[w] - CF[w] * Xm;
    X[w] = Xm;
  }
}

// Dirichlet tke from the stress at the column's two u-faces and two v-faces: fac * 0.5 * |stress sum|
__device__ __forceinline__ double stress_tke(double fac, const double *su, const double *sv, long a2, long ni)
{
  const double sx = su[a2] + su[a2 + 1], sy = sv[a2] + sv[a2 + ni];
  return fac * 0.5 * sqrt(sx * sx + sy * sy);
}
