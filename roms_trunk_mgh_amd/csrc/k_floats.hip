// k_floats.hip -- Lagrangian floats (FLOATS): step_floats_tile (ROMS/Nonlinear/step_floats.F:80-1053) and
// interp_floats (ROMS/Nonlinear/interp_floats.F:56-541) for SOLVE3D, FLOATS, with or without MASKING, in the
// DISTRIBUTE form (ownership switch and SUM collection).  Not built: FLOAT_VWALK (nudg = 0), FLOAT_STICKY,
// FLOAT_BIOLOGY / FLOAT_OYSTER, the 2-D branch, N-S periodic grids.
//
// One thread per float; every statement of the reference in the reference's order, so that the result is the
// reference's bit for bit (the build does not contract multiply-adds).  The work is a scattered gather: about eight
// corner values of a handful of resident 3-D fields per float and interpolation.
//
// track lives on the device as a structure of arrays, the float index fastest:
//   trk[((lev * NFV) + (v - 1)) * Nfloats + l],   lev = 0..NFT, v = 1..NFV = NT + 10, l = 0..Nfloats-1,
// followed by one more row of Nfloats doubles, the work array of the collection of `bounded` (:1036-1049).
//
// Precondition (the reference rests on the same): a float moves less than one cell per step, so its owner reads
// at most two ghost points.  Every gather clamps its horizontal index to the allocated extents LBi:UBi, LBj:UBj --
// under the precondition the clamp never acts; without it a float that was handed over far outside the grid reads
// an edge value instead of unmapped memory.
#include "roms_dev.h"
#include <vector>

namespace {
// mod_floats.F:80-90 (1-based rows of track) and :125-127
enum { itstr = 0, ixgrd = 1, iygrd = 2, izgrd = 3, iflon = 4, iflat = 5, idpth = 6, ixrhs = 7, iyrhs = 8, izrhs = 9, ifden = 10 };
enum { flt_Lagran = 1, flt_Isobar = 2, flt_Geopot = 3 };
enum { NFT = 4, NTINFO = 10 };
// gtype of interp_floats: r2dvar, r3dvar, w3dvar, -u3dvar, -v3dvar, -w3dvar
enum { FG_R2D = 0, FG_R3D, FG_W3D, FG_NU3D, FG_NV3D, FG_NW3D };

struct FltStore {
  int n = 0, NFV = 0;
  long nij = 0;
  double *trk = nullptr;         // (5 * NFV + 1) * n
  int *ibuf = nullptr;           // bounded[n], Ftype[n]
  double *dbuf = nullptr;        // Tinfo[10 * n], Fz0[n]
  double *xc = nullptr, *xc_base = nullptr, *yc = nullptr, *yc_base = nullptr;
} g_flt;

struct FltArgs {
  int n, NFV, nnew, phase, master;
  int nfm3, nfm2, nfm1, nf, nfp1;
  double time;
  double *trk;
  int *bounded;
  const int *Ftype;
  const double *Tinfo, *Fz0, *xc, *yc;
};

struct FltGrid {
  int LBi, UBi, LBj, UBj, Lm, Mm, N;
  long ni, nij;
  bool masking, ewp;
  gcd_t pm, pn, Hz, rmask;
};
}  // namespace

// INT() of a position; the clamp keeps the conversion defined for any double (the indices are clamped to the grid
// right after)
__device__ __forceinline__ int flt_int(double x) { return (int)fmin(fmax(x, -2.0e9), 2.0e9); }
__device__ __forceinline__ int flt_nint(double x) { return (int)round(fmin(fmax(x, -2.0e9), 2.0e9)); }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ long flt_q(const FltGrid &g, int i, int j)
{
  i = imin(imax(i, g.LBi), g.UBi);
  j = imin(imax(j, g.LBj), g.UBj);
  return (long)(i - g.LBi) + (long)(j - g.LBj) * g.ni;
}

// interp_floats.F:171-538 for one float at (x, y, z) = track(ixgrd / iygrd / izgrd, itime, l); A points at the plane
// k = LBk of the field (LBk = 0 for a w-type field, 1 otherwise).  nudg(l) = 0 (no FLOAT_VWALK), added where the
// reference adds it.
template <int GT>
__device__ double flt_interp(const FltGrid &g, gcd_t A, bool maskit, double x, double y, double z)
{
  constexpr bool Krvar = GT == FG_R3D || GT == FG_NU3D || GT == FG_NV3D;
  constexpr bool Kwvar = GT == FG_W3D || GT == FG_NW3D;
  constexpr bool rho = GT == FG_R2D || GT == FG_R3D || GT == FG_W3D || GT == FG_NW3D;
  constexpr int LBk = Kwvar ? 0 : 1;
  const int N = g.N, Lm = g.Lm, Mm = g.Mm;
  const bool Lmask = g.masking && maskit;                                                   // :140-144
  const double nudg = 0.0;
#define A3(i, j, k) A[flt_q(g, i, j) + (long)((k) - LBk) * g.nij]
  int k1, k2;
  double r1, r2;
  if (Krvar) {                                                                              // :179-184
    const int Kr = flt_int(z + 0.5);
    k1 = imin(imax(Kr, 1), N);
    k2 = imin(imax(Kr + 1, 1), N);
    r2 = (double)(k2 - k1) * (z + 0.5 - (double)k1);
  } else if (Kwvar) {                                                                       // :185-189
    const int Kw = flt_int(z);
    k1 = imin(imax(Kw, 0), N);
    k2 = imin(imax(Kw + 1, 0), N);
    r2 = (double)(k2 - k1) * (z - (double)k1);
  } else {
    k1 = 1;
    k2 = 1;
    r2 = 0.0;
  }
  r1 = 1.0 - r2;
  double s111 = 1.0, s211 = 1.0, s121 = 1.0, s221 = 1.0, s112 = 1.0, s212 = 1.0, s122 = 1.0, s222 = 1.0;
  double t111 = 1.0, t211 = 1.0, t121 = 1.0, t221 = 1.0, t112 = 1.0, t212 = 1.0, t122 = 1.0, t222 = 1.0;
  if (rho) {                                                                                // :201-298
    const int Ir = flt_int(x), Jr = flt_int(y);
    const int i1 = imin(imax(Ir, 0), Lm + 1), i2 = imin(imax(Ir + 1, 1), Lm + 1);
    const int j1 = imin(imax(Jr, 0), Mm + 1), j2 = imin(imax(Jr + 1, 1), Mm + 1);
    const double p2 = (double)(i2 - i1) * (x - (double)i1), q2 = (double)(j2 - j1) * (y - (double)j1);
    const double p1 = 1.0 - p2, q1 = 1.0 - q2;
    const long c11 = flt_q(g, i1, j1), c21 = flt_q(g, i2, j1), c12 = flt_q(g, i1, j2), c22 = flt_q(g, i2, j2);
    if (GT == FG_NW3D) {                                                                    // :217-246
      int khm = imin(imax(k1, 1), N), khp = imin(imax(k1 + 1, 1), N);
      long m = (long)(khm - 1) * g.nij, p = (long)(khp - 1) * g.nij;
      s111 = 2.0 * g.pm[c11] * g.pn[c11] / (g.Hz[c11 + m] + g.Hz[c11 + p]);
      s211 = 2.0 * g.pm[c21] * g.pn[c21] / (g.Hz[c21 + m] + g.Hz[c21 + p]);
      s121 = 2.0 * g.pm[c12] * g.pn[c12] / (g.Hz[c12 + m] + g.Hz[c12 + p]);
      s221 = 2.0 * g.pm[c22] * g.pn[c22] / (g.Hz[c22 + m] + g.Hz[c22 + p]);
      t111 = 2.0 / (g.Hz[c11 + m] + g.Hz[c11 + p]);
      t211 = 2.0 / (g.Hz[c21 + m] + g.Hz[c21 + p]);
      t121 = 2.0 / (g.Hz[c12 + m] + g.Hz[c12 + p]);
      t221 = 2.0 / (g.Hz[c22 + m] + g.Hz[c22 + p]);
      khm = imin(imax(k2, 1), N);
      khp = imin(imax(k2 + 1, 1), N);
      m = (long)(khm - 1) * g.nij;
      p = (long)(khp - 1) * g.nij;
      s112 = 2.0 * g.pm[c11] * g.pn[c11] / (g.Hz[c11 + m] + g.Hz[c11 + p]);
      s212 = 2.0 * g.pm[c21] * g.pn[c21] / (g.Hz[c21 + m] + g.Hz[c21 + p]);
      s122 = 2.0 * g.pm[c12] * g.pn[c12] / (g.Hz[c12 + m] + g.Hz[c12 + p]);
      s222 = 2.0 * g.pm[c22] * g.pn[c22] / (g.Hz[c22 + m] + g.Hz[c22 + p]);
      t112 = 2.0 / (g.Hz[c11 + m] + g.Hz[c11 + p]);
      t212 = 2.0 / (g.Hz[c21 + m] + g.Hz[c21 + p]);
      t122 = 2.0 / (g.Hz[c12 + m] + g.Hz[c12 + p]);
      t222 = 2.0 / (g.Hz[c22 + m] + g.Hz[c22 + p]);
    }
    const long o1 = (long)(k1 - LBk) * g.nij, o2 = (long)(k2 - LBk) * g.nij;
    const double a111 = A[c11 + o1], a211 = A[c21 + o1], a121 = A[c12 + o1], a221 = A[c22 + o1];
    const double a112 = A[c11 + o2], a212 = A[c21 + o2], a122 = A[c12 + o2], a222 = A[c22 + o2];
    if (Lmask) {                                                                            // :249-280
      const double m11 = g.rmask[c11], m21 = g.rmask[c21], m12 = g.rmask[c12], m22 = g.rmask[c22];
      const double cff1 = p1 * q1 * r1 * m11 + p2 * q1 * r1 * m21 + p1 * q2 * r1 * m12 + p2 * q2 * r1 * m22 +
                          p1 * q1 * r2 * m11 + p2 * q1 * r2 * m21 + p1 * q2 * r2 * m12 + p2 * q2 * r2 * m22;
      if (cff1 > 0.0) {
        const double cff2 = p1 * q1 * r1 * m11 * s111 * a111 + p2 * q1 * r1 * m21 * s211 * a211 +
                            p1 * q2 * r1 * m12 * s121 * a121 + p2 * q2 * r1 * m22 * s221 * a221 +
                            p1 * q1 * r2 * m11 * s112 * a112 + p2 * q1 * r2 * m21 * s212 * a212 +
                            p1 * q2 * r2 * m12 * s122 * a122 + p2 * q2 * r2 * m22 * s222 * a222;
        const double cff3 = (p1 * q1 * r1 * m11 * t111 + p2 * q1 * r1 * m21 * t211 + p1 * q2 * r1 * m12 * t121 +
                             p2 * q2 * r1 * m22 * t221 + p1 * q1 * r2 * m11 * t112 + p2 * q1 * r2 * m21 * t212 +
                             p1 * q2 * r2 * m12 * t122 + p2 * q2 * r2 * m22 * t222) * nudg;
        return cff2 / cff1 + cff3;
      }
      return 0.0;
    }
    return p1 * q1 * r1 * s111 * a111 + p2 * q1 * r1 * s211 * a211 + p1 * q2 * r1 * s121 * a121 +          // :282-297
           p2 * q2 * r1 * s221 * a221 + p1 * q1 * r2 * s112 * a112 + p2 * q1 * r2 * s212 * a212 +
           p1 * q2 * r2 * s122 * a122 + p2 * q2 * r2 * s222 * a222 +
           (p1 * q1 * r1 * t111 + p2 * q1 * r1 * t211 + p1 * q2 * r1 * t121 + p2 * q2 * r1 * t221 +
            p1 * q1 * r2 * t112 + p2 * q1 * r2 * t212 + p1 * q2 * r2 * t122 + p2 * q2 * r2 * t222) * nudg;
  }
  // horizontal velocity points, :304-534
  const int Ir = flt_int(x), Jr = flt_int(y), Iu = flt_int(x + 0.5), Jv = flt_int(y + 0.5);
  bool halo = false;
  int Irn = 0, Jrn = 0;
  if (Lmask) {                                                                              // :326-386
    // the periodic Irnm1 ... Jrnp1 of :329-358 are never used: the test reads Amask(Irn+-1, Jrn+-1) directly
    Irn = flt_nint(x);
    Jrn = flt_nint(y);
    auto land = [&](int i, int j) { return g.rmask[flt_q(g, i, j)] < 0.5; };
    if (land(Irn, Jrn)) halo = true;
    else if (Ir < Irn && land(Irn - 1, Jrn)) halo = true;
    else if (Ir == Irn && land(Irn + 1, Jrn)) halo = true;
    else if (Jr < Jrn && land(Irn, Jrn - 1)) halo = true;
    else if (Jr == Jrn && land(Irn, Jrn + 1)) halo = true;
    else if (Ir < Irn && Jr < Jrn && land(Irn - 1, Jrn - 1)) halo = true;
    else if (Ir == Irn && Jr < Jrn && land(Irn + 1, Jrn - 1)) halo = true;
    else if (Ir < Irn && Jr == Jrn && land(Irn - 1, Jrn + 1)) halo = true;
    else if (Ir == Irn && Jr == Jrn && land(Irn + 1, Jrn + 1)) halo = true;
  }
  if (GT == FG_NU3D) {
    if (halo) {                                                                             // :402-422
      const int i1 = imin(imax(Iu, 1), Lm + 1), i2 = imin(imax(Iu + 1, 1), Lm + 1), j1 = Jrn;
      const double p2 = (double)(i2 - i1) * (x - (double)i1 + 0.5), p1 = 1.0 - p2, q1 = 1.0;
      s111 = 0.5 * (g.pm[flt_q(g, i1 - 1, j1)] + g.pm[flt_q(g, i1, j1)]);
      s211 = 0.5 * (g.pm[flt_q(g, i2 - 1, j1)] + g.pm[flt_q(g, i2, j1)]);
      s112 = s111;
      s212 = s112;
      return p1 * q1 * r1 * s111 * A3(i1, j1, k1) + p2 * q1 * r1 * s211 * A3(i2, j1, k1) +
             p1 * q1 * r2 * s112 * A3(i1, j1, k2) + p2 * q1 * r2 * s212 * A3(i2, j1, k2) + nudg;
    }
    const int i1 = imin(imax(Iu, 1), Lm + 1), i2 = imin(imax(Iu + 1, 1), Lm + 1);           // :428-459
    const int j1 = imin(imax(Jr, 0), Mm + 1), j2 = imin(imax(Jr + 1, 0), Mm + 1);
    const double p2 = (double)(i2 - i1) * (x - (double)i1 + 0.5), q2 = (double)(j2 - j1) * (y - (double)j1);
    const double p1 = 1.0 - p2, q1 = 1.0 - q2;
    s111 = 0.5 * (g.pm[flt_q(g, i1 - 1, j1)] + g.pm[flt_q(g, i1, j1)]);
    s211 = 0.5 * (g.pm[flt_q(g, i2 - 1, j1)] + g.pm[flt_q(g, i2, j1)]);
    s121 = 0.5 * (g.pm[flt_q(g, i1 - 1, j2)] + g.pm[flt_q(g, i1, j2)]);
    s221 = 0.5 * (g.pm[flt_q(g, i2 - 1, j2)] + g.pm[flt_q(g, i2, j2)]);
    s112 = s111;
    s212 = s112;
    s122 = s121;
    s222 = s221;
    return p1 * q1 * r1 * s111 * A3(i1, j1, k1) + p2 * q1 * r1 * s211 * A3(i2, j1, k1) +
           p1 * q2 * r1 * s121 * A3(i1, j2, k1) + p2 * q2 * r1 * s221 * A3(i2, j2, k1) +
           p1 * q1 * r2 * s112 * A3(i1, j1, k2) + p2 * q1 * r2 * s212 * A3(i2, j1, k2) +
           p1 * q2 * r2 * s122 * A3(i1, j2, k2) + p2 * q2 * r2 * s222 * A3(i2, j2, k2) + nudg;
  }
  // v-points
  if (halo) {                                                                               // :475-495
    const int i1 = Irn, j1 = imin(imax(Jv, 1), Mm + 1), j2 = imin(imax(Jv + 1, 1), Mm + 1);
    const double q2 = (double)(j2 - j1) * (y - (double)j1 + 0.5), p1 = 1.0, q1 = 1.0 - q2;
    s111 = 0.5 * (g.pn[flt_q(g, i1, j1 - 1)] + g.pn[flt_q(g, i1, j1)]);
    s121 = 0.5 * (g.pn[flt_q(g, i1, j2 - 1)] + g.pn[flt_q(g, i1, j2)]);
    s112 = s111;
    s122 = s121;
    return p1 * q1 * r1 * s111 * A3(i1, j1, k1) + p1 * q2 * r1 * s121 * A3(i1, j2, k1) +
           p1 * q1 * r2 * s112 * A3(i1, j1, k2) + p1 * q2 * r2 * s122 * A3(i1, j2, k2) + nudg;
  }
  const int i1 = imin(imax(Ir, 0), Lm + 1), i2 = imin(imax(Ir + 1, 1), Lm + 1);             // :501-532
  const int j1 = imin(imax(Jv, 1), Mm + 1), j2 = imin(imax(Jv + 1, 1), Mm + 1);
  const double p2 = (double)(i2 - i1) * (x - (double)i1), q2 = (double)(j2 - j1) * (y - (double)j1 + 0.5);
  const double p1 = 1.0 - p2, q1 = 1.0 - q2;
  s111 = 0.5 * (g.pn[flt_q(g, i1, j1 - 1)] + g.pn[flt_q(g, i1, j1)]);
  s211 = 0.5 * (g.pn[flt_q(g, i2, j1 - 1)] + g.pn[flt_q(g, i2, j1)]);
  s121 = 0.5 * (g.pn[flt_q(g, i1, j2 - 1)] + g.pn[flt_q(g, i1, j2)]);
  s221 = 0.5 * (g.pn[flt_q(g, i2, j2 - 1)] + g.pn[flt_q(g, i2, j2)]);
  s112 = s111;
  s212 = s112;
  s122 = s121;
  s222 = s221;
  return p1 * q1 * r1 * s111 * A3(i1, j1, k1) + p2 * q1 * r1 * s211 * A3(i2, j1, k1) +
         p1 * q2 * r1 * s121 * A3(i1, j2, k1) + p2 * q2 * r1 * s221 * A3(i2, j2, k1) +
         p1 * q1 * r2 * s112 * A3(i1, j1, k2) + p2 * q1 * r2 * s212 * A3(i2, j1, k2) +
         p1 * q2 * r2 * s122 * A3(i1, j2, k2) + p2 * q2 * r2 * s222 * A3(i2, j2, k2) + nudg;
#undef A3
}

// The vertical position of an isobaric or geopotential float at (x, y): the bilinear z_w search from the surface
// down, step_floats.F:280-342 (predictor) = :513-575 (corrector).  *zgrd stays untouched when no level brackets it.
__device__ void flt_zsearch(const FltGrid &g, gcd_t z_w, int ftype, double fz0, double x, double y, double *zgrd)
{
  const int N = g.N, Lm = g.Lm, Mm = g.Mm;
  const int Ir = flt_int(x), Jr = flt_int(y);
  const int i1 = imin(imax(Ir, 0), Lm + 1), i2 = imin(imax(Ir + 1, 1), Lm + 1);
  const int j1 = imin(imax(Jr, 0), Mm + 1), j2 = imin(imax(Jr + 1, 0), Mm + 1);             // MAX(Jr+1,0): as written
  const double p2 = (double)(i2 - i1) * (x - (double)i1), q2 = (double)(j2 - j1) * (y - (double)j1);
  const double p1 = 1.0 - p2, q1 = 1.0 - q2;
  const long c11 = flt_q(g, i1, j1), c21 = flt_q(g, i2, j1), c12 = flt_q(g, i1, j2), c22 = flt_q(g, i2, j2);
  double m11 = 1.0, m21 = 1.0, m12 = 1.0, m22 = 1.0, cff8 = 1.0;
  if (g.masking) {
    m11 = g.rmask[c11]; m21 = g.rmask[c21]; m12 = g.rmask[c12]; m22 = g.rmask[c22];
    cff8 = p1 * q1 * m11 + p2 * q1 * m21 + p1 * q2 * m12 + p2 * q2 * m22;
  }
  auto level = [&](int k) {
    const long o = (long)k * g.nij;
    if (g.masking) {
      const double cff7 = p1 * q1 * z_w[c11 + o] * m11 + p2 * q1 * z_w[c21 + o] * m21 +
                          p1 * q2 * z_w[c12 + o] * m12 + p2 * q2 * z_w[c22 + o] * m22;
      return cff8 > 0.0 ? cff7 / cff8 : 0.0;
    }
    return p1 * q1 * z_w[c11 + o] + p2 * q1 * z_w[c21 + o] + p1 * q2 * z_w[c12 + o] + p2 * q2 * z_w[c22 + o];
  };
  const double cff9 = level(N);
  double cff6 = cff9;
  const double zfloat = ftype == flt_Geopot ? fz0 : fz0 + cff9;
  for (int k = N - 1; k >= 0; k--) {
    const double cff5 = level(k);
    if ((zfloat - cff5) * (cff6 - zfloat) >= 0.0) *zgrd = (double)k + (zfloat - cff5) / (cff6 - cff5);
    cff6 = cff5;
  }
}

// phase 0 = the whole routine; with E-W periodicity on more than one tile column the reference collects in the
// middle (:604-627): phase 1 = up to the periodic shift, phase 2 = from the second ownership test on
__global__ void __launch_bounds__(64) k_floats(const RomsDev *__restrict__ c, FltArgs a)
{
  const int l = blockIdx.x * 64 + threadIdx.x;
  if (l >= a.n) return;
  const roms_bounds_t &b = c->b;
  FltGrid g;
  g.LBi = b.LBi; g.UBi = b.UBi; g.LBj = b.LBj; g.UBj = b.UBj; g.Lm = b.Lm; g.Mm = b.Mm; g.N = b.N;
  g.ni = b.UBi - b.LBi + 1;
  g.nij = g.ni * (long)(b.UBj - b.LBj + 1);
  g.masking = c->p.masking != 0;
  g.ewp = b.EWperiodic != 0;
  g.pm = (gcd_t)c->F.pm; g.pn = (gcd_t)c->F.pn; g.Hz = (gcd_t)c->F.Hz; g.rmask = (gcd_t)c->F.rmask;
  const int N = b.N, NT = b.NT, Lm = b.Lm, Mm = b.Mm;
  const long n3r = g.nij * N;
  const int nfm3 = a.nfm3, nfm2 = a.nfm2, nfm1 = a.nfm1, nf = a.nf, nfp1 = a.nfp1;
  const double dt = c->p.dt;
  const double spval = 1.0e37, Fspv = 0.0;
  const bool Lmask = true, Gmask = false;               // interp_floats itself drops maskit without MASKING
  double *__restrict__ trk = a.trk;
#define TR(v, lev) trk[((long)(lev) * a.NFV + ((v) - 1)) * a.n + l]
  bool bounded = a.bounded[l] != 0;
  const int ftype = a.Ftype[l];
  const double *Ti = a.Tinfo + (long)NTINFO * l;
  const double Xstr = (double)b.Istr - 0.5, Xend = (double)b.Iend + 0.5;
  const double Ystr = (double)b.Jstr - 0.5, Yend = (double)b.Jend + 0.5;
  // the ownership switch, :191-207 with the position at level nf, :609-625 with the one at nfp1
  auto own = [&](int lev) {
    const double x = TR(ixgrd, lev), y = TR(iygrd, lev);
    if (Xstr <= x && x < Xend && Ystr <= y && y < Yend) return true;
    if (a.master && !bounded) return true;
    for (int j = 0; j <= NFT; j++)
      for (int i = 1; i <= a.NFV; i++) TR(i, j) = Fspv;
    return false;
  };
  gcd_t u = (gcd_t)c->F.u + n3r * (a.nnew - 1), v = (gcd_t)c->F.v + n3r * (a.nnew - 1), W = (gcd_t)c->F.W;
  auto slopes = [&](bool mine) {                         // :353-389 = :755-791
    if (!mine) return;
    if (!bounded) { TR(ixrhs, nfp1) = spval; TR(iyrhs, nfp1) = spval; TR(izrhs, nfp1) = spval; return; }
    const double x = TR(ixgrd, nfp1), y = TR(iygrd, nfp1), z = TR(izgrd, nfp1);
    TR(ixrhs, nfp1) = flt_interp<FG_NU3D>(g, u, Lmask, x, y, z);
    TR(iyrhs, nfp1) = flt_interp<FG_NV3D>(g, v, Lmask, x, y, z);
    TR(izrhs, nfp1) = flt_interp<FG_NW3D>(g, W, Lmask, x, y, z);
  };
  bool mine;
  if (a.phase != 2) {
    mine = own(nf);
    // Milne predictor, :238-346
    {
      const double cff1 = 8.0 / 3.0, cff2 = 4.0 / 3.0;
      if (mine && bounded) {
        TR(ixgrd, nfp1) = TR(ixgrd, nfm3) + dt * (cff1 * TR(ixrhs, nf) - cff2 * TR(ixrhs, nfm1) + cff1 * TR(ixrhs, nfm2));
        TR(iygrd, nfp1) = TR(iygrd, nfm3) + dt * (cff1 * TR(iyrhs, nf) - cff2 * TR(iyrhs, nfm1) + cff1 * TR(iyrhs, nfm2));
        if (ftype == flt_Lagran) {
          TR(izgrd, nfp1) = TR(izgrd, nfm3) + dt * (cff1 * TR(izrhs, nf) - cff2 * TR(izrhs, nfm1) + cff1 * TR(izrhs, nfm2));
        } else if (ftype == flt_Isobar || ftype == flt_Geopot) {
          double z = TR(izgrd, nfp1);
          flt_zsearch(g, (gcd_t)c->F.z_w, ftype, a.Fz0[l], TR(ixgrd, nfp1), TR(iygrd, nfp1), &z);
          TR(izgrd, nfp1) = z;
        }
      }
    }
    slopes(mine);
    // Hamming corrector, :465-579
    {
      const double cff1 = 9.0 / 8.0, cff2 = 1.0 / 8.0, cff3 = 3.0 / 8.0, cff4 = 6.0 / 8.0;
      if (mine && bounded) {
        TR(ixgrd, nfp1) = cff1 * TR(ixgrd, nf) - cff2 * TR(ixgrd, nfm2) +
                          dt * (cff3 * TR(ixrhs, nfp1) + cff4 * TR(ixrhs, nf) - cff3 * TR(ixrhs, nfm1));
        TR(iygrd, nfp1) = cff1 * TR(iygrd, nf) - cff2 * TR(iygrd, nfm2) +
                          dt * (cff3 * TR(iyrhs, nfp1) + cff4 * TR(iyrhs, nf) - cff3 * TR(iyrhs, nfm1));
        if (ftype == flt_Lagran) {
          TR(izgrd, nfp1) = cff1 * TR(izgrd, nf) - cff2 * TR(izgrd, nfm2) +
                            dt * (cff3 * TR(izrhs, nfp1) + cff4 * TR(izrhs, nf) - cff3 * TR(izrhs, nfm1));
        } else if (ftype == flt_Isobar || ftype == flt_Geopot) {
          double z = TR(izgrd, nfp1);
          flt_zsearch(g, (gcd_t)c->F.z_w, ftype, a.Fz0[l], TR(ixgrd, nfp1), TR(iygrd, nfp1), &z);
          TR(izgrd, nfp1) = z;
        }
      }
    }
    // float status in xi, :585-637
    if (g.ewp) {
      const double cff1 = (double)Lm;
      if (mine && bounded) {
        if (TR(ixgrd, nfp1) >= (double)(Lm + 1) - 0.5) {
          TR(ixgrd, nfp1) = TR(ixgrd, nfp1) - cff1;
          TR(ixgrd, nf) = TR(ixgrd, nf) - cff1;
          TR(ixgrd, nfm1) = TR(ixgrd, nfm1) - cff1;
          TR(ixgrd, nfm2) = TR(ixgrd, nfm2) - cff1;
          TR(ixgrd, nfm3) = TR(ixgrd, nfm3) - cff1;
        } else if (TR(ixgrd, nfp1) < 0.5) {
          TR(ixgrd, nfp1) = cff1 + TR(ixgrd, nfp1);
          TR(ixgrd, nf) = cff1 + TR(ixgrd, nf);
          TR(ixgrd, nfm1) = cff1 + TR(ixgrd, nfm1);
          TR(ixgrd, nfm2) = cff1 + TR(ixgrd, nfm2);
          TR(ixgrd, nfm3) = cff1 + TR(ixgrd, nfm3);
        }
      }
    } else if (mine && bounded) {
      if (TR(ixgrd, nfp1) >= (double)(Lm + 1) - 0.5 || TR(ixgrd, nfp1) < 0.5) bounded = false;
    }
    if (a.phase == 1) return;                            // bounded cannot have changed: E-W periodic
  } else {
    mine = own(nfp1);                                    // :609-625, after the collection
  }
  // float status in eta (N-S periodic grids are not built), :682-691
  if (mine && bounded) {
    if (TR(iygrd, nfp1) >= (double)(Mm + 1) - 0.5 || TR(iygrd, nfp1) < 0.5) bounded = false;
  }
  // release, :698-748
  const double HalfDT = 0.5 * dt;
  const bool window = a.time - HalfDT <= Ti[itstr] && a.time + HalfDT > Ti[itstr];
  if (!bounded && window) {
    bounded = true;
    if (Ti[ixgrd] < 0.5 || Ti[iygrd] < 0.5 || Ti[ixgrd] > (double)Lm + 0.5 || Ti[iygrd] > (double)Mm + 0.5)
      bounded = false;                                   // outside application grid
    if (Xstr <= Ti[ixgrd] && Ti[ixgrd] < Xend && Ystr <= Ti[iygrd] && Ti[iygrd] < Yend && bounded) {
      for (int j = 0; j <= NFT; j++) {
        TR(ixgrd, j) = Ti[ixgrd];
        TR(iygrd, j) = Ti[iygrd];
        TR(izgrd, j) = Ti[izgrd];
      }
      mine = true;
    } else {
      mine = false;
      for (int j = 0; j <= NFT; j++)
        for (int i = 1; i <= a.NFV; i++) TR(i, j) = Fspv;
    }
  }
  // slopes at the corrected position, :755-791; newly released floats: the same slopes at all levels, :836-859
  slopes(mine);
  if (mine && bounded && window) {
    const double xrhs = TR(ixrhs, nfp1), yrhs = TR(iyrhs, nfp1), zrhs = TR(izrhs, nfp1);
    for (int i = 0; i <= NFT; i++) {
      TR(ixrhs, i) = xrhs;
      TR(iyrhs, i) = yrhs;
      TR(izrhs, i) = zrhs;
    }
  }
  // outputs at the corrected position, :865-960
  if (mine) {
    if (!bounded) {
      TR(iflon, nfp1) = spval; TR(iflat, nfp1) = spval; TR(idpth, nfp1) = spval; TR(ifden, nfp1) = spval;
      for (int itrc = 1; itrc <= NT; itrc++) TR(ifden + itrc, nfp1) = spval;
    } else {
      const double x = TR(ixgrd, nfp1), y = TR(iygrd, nfp1), z = TR(izgrd, nfp1);
      TR(iflon, nfp1) = flt_interp<FG_R2D>(g, (gcd_t)a.xc, Gmask, x, y, z);
      TR(iflat, nfp1) = flt_interp<FG_R2D>(g, (gcd_t)a.yc, Gmask, x, y, z);
      TR(idpth, nfp1) = flt_interp<FG_W3D>(g, (gcd_t)c->F.z_w, Lmask, x, y, z);
      TR(ifden, nfp1) = flt_interp<FG_R3D>(g, (gcd_t)c->F.rho, Lmask, x, y, z);
      for (int itrc = 1; itrc <= NT; itrc++)                                        // ifTvar(itrc) = 10 + itrc
        TR(ifden + itrc, nfp1) = flt_interp<FG_R3D>(g, (gcd_t)c->F.t + n3r * ((a.nnew - 1) + 3L * (itrc - 1)), Lmask, x, y, z);
    }
  }
  // reflection at the surface and at the bottom, :1009-1021 (the reference negates the whole row NFT+1 times: an odd
  // number, so once)
  if (mine && bounded) {
    if (TR(izgrd, nfp1) > (double)N) {
      for (int j = 0; j <= NFT; j++) TR(izgrd, j) = 2.0 * (double)N - TR(izgrd, j);
    } else if (TR(izgrd, nfp1) < 0.0) {
      for (int j = 0; j <= NFT; j++) TR(izgrd, j) = -TR(izgrd, j);
    }
  }
  a.bounded[l] = bounded ? 1 : 0;
  trk[(long)(NFT + 1) * a.NFV * a.n + l] = bounded ? 1.0 : Fspv;                       // :1036-1041
#undef TR
}

// :1043-1049 after the SUM
__global__ void __launch_bounds__(64) k_floats_bounded(const double *__restrict__ Fwrk, int *__restrict__ bounded, int n)
{
  const int l = blockIdx.x * 64 + threadIdx.x;
  if (l < n) bounded[l] = Fwrk[l] != 0.0 ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ the C ABI --
// (roms_hip_set_bounds: the floats' coordinate arrays have the old extents)
void floats_release()
{
  if (g_flt.trk) (void)hipFree(g_flt.trk);
  if (g_flt.ibuf) (void)hipFree(g_flt.ibuf);
  if (g_flt.dbuf) (void)hipFree(g_flt.dbuf);
  if (g_flt.xc_base) (void)hipFree(g_flt.xc_base);
  if (g_flt.yc_base) (void)hipFree(g_flt.yc_base);
  g_flt = FltStore{};
}

static long flt_track_count() { return (long)(NFT + 1) * g_flt.NFV * g_flt.n; }

extern "C" int roms_hip_set_floats(int Nfloats, const int *Ftype, const double *Tinfo, const double *Fz0,
                                   const double *xcoord, const double *ycoord)
{
  const char *me = "roms_hip_set_floats";
  if (int rc = roms_setup_check(me)) return rc;
  if (Nfloats < 0) return roms_fail(me, "floats: Nfloats < 0");
  if (Nfloats == 0) {
    if (g_flt.n) HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    floats_release();
    return 0;
  }
  if (!Ftype || !Tinfo || !Fz0 || !xcoord || !ycoord) return roms_fail(me, "floats: null argument");
  const roms_bounds_t &b = g_ctx.b;
  if (b.NSperiodic) return roms_fail(me, "floats: N-S periodic grids are not built");
  for (int l = 0; l < Nfloats; l++)
    if (Ftype[l] < flt_Lagran || Ftype[l] > flt_Geopot) {
      char msg[160];
      snprintf(msg, sizeof msg, "floats: Ftype(%d) = %d is outside 1..3 (flt_Lagran, flt_Isobar, flt_Geopot)", l + 1, Ftype[l]);
      return roms_fail(me, msg);
    }
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  floats_release();
  const long nij = (long)(b.UBi - b.LBi + 1) * (long)(b.UBj - b.LBj + 1);
  const int NFV = b.NT + 10;
  const size_t ntrk = ((size_t)(NFT + 1) * NFV + 1) * Nfloats;
  const long g = g_ctx.guard;
  auto fail = [&](const char *what) { floats_release(); return roms_fail(me, what); };
  if (hipMalloc(&g_flt.trk, sizeof(double) * ntrk) != hipSuccess) return fail("floats: hipMalloc failed");
  if (hipMalloc(&g_flt.ibuf, sizeof(int) * 2 * (size_t)Nfloats) != hipSuccess) return fail("floats: hipMalloc failed");
  if (hipMalloc(&g_flt.dbuf, sizeof(double) * (NTINFO + 1) * (size_t)Nfloats) != hipSuccess) return fail("floats: hipMalloc failed");
  // the coordinate arrays are gathered like fields: the same slack in front and behind
  if (hipMalloc(&g_flt.xc_base, sizeof(double) * (nij + 2 * g)) != hipSuccess) return fail("floats: hipMalloc failed");
  if (hipMalloc(&g_flt.yc_base, sizeof(double) * (nij + 2 * g)) != hipSuccess) return fail("floats: hipMalloc failed");
  g_flt.xc = g_flt.xc_base + g;
  g_flt.yc = g_flt.yc_base + g;
  g_flt.n = Nfloats; g_flt.NFV = NFV; g_flt.nij = nij;
  hipStream_t st = g_ctx.stream;
  HIP_TRY(hipMemsetAsync(g_flt.trk, 0, sizeof(double) * ntrk, st));                    // track and bounded zero-filled
  HIP_TRY(hipMemsetAsync(g_flt.ibuf, 0, sizeof(int) * 2 * (size_t)Nfloats, st));
  HIP_TRY(hipMemsetAsync(g_flt.xc_base, 0, sizeof(double) * (nij + 2 * g), st));
  HIP_TRY(hipMemsetAsync(g_flt.yc_base, 0, sizeof(double) * (nij + 2 * g), st));
  HIP_TRY(hipMemcpyAsync(g_flt.ibuf + Nfloats, Ftype, sizeof(int) * Nfloats, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(g_flt.dbuf, Tinfo, sizeof(double) * NTINFO * (size_t)Nfloats, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(g_flt.dbuf + NTINFO * (size_t)Nfloats, Fz0, sizeof(double) * Nfloats, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(g_flt.xc, xcoord, sizeof(double) * nij, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(g_flt.yc, ycoord, sizeof(double) * nij, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

// host order track(NFV,0:NFT,Nfloats) <-> device order [lev][v][l]
static int flt_transfer(const char *me, double *track, long n_track, int *bounded, long n_bounded, bool put)
{
  if (!g_ctx.inited) return roms_fail(me, "library not initialised");
  if (!g_flt.n) return roms_fail(me, "floats: none set (roms_hip_set_floats)");
  if (!track || !bounded) return roms_fail(me, "floats: null argument");
  if (n_track != flt_track_count() || n_bounded != g_flt.n) {
    char msg[200];
    snprintf(msg, sizeof msg, "floats: track has %ld doubles and bounded %d entries, the host arrays %ld and %ld",
             flt_track_count(), g_flt.n, n_track, n_bounded);
    return roms_fail(me, msg);
  }
  const int n = g_flt.n, NFV = g_flt.NFV;
  std::vector<double> tmp((size_t)n_track);
  std::vector<int> ib((size_t)n);
  if (put) {
    for (int l = 0; l < n; l++)
      for (int lev = 0; lev <= NFT; lev++)
        for (int v = 0; v < NFV; v++) tmp[((size_t)lev * NFV + v) * n + l] = track[v + (size_t)NFV * (lev + (size_t)(NFT + 1) * l)];
    for (int l = 0; l < n; l++) ib[l] = bounded[l] != 0;
    HIP_TRY(hipMemcpyAsync(g_flt.trk, tmp.data(), sizeof(double) * n_track, hipMemcpyHostToDevice, g_ctx.stream));
    HIP_TRY(hipMemcpyAsync(g_flt.ibuf, ib.data(), sizeof(int) * n, hipMemcpyHostToDevice, g_ctx.stream));
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    return 0;
  }
  HIP_TRY(hipMemcpyAsync(tmp.data(), g_flt.trk, sizeof(double) * n_track, hipMemcpyDeviceToHost, g_ctx.stream));
  HIP_TRY(hipMemcpyAsync(ib.data(), g_flt.ibuf, sizeof(int) * n, hipMemcpyDeviceToHost, g_ctx.stream));
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  for (int l = 0; l < n; l++)
    for (int lev = 0; lev <= NFT; lev++)
      for (int v = 0; v < NFV; v++) track[v + (size_t)NFV * (lev + (size_t)(NFT + 1) * l)] = tmp[((size_t)lev * NFV + v) * n + l];
  for (int l = 0; l < n; l++) bounded[l] = ib[l];
  return 0;
}

extern "C" int roms_hip_floats_put(const double *track, long n_track, const int *bounded, long n_bounded)
{
  return flt_transfer("roms_hip_floats_put", const_cast<double *>(track), n_track, const_cast<int *>(bounded), n_bounded, true);
}

extern "C" int roms_hip_floats_get(double *track, long n_track, int *bounded, long n_bounded)
{
  return flt_transfer("roms_hip_floats_get", track, n_track, bounded, n_bounded, false);
}

extern "C" int roms_hip_step_floats(const roms_step_idx_t *s, double time, const int nfl[5])
{
  const char *me = "roms_hip_step_floats";
  if (!s || !nfl) return roms_fail(me, "null argument");
  {
    int seen = 0;
    for (int q = 0; q < 5; q++)
      if (nfl[q] >= 0 && nfl[q] <= NFT) seen |= 1 << nfl[q];
    if (seen != 31) return roms_fail(me, "floats: nfl = {nfm3, nfm2, nfm1, nf, nfp1} is not a permutation of 0..4");
  }
  if (!g_flt.n) return 0;                                  // no roms_hip_set_floats, or Nfloats = 0
  int rc = roms_entry_check(me);
  if (rc) return rc;
  if (s->nnew < 1 || s->nnew > 2) return roms_fail(me, "floats: nnew outside 1..2");
  const roms_bounds_t &b = g_ctx.b;
  if (b.NSperiodic) return roms_fail(me, "floats: N-S periodic grids are not built");
  if (b.NT + 10 != g_flt.NFV || (long)(b.UBi - b.LBi + 1) * (long)(b.UBj - b.LBj + 1) != g_flt.nij)
    return roms_fail(me, "floats: the bounds changed after roms_hip_set_floats");
  ScopedTimer tm("step_floats");
  FltArgs a;
  a.n = g_flt.n; a.NFV = g_flt.NFV; a.nnew = s->nnew; a.master = g_ctx.rank == 0;
  a.nfm3 = nfl[0]; a.nfm2 = nfl[1]; a.nfm1 = nfl[2]; a.nf = nfl[3]; a.nfp1 = nfl[4];
  a.time = time;
  a.trk = g_flt.trk; a.bounded = g_flt.ibuf; a.Ftype = g_flt.ibuf + g_flt.n;
  a.Tinfo = g_flt.dbuf; a.Fz0 = g_flt.dbuf + (size_t)NTINFO * g_flt.n;
  a.xc = g_flt.xc; a.yc = g_flt.yc;
  const dim3 grid((unsigned)((a.n + 63) / 64)), blk(64);
  const bool tiled = b.ntileI * b.ntileJ > 1 || g_ctx.loopback;
  const bool mid = tiled && b.EWperiodic && (b.ntileI > 1 || g_ctx.loopback);              // :605
  if (mid) {
    a.phase = 1;
    hipLaunchKernelGGL(k_floats, grid, blk, 0, g_ctx.stream, g_ctx.devc, a);
    KERNEL_CHECK("k_floats");
    rc = halo_allreduce_sum(g_flt.trk, flt_track_count());
    if (rc) return rc;
    a.phase = 2;
  } else {
    a.phase = 0;
  }
  hipLaunchKernelGGL(k_floats, grid, blk, 0, g_ctx.stream, g_ctx.devc, a);
  KERNEL_CHECK("k_floats");
  if (tiled) {                                           // :1030-1049: track and the bounded switch in one message
    rc = halo_allreduce_sum(g_flt.trk, flt_track_count() + a.n);
    if (rc) return rc;
    hipLaunchKernelGGL(k_floats_bounded, grid, blk, 0, g_ctx.stream, (const double *)(g_flt.trk + flt_track_count()),
                       g_flt.ibuf, a.n);
    KERNEL_CHECK("k_floats_bounded");
  }
  return 0;
}
