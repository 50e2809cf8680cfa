// bio_sink.h -- the vertical sinking every ROMS ecosystem model and the sediment settling share: a column of grid-box
// averages is reconstructed as parabolic segments (PPM limiter, WENO reconciliation of the interface values, a second
// limiter) and moved by a semi-Lagrangian flux that is free of a CFL limit, because the departure point of an interface
// may lie any number of cells above it.  Restated from ROMS/Nonlinear/Biology/npzd_Powell.h:460-630 (the same text
// stands in fennel.h, npzd_Franks.h, npzd_iron.h, nemuro.h and sed_settling.F) in the reference's operation order,
// with the default (strictly monotone) end conditions :535-537, :546-548; LINEAR_CONTINUATION and NEUMANN are not
// built.  The bottom is open: FC(0) leaves the column, as the reference has it; FC(N) = 0.
//
// Where the column lives.  The reference holds qc, bL, bR, WL, WR, FC and ksource per column (7 N numbers).  Here:
//   * the constituent itself is ONE column in LDS, updated in place: cell k-1 gets its new value as soon as FC(k-1) is
//     known, and no later flux reads a cell below its own interface (ksource(k) >= k);
//   * the reconstruction runs as one ascending sweep over a register window (the slopes and the PPM result of the
//     cell below wait one level for the reconciliation with the cell above), and only the finished bL, bR go to
//     memory: two 3-D scratch slots, one double per lane along i;
//   * WL, WR, ksource and FC are scalars of the flux sweep (FC(k-2) waits in a register for the update of cell k-1).
// The departure cell is looked for upwards from k and the search stops at the first interface at or above the
// departure point; the reference tests every interface up to N-1, which is the same thing for z_w increasing with k.
#pragma once
#include "roms_dev.h"

// PPM of one cell, npzd_Powell.h:481-514: the slopes FCm = FC(k-1), FCk = FC(k) towards the cells below and above,
// the thicknesses of the three cells; bR, bL: the side values, WR, WL: the measures of quadratic variation
struct BioPpm { double bR, bL, WR, WL; };
__device__ __forceinline__ BioPpm bio_ppm(double q0, double FCm, double FCk, double hm, double h0, double hp)
{
  double dltR = h0 * FCk, dltL = h0 * FCm;
  double cff = hm + 2.0 * h0 + hp;
  const double cffR = cff * FCk, cffL = cff * FCm;
  if (dltR * dltL <= 0.0) {
    dltR = 0.0;
    dltL = 0.0;
  } else if (fabs(dltR) > fabs(cffL)) {
    dltR = cffL;
  } else if (fabs(dltL) > fabs(cffR)) {
    dltL = cffR;
  }
  const double Hz_inv3 = 1.0 / (hm + h0 + hp);
  cff = (dltR - dltL) * Hz_inv3;
  dltR = dltR - cff * hp;
  dltL = dltL + cff * hm;
  BioPpm r;
  r.bR = q0 + dltR;
  r.bL = q0 - dltL;
  const double a = 2.0 * dltR - dltL, b = dltR - 2.0 * dltL;
  r.WR = a * a;
  r.WL = b * b;
  return r;
}

// the second monotonicity constraint, npzd_Powell.h:556-573, on the reconciled side values of a cell of average q0
__device__ __forceinline__ void bio_limit2(double q0, double &bR, double &bL)
{
  double dltR = bR - q0, dltL = q0 - bL;
  const double cffR = 2.0 * dltR, cffL = 2.0 * dltL;
  if (dltR * dltL < 0.0) {
    dltR = 0.0;
    dltL = 0.0;
  } else if (fabs(dltR) > fabs(cffL)) {
    dltR = cffL;
  } else if (fabs(dltL) > fabs(cffR)) {
    dltL = cffR;
  }
  bR = q0 + dltR;
  bL = q0 - dltL;
}

// One column, N >= 4 levels (N <= NMAX).  Hz, z_w: the arrays of the grid, a = the column's 2-D index, nij = the points
// of a plane; q: the column of the constituent in LDS, level k at q[(k - 1) * QS], replaced by the new column; bLa,
// bRa: two 3-D scratch arrays (rho-levels); cff = dtdays * |w|.  Returns FC(0), what left through the bottom.
template <int NMAX, int QS>
__device__ __forceinline__ double sink_column(gcd_t Hz, gcd_t z_w, long a, long nij, int N, double *__restrict__ q, gd_t bLa,
                                              gd_t bRa, double cff)
{
  auto r3 = [&](int k) { return a + (long)(k - 1) * nij; };      // rho-type level k = 1..N
  auto w3 = [&](int k) { return a + (long)k * nij; };            // W-type level k = 0..N
  // ---------- reconstruction, :468-573 ----------
  {
    const double q1 = q[0], qN = q[(N - 1) * QS];
    bLa[r3(1)] = q1;                                             // :546-548 and :535-536: the bottom and the top cell are
    bRa[r3(1)] = q1;                                             // piecewise constant (the second limiter leaves them so)
    bLa[r3(N)] = qN;
    bRa[r3(N)] = qN;
    double hm = Hz[r3(1)], h0 = Hz[r3(2)], qm = q1, q0 = q[QS];
    double FCm = (q0 - qm) * (1.0 / (hm + h0));                  // FC(1), :476
    BioPpm P1{0.0, 0.0, 0.0, 0.0};
    double qP1 = 0.0;
#pragma unroll 1
    for (int k = 2; k <= N - 1; k++) {
      const double hp = Hz[r3(k + 1)], qp = q[k * QS];
      const double FCk = (qp - q0) * (1.0 / (h0 + hp));
      BioPpm P0 = bio_ppm(q0, FCm, FCk, hm, h0, hp);
      if (k >= 3) {
        // WENO reconciliation of the interface between k-1 and k (:517-525, index k-1 in 2 .. N-2), then cell k-1 is
        // finished: the end condition bL(2) = qc(1) (:546), the second limiter
        const double dltL = fmax(1.0E-14, P1.WL), dltR = fmax(1.0E-14, P0.WR);
        P1.bR = (dltR * P1.bR + dltL * P0.bL) / (dltR + dltL);
        P0.bL = P1.bR;
        if (k == 3) P1.bL = q1;
        bio_limit2(qP1, P1.bR, P1.bL);
        bLa[r3(k - 1)] = P1.bL;
        bRa[r3(k - 1)] = P1.bR;
      }
      P1 = P0;
      qP1 = q0;
      hm = h0; h0 = hp; qm = q0; q0 = qp; FCm = FCk;
    }
    // cell N-1: bR(N-1) = qc(N) (:537); with N = 3 it would also be cell 2 (the launcher refuses N < 4)
    P1.bR = qN;
    bio_limit2(qP1, P1.bR, P1.bL);
    bLa[r3(N - 1)] = P1.bL;
    bRa[r3(N - 1)] = P1.bR;
  }
  // ---------- semi-Lagrangian flux and update, :589-628 ----------
  double FC0 = 0.0, FCprev = 0.0;
#pragma unroll 1
  for (int k = 1; k <= N; k++) {
    const double WL = z_w[w3(k - 1)] + cff;                      // the departure point of interface k-1
    double FC = 0.0;
    int ks = k;
#pragma unroll 1
    for (int m = k; m <= N - 1; m++) {                           // whole cells below it, summed upwards from k
      if (!(WL > z_w[w3(m)])) break;
      ks = m + 1;
      FC = FC + Hz[r3(m)] * q[(m - 1) * QS];
    }
    const double hs = Hz[r3(ks)], qs = q[(ks - 1) * QS], bl = bLa[r3(ks)], br = bRa[r3(ks)];
    const double cu = fmin(1.0, (WL - z_w[w3(ks - 1)]) * (1.0 / hs));
    FC = FC + hs * cu * (bl + cu * (0.5 * (br - bl) - (1.5 - cu) * (br + bl - 2.0 * qs)));
    if (k == 1) FC0 = FC;
    else q[(k - 2) * QS] = q[(k - 2) * QS] + (FC - FCprev) * (1.0 / Hz[r3(k - 1)]);   // cell k-1: FC(k-1) - FC(k-2)
    FCprev = FC;
  }
  q[(N - 1) * QS] = q[(N - 1) * QS] + (0.0 - FCprev) * (1.0 / Hz[r3(N)]);               // FC(N) = 0: no flux through the surface
  return FC0;
}
