// step2d_common.h -- what k_step2d.hip and k_step2d_mom.hip share: the launch descriptor of a step2d call and the
// point formulas of step2d_LF_AM3.h that more than one kernel evaluates, each written once as a function of VALUES
// (no loads inside: the fused kernel requests its inputs before its first barrier, the split kernels load where
// they stand).
#pragma once
#include "roms_dev.h"

struct S2 {
  int krhs, kstp, knew, nstp, nnew, iif, iic, ntfirst, predictor;
  int ew_images;   // 1 = one tile, E-W periodic: the tiles are staged through the periodic wrap and the thread that
                   // owns a column next to the seam also stores its periodic images (columns Lm+1.. and ..0)
};

// how step2d_impl calls the momentum kernel
enum class K2dLaunch {
  FusedOneTile,    // free surface, fast-time averages and momentum; DUon/DVom evaluated in place (S2::ew_images set)
  FusedTiles,      // the same on several tiles: exchanged DUon/DVom in, the next call's fluxes out (DUnext/DVnext)
  Split            // momentum only: zeta_new, zwrk and the exchanged fluxes come from k2d_flux / k2d_zeta
};
int roms_launch_k2d_mom_lds(const S2 &s, K2dLaunch mode, const double *DUon, const double *DVom,
                            const double *zeta_new, const double *zwrk, double *DUnext, double *DVnext);

__device__ __forceinline__ int wrap_i(const roms_bounds_t &b, int i)
{
  return (i < 1) ? i + b.Lm : ((i > b.Lm) ? i - b.Lm : i);
}

// DUon / DVom, :509-544: the transport through a u / v face from the velocity there, the face's width and the total
// depths D = zeta + h of the two cells it separates
__device__ __forceinline__ double flux_u(const double ubar, const double on_u, const double D, const double D_west)
{
  return ubar * ((0.5 * on_u) * (D + D_west));
}
__device__ __forceinline__ double flux_v(const double vbar, const double om_v, const double D, const double D_south)
{
  return vbar * ((0.5 * om_v) * (D + D_south));
}

// One free-surface point, :770-868: the new free surface zn and the time-weighted zw the pressure gradient uses.
// zs_a = zeta(kstp), zk_a = zeta(krhs), rz_k / rz_p = rzeta(kstp) / rzeta(3-kstp) (read by the corrector after the
// first step only), rm = rmask (read under MASKING only)
__device__ __forceinline__ void zeta_step(const roms_params_t &p, const S2 &s, const double rhs, const double pm_a,
                                          const double pn_a, const double zs_a, const double zk_a, const double rz_k,
                                          const double rz_p, const double rm, const bool masking, double &zn,
                                          double &zw)
{
  const double dtfast = p.dtfast;
  if (s.iif == 1) {
    const double cff1 = dtfast;
    zn = zs_a + pm_a * pn_a * cff1 * rhs;
    if (masking) zn = zn * rm;                                    // MASKING, :778
    zw = 0.5 * (zs_a + zn);
  } else if (s.predictor) {
    const double cff1 = 2.0 * dtfast;
    const double cff4 = 4.0 / 25.0;
    const double cff5 = 1.0 - 2.0 * cff4;
    zn = zs_a + pm_a * pn_a * cff1 * rhs;
    if (masking) zn = zn * rm;                                    // :804
    zw = cff5 * zk_a + cff4 * (zs_a + zn);
  } else {
    const double cff1 = dtfast * 5.0 / 12.0;
    const double cff2 = dtfast * 8.0 / 12.0;
    const double cff3 = dtfast * 1.0 / 12.0;
    const double cff4 = 2.0 / 5.0;
    const double cff5 = 1.0 - cff4;
    const double cff = cff1 * rhs;
    zn = zs_a + pm_a * pn_a * (cff + cff2 * rz_k - cff3 * rz_p);
    if (masking) zn = zn * rm;                                    // :835
    zw = cff5 * zn + cff4 * zk_a;
  }
}

// Fast-time averaging of one point, :614-682.  The running sums of a step: the first predictor of the loop starts
// them (it reads none of the old ones), the later predictors add to all five, a corrector to DU_avg2 / DV_avg2 only.
struct FastAvg {
  double Zt1, DU1, DU2, DV1, DV2;
};
__device__ __forceinline__ bool avg_reads_sums1(const S2 &s) { return s.predictor && s.iif != 1; }   // Zt, DU, DV_avg1
__device__ __forceinline__ bool avg_reads_sums2(const S2 &s) { return !(s.predictor && s.iif == 1); } // DU, DV_avg2
__device__ __forceinline__ bool avg_stores_sums1(const S2 &s) { return s.predictor != 0; }            // _avg2: always
// old = the sums so far (only what avg_reads_* names is looked at), zk_a = zeta(krhs) (predictors after the first)
__device__ __forceinline__ FastAvg fast_average(const roms_params_t &p, const S2 &s, const FastAvg &old,
                                                const double DUon, const double DVom, const double zk_a)
{
  const int iif = s.iif;
  if (s.predictor && iif == 1) {
    const double cff2 = (-1.0 / 12.0) * p.weight2[iif];
    return FastAvg{0.0, 0.0, cff2 * DUon, 0.0, cff2 * DVom};
  }
  if (s.predictor) {
    const double cff1 = p.weight1[iif - 2];
    const double cff2 = (8.0 / 12.0) * p.weight2[iif - 1] - (1.0 / 12.0) * p.weight2[iif];
    return FastAvg{old.Zt1 + cff1 * zk_a, old.DU1 + cff1 * DUon, old.DU2 + cff2 * DUon, old.DV1 + cff1 * DVom,
                   old.DV2 + cff2 * DVom};
  }
  const double cff2 = (iif == 1) ? p.weight2[iif - 1] : (5.0 / 12.0) * p.weight2[iif - 1];
  return FastAvg{old.Zt1, old.DU1, old.DU2 + cff2 * DUon, old.DV1, old.DV2 + cff2 * DVom};
}
// The new sums of point o go to the shared arrays; inU / inV: o is a u / v point of the averaging range too
__device__ __forceinline__ void store_average(const RomsDev *__restrict__ c, const S2 &s, const long o, const bool inU,
                                              const bool inV, const FastAvg &n)
{
  if (avg_stores_sums1(s)) {
    GF(Zt_avg1)[o] = n.Zt1;
    if (inU) GF(DU_avg1)[o] = n.DU1;
    if (inV) GF(DV_avg1)[o] = n.DV1;
  }
  if (inU) GF(DU_avg2)[o] = n.DU2;
  if (inV) GF(DV_avg2)[o] = n.DV2;
}
// Averaging of point o with the old sums read where they stand (kernels that did not request them earlier)
__device__ __forceinline__ void average_point(const RomsDev *__restrict__ c, const S2 &s, const long o, const bool inU,
                                              const bool inV, const double DUon, const double DVom, const long nij)
{
  FastAvg old{0.0, 0.0, 0.0, 0.0, 0.0};
  double zk_a = 0.0;
  if (avg_reads_sums1(s)) {
    old.Zt1 = GF(Zt_avg1)[o];
    zk_a = ((gcd_t)(c->F.zeta + (long)(s.krhs - 1) * nij))[o];
    if (inU) old.DU1 = GF(DU_avg1)[o];
    if (inV) old.DV1 = GF(DV_avg1)[o];
  }
  if (avg_reads_sums2(s)) {
    if (inU) old.DU2 = GF(DU_avg2)[o];
    if (inV) old.DV2 = GF(DV_avg2)[o];
  }
  store_average(c, s, o, inU, inV, fast_average(c->p, s, old, DUon, DVom, zk_a));
}
