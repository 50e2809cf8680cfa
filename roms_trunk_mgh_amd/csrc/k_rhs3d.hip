// k_rhs3d.hip -- right-hand side of the 3-D momentum equations, rhs3d_tile
// (ROMS/Nonlinear/rhs3d.F:174-1673): Coriolis (:467-505), curvilinear metric
// terms (:509-560), third-order upstream-biased horizontal advection
// (UV_U3HADVECTION, :596-982), fourth-order centred vertical advection
// (:1009-1260) and the vertical integral rufrc/rvfrc (:1560-1660); plus the
// rhs3d(ng,tile) driver (rhs3d.F:25-170).  The kernel is instantiated for the
// pairs <HADV, VADV> of roms_params_t.uv_adv (enum roms_uv_hadv, roms_uv_vadv):
// UV_C2ADVECTION (:605-656, :1079-1107, :1330-1361), UV_C4ADVECTION (:685-705,
// :761-778, :829-849, :902-919, :1108-1176, :1362-1433) and UV_SADVECTION, whose
// vertical term and vertical integral are the column kernel k_rhs3d_vspline
// (:1016-1078, :1267-1329) behind the VADV = SPLINES instantiation.
//
// A 64 x 4 workgroup sweeps its columns upward level by level.  For every
// level the five fields the horizontal operators read -- u, v, Huon, Hvom
// (2-point C-grid halo) and Hz -- are staged into LDS once (68 x 8 doubles per
// field, 21.8 KB per workgroup) and the third-order upstream fluxes, Coriolis
// and curvilinear terms are evaluated from LDS.  HBM/L2 sees each plane ~1.5x
// (halo rows) instead of the ~12 re-reads per point of the direct version.
// The k-window of u, v for the 4th-order vertical advection stays in VGPRs and
// the vertical sums rufrc/rvfrc accumulate in registers.
#include "roms_dev.h"

namespace {

#define Gadv (-0.25)

struct T3 {
  const double *u, *v, *Hu, *Hv, *Hz;      // LDS tiles
  int i0, j0;
  int Istr, Iend, Jstr, Jend;
  bool s_edge, n_edge, w_edge, e_edge;
  __device__ __forceinline__ int at(int i, int j) const { return (i - i0) + (j - j0) * TP; }
};

__device__ __forceinline__ int ex_uxx(const T3 &L, int i) {           // rhs3d.F:668-685
  if (L.w_edge && i == L.Istr) return L.Istr + 1;
  if (L.e_edge && i == L.Iend + 1) return L.Iend;
  return i;
}
__device__ __forceinline__ int ey_uee(const T3 &L, int j) {           // :717-733
  if (L.s_edge && j == L.Jstr - 1) return L.Jstr;
  if (L.n_edge && j == L.Jend + 1) return L.Jend;
  return j;
}
__device__ __forceinline__ int ex_vxx(const T3 &L, int i) {           // :770-786
  if (L.w_edge && i == L.Istr - 1) return L.Istr;
  if (L.e_edge && i == L.Iend + 1) return L.Iend;
  return i;
}
__device__ __forceinline__ int ey_vee(const T3 &L, int j) {           // :820-838
  if (L.s_edge && j == L.Jstr) return L.Jstr + 1;
  if (L.n_edge && j == L.Jend + 1) return L.Jend;
  return j;
}

__device__ __forceinline__ double UFx_u3(const T3 &L, int i, int j)   // :711-730
{
  const int a = L.at(i, j);
  const double cff1 = L.u[a] + L.u[a + 1];
  const int ia = ex_uxx(L, i), ib = ex_uxx(L, i + 1);
  const double cff = (cff1 > 0.0) ? d2x(L.u, L.at(ia, j)) : d2x(L.u, L.at(ib, j));
  return 0.25 * (cff1 + Gadv * cff) *
         (L.Hu[a] + L.Hu[a + 1] + Gadv * 0.5 * (d2x(L.Hu, L.at(ia, j)) + d2x(L.Hu, L.at(ib, j))));
}
__device__ __forceinline__ double UFe_u3(const T3 &L, int i, int j)   // :780-798
{
  const int a = L.at(i, j);
  const double cff1 = L.u[a] + L.u[a - TP];
  const double cff2 = L.Hv[a] + L.Hv[a - 1];
  const double cff = (cff2 > 0.0) ? d2y(L.u, L.at(i, ey_uee(L, j - 1))) : d2y(L.u, L.at(i, ey_uee(L, j)));
  return 0.25 * (cff1 + Gadv * cff) * (cff2 + Gadv * 0.5 * (d2x(L.Hv, a) + d2x(L.Hv, a - 1)));
}
__device__ __forceinline__ double VFx_u3(const T3 &L, int i, int j)   // :855-873
{
  const int a = L.at(i, j);
  const double cff1 = L.v[a] + L.v[a - 1];
  const double cff2 = L.Hu[a] + L.Hu[a - TP];
  const double cff = (cff2 > 0.0) ? d2x(L.v, L.at(ex_vxx(L, i - 1), j)) : d2x(L.v, L.at(ex_vxx(L, i), j));
  return 0.25 * (cff1 + Gadv * cff) * (cff2 + Gadv * 0.5 * (d2y(L.Hu, a) + d2y(L.Hu, a - TP)));
}
__device__ __forceinline__ double VFe_u3(const T3 &L, int i, int j)   // :921-940
{
  const int a = L.at(i, j);
  const double cff1 = L.v[a] + L.v[a + TP];
  const int ja = ey_vee(L, j), jb = ey_vee(L, j + 1);
  const double cff = (cff1 > 0.0) ? d2y(L.v, L.at(i, ja)) : d2y(L.v, L.at(i, jb));
  return 0.25 * (cff1 + Gadv * cff) *
         (L.Hv[a] + L.Hv[a + TP] + Gadv * 0.5 * (d2y(L.Hv, L.at(i, ja)) + d2y(L.Hv, L.at(i, jb))));
}

// UV_C4ADVECTION: fourth-order centred, the second differences and their edge copies of the upstream form
#define C6 (1.0 / 6.0)
__device__ __forceinline__ double UFx_c4(const T3 &L, int i, int j)   // :689-705
{
  const int a = L.at(i, j);
  const int ia = L.at(ex_uxx(L, i), j), ib = L.at(ex_uxx(L, i + 1), j);
  return 0.25 * (L.u[a] + L.u[a + 1] - C6 * (d2x(L.u, ia) + d2x(L.u, ib))) *
         (L.Hu[a] + L.Hu[a + 1] - C6 * (d2x(L.Hu, ia) + d2x(L.Hu, ib)));
}
__device__ __forceinline__ double UFe_c4(const T3 &L, int i, int j)   // :762-778
{
  const int a = L.at(i, j);
  return 0.25 * (L.u[a] + L.u[a - TP] - C6 * (d2y(L.u, L.at(i, ey_uee(L, j))) + d2y(L.u, L.at(i, ey_uee(L, j - 1))))) *
         (L.Hv[a] + L.Hv[a - 1] - C6 * (d2x(L.Hv, a) + d2x(L.Hv, a - 1)));
}
__device__ __forceinline__ double VFx_c4(const T3 &L, int i, int j)   // :833-849
{
  const int a = L.at(i, j);
  return 0.25 * (L.v[a] + L.v[a - 1] - C6 * (d2x(L.v, L.at(ex_vxx(L, i), j)) + d2x(L.v, L.at(ex_vxx(L, i - 1), j)))) *
         (L.Hu[a] + L.Hu[a - TP] - C6 * (d2y(L.Hu, a) + d2y(L.Hu, a - TP)));
}
__device__ __forceinline__ double VFe_c4(const T3 &L, int i, int j)   // :903-919
{
  const int a = L.at(i, j);
  const int ja = L.at(i, ey_vee(L, j)), jb = L.at(i, ey_vee(L, j + 1));
  return 0.25 * (L.v[a] + L.v[a + TP] - C6 * (d2y(L.v, ja) + d2y(L.v, jb))) *
         (L.Hv[a] + L.Hv[a + TP] - C6 * (d2y(L.Hv, ja) + d2y(L.Hv, jb)));
}
// UV_C2ADVECTION: second-order centred, :609-656
__device__ __forceinline__ double UFx_c2(const T3 &L, int a) { return 0.25 * (L.u[a] + L.u[a + 1]) * (L.Hu[a] + L.Hu[a + 1]); }
__device__ __forceinline__ double UFe_c2(const T3 &L, int a) { return 0.25 * (L.u[a - TP] + L.u[a]) * (L.Hv[a - 1] + L.Hv[a]); }
__device__ __forceinline__ double VFx_c2(const T3 &L, int a) { return 0.25 * (L.v[a - 1] + L.v[a]) * (L.Hu[a - TP] + L.Hu[a]); }
__device__ __forceinline__ double VFe_c2(const T3 &L, int a) { return 0.25 * (L.v[a] + L.v[a + TP]) * (L.Hv[a] + L.Hv[a + TP]); }

#define FLUX_AT(F)                                                                          \
  template <int HADV>                                                                       \
  __device__ __forceinline__ double F##_at(const T3 &L, int i, int j)                       \
  {                                                                                         \
    if constexpr (HADV == ROMS_UVH_C2) return F##_c2(L, L.at(i, j));                        \
    else if constexpr (HADV == ROMS_UVH_C4) return F##_c4(L, i, j);                         \
    else return F##_u3(L, i, j);                                                            \
  }
FLUX_AT(UFx) FLUX_AT(UFe) FLUX_AT(VFx) FLUX_AT(VFe)
#undef FLUX_AT
#undef C6

template <int HADV, int VADV>
__device__ __forceinline__ void rhs3d_lds_body(const RomsDev *__restrict__ c, int nrhs)
{
  DEV_PROLOGUE(c)
  const Blk XB = xcd_block();
  // two LDS buffers: level k+1 is fetched into registers while level k is computed from LDS, and is
  // stored into the other buffer at the top of the next iteration -- one barrier per level, and the
  // global-load latency of a level overlaps the arithmetic of the previous one
  constexpr int TT = TJ * TP;
  __shared__ double sU[2 * TT], sV[2 * TT], sHu[2 * TT], sHv[2 * TT], sHz[2 * TT];
  const roms_params_t &p = c->p;
  const int i0 = b.Istr + XB.x * BLK_X, j0 = b.Jstr + XB.y * BLK_Y;
  const int i = i0 + threadIdx.x, j = j0 + threadIdx.y;
  const bool active = i <= b.Iend && j <= b.Jend;
  const bool do_u = active && i >= b.IstrU, do_v = active && j >= b.JstrV;
  const gcd_t ug = (gcd_t)(c->F.u + (long)(nrhs - 1) * n3r);
  const gcd_t vg = (gcd_t)(c->F.v + (long)(nrhs - 1) * n3r);
  const gcd_t Wg = (gcd_t)(c->F.W);
  const gd_t ru = (gd_t)(c->F.ru + (long)(nrhs - 1) * n3w);
  const gd_t rv = (gd_t)(c->F.rv + (long)(nrhs - 1) * n3w);
  const int ic = active ? i : b.Iend, jc = active ? j : b.Jend;     // clamped for address formation only
  const long c0 = I2(ic, jc);
  T3 L;
  L.i0 = i0 - 2; L.j0 = j0 - 2;
  L.Istr = b.Istr; L.Iend = b.Iend; L.Jstr = b.Jstr; L.Jend = b.Jend;
  L.s_edge = b.south_edge && !b.NSperiodic; L.n_edge = b.north_edge && !b.NSperiodic;
  L.w_edge = b.west_edge && !b.EWperiodic;  L.e_edge = b.east_edge && !b.EWperiodic;
  const bool cor = p.uv_cor != 0, curv = p.curvgrid != 0 && p.uv_adv != 0, adv = p.uv_adv != 0;
  const bool nudge = c->clima.m3 != 0;                 // LnudgeM3CLM (uniform)
  const int t = L.at(i, j);
  const int tid = threadIdx.y * BLK_X + threadIdx.x;
  // per-thread constants of the cell terms
  const double fomn0 = GF(fomn)[c0], fomnw = GF(fomn)[c0 - 1], fomns = GF(fomn)[c0 - ni];
  double dndx0 = 0, dndxw = 0, dndxs = 0, dmde0 = 0, dmdew = 0, dmdes = 0;
  if (curv) {
    dndx0 = GF(dndx)[c0]; dndxw = GF(dndx)[c0 - 1]; dndxs = GF(dndx)[c0 - ni];
    dmde0 = GF(dmde)[c0]; dmdew = GF(dmde)[c0 - 1]; dmdes = GF(dmde)[c0 - ni];
  }
  double u_m1 = 0.0, u_0 = ug[c0], u_p1 = ug[c0 + nij], u_p2;
  double v_m1 = 0.0, v_0 = vg[c0], v_p1 = vg[c0 + nij], v_p2;
  double FCu_prev = 0.0, FCv_prev = 0.0, sum_u = 0.0, sum_v = 0.0;
  // weights of the vertical flux: :1178-1179, under UV_C4ADVECTION :1109-1110
  const double c9 = VADV == ROMS_UVV_C4 ? 9.0 / 32.0 : 9.0 / 16.0, c1 = VADV == ROMS_UVV_C4 ? 1.0 / 32.0 : 1.0 / 16.0;
  // what the instantiation's vertical flux reads: the outer points of the W stencil only with the fourth-order
  // averaged W of the default, and neither W nor the k-window of u, v with the splines (k_rhs3d_vspline)
  constexpr bool VW4 = VADV == ROMS_UVV_C4W, VHERE = VADV != ROMS_UVV_SPLINES;

  // staging slots of this thread: tile elements tid, tid+256, tid+512 (the tile has 544)
  constexpr int NSLOT = (TT + BLK_X * BLK_Y - 1) / (BLK_X * BLK_Y);
  long gof[NSLOT];
#pragma unroll
  for (int q = 0; q < NSLOT; q++) {
    const int e = tid + q * BLK_X * BLK_Y;
    const int li = e % TP, lj = (e / TP) % TJ;
    int gi = i0 - 2 + li, gj = j0 - 2 + lj;
    gi = gi < b.LBi ? b.LBi : (gi > b.UBi ? b.UBi : gi);
    gj = gj < b.LBj ? b.LBj : (gj > b.UBj ? b.UBj : gj);
    gof[q] = I2(gi, gj);
  }
  const gcd_t gU = (gcd_t)ug, gV = (gcd_t)vg, gHu = (gcd_t)c->F.Huon, gHv = (gcd_t)c->F.Hvom, gHz = (gcd_t)c->F.Hz;
  const gcd_t gW = (gcd_t)Wg;
  const gd_t gru = (gd_t)ru, grv = (gd_t)rv;
  // staged values of the next level (plain arrays and scalars, constant indices only: a struct returned from a
  // conditional load ended up in scratch memory, with a vmcnt(0) wait right behind the loads)
  double Ru[NSLOT], Rv[NSLOT], Rhu[NSLOT], Rhv[NSLOT], Rhz[NSLOT];
  struct Own { double up2, vp2, ru, rv, w0, wm1, wp1, wm2, wmn, wpn, wm2n; };
  auto gload = [&](int k) {
    const long koff = (long)(k - 1) * nij;
#pragma unroll
    for (int q = 0; q < NSLOT; q++) {
      const long g = gof[q] + koff;
      // slots wholly inside the tile load unconditionally; the last one only where it has an element
      if ((q + 1) * BLK_X * BLK_Y <= TT || tid < TT - q * BLK_X * BLK_Y) {
        Ru[q] = gU[g]; Rv[q] = gV[g]; Rhu[q] = gHu[g]; Rhv[q] = gHv[g]; Rhz[q] = gHz[g];
      }
    }
  };
  auto oload = [&](int k, Own &P) {
    const long koff = (long)(k - 1) * nij;
    const long cw = c0 + (long)k * nij;
    const long c2 = c0 + ((k + 2 <= N) ? koff + 2 * nij : koff);      // clamped: unused above N-2
    if constexpr (VHERE) {                 // the k-window of the column: every level once, whatever the order
      P.up2 = gU[c2];
      P.vp2 = gV[c2];
    }
    P.ru = do_u ? gru[cw] : 0.0;
    P.rv = do_v ? grv[cw] : 0.0;
    if constexpr (VW4) {
      P.w0 = gW[cw];
      // the W stencil of the vertical flux (k < N, u: i-2..i+1, v: j-2..j+1); inactive lanes read their own point
      P.wm1 = do_u ? gW[cw - 1] : P.w0; P.wp1 = do_u ? gW[cw + 1] : P.w0; P.wm2 = do_u ? gW[cw - 2] : P.w0;
      P.wmn = do_v ? gW[cw - ni] : P.w0; P.wpn = do_v ? gW[cw + ni] : P.w0; P.wm2n = do_v ? gW[cw - 2 * ni] : P.w0;
    } else if constexpr (VHERE) {                                       // the two-point sums W(i)+W(i-1), W(j)+W(j-1)
      P.w0 = gW[cw];
      P.wm1 = do_u ? gW[cw - 1] : P.w0;
      P.wmn = do_v ? gW[cw - ni] : P.w0;
    }
  };
#pragma unroll
  for (int q = 0; q < NSLOT; q++) Ru[q] = Rv[q] = Rhu[q] = Rhv[q] = Rhz[q] = 0.0;
  gload(1);
  Own P{};
  oload(1, P);

  for (int k = 1; k <= N; k++) {
    const int buf = (k & 1) * TT;
    double *bU = sU + buf, *bV = sV + buf, *bHu = sHu + buf, *bHv = sHv + buf, *bHz = sHz + buf;
#pragma unroll
    for (int q = 0; q < NSLOT; q++) {
      const int e = tid + q * BLK_X * BLK_Y;
      if (e < TT) { bU[e] = Ru[q]; bV[e] = Rv[q]; bHu[e] = Rhu[q]; bHv[e] = Rhv[q]; bHz[e] = Rhz[q]; }
    }
    __syncthreads();
    const Own Pk = P;
    { const int kn = k < N ? k + 1 : N; gload(kn); oload(kn, P); }   // in flight while level k is computed
    L.u = bU; L.v = bV; L.Hu = bHu; L.Hv = bHv; L.Hz = bHz;
    u_p2 = Pk.up2;
    v_p2 = Pk.vp2;
    const long cw = c0 + (long)k * nij;
    double ruv = Pk.ru;
    double rvv = Pk.rv;
    if (active) {
      if (cor) {
        const double cf0 = 0.5 * bHz[t] * fomn0;
        const double a0 = cf0 * (bV[t] + bV[t + TP]), b0 = cf0 * (bU[t] + bU[t + 1]);
        if (do_u) {
          const double cf1 = 0.5 * bHz[t - 1] * fomnw;
          const double a1 = cf1 * (bV[t - 1] + bV[t - 1 + TP]);
          ruv = ruv + 0.5 * (a0 + a1);
        }
        if (do_v) {
          const double cf2 = 0.5 * bHz[t - TP] * fomns;
          const double b2 = cf2 * (bU[t - TP] + bU[t - TP + 1]);
          rvv = rvv - 0.5 * (b0 + b2);
        }
      }
      if (curv) {
        auto cell = [&](int q, double dn, double dm, double &ufx, double &vfe) {
          const double cff1 = 0.5 * (bV[q] + bV[q + TP]);
          const double cff2 = 0.5 * (bU[q] + bU[q + 1]);
          const double cff3 = cff1 * dn;
          const double cff4 = cff2 * dm;
          const double cff = bHz[q] * (cff3 - cff4);
          ufx = cff * cff1;
          vfe = cff * cff2;
        };
        double a0, b0, a1, b1;
        cell(t, dndx0, dmde0, a0, b0);
        if (do_u) { cell(t - 1, dndxw, dmdew, a1, b1); ruv = ruv + 0.5 * (a0 + a1); }
        if (do_v) { cell(t - TP, dndxs, dmdes, a1, b1); rvv = rvv - 0.5 * (b0 + b1); }
      }
      if (nudge) {                                     // nudging of 3-D momentum climatology, rhs3d.F:571-594
        const long ck = c0 + (long)(k - 1) * nij;
        const gcd_t cof = (gcd_t)c->clima.M3nudgcof;
        if (do_u) {
          const double cff = 0.25 * (cof[ck - 1] + cof[ck]) * GF(om_u)[c0] * GF(on_u)[c0];
          ruv = ruv + cff * (bHz[t - 1] + bHz[t]) * (((gcd_t)c->clima.uclm)[ck] - bU[t]);
        }
        if (do_v) {
          const double cff = 0.25 * (cof[ck - ni] + cof[ck]) * GF(om_v)[c0] * GF(on_v)[c0];
          rvv = rvv + cff * (bHz[t - TP] + bHz[t]) * (((gcd_t)c->clima.vclm)[ck] - bV[t]);
        }
      }
      if (adv) {
        if (do_u) {
          const double cff1 = UFx_at<HADV>(L, i, j) - UFx_at<HADV>(L, i - 1, j);
          const double cff2 = UFe_at<HADV>(L, i, j + 1) - UFe_at<HADV>(L, i, j);
          ruv = ruv - (cff1 + cff2);
        }
        if (do_v) {
          const double cff1 = VFx_at<HADV>(L, i + 1, j) - VFx_at<HADV>(L, i, j);
          const double cff2 = VFe_at<HADV>(L, i, j) - VFe_at<HADV>(L, i, j - 1);
          rvv = rvv - (cff1 + cff2);
        }
        double FCu = 0.0, FCv = 0.0;
        if (VHERE && k < N) {
          if (do_u) {
            const double um = (k == 1) ? u_0 : u_m1;
            const double up = (k == N - 1) ? u_p1 : u_p2;
            if constexpr (VADV == ROMS_UVV_C4W)
              FCu = (c9 * (u_0 + u_p1) - c1 * (um + up)) *
                    (c9 * (Pk.w0 + Pk.wm1) - c1 * (Pk.wp1 + Pk.wm2));
            else if constexpr (VADV == ROMS_UVV_C4) FCu = (c9 * (u_0 + u_p1) - c1 * (um + up)) * (Pk.w0 + Pk.wm1);   // :1111-1158
            else FCu = 0.25 * (u_0 + u_p1) * (Pk.w0 + Pk.wm1);                                                     // :1080-1091
          }
          if (do_v) {
            const double vm = (k == 1) ? v_0 : v_m1;
            const double vp = (k == N - 1) ? v_p1 : v_p2;
            if constexpr (VADV == ROMS_UVV_C4W)
              FCv = (c9 * (v_0 + v_p1) - c1 * (vm + vp)) *
                    (c9 * (Pk.w0 + Pk.wmn) - c1 * (Pk.wpn + Pk.wm2n));
            else if constexpr (VADV == ROMS_UVV_C4) FCv = (c9 * (v_0 + v_p1) - c1 * (vm + vp)) * (Pk.w0 + Pk.wmn);   // :1368-1415
            else FCv = 0.25 * (v_0 + v_p1) * (Pk.w0 + Pk.wmn);                                                     // :1334-1345
          }
        }
        if constexpr (VHERE) {
          ruv = ruv - (FCu - FCu_prev);
          rvv = rvv - (FCv - FCv_prev);
          FCu_prev = FCu; FCv_prev = FCv;
        }
      }
      if (do_u) { gru[cw] = ruv; sum_u = (k == 1) ? ruv : sum_u + ruv; }
      if (do_v) { grv[cw] = rvv; sum_v = (k == 1) ? rvv : sum_v + rvv; }
    }
    u_m1 = u_0; u_0 = u_p1; u_p1 = u_p2;
    v_m1 = v_0; v_0 = v_p1; v_p1 = v_p2;
  }
  // with the splines ru, rv are not final here: the column kernel behind this one forms the vertical integral
  if (VHERE && do_u) {
    const double cff = GF(om_u)[c0] * GF(on_u)[c0];
    const double cff1 = GF(sustr)[c0] * cff;
    const double cff2 = -GF(bustr)[c0] * cff;
    GF(rufrc)[c0] = sum_u + cff1 + cff2;
  }
  if (VHERE && do_v) {
    const double cff = GF(om_v)[c0] * GF(on_v)[c0];
    const double cff1 = GF(svstr)[c0] * cff;
    const double cff2 = -GF(bvstr)[c0] * cff;
    GF(rvfrc)[c0] = sum_v + cff1 + cff2;
  }
}

template <int HADV, int VADV>
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_rhs3d_lds(const RomsDev *__restrict__ c, int nrhs) { rhs3d_lds_body<HADV, VADV>(c, nrhs); }

// UV_SADVECTION: vertical advection with conservative parabolic splines (rhs3d.F:1016-1078 for u, :1267-1329 for v),
// its subtraction from ru, rv(nrhs) (:1257-1265) and the vertical integral rufrc, rvfrc (:1534-1666).  One thread per
// column, u then v: the forward elimination leaves FC(k), CF(k) of k = 1..N-1 in LDS ([level][thread]: a thread only
// meets its own column, so there is no barrier), the back-substitution finishes CF there, and the third sweep forms
// the flux level by level, subtracts its difference and sums the finished values in the reference's order.  DC is
// evaluated from Hz where it is used (the same expression, so the same value, in both sweeps).
template <int NMAX>
__global__ void __launch_bounds__(BLK_X)
k_rhs3d_vspline(const RomsDev *__restrict__ c, int nrhs)
{
  DEV_PROLOGUE(c)
  __shared__ double sFC[NMAX][BLK_X], sCF[NMAX][BLK_X];
  const int tx = threadIdx.x;
  const int i = b.Istr + blockIdx.x * BLK_X + tx, j = b.Jstr + blockIdx.y;
  if (i > b.Iend || j > b.Jend) return;
  const long c0 = I2(i, j);
  const gcd_t Hz = (gcd_t)c->F.Hz, W = (gcd_t)c->F.W;
  const double c9 = 9.0 / 16.0, c1 = 1.0 / 16.0, c3 = 1.0 / 3.0, c4 = 1.0 / 6.0;
  auto column = [&](long off, gcd_t q, gd_t r, gd_t frc, double stress_s, double stress_b, double area) {
    auto DC = [&](int k) {
      const long a = c0 + (long)(k - 1) * nij;
      return c9 * (Hz[a] + Hz[a - off]) - c1 * (Hz[a + off] + Hz[a - 2 * off]);
    };
    double FCp = 0.0, CFp = 0.0, dc = DC(1), qk = q[c0];
    for (int k = 1; k <= N - 1; k++) {
      const double dcn = DC(k + 1), qn = q[c0 + (long)k * nij];
      const double cff = 1.0 / (2.0 * dcn + dc * (2.0 - FCp));
      FCp = cff * dcn;
      CFp = cff * (6.0 * (qn - qk) - dc * CFp);
      sFC[k][tx] = FCp;
      sCF[k][tx] = CFp;
      dc = dcn; qk = qn;
    }
    double CFn = 0.0;                                   // CF(N)
    for (int k = N - 1; k >= 1; k--) {
      CFn = sCF[k][tx] - sFC[k][tx] * CFn;
      sCF[k][tx] = CFn;
    }
    double FCm = 0.0, CFm = 0.0, sum = 0.0;             // FC(0), CF(0)
    for (int k = 1; k <= N; k++) {
      const long cw = c0 + (long)k * nij;
      double FCk = 0.0;                                 // FC(N)
      if (k < N) {
        const double CFk = sCF[k][tx];
        FCk = (c9 * (W[cw] + W[cw - off]) - c1 * (W[cw + off] + W[cw - 2 * off])) *
              (q[cw - nij] + DC(k) * (c3 * CFk + c4 * CFm));
        CFm = CFk;
      }
      const double rk = r[cw] - (FCk - FCm);
      r[cw] = rk;
      sum = (k == 1) ? rk : sum + rk;
      FCm = FCk;
    }
    const double cff1 = stress_s * area;
    const double cff2 = -stress_b * area;
    frc[c0] = sum + cff1 + cff2;
  };
  if (i >= b.IstrU)
    column(1, (gcd_t)(c->F.u + (long)(nrhs - 1) * n3r), (gd_t)(c->F.ru + (long)(nrhs - 1) * n3w), GF(rufrc),
           GF(sustr)[c0], GF(bustr)[c0], GF(om_u)[c0] * GF(on_u)[c0]);
  if (j >= b.JstrV)
    column(ni, (gcd_t)(c->F.v + (long)(nrhs - 1) * n3r), (gd_t)(c->F.rv + (long)(nrhs - 1) * n3w), GF(rvfrc),
           GF(svstr)[c0], GF(bvstr)[c0], GF(om_v)[c0] * GF(on_v)[c0]);
}

}  // namespace

// roms_params_t.uv_adv: 0, or one of the six scheme pairs the reference can be compiled to (roms_hip.h)
int roms_uv_adv_check(const char *where)
{
  const int a = g_ctx.p.uv_adv;
  if (a == 0) return 0;
  static const int pairs[6][2] = {{ROMS_UVH_U3, ROMS_UVV_C4W}, {ROMS_UVH_U3, ROMS_UVV_SPLINES}, {ROMS_UVH_C2, ROMS_UVV_C2},
                                  {ROMS_UVH_C2, ROMS_UVV_SPLINES}, {ROMS_UVH_C4, ROMS_UVV_C4}, {ROMS_UVH_C4, ROMS_UVV_SPLINES}};
  for (const auto &q : pairs)
    if (a == ROMS_UV_ADV(q[0], q[1])) return 0;
  return roms_fail(where, "uv_adv is neither 0 nor ROMS_UV_ADV(h, v) of a momentum advection pair the reference can be "
                          "compiled to: (U3, C4W), (U3, SPLINES), (C2, C2), (C2, SPLINES), (C4, C4), (C4, SPLINES)");
}

extern "C" int roms_hip_rhs3d_tile(const roms_step_idx_t *s)
{
  int rc = roms_entry_check("roms_hip_rhs3d_tile");
  if (rc) return rc;
  if ((rc = roms_uv_adv_check("roms_hip_rhs3d_tile"))) return rc;
  if ((rc = check_lbc())) return rc;
  ScopedTimer tm("rhs3d_tile");
  const roms_bounds_t &b = g_ctx.b;
  if (b.N < 4) return roms_fail("roms_hip_rhs3d_tile", "needs N >= 4 levels (the vertical stencils of the column read k-1 .. k+2)");
  // without UV_ADV (uv_adv = 0) the advection is a uniform branch not taken: the default instantiation
  const int uv = g_ctx.p.uv_adv, hadv = uv ? ROMS_UV_HADV(uv) : ROMS_UVH_U3, vadv = uv ? ROMS_UV_VADV(uv) : ROMS_UVV_C4W;
  const bool spl = vadv == ROMS_UVV_SPLINES;
  if (spl && b.N > ROMS_MAXN) return roms_fail("roms_hip_rhs3d_tile", "N > 64 not instantiated");
  const auto kernel = hadv == ROMS_UVH_C2 ? (spl ? k_rhs3d_lds<ROMS_UVH_C2, ROMS_UVV_SPLINES> : k_rhs3d_lds<ROMS_UVH_C2, ROMS_UVV_C2>)
                      : hadv == ROMS_UVH_C4 ? (spl ? k_rhs3d_lds<ROMS_UVH_C4, ROMS_UVV_SPLINES> : k_rhs3d_lds<ROMS_UVH_C4, ROMS_UVV_C4>)
                                            : (spl ? k_rhs3d_lds<ROMS_UVH_U3, ROMS_UVV_SPLINES> : k_rhs3d_lds<ROMS_UVH_U3, ROMS_UVV_C4W>);
  hipLaunchKernelGGL(kernel, grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1), block2d(), 0, g_ctx.stream,
                     g_ctx.devc, s->nrhs);
  KERNEL_CHECK("k_rhs3d_lds");
  if (spl) {
    const dim3 grid((unsigned)((b.Iend - b.Istr + BLK_X) / BLK_X), (unsigned)(b.Jend - b.Jstr + 1), 1), block(BLK_X, 1, 1);
    if (b.N <= 16) hipLaunchKernelGGL(k_rhs3d_vspline<16>, grid, block, 0, g_ctx.stream, g_ctx.devc, s->nrhs);
    else if (b.N <= 32) hipLaunchKernelGGL(k_rhs3d_vspline<32>, grid, block, 0, g_ctx.stream, g_ctx.devc, s->nrhs);
    else if (b.N <= 48) hipLaunchKernelGGL(k_rhs3d_vspline<48>, grid, block, 0, g_ctx.stream, g_ctx.devc, s->nrhs);
    else hipLaunchKernelGGL(k_rhs3d_vspline<64>, grid, block, 0, g_ctx.stream, g_ctx.devc, s->nrhs);
    KERNEL_CHECK("k_rhs3d_vspline");
  }
  return 0;
}

// Inside roms_hip_rhs3d the start of the corrector t(nnew) = Hz*t(nstp) + explicit vertical flux divergence moves from
// k_pre_t into the rotated harmonic mixing kernel (k_mix.hip, k_t3dmix_geo<0, ISO, false, true>), which otherwise loads the
// value just stored, adds its term and stores it again: nothing between the two touches t(nnew) (prsgrd reads no
// tracer; t3dbc_tile and the exchanges at the end of the predictor work on level 3, pre_step3d.F:1131-1149).  Where the
// mixing kernel cannot form the start -- along s-surfaces, with TS_MIX_STABILITY, diagnostics, an explicit part of the
// vertical diffusion (lambda < 1) or nrhs /= nstp -- the two entries run as they do on their own.
static bool rhs3d_fuses_tstart(const roms_step_idx_t *s)
{
  const roms_params_t &p = g_ctx.p;
  return p.ts_dif2 && (p.mix_geo_ts || p.mix_iso_ts) && !p.ts_mix_stability && p.lambda == 1.0 && !dia_on() &&
         s->nrhs == s->nstp;
}

// Inside roms_hip_rhs3d the predictor's start of u, v(nnew) (k_pre_uv) moves into the pressure-gradient kernel of
// prsgrd32 (k_prsgrd.hip, k_prsgrd32<true>): that kernel overwrites ru, rv(nrhs) at exactly the point whose old value the
// start has just read as its AB3 term, and both read Hz of the same two cells.  Nothing between the two reads u, v(nnew) or
// ru, rv: the tracer half of the predictor reads neither, t3dbc_tile and the exchanges at its end act on t(3)
// (pre_step3d.F:1131-1149).  With lambda = 1 the explicit vertical viscous flux is identically zero, so the start at level
// k needs level k alone (and the stresses at k = 1 and k = N) and the downward march of the pressure kernel gives the bits
// of the upward one.  With an explicit part (lambda < 1) or another pressure-gradient algorithm the two entries run as they
// do on their own.
static bool rhs3d_fuses_uvstart(const roms_step_idx_t *s)
{
  (void)s;
  const roms_params_t &p = g_ctx.p;
  return p.pgf == PGF_DJ_GRADPS && p.lambda == 1.0;
}

int roms_uv_mix_check(const char *where);    // k_uv3dmix2.hip

// rhs3d(ng,tile) -- rhs3d.F:25-170: pre_step3d, prsgrd, t3dmix2, t3dmix4, rhs3d_tile, uv3dmix2, uv3dmix4
extern "C" int roms_hip_rhs3d(const roms_step_idx_t *s)
{
  int rc = roms_entry_check("roms_hip_rhs3d");
  if (rc) return rc;
  if ((rc = roms_uv_adv_check("roms_hip_rhs3d"))) return rc;          // before the first piece has changed anything
  if ((rc = roms_uv_mix_check("roms_hip_rhs3d"))) return rc;
  const bool fused = rhs3d_fuses_tstart(s);
  const bool uvstart = rhs3d_fuses_uvstart(s);
  if ((rc = pre_step3d_entry(s, fused, uvstart))) return rc;
  if ((rc = prsgrd_entry(s, uvstart))) return rc;
  if (g_ctx.p.ts_dif2 && (rc = t3dmix2_entry(s, fused))) return rc;
  if (g_ctx.p.ts_dif4 && (rc = roms_hip_t3dmix4(s))) return rc;
  if ((rc = roms_hip_rhs3d_tile(s))) return rc;
  if (g_ctx.p.uv_vis2 && (rc = roms_hip_uv3dmix2(s))) return rc;
  if (g_ctx.p.uv_vis4 && (rc = roms_hip_uv3dmix4(s))) return rc;
  return 0;
}
