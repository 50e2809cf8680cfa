// uvgeo.h -- the level body of the horizontal viscosity rotated to geopotential surfaces (MIX_GEO_UV), stated once
// for the three operators that share it (k_uv3dmix2.hip):
//
//   UVGEO_HARM   uv3dmix2_geo_tile (ROMS/Nonlinear/uv3dmix2_geo.h:116-756): on u, v(nrhs) with visc2, Hz inside the
//                horizontal fluxes, the increment added to u, v(nnew) and rufrc, rvfrc
//   UVGEO_FIRST  K_LOOP1 of uv3dmix4_geo_tile (uv3dmix4_geo.h:322-801): on u, v(nrhs) with visc4, no Hz in the fluxes
//                (:528-529, :580-581), the divergence divided by the face Hz (:765, :785) -> LapU, LapV
//   UVGEO_SECOND K_LOOP2 (:982-1476): on LapU, LapV with visc4, Hz inside the fluxes (:1160, :1205), the increment
//                subtracted (:1439-1440, :1462-1463)
//
// The reference marches k over two-level slabs of fourteen private arrays; here a workgroup owns BLK_X x BLK_Y columns
// and keeps the slabs of its patch (own points plus one ring) in LDS, marching k upward: the slopes of z_r at u- and
// v-faces (their averages to rho- and psi-points, the reference's dZdx_r/_p, dZde_r/_p, are formed where they are
// used: the same 0.5*(a + b)), the four horizontal gradients, the two vertical ones, and the four horizontal fluxes
// of the level.  The vertical fluxes UFsx, UFse, VFsx, VFse are only ever read at the point that made them and wait
// in registers.  Every value is the reference's expression in the reference's order, evaluated on the reference's
// ranges for the patch taken as a tile, so the result does not depend on the partition (workgroups or tiles).  Two
// barriers per level.
//
// The ranges of all three are those of one tile (Istr, IstrU, Iend, Jstr, JstrV, Jend): output on IstrU:Iend x
// Jstr:Jend (u) and Istr:Iend x JstrV:Jend (v), slopes and vertical gradients one point further out, rho-points on
// IstrU-1:Iend x JstrV-1:Jend, psi-points on Istr:Iend+1 x Jstr:Jend+1.  K_LOOP1 runs them for the tile grown to
// (Istrm1, IstrUm1, Iendp1, Jstrm1, JstrVm1, Jendp1): IstrUm2 = IstrUm1 - 1, Istrm2 = Istrm1 - 1, Iendp2 = Iendp1 + 1
// on a physical edge as inside the domain (get_bounds.F:1348-1598), so the grown tile is cut into the same one-ring
// patches and no wider patch is needed.
#ifndef ROMS_UVGEO_H
#define ROMS_UVGEO_H
#include "roms_dev.h"

enum { UVGEO_HARM = 0, UVGEO_FIRST = 1, UVGEO_SECOND = 2 };

struct GeoTile { int Istr, IstrU, Iend, Jstr, JstrV, Jend; };

#ifdef __HIPCC__
__device__ __forceinline__ double gmin0(double a) { return a < 0.0 ? a : 0.0; }   // MIN(a, 0)
__device__ __forceinline__ double gmax0(double a) { return a > 0.0 ? a : 0.0; }   // MAX(a, 0)
#define GEO_W (BLK_X + 2)
#define GEO_H (BLK_Y + 2)
#define GEO_P (GEO_W * GEO_H)
static_assert(20 * GEO_P * sizeof(double) <= 64 * 1024, "LDS of a rotated-viscosity workgroup");

// u, v: the fields the operator acts on (level stride nij, N levels); visc_r, visc_p: its coefficients; un, vn:
// u, v(nnew) (UVGEO_HARM, UVGEO_SECOND) or LapU, LapV (UVGEO_FIRST)
template <int MODE>
__device__ __forceinline__ void uvgeo_march(const RomsDev *__restrict__ c, const GeoTile T, const gcd_t u, const gcd_t v,
                                            const gcd_t visc_r, const gcd_t visc_p, const gd_t un, const gd_t vn)
{
  DEV_PROLOGUE(c)
  __shared__ double sUFx[GEO_P], sVFe[GEO_P], sUFe[GEO_P], sVFx[GEO_P];            // fluxes of the level
  __shared__ double sSx[2][GEO_P], sSe[2][GEO_P];                                  // slopes at u- / v-faces
  __shared__ double sdnUdx[2][GEO_P], sdmUde[2][GEO_P], sdnVdx[2][GEO_P], sdmVde[2][GEO_P];
  __shared__ double sdUdz[2][GEO_P], sdVdz[2][GEO_P];
  const Blk XB = xcd_block();
  const int i0 = T.Istr + XB.x * BLK_X, j0 = T.Jstr + XB.y * BLK_Y;
  // the patch as a tile
  const int Istr = i0, Iend = (i0 + BLK_X - 1 < T.Iend) ? i0 + BLK_X - 1 : T.Iend;
  const int Jstr = j0, Jend = (j0 + BLK_Y - 1 < T.Jend) ? j0 + BLK_Y - 1 : T.Jend;
  const int IstrU = i0 > T.IstrU ? i0 : T.IstrU, JstrV = j0 > T.JstrV ? j0 : T.JstrV;
  const int tid = threadIdx.y * BLK_X + threadIdx.x;
  const bool msk = c->p.masking != 0;
  const double dt = c->p.dt;
  const gcd_t z_r = (gcd_t)c->F.z_r, Hz = (gcd_t)c->F.Hz, pm = (gcd_t)c->F.pm, pn = (gcd_t)c->F.pn;
  const gcd_t on_r = (gcd_t)c->F.on_r, om_r = (gcd_t)c->F.om_r, on_p = (gcd_t)c->F.on_p, om_p = (gcd_t)c->F.om_p;
#define GL(i, j) (((j) - (j0 - 1)) * GEO_W + ((i) - (i0 - 1)))
#define dZdx_p(i, j, s) (0.5 * (sSx[s][GL(i, (j) - 1)] + sSx[s][GL(i, j)]))
#define dZde_p(i, j, s) (0.5 * (sSe[s][GL((i) - 1, j)] + sSe[s][GL(i, j)]))
#define dZdx_r(i, j, s) (0.5 * (sSx[s][GL(i, j)] + sSx[s][GL((i) + 1, j)]))
#define dZde_r(i, j, s) (0.5 * (sSe[s][GL(i, j)] + sSe[s][GL(i, (j) + 1)]))
#define dnUdx(i, j, s) sdnUdx[s][GL(i, j)]
#define dmUde(i, j, s) sdmUde[s][GL(i, j)]
#define dnVdx(i, j, s) sdnVdx[s][GL(i, j)]
#define dmVde(i, j, s) sdmVde[s][GL(i, j)]
#define dUdz(i, j, s) sdUdz[s][GL(i, j)]
#define dVdz(i, j, s) sdVdz[s][GL(i, j)]
#define UFx(i, j) sUFx[GL(i, j)]
#define VFe(i, j) sVFe[GL(i, j)]
#define UFe(i, j) sUFe[GL(i, j)]
#define VFx(i, j) sVFx[GL(i, j)]
  // the thread's own column
  const int io = i0 + (int)threadIdx.x, jo = j0 + (int)threadIdx.y;
  const bool own = io <= Iend && jo <= Jend;
  const bool do_u = own && io >= IstrU, do_v = own && jo >= JstrV;
  double UFsx1 = 0.0, UFse1 = 0.0, VFsx1 = 0.0, VFse1 = 0.0;        // the k1 level of the vertical fluxes
  double ruf = 0.0, rvf = 0.0;
  const long ao = own ? I2(io, jo) : 0;
  if constexpr (MODE != UVGEO_FIRST) {
    if (do_u) ruf = c->F.rufrc[ao];
    if (do_v) rvf = c->F.rvfrc[ao];
  }
  // every thread looks after at most two points of the patch (q = tid, tid + 256); what those points need from the
  // k-independent fields for the gradients of a level -- the metric factors of the reference's expressions with their
  // masks, formed exactly as the reference forms them -- is kept in registers across the levels.  (The factors of the
  // flux phase as well: 282 registers, one workgroup per CU, 2.09 ms against 1.88 -- measured and left out.)
  constexpr int NPT = (GEO_P + BLK_X * BLK_Y - 1) / (BLK_X * BLK_Y);
  static_assert(NPT == 2, "patch points per thread");
  long pa[NPT];
  int flag[NPT];                                   // 1: u-face range, 2: v-face, 4: rho, 8: psi
  double cU[NPT], cV[NPT], cR1[NPT], cR2[NPT], pnE[NPT], pnW[NPT], pmN[NPT], pmS[NPT];
  double cP1[NPT], cP2[NPT], pmA[NPT], pmB[NPT], pnA[NPT], pnB[NPT];
#pragma unroll
  for (int r = 0; r < NPT; r++) {
    const int q = tid + r * BLK_X * BLK_Y;
    flag[r] = 0; pa[r] = 0;
    cU[r] = cV[r] = cR1[r] = cR2[r] = pnE[r] = pnW[r] = pmN[r] = pmS[r] = 0.0;
    cP1[r] = cP2[r] = pmA[r] = pmB[r] = pnA[r] = pnB[r] = 0.0;
    if (q < GEO_P) {
      const int i = i0 - 1 + q % GEO_W, j = j0 - 1 + q / GEO_W;
      const long a = I2(i, j);
      pa[r] = a;
      if (i >= IstrU - 1 && i <= Iend + 1 && j >= Jstr - 1 && j <= Jend + 1) flag[r] |= 1;
      if (i >= Istr - 1 && i <= Iend + 1 && j >= JstrV - 1 && j <= Jend + 1) flag[r] |= 2;
      if (i >= IstrU - 1 && i <= Iend && j >= JstrV - 1 && j <= Jend) flag[r] |= 4;
      if (i >= Istr && i <= Iend + 1 && j >= Jstr && j <= Jend + 1) flag[r] |= 8;
      if (flag[r] & 1) {
        double cff = 0.5 * (pm[a - 1] + pm[a]);
        if (msk) cff = cff * umaskw(c, a);
        cU[r] = cff;
      }
      if (flag[r] & 2) {
        double cff = 0.5 * (pn[a - ni] + pn[a]);
        if (msk) cff = cff * vmaskw(c, a);
        cV[r] = cff;
      }
      if (flag[r] & 4) {
        const double m = msk ? rmaskw(c, a) : 1.0;
        double cff = 0.5 * pm[a];
        if (msk) cff = cff * m;
        cR1[r] = cff;
        cff = 0.5 * pn[a];
        if (msk) cff = cff * m;
        cR2[r] = cff;
        pnE[r] = pn[a] + pn[a + 1]; pnW[r] = pn[a - 1] + pn[a];
        pmN[r] = pm[a] + pm[a + ni]; pmS[r] = pm[a - ni] + pm[a];
      }
      if (flag[r] & 8) {
        const double m = msk ? pmaskw(c, a) : 1.0;
        double cff = 0.125 * (pn[a - 1] + pn[a] + pn[a - 1 - ni] + pn[a - ni]);
        if (msk) cff = cff * m;
        cP1[r] = cff;
        cff = 0.125 * (pm[a - 1] + pm[a] + pm[a - 1 - ni] + pm[a - ni]);
        if (msk) cff = cff * m;
        cP2[r] = cff;
        pmA[r] = pm[a - 1] + pm[a]; pmB[r] = pm[a - 1 - ni] + pm[a - ni];
        pnA[r] = pn[a - ni] + pn[a]; pnB[r] = pn[a - 1 - ni] + pn[a - 1];
      }
    }
  }
  int k1, k2 = 1;
  for (int k = 0; k <= N; k++) {
    k1 = k2;
    k2 = 1 - k1;
    // ---- phase 1: everything of level k+1 that depends on the fields alone -> slot k2
#pragma unroll
    for (int r = 0; r < NPT; r++) {
      const int q = tid + r * BLK_X * BLK_Y;
      const long a = pa[r];
      const bool inU = flag[r] & 1, inV = flag[r] & 2, inR = flag[r] & 4, inP = flag[r] & 8;
      if (k < N) {
        const long ak = a + (long)k * nij;                                                    // level k+1
        if (inU) sSx[k2][q] = cU[r] * (z_r[ak] - z_r[ak - 1]);                                // uv3dmix2_geo.h:303-340
        if (inV) sSe[k2][q] = cV[r] * (z_r[ak] - z_r[ak - ni]);
        if (inR) {                                                                            // :345-412
          sdnUdx[k2][q] = cR1[r] * (pnE[r] * u[ak + 1] - pnW[r] * u[ak]);
          sdmVde[k2][q] = cR2[r] * (pmN[r] * v[ak + ni] - pmS[r] * v[ak]);
        }
        if (inP) {
          sdmUde[k2][q] = cP1[r] * (pmA[r] * u[ak] - pmB[r] * u[ak - ni]);
          sdnVdx[k2][q] = cP2[r] * (pnA[r] * v[ak] - pnB[r] * v[ak - 1]);
        }
      }
      if (k == 0 || k == N) {                                                                 // :414-440
        if (inU) sdUdz[k2][q] = 0.0;
        if (inV) sdVdz[k2][q] = 0.0;
      } else {
        const long ak = a + (long)k * nij, al = ak - nij;                                     // levels k+1, k
        if (inU) {
          const double cff = 1.0 / (0.5 * (z_r[ak - 1] - z_r[al - 1] + z_r[ak] - z_r[al]));
          sdUdz[k2][q] = cff * (u[ak] - u[al]);
        }
        if (inV) {
          const double cff = 1.0 / (0.5 * (z_r[ak - ni] - z_r[al - ni] + z_r[ak] - z_r[al]));
          sdVdz[k2][q] = cff * (v[ak] - v[al]);
        }
      }
    }
    __syncthreads();
    double UFsx2 = 0.0, UFse2 = 0.0, VFsx2 = 0.0, VFse2 = 0.0;       // k == N: zero (:433-440)
    if (k > 0) {
      // ---- phase 2: the rotated horizontal fluxes of level k (:463-541)
      for (int q = tid; q < GEO_P; q += BLK_X * BLK_Y) {
        const int i = i0 - 1 + q % GEO_W, j = j0 - 1 + q / GEO_W;
        const long a = I2(i, j), ak = a + (long)(k - 1) * nij;
        if (i >= IstrU - 1 && i <= Iend && j >= JstrV - 1 && j <= Jend) {
          const double zx = dZdx_r(i, j, k1), ze = dZde_r(i, j, k1);
          const double cff1 = gmin0(zx), cff2 = gmax0(zx), cff3 = gmin0(ze), cff4 = gmax0(ze);
          double cff;
          if constexpr (MODE == UVGEO_FIRST)
            cff = on_r[a] * (dnUdx(i, j, k1) - 0.5 * pn[a] * (cff1 * (dUdz(i, j, k1) + dUdz(i + 1, j, k2)) + cff2 * (dUdz(i, j, k2) + dUdz(i + 1, j, k1)))) -
                  om_r[a] * (dmVde(i, j, k1) - 0.5 * pm[a] * (cff3 * (dVdz(i, j, k1) + dVdz(i, j + 1, k2)) + cff4 * (dVdz(i, j, k2) + dVdz(i, j + 1, k1))));
          else
            cff = Hz[ak] *
                (on_r[a] * (dnUdx(i, j, k1) - 0.5 * pn[a] * (cff1 * (dUdz(i, j, k1) + dUdz(i + 1, j, k2)) + cff2 * (dUdz(i, j, k2) + dUdz(i + 1, j, k1)))) -
                 om_r[a] * (dmVde(i, j, k1) - 0.5 * pm[a] * (cff3 * (dVdz(i, j, k1) + dVdz(i, j + 1, k2)) + cff4 * (dVdz(i, j, k2) + dVdz(i, j + 1, k1)))));
          if (msk) cff = cff * rmaskw(c, a);
          sUFx[q] = on_r[a] * on_r[a] * visc_r[a] * cff;
          sVFe[q] = om_r[a] * om_r[a] * visc_r[a] * cff;
        }
        if (i >= Istr && i <= Iend + 1 && j >= Jstr && j <= Jend + 1) {
          const double pm_p = 0.25 * (pm[a - 1 - ni] + pm[a - 1] + pm[a - ni] + pm[a]);
          const double pn_p = 0.25 * (pn[a - 1 - ni] + pn[a - 1] + pn[a - ni] + pn[a]);
          const double zx = dZdx_p(i, j, k1), ze = dZde_p(i, j, k1);
          const double cff1 = gmin0(zx), cff2 = gmax0(zx), cff3 = gmin0(ze), cff4 = gmax0(ze);
          double cff;
          if constexpr (MODE == UVGEO_FIRST)
            cff = on_p[a] * (dnVdx(i, j, k1) - 0.5 * pn_p * (cff1 * (dVdz(i - 1, j, k1) + dVdz(i, j, k2)) + cff2 * (dVdz(i - 1, j, k2) + dVdz(i, j, k1)))) +
                  om_p[a] * (dmUde(i, j, k1) - 0.5 * pm_p * (cff3 * (dUdz(i, j - 1, k1) + dUdz(i, j, k2)) + cff4 * (dUdz(i, j - 1, k2) + dUdz(i, j, k1))));
          else
            cff = 0.25 * (Hz[ak - 1] + Hz[ak] + Hz[ak - 1 - ni] + Hz[ak - ni]) *
                (on_p[a] * (dnVdx(i, j, k1) - 0.5 * pn_p * (cff1 * (dVdz(i - 1, j, k1) + dVdz(i, j, k2)) + cff2 * (dVdz(i - 1, j, k2) + dVdz(i, j, k1)))) +
                 om_p[a] * (dmUde(i, j, k1) - 0.5 * pm_p * (cff3 * (dUdz(i, j - 1, k1) + dUdz(i, j, k2)) + cff4 * (dUdz(i, j - 1, k2) + dUdz(i, j, k1)))));
          if (msk) cff = cff * pmaskw(c, a);
          sUFe[q] = om_p[a] * om_p[a] * visc_p[a] * cff;
          sVFx[q] = on_p[a] * on_p[a] * visc_p[a] * cff;
        }
      }
      // ---- the vertical fluxes through the top of level k, at the thread's own faces (:546-700)
      if (k < N) {
        const int i = io, j = jo;
        if (do_u) {
          const long a = ao;
          double cff = 0.25 * (visc_r[a - 1] + visc_r[a]);
          const double fac1 = cff * c->F.on_u[a], fac2 = cff * c->F.om_u[a];
          cff = 0.5 * (pn[a - 1] + pn[a]);
          const double dnUdz = cff * dUdz(i, j, k2);
          const double dnVdz = cff * 0.25 * (dVdz(i - 1, j + 1, k2) + dVdz(i, j + 1, k2) + dVdz(i - 1, j, k2) + dVdz(i, j, k2));
          cff = 0.5 * (pm[a - 1] + pm[a]);
          const double dmUdz = cff * dUdz(i, j, k2);
          const double dmVdz = cff * 0.25 * (dVdz(i - 1, j + 1, k2) + dVdz(i, j + 1, k2) + dVdz(i - 1, j, k2) + dVdz(i, j, k2));
          const double xr1 = gmin0(dZdx_r(i - 1, j, k1)), xr2 = gmin0(dZdx_r(i, j, k2));
          const double xr3 = gmax0(dZdx_r(i - 1, j, k2)), xr4 = gmax0(dZdx_r(i, j, k1));
          const double ep1 = gmin0(dZde_p(i, j, k1)), ep2 = gmin0(dZde_p(i, j + 1, k2));
          const double ep3 = gmax0(dZde_p(i, j, k2)), ep4 = gmax0(dZde_p(i, j + 1, k1));
          const double xp5 = gmin0(dZdx_p(i, j, k1)), xp6 = gmin0(dZdx_p(i, j + 1, k2));
          const double xp7 = gmax0(dZdx_p(i, j, k2)), xp8 = gmax0(dZdx_p(i, j + 1, k1));
          const double er5 = gmin0(dZde_r(i - 1, j, k1)), er6 = gmin0(dZde_r(i, j, k2));
          const double er7 = gmax0(dZde_r(i - 1, j, k2)), er8 = gmax0(dZde_r(i, j, k1));
          UFsx2 = fac1 * (xr1 * (xr1 * dnUdz - dnUdx(i - 1, j, k1)) + xr2 * (xr2 * dnUdz - dnUdx(i, j, k2)) +
                          xr3 * (xr3 * dnUdz - dnUdx(i - 1, j, k2)) + xr4 * (xr4 * dnUdz - dnUdx(i, j, k1)));
          UFse2 = fac2 * (ep1 * (ep1 * dmUdz - dmUde(i, j, k1)) + ep2 * (ep2 * dmUdz - dmUde(i, j + 1, k2)) +
                          ep3 * (ep3 * dmUdz - dmUde(i, j, k2)) + ep4 * (ep4 * dmUdz - dmUde(i, j + 1, k1)));
          UFsx2 = UFsx2 +
                  fac1 * (ep1 * (xp5 * dnVdz - dnVdx(i, j, k1)) + ep2 * (xp6 * dnVdz - dnVdx(i, j + 1, k2)) +
                          ep3 * (xp7 * dnVdz - dnVdx(i, j, k2)) + ep4 * (xp8 * dnVdz - dnVdx(i, j + 1, k1)));
          UFse2 = UFse2 -
                  fac2 * (xr1 * (er5 * dmVdz - dmVde(i - 1, j, k1)) + xr2 * (er6 * dmVdz - dmVde(i, j, k2)) +
                          xr3 * (er7 * dmVdz - dmVde(i - 1, j, k2)) + xr4 * (er8 * dmVdz - dmVde(i, j, k1)));
        }
        if (do_v) {
          const long a = ao;
          double cff = 0.25 * (visc_r[a - ni] + visc_r[a]);
          const double fac1 = cff * c->F.on_v[a], fac2 = cff * c->F.om_v[a];
          cff = 0.5 * (pn[a - ni] + pn[a]);
          const double dnUdz = cff * 0.25 * (dUdz(i, j, k2) + dUdz(i + 1, j, k2) + dUdz(i, j - 1, k2) + dUdz(i + 1, j - 1, k2));
          const double dnVdz = cff * dVdz(i, j, k2);
          cff = 0.5 * (pm[a - ni] + pm[a]);
          const double dmUdz = cff * 0.25 * (dUdz(i, j, k2) + dUdz(i + 1, j, k2) + dUdz(i, j - 1, k2) + dUdz(i + 1, j - 1, k2));
          const double dmVdz = cff * dVdz(i, j, k2);
          const double xp1 = gmin0(dZdx_p(i, j, k1)), xp2 = gmin0(dZdx_p(i + 1, j, k2));
          const double xp3 = gmax0(dZdx_p(i, j, k2)), xp4 = gmax0(dZdx_p(i + 1, j, k1));
          const double er1 = gmin0(dZde_r(i, j - 1, k1)), er2 = gmin0(dZde_r(i, j, k2));
          const double er3 = gmax0(dZde_r(i, j - 1, k2)), er4 = gmax0(dZde_r(i, j, k1));
          const double xr5 = gmin0(dZdx_r(i, j - 1, k1)), xr6 = gmin0(dZdx_r(i, j, k2));
          const double xr7 = gmax0(dZdx_r(i, j - 1, k2)), xr8 = gmax0(dZdx_r(i, j, k1));
          const double ep5 = gmin0(dZde_p(i, j, k1)), ep6 = gmin0(dZde_p(i + 1, j, k2));
          const double ep7 = gmax0(dZde_p(i, j, k2)), ep8 = gmax0(dZde_p(i + 1, j, k1));
          VFsx2 = fac1 * (xp1 * (xp1 * dnVdz - dnVdx(i, j, k1)) + xp2 * (xp2 * dnVdz - dnVdx(i + 1, j, k2)) +
                          xp3 * (xp3 * dnVdz - dnVdx(i, j, k2)) + xp4 * (xp4 * dnVdz - dnVdx(i + 1, j, k1)));
          VFse2 = fac2 * (er1 * (er1 * dmVdz - dmVde(i, j - 1, k1)) + er2 * (er2 * dmVdz - dmVde(i, j, k2)) +
                          er3 * (er3 * dmVdz - dmVde(i, j - 1, k2)) + er4 * (er4 * dmVdz - dmVde(i, j, k1)));
          VFsx2 = VFsx2 -
                  fac1 * (er1 * (xr5 * dnUdz - dnUdx(i, j - 1, k1)) + er2 * (xr6 * dnUdz - dnUdx(i, j, k2)) +
                          er3 * (xr7 * dnUdz - dnUdx(i, j - 1, k2)) + er4 * (xr8 * dnUdz - dnUdx(i, j, k1)));
          VFse2 = VFse2 +
                  fac2 * (xp1 * (ep5 * dmUdz - dmUde(i, j, k1)) + xp2 * (ep6 * dmUdz - dmUde(i + 1, j, k2)) +
                          xp3 * (ep7 * dmUdz - dmUde(i, j, k2)) + xp4 * (ep8 * dmUdz - dmUde(i + 1, j, k1)));
        }
      }
    }
    __syncthreads();
    if (k > 0) {
      // ---- phase 3, level k
      const int i = io, j = jo;
      const long ak = ao + (long)(k - 1) * nij;
      if constexpr (MODE == UVGEO_FIRST) {
        // the first harmonic operator (uv3dmix4_geo.h:761-799)
        if (do_u) {
          const long a = ao;
          const double cff = 0.125 * (pm[a - 1] + pm[a]) * (pn[a - 1] + pn[a]);
          const double cff1 = 1.0 / (0.5 * (Hz[ak - 1] + Hz[ak]));
          double lap = cff * ((pn[a - 1] + pn[a]) * (UFx(i, j) - UFx(i - 1, j)) + (pm[a - 1] + pm[a]) * (UFe(i, j + 1) - UFe(i, j))) +
                       cff1 * ((UFsx2 + UFse2) - (UFsx1 + UFse1));
          if (msk) lap = lap * umaskw(c, a);
          un[ak] = lap;
        }
        if (do_v) {
          const long a = ao;
          const double cff = 0.125 * (pm[a] + pm[a - ni]) * (pn[a] + pn[a - ni]);
          const double cff1 = 1.0 / (0.5 * (Hz[ak - ni] + Hz[ak]));
          double lap = cff * ((pn[a - ni] + pn[a]) * (VFx(i + 1, j) - VFx(i, j)) - (pm[a - ni] + pm[a]) * (VFe(i, j) - VFe(i, j - 1))) +
                       cff1 * ((VFsx2 + VFse2) - (VFsx1 + VFse1));
          if (msk) lap = lap * vmaskw(c, a);
          vn[ak] = lap;
        }
      } else {
        // the time step; momentum is Hz*u, Hz*v here (uv3dmix2_geo.h:710-752, uv3dmix4_geo.h:1430-1474)
        if (do_u) {
          const long a = ao;
          const double cff = dt * 0.25 * (pm[a - 1] + pm[a]) * (pn[a - 1] + pn[a]);
          const double cff1 = 0.5 * (pn[a - 1] + pn[a]) * (UFx(i, j) - UFx(i - 1, j));
          const double cff2 = 0.5 * (pm[a - 1] + pm[a]) * (UFe(i, j + 1) - UFe(i, j));
          const double cff3 = UFsx2 - UFsx1;
          const double cff4 = UFse2 - UFse1;
          const double cff5 = cff * (cff1 + cff2);
          const double cff6 = dt * (cff3 + cff4);
          if constexpr (MODE == UVGEO_SECOND) {
            ruf = ruf - cff1 - cff2 - cff3 - cff4;
            un[ak] = un[ak] - cff5 - cff6;
          } else {
            ruf = ruf + cff1 + cff2 + cff3 + cff4;
            un[ak] = un[ak] + cff5 + cff6;
          }
        }
        if (do_v) {
          const long a = ao;
          const double cff = dt * 0.25 * (pm[a] + pm[a - ni]) * (pn[a] + pn[a - ni]);
          const double cff1 = 0.5 * (pn[a - ni] + pn[a]) * (VFx(i + 1, j) - VFx(i, j));
          const double cff2 = 0.5 * (pm[a - ni] + pm[a]) * (VFe(i, j) - VFe(i, j - 1));
          const double cff3 = VFsx2 - VFsx1;
          const double cff4 = VFse2 - VFse1;
          const double cff5 = cff * (cff1 - cff2);
          const double cff6 = dt * (cff3 + cff4);
          if constexpr (MODE == UVGEO_SECOND) {
            rvf = rvf - cff1 + cff2 - cff3 - cff4;
            vn[ak] = vn[ak] - cff5 - cff6;
          } else {
            rvf = rvf + cff1 - cff2 + cff3 + cff4;
            vn[ak] = vn[ak] + cff5 + cff6;
          }
        }
      }
    }
    UFsx1 = UFsx2; UFse1 = UFse2; VFsx1 = VFsx2; VFse1 = VFse2;
  }
  if constexpr (MODE != UVGEO_FIRST) {
    if (do_u) c->F.rufrc[ao] = ruf;
    if (do_v) c->F.rvfrc[ao] = rvf;
  }
#undef GL
#undef dZdx_p
#undef dZde_p
#undef dZdx_r
#undef dZde_r
#undef dnUdx
#undef dmUde
#undef dnVdx
#undef dmVde
#undef dUdz
#undef dVdz
#undef UFx
#undef VFe
#undef UFe
#undef VFx
}
#endif  // __HIPCC__
#endif
