/*
 * oracle_uvmix_geo.c -- TEST INFRASTRUCTURE ONLY: CPU restatement of
 *   uv3dmix2_geo_tile   ROMS/Nonlinear/uv3dmix2_geo.h:116-756 (UV_VIS2 with MIX_GEO_UV: harmonic viscosity rotated to
 *                       geopotential surfaces; roms_params_t.uv_vis2 = 2)
 *   uv3dmix4_geo_tile   ROMS/Nonlinear/uv3dmix4_geo.h:262-1478 (UV_VIS4 with MIX_GEO_UV: the biharmonic one, the rotated
 *                       harmonic operator applied twice; roms_params_t.uv_vis4 = 2)
 * loop for loop, with the reference's two-level slabs (k1, k2) and its order of operations; the level body the three
 * K_LOOPs share is stated once (geo_levels).  Pinned bit for bit against the reference built with MIX_GEO_UV instead of
 * MIX_S_UV (oracle/_ref/UPWELLING_GEOUV, SEAMOUNT_GEOUV, UPWELLING_MASK_GEOUV; tests/golden/ref_geouv.npz) and, for
 * the biharmonic operator, with UV_VIS4 as well (oracle/_ref/UPWELLING_GEOUV4, SEAMOUNT_GEOUV4, UPWELLING_MASK_GEOUV4,
 * UPWELLING_MASK_WET_GEOUV4; tests/golden/ref_geouv4.npz).  Never linked into the product.
 */
#include <stdio.h>
#include "oracle.h"

#define visc4_p(i,j)  F->visc4_p[I2(i,j)]
#define visc4_r(i,j)  F->visc4_r[I2(i,j)]

/* the loop ranges of a level body, (i from, i to, j from, j to) each: the slopes at u- and v-faces with dUdz, dVdz (U, V),
 * psi- and rho-points (P, R), the u- and v-points of the result (OU, OV) */
typedef struct { int U[4], V[4], P[4], R[4], OU[4], OV[4]; } geo_ranges_t;

/* what a level body does with the fluxes of a level: uv3dmix2_geo.h:710-752 (add to u, v(nnew), rufrc, rvfrc);
 * uv3dmix4_geo.h:761-799 (the first harmonic operator -> LapU, LapV); uv3dmix4_geo.h:1430-1474 (subtract) */
enum { GEO_HARM = 0, GEO_FIRST, GEO_SECOND };

/* K_LOOP of the rotated operator: uv3dmix2_geo.h:294-754, and K_LOOP1 (:322-801), K_LOOP2 (:981-1476) of uv3dmix4_geo.h,
 * which are the same statements on other ranges, velocities and coefficients, with Hz inside the horizontal fluxes or
 * not.  UU_, VV_: (LBi:UBi,LBj:UBj,N) arrays the gradients are taken of; vr_, vp_: the coefficient at rho- and
 * psi-points; LapU_, LapV_: (LBi:UBi,LBj:UBj,N), the result of GEO_FIRST. */
static void geo_levels(OARGS, const double *UU_, const double *VV_, const double *vr_, const double *vp_,
                       const geo_ranges_t *R, int mode, double *LapU_, double *LapV_)
{
  ORACLE_PROLOGUE
  const int nnew = s->nnew;
  const int hz_in_flux = mode != GEO_FIRST;
  const double dt = p->dt;
  const long n2 = nis * njs;
#define UU(i,j,k) UU_[I3(i,j,k)]
#define VV(i,j,k) VV_[I3(i,j,k)]
#define visc_r(i,j) vr_[I2(i,j)]
#define visc_p(i,j) vp_[I2(i,j)]
#define LapU(i,j,k) LapU_[I3(i,j,k)]
#define LapV(i,j,k) LapV_[I3(i,j,k)]
  double cff, fac1, fac2, pm_p, pn_p, cff1, cff2, cff3, cff4, cff5, cff6, cff7, cff8, dmUdz, dnUdz, dmVdz, dnVdz;
  double *UFe_ = walloc(n2), *VFe_ = walloc(n2), *UFx_ = walloc(n2), *VFx_ = walloc(n2);
  double *UFse_ = walloc(2 * n2), *UFsx_ = walloc(2 * n2), *VFse_ = walloc(2 * n2), *VFsx_ = walloc(2 * n2);
  double *dmUde_ = walloc(2 * n2), *dmVde_ = walloc(2 * n2), *dnUdx_ = walloc(2 * n2), *dnVdx_ = walloc(2 * n2);
  double *dUdz_ = walloc(2 * n2), *dVdz_ = walloc(2 * n2);
  double *dZde_p_ = walloc(2 * n2), *dZde_r_ = walloc(2 * n2), *dZdx_p_ = walloc(2 * n2), *dZdx_r_ = walloc(2 * n2);
#define UFe(i,j) UFe_[WS2(i,j)]
#define VFe(i,j) VFe_[WS2(i,j)]
#define UFx(i,j) UFx_[WS2(i,j)]
#define VFx(i,j) VFx_[WS2(i,j)]
#define SL(A,i,j,k) A[WS2(i,j) + (long)((k) - 1) * n2]
#define UFse(i,j,k) SL(UFse_,i,j,k)
#define UFsx(i,j,k) SL(UFsx_,i,j,k)
#define VFse(i,j,k) SL(VFse_,i,j,k)
#define VFsx(i,j,k) SL(VFsx_,i,j,k)
#define dmUde(i,j,k) SL(dmUde_,i,j,k)
#define dmVde(i,j,k) SL(dmVde_,i,j,k)
#define dnUdx(i,j,k) SL(dnUdx_,i,j,k)
#define dnVdx(i,j,k) SL(dnVdx_,i,j,k)
#define dUdz(i,j,k) SL(dUdz_,i,j,k)
#define dVdz(i,j,k) SL(dVdz_,i,j,k)
#define dZde_p(i,j,k) SL(dZde_p_,i,j,k)
#define dZde_r(i,j,k) SL(dZde_r_,i,j,k)
#define dZdx_p(i,j,k) SL(dZdx_p_,i,j,k)
#define dZdx_r(i,j,k) SL(dZdx_r_,i,j,k)
  int k1, k2 = 1;
  for (int k = 0; k <= N; k++) {
    k1 = k2;
    k2 = 3 - k1;
    if (k < N) {
      /* slopes at RHO- and PSI-points (:303-340) */
      for (int j = R->U[2]; j <= R->U[3]; j++)
        for (int i = R->U[0]; i <= R->U[1]; i++) {
          cff = 0.5 * (pm(i - 1, j) + pm(i, j));
          if (p->masking) cff = cff * umask(i, j);
          if (p->wet_dry) cff = cff * umask_wet(i, j);
          UFx(i, j) = cff * (z_r(i, j, k + 1) - z_r(i - 1, j, k + 1));
        }
      for (int j = R->V[2]; j <= R->V[3]; j++)
        for (int i = R->V[0]; i <= R->V[1]; i++) {
          cff = 0.5 * (pn(i, j - 1) + pn(i, j));
          if (p->masking) cff = cff * vmask(i, j);
          if (p->wet_dry) cff = cff * vmask_wet(i, j);
          VFe(i, j) = cff * (z_r(i, j, k + 1) - z_r(i, j - 1, k + 1));
        }
      for (int j = R->P[2]; j <= R->P[3]; j++)
        for (int i = R->P[0]; i <= R->P[1]; i++) {
          dZdx_p(i, j, k2) = 0.5 * (UFx(i, j - 1) + UFx(i, j));
          dZde_p(i, j, k2) = 0.5 * (VFe(i - 1, j) + VFe(i, j));
        }
      for (int j = R->R[2]; j <= R->R[3]; j++)
        for (int i = R->R[0]; i <= R->R[1]; i++) {
          dZdx_r(i, j, k2) = 0.5 * (UFx(i, j) + UFx(i + 1, j));
          dZde_r(i, j, k2) = 0.5 * (VFe(i, j) + VFe(i, j + 1));
        }
      /* horizontal gradients of momentum (:345-412) */
      for (int j = R->R[2]; j <= R->R[3]; j++)
        for (int i = R->R[0]; i <= R->R[1]; i++) {
          cff = 0.5 * pm(i, j);
          if (p->masking) cff = cff * rmask(i, j);
          if (p->wet_dry) cff = cff * rmask_wet(i, j);
          dnUdx(i, j, k2) = cff * ((pn(i, j) + pn(i + 1, j)) * UU(i + 1, j, k + 1) - (pn(i - 1, j) + pn(i, j)) * UU(i, j, k + 1));
        }
      for (int j = R->P[2]; j <= R->P[3]; j++)
        for (int i = R->P[0]; i <= R->P[1]; i++) {
          cff = 0.125 * (pn(i - 1, j) + pn(i, j) + pn(i - 1, j - 1) + pn(i, j - 1));
          if (p->masking) cff = cff * pmask(i, j);
          if (p->wet_dry) cff = cff * pmask_wet(i, j);
          dmUde(i, j, k2) = cff * ((pm(i - 1, j) + pm(i, j)) * UU(i, j, k + 1) - (pm(i - 1, j - 1) + pm(i, j - 1)) * UU(i, j - 1, k + 1));
        }
      for (int j = R->P[2]; j <= R->P[3]; j++)
        for (int i = R->P[0]; i <= R->P[1]; i++) {
          cff = 0.125 * (pm(i - 1, j) + pm(i, j) + pm(i - 1, j - 1) + pm(i, j - 1));
          if (p->masking) cff = cff * pmask(i, j);
          if (p->wet_dry) cff = cff * pmask_wet(i, j);
          dnVdx(i, j, k2) = cff * ((pn(i, j - 1) + pn(i, j)) * VV(i, j, k + 1) - (pn(i - 1, j - 1) + pn(i - 1, j)) * VV(i - 1, j, k + 1));
        }
      for (int j = R->R[2]; j <= R->R[3]; j++)
        for (int i = R->R[0]; i <= R->R[1]; i++) {
          cff = 0.5 * pn(i, j);
          if (p->masking) cff = cff * rmask(i, j);
          if (p->wet_dry) cff = cff * rmask_wet(i, j);
          dmVde(i, j, k2) = cff * ((pm(i, j) + pm(i, j + 1)) * VV(i, j + 1, k + 1) - (pm(i, j - 1) + pm(i, j)) * VV(i, j, k + 1));
        }
    }
    if (k == 0 || k == N) {
      for (int j = R->U[2]; j <= R->U[3]; j++)
        for (int i = R->U[0]; i <= R->U[1]; i++) dUdz(i, j, k2) = 0.0;
      for (int j = R->V[2]; j <= R->V[3]; j++)
        for (int i = R->V[0]; i <= R->V[1]; i++) dVdz(i, j, k2) = 0.0;
      for (int j = R->OU[2]; j <= R->OU[3]; j++)
        for (int i = R->OU[0]; i <= R->OU[1]; i++) { UFsx(i, j, k2) = 0.0; UFse(i, j, k2) = 0.0; }
      for (int j = R->OV[2]; j <= R->OV[3]; j++)
        for (int i = R->OV[0]; i <= R->OV[1]; i++) { VFsx(i, j, k2) = 0.0; VFse(i, j, k2) = 0.0; }
    } else {
      for (int j = R->U[2]; j <= R->U[3]; j++)
        for (int i = R->U[0]; i <= R->U[1]; i++) {
          cff = 1.0 / (0.5 * (z_r(i - 1, j, k + 1) - z_r(i - 1, j, k) + z_r(i, j, k + 1) - z_r(i, j, k)));
          dUdz(i, j, k2) = cff * (UU(i, j, k + 1) - UU(i, j, k));
        }
      for (int j = R->V[2]; j <= R->V[3]; j++)
        for (int i = R->V[0]; i <= R->V[1]; i++) {
          cff = 1.0 / (0.5 * (z_r(i, j - 1, k + 1) - z_r(i, j - 1, k) + z_r(i, j, k + 1) - z_r(i, j, k)));
          dVdz(i, j, k2) = cff * (VV(i, j, k + 1) - VV(i, j, k));
        }
    }
    if (k > 0) {
      /* rotated viscous flux along geopotentials, XI- and ETA-components (:463-541) */
      for (int j = R->R[2]; j <= R->R[3]; j++)
        for (int i = R->R[0]; i <= R->R[1]; i++) {
          cff1 = MIN(dZdx_r(i, j, k1), 0.0);
          cff2 = MAX(dZdx_r(i, j, k1), 0.0);
          cff3 = MIN(dZde_r(i, j, k1), 0.0);
          cff4 = MAX(dZde_r(i, j, k1), 0.0);
          cff = on_r(i, j) * (dnUdx(i, j, k1) - 0.5 * pn(i, j) * (cff1 * (dUdz(i, j, k1) + dUdz(i + 1, j, k2)) + cff2 * (dUdz(i, j, k2) + dUdz(i + 1, j, k1)))) -
                om_r(i, j) * (dmVde(i, j, k1) - 0.5 * pm(i, j) * (cff3 * (dVdz(i, j, k1) + dVdz(i, j + 1, k2)) + cff4 * (dVdz(i, j, k2) + dVdz(i, j + 1, k1))));
          if (hz_in_flux) cff = Hz(i, j, k) * cff;        /* not in the first operator of uv3dmix4_geo.h (:501-512) */
          if (p->masking) cff = cff * rmask(i, j);
          if (p->wet_dry) cff = cff * rmask_wet(i, j);
          UFx(i, j) = on_r(i, j) * on_r(i, j) * visc_r(i, j) * cff;
          VFe(i, j) = om_r(i, j) * om_r(i, j) * visc_r(i, j) * cff;
        }
      for (int j = R->P[2]; j <= R->P[3]; j++)
        for (int i = R->P[0]; i <= R->P[1]; i++) {
          pm_p = 0.25 * (pm(i - 1, j - 1) + pm(i - 1, j) + pm(i, j - 1) + pm(i, j));
          pn_p = 0.25 * (pn(i - 1, j - 1) + pn(i - 1, j) + pn(i, j - 1) + pn(i, j));
          cff1 = MIN(dZdx_p(i, j, k1), 0.0);
          cff2 = MAX(dZdx_p(i, j, k1), 0.0);
          cff3 = MIN(dZde_p(i, j, k1), 0.0);
          cff4 = MAX(dZde_p(i, j, k1), 0.0);
          cff = on_p(i, j) * (dnVdx(i, j, k1) - 0.5 * pn_p * (cff1 * (dVdz(i - 1, j, k1) + dVdz(i, j, k2)) + cff2 * (dVdz(i - 1, j, k2) + dVdz(i, j, k1)))) +
                om_p(i, j) * (dmUde(i, j, k1) - 0.5 * pm_p * (cff3 * (dUdz(i, j - 1, k1) + dUdz(i, j, k2)) + cff4 * (dUdz(i, j - 1, k2) + dUdz(i, j, k1))));
          if (hz_in_flux) cff = 0.25 * (Hz(i - 1, j, k) + Hz(i, j, k) + Hz(i - 1, j - 1, k) + Hz(i, j - 1, k)) * cff;
          if (p->masking) cff = cff * pmask(i, j);
          if (p->wet_dry) cff = cff * pmask_wet(i, j);
          UFe(i, j) = om_p(i, j) * om_p(i, j) * visc_p(i, j) * cff;
          VFx(i, j) = on_p(i, j) * on_p(i, j) * visc_p(i, j) * cff;
        }
      /* vertical flux due to the sloping coordinate surfaces (:546-700) */
      if (k < N) {
        for (int j = R->OU[2]; j <= R->OU[3]; j++)
          for (int i = R->OU[0]; i <= R->OU[1]; i++) {
            cff = 0.25 * (visc_r(i - 1, j) + visc_r(i, j));
            fac1 = cff * on_u(i, j);
            fac2 = cff * om_u(i, j);
            cff = 0.5 * (pn(i - 1, j) + pn(i, j));
            dnUdz = cff * dUdz(i, j, k2);
            dnVdz = cff * 0.25 * (dVdz(i - 1, j + 1, k2) + dVdz(i, j + 1, k2) + dVdz(i - 1, j, k2) + dVdz(i, j, k2));
            cff = 0.5 * (pm(i - 1, j) + pm(i, j));
            dmUdz = cff * dUdz(i, j, k2);
            dmVdz = cff * 0.25 * (dVdz(i - 1, j + 1, k2) + dVdz(i, j + 1, k2) + dVdz(i - 1, j, k2) + dVdz(i, j, k2));
            cff1 = MIN(dZdx_r(i - 1, j, k1), 0.0);
            cff2 = MIN(dZdx_r(i, j, k2), 0.0);
            cff3 = MAX(dZdx_r(i - 1, j, k2), 0.0);
            cff4 = MAX(dZdx_r(i, j, k1), 0.0);
            UFsx(i, j, k2) = fac1 * (cff1 * (cff1 * dnUdz - dnUdx(i - 1, j, k1)) + cff2 * (cff2 * dnUdz - dnUdx(i, j, k2)) +
                                     cff3 * (cff3 * dnUdz - dnUdx(i - 1, j, k2)) + cff4 * (cff4 * dnUdz - dnUdx(i, j, k1)));
            cff1 = MIN(dZde_p(i, j, k1), 0.0);
            cff2 = MIN(dZde_p(i, j + 1, k2), 0.0);
            cff3 = MAX(dZde_p(i, j, k2), 0.0);
            cff4 = MAX(dZde_p(i, j + 1, k1), 0.0);
            UFse(i, j, k2) = fac2 * (cff1 * (cff1 * dmUdz - dmUde(i, j, k1)) + cff2 * (cff2 * dmUdz - dmUde(i, j + 1, k2)) +
                                     cff3 * (cff3 * dmUdz - dmUde(i, j, k2)) + cff4 * (cff4 * dmUdz - dmUde(i, j + 1, k1)));
            cff1 = MIN(dZde_p(i, j, k1), 0.0);
            cff2 = MIN(dZde_p(i, j + 1, k2), 0.0);
            cff3 = MAX(dZde_p(i, j, k2), 0.0);
            cff4 = MAX(dZde_p(i, j + 1, k1), 0.0);
            cff5 = MIN(dZdx_p(i, j, k1), 0.0);
            cff6 = MIN(dZdx_p(i, j + 1, k2), 0.0);
            cff7 = MAX(dZdx_p(i, j, k2), 0.0);
            cff8 = MAX(dZdx_p(i, j + 1, k1), 0.0);
            UFsx(i, j, k2) = UFsx(i, j, k2) +
                             fac1 * (cff1 * (cff5 * dnVdz - dnVdx(i, j, k1)) + cff2 * (cff6 * dnVdz - dnVdx(i, j + 1, k2)) +
                                     cff3 * (cff7 * dnVdz - dnVdx(i, j, k2)) + cff4 * (cff8 * dnVdz - dnVdx(i, j + 1, k1)));
            cff1 = MIN(dZdx_r(i - 1, j, k1), 0.0);
            cff2 = MIN(dZdx_r(i, j, k2), 0.0);
            cff3 = MAX(dZdx_r(i - 1, j, k2), 0.0);
            cff4 = MAX(dZdx_r(i, j, k1), 0.0);
            cff5 = MIN(dZde_r(i - 1, j, k1), 0.0);
            cff6 = MIN(dZde_r(i, j, k2), 0.0);
            cff7 = MAX(dZde_r(i - 1, j, k2), 0.0);
            cff8 = MAX(dZde_r(i, j, k1), 0.0);
            UFse(i, j, k2) = UFse(i, j, k2) -
                             fac2 * (cff1 * (cff5 * dmVdz - dmVde(i - 1, j, k1)) + cff2 * (cff6 * dmVdz - dmVde(i, j, k2)) +
                                     cff3 * (cff7 * dmVdz - dmVde(i - 1, j, k2)) + cff4 * (cff8 * dmVdz - dmVde(i, j, k1)));
          }
        for (int j = R->OV[2]; j <= R->OV[3]; j++)
          for (int i = R->OV[0]; i <= R->OV[1]; i++) {
            cff = 0.25 * (visc_r(i, j - 1) + visc_r(i, j));
            fac1 = cff * on_v(i, j);
            fac2 = cff * om_v(i, j);
            cff = 0.5 * (pn(i, j - 1) + pn(i, j));
            dnUdz = cff * 0.25 * (dUdz(i, j, k2) + dUdz(i + 1, j, k2) + dUdz(i, j - 1, k2) + dUdz(i + 1, j - 1, k2));
            dnVdz = cff * dVdz(i, j, k2);
            cff = 0.5 * (pm(i, j - 1) + pm(i, j));
            dmUdz = cff * 0.25 * (dUdz(i, j, k2) + dUdz(i + 1, j, k2) + dUdz(i, j - 1, k2) + dUdz(i + 1, j - 1, k2));
            dmVdz = cff * dVdz(i, j, k2);
            cff1 = MIN(dZdx_p(i, j, k1), 0.0);
            cff2 = MIN(dZdx_p(i + 1, j, k2), 0.0);
            cff3 = MAX(dZdx_p(i, j, k2), 0.0);
            cff4 = MAX(dZdx_p(i + 1, j, k1), 0.0);
            VFsx(i, j, k2) = fac1 * (cff1 * (cff1 * dnVdz - dnVdx(i, j, k1)) + cff2 * (cff2 * dnVdz - dnVdx(i + 1, j, k2)) +
                                     cff3 * (cff3 * dnVdz - dnVdx(i, j, k2)) + cff4 * (cff4 * dnVdz - dnVdx(i + 1, j, k1)));
            cff1 = MIN(dZde_r(i, j - 1, k1), 0.0);
            cff2 = MIN(dZde_r(i, j, k2), 0.0);
            cff3 = MAX(dZde_r(i, j - 1, k2), 0.0);
            cff4 = MAX(dZde_r(i, j, k1), 0.0);
            VFse(i, j, k2) = fac2 * (cff1 * (cff1 * dmVdz - dmVde(i, j - 1, k1)) + cff2 * (cff2 * dmVdz - dmVde(i, j, k2)) +
                                     cff3 * (cff3 * dmVdz - dmVde(i, j - 1, k2)) + cff4 * (cff4 * dmVdz - dmVde(i, j, k1)));
            cff1 = MIN(dZde_r(i, j - 1, k1), 0.0);
            cff2 = MIN(dZde_r(i, j, k2), 0.0);
            cff3 = MAX(dZde_r(i, j - 1, k2), 0.0);
            cff4 = MAX(dZde_r(i, j, k1), 0.0);
            cff5 = MIN(dZdx_r(i, j - 1, k1), 0.0);
            cff6 = MIN(dZdx_r(i, j, k2), 0.0);
            cff7 = MAX(dZdx_r(i, j - 1, k2), 0.0);
            cff8 = MAX(dZdx_r(i, j, k1), 0.0);
            VFsx(i, j, k2) = VFsx(i, j, k2) -
                             fac1 * (cff1 * (cff5 * dnUdz - dnUdx(i, j - 1, k1)) + cff2 * (cff6 * dnUdz - dnUdx(i, j, k2)) +
                                     cff3 * (cff7 * dnUdz - dnUdx(i, j - 1, k2)) + cff4 * (cff8 * dnUdz - dnUdx(i, j, k1)));
            cff1 = MIN(dZdx_p(i, j, k1), 0.0);
            cff2 = MIN(dZdx_p(i + 1, j, k2), 0.0);
            cff3 = MAX(dZdx_p(i, j, k2), 0.0);
            cff4 = MAX(dZdx_p(i + 1, j, k1), 0.0);
            cff5 = MIN(dZde_p(i, j, k1), 0.0);
            cff6 = MIN(dZde_p(i + 1, j, k2), 0.0);
            cff7 = MAX(dZde_p(i, j, k2), 0.0);
            cff8 = MAX(dZde_p(i + 1, j, k1), 0.0);
            VFse(i, j, k2) = VFse(i, j, k2) +
                             fac2 * (cff1 * (cff5 * dmUdz - dmUde(i, j, k1)) + cff2 * (cff6 * dmUdz - dmUde(i + 1, j, k2)) +
                                     cff3 * (cff7 * dmUdz - dmUde(i, j, k2)) + cff4 * (cff8 * dmUdz - dmUde(i + 1, j, k1)));
          }
      }
      if (mode == GEO_FIRST) {
        /* first harmonic operator (m s^-3/2), uv3dmix4_geo.h:761-799 */
        for (int j = R->OU[2]; j <= R->OU[3]; j++)
          for (int i = R->OU[0]; i <= R->OU[1]; i++) {
            cff = 0.125 * (pm(i - 1, j) + pm(i, j)) * (pn(i - 1, j) + pn(i, j));
            cff1 = 1.0 / (0.5 * (Hz(i - 1, j, k) + Hz(i, j, k)));
            LapU(i, j, k) = cff * ((pn(i - 1, j) + pn(i, j)) * (UFx(i, j) - UFx(i - 1, j)) +
                                   (pm(i - 1, j) + pm(i, j)) * (UFe(i, j + 1) - UFe(i, j))) +
                            cff1 * ((UFsx(i, j, k2) + UFse(i, j, k2)) - (UFsx(i, j, k1) + UFse(i, j, k1)));
            if (p->masking) LapU(i, j, k) = LapU(i, j, k) * umask(i, j);
            if (p->wet_dry) LapU(i, j, k) = LapU(i, j, k) * umask_wet(i, j);
          }
        for (int j = R->OV[2]; j <= R->OV[3]; j++)
          for (int i = R->OV[0]; i <= R->OV[1]; i++) {
            cff = 0.125 * (pm(i, j) + pm(i, j - 1)) * (pn(i, j) + pn(i, j - 1));
            cff1 = 1.0 / (0.5 * (Hz(i, j - 1, k) + Hz(i, j, k)));
            LapV(i, j, k) = cff * ((pn(i, j - 1) + pn(i, j)) * (VFx(i + 1, j) - VFx(i, j)) -
                                   (pm(i, j - 1) + pm(i, j)) * (VFe(i, j) - VFe(i, j - 1))) +
                            cff1 * ((VFsx(i, j, k2) + VFse(i, j, k2)) - (VFsx(i, j, k1) + VFse(i, j, k1)));
            if (p->masking) LapV(i, j, k) = LapV(i, j, k) * vmask(i, j);
            if (p->wet_dry) LapV(i, j, k) = LapV(i, j, k) * vmask_wet(i, j);
          }
        continue;
      }
      /* time-step the term; momentum is HzU, HzV here (uv3dmix2_geo.h:710-752 added, uv3dmix4_geo.h:1430-1474
       * subtracted term by term) */
      for (int j = R->OU[2]; j <= R->OU[3]; j++)
        for (int i = R->OU[0]; i <= R->OU[1]; i++) {
          cff = dt * 0.25 * (pm(i - 1, j) + pm(i, j)) * (pn(i - 1, j) + pn(i, j));
          cff1 = 0.5 * (pn(i - 1, j) + pn(i, j)) * (UFx(i, j) - UFx(i - 1, j));
          cff2 = 0.5 * (pm(i - 1, j) + pm(i, j)) * (UFe(i, j + 1) - UFe(i, j));
          cff3 = UFsx(i, j, k2) - UFsx(i, j, k1);
          cff4 = UFse(i, j, k2) - UFse(i, j, k1);
          cff5 = cff * (cff1 + cff2);
          cff6 = dt * (cff3 + cff4);
          if (mode == GEO_HARM) {
            rufrc(i, j) = rufrc(i, j) + cff1 + cff2 + cff3 + cff4;
            u(i, j, k, nnew) = u(i, j, k, nnew) + cff5 + cff6;
          } else {
            rufrc(i, j) = rufrc(i, j) - cff1 - cff2 - cff3 - cff4;
            u(i, j, k, nnew) = u(i, j, k, nnew) - cff5 - cff6;
          }
        }
      for (int j = R->OV[2]; j <= R->OV[3]; j++)
        for (int i = R->OV[0]; i <= R->OV[1]; i++) {
          cff = dt * 0.25 * (pm(i, j) + pm(i, j - 1)) * (pn(i, j) + pn(i, j - 1));
          cff1 = 0.5 * (pn(i, j - 1) + pn(i, j)) * (VFx(i + 1, j) - VFx(i, j));
          cff2 = 0.5 * (pm(i, j - 1) + pm(i, j)) * (VFe(i, j) - VFe(i, j - 1));
          cff3 = VFsx(i, j, k2) - VFsx(i, j, k1);
          cff4 = VFse(i, j, k2) - VFse(i, j, k1);
          cff5 = cff * (cff1 - cff2);
          cff6 = dt * (cff3 + cff4);
          if (mode == GEO_HARM) {
            rvfrc(i, j) = rvfrc(i, j) + cff1 - cff2 + cff3 + cff4;
            v(i, j, k, nnew) = v(i, j, k, nnew) + cff5 + cff6;
          } else {
            rvfrc(i, j) = rvfrc(i, j) - cff1 + cff2 - cff3 - cff4;
            v(i, j, k, nnew) = v(i, j, k, nnew) - cff5 - cff6;
          }
        }
    }
  }
  free(UFe_); free(VFe_); free(UFx_); free(VFx_); free(UFse_); free(UFsx_); free(VFse_); free(VFsx_);
  free(dmUde_); free(dmVde_); free(dnUdx_); free(dnVdx_); free(dUdz_); free(dVdz_);
  free(dZde_p_); free(dZde_r_); free(dZdx_p_); free(dZdx_r_);
}

/* the loop ranges of uv3dmix2_geo.h and of K_LOOP2 of uv3dmix4_geo.h */
static geo_ranges_t geo_tile_ranges(const roms_bounds_t *b)
{
  const geo_ranges_t R = {{b->IstrU - 1, b->Iend + 1, b->Jstr - 1, b->Jend + 1}, {b->Istr - 1, b->Iend + 1, b->JstrV - 1, b->Jend + 1},
                          {b->Istr, b->Iend + 1, b->Jstr, b->Jend + 1},          {b->IstrU - 1, b->Iend, b->JstrV - 1, b->Jend},
                          {b->IstrU, b->Iend, b->Jstr, b->Jend},                 {b->Istr, b->Iend, b->JstrV, b->Jend}};
  return R;
}

/* MIX_GEO_UV is one CPP switch for both operators (uv3dmix.F:21-34): when uv_vis2 and uv_vis4 are both set, both are 1
 * (MIX_S_UV) or both are 2 (MIX_GEO_UV); (1, 2) and (2, 1) are a model the reference cannot be compiled to */
static char o_error_text[256];
const char *oracle_last_error(void) { return o_error_text; }
int o_uv_mix_check(const roms_params_t *p, const char *where)
{
  if (p->uv_vis2 && p->uv_vis4 && (p->uv_vis2 == 2) != (p->uv_vis4 == 2)) {
    snprintf(o_error_text, sizeof o_error_text,
             "%s: uv_vis2 = %d and uv_vis4 = %d disagree about MIX_GEO_UV: when both are set both are 1 (MIX_S_UV) or both "
             "are 2 (MIX_GEO_UV), one CPP switch in the reference (uv3dmix.F:21-34)", where, p->uv_vis2, p->uv_vis4);
    return 12;
  }
  return 0;
}

int oracle_uv3dmix2_geo(OARGS)
{
  ORACLE_PROLOGUE
  const geo_ranges_t R = geo_tile_ranges(b);
  const double *UU_ = &u(LBi, LBj, 1, s->nrhs), *VV_ = &v(LBi, LBj, 1, s->nrhs);
  geo_levels(b, p, s, F, UU_, VV_, F->visc2_r, F->visc2_p, &R, GEO_HARM, NULL, NULL);
  return 0;
}

/* uv3dmix4_geo_tile -- uv3dmix4_geo.h:262-1478 (UV_VIS4 with MIX_GEO_UV; roms_params_t.uv_vis4 = 2): the rotated
 * harmonic operator twice, LapU, LapV between them with the rule for closed or gradient edges and the corners */
int oracle_uv3dmix4_geo(OARGS)
{
  ORACLE_PROLOGUE
  const double gamma2 = p->gamma2;
  if (b->NghostPoints != 3) return 8;                        /* inp_par.F:268-270 */
  if (s->nrhs == s->nnew) return 9;
  const geo_ranges_t R1 = {{IstrUm2, Iendp2, Jstrm2, Jendp2}, {Istrm2, Iendp2, JstrVm2, Jendp2},     /* K_LOOP1, :330-799 */
                           {Istrm1, Iendp2, Jstrm1, Jendp2},  {IstrUm2, Iendp1, JstrVm2, Jendp1},
                           {IstrUm1, Iendp1, Jstrm1, Jendp1}, {Istrm1, Iendp1, JstrVm1, Jendp1}};
  const geo_ranges_t R2 = geo_tile_ranges(b);
  const double *UU_ = &u(LBi, LBj, 1, s->nrhs), *VV_ = &v(LBi, LBj, 1, s->nrhs);
  double *LapU_ = walloc(n3r), *LapV_ = walloc(n3r);
  geo_levels(b, p, s, F, UU_, VV_, F->visc4_r, F->visc4_p, &R1, GEO_FIRST, LapU_, LapV_);
  /* closed or gradient conditions (except periodic) on the first operator, :806-928 */
  if (!EWperiodic) {
    if (west_edge) {
      const int cu = o_lbc(p, LBS_WEST, LBV_U) == LBC_CLOSED, cv = o_lbc(p, LBS_WEST, LBV_V) == LBC_CLOSED;
      for (int k = 1; k <= N; k++) {
        for (int j = Jstrm1; j <= Jendp1; j++) LapU(IstrU - 1, j, k) = cu ? 0.0 : LapU(IstrU, j, k);
        for (int j = JstrVm1; j <= Jendp1; j++) LapV(Istr - 1, j, k) = cv ? gamma2 * LapV(Istr, j, k) : 0.0;
      }
    }
    if (east_edge) {
      const int cu = o_lbc(p, LBS_EAST, LBV_U) == LBC_CLOSED, cv = o_lbc(p, LBS_EAST, LBV_V) == LBC_CLOSED;
      for (int k = 1; k <= N; k++) {
        for (int j = Jstrm1; j <= Jendp1; j++) LapU(Iend + 1, j, k) = cu ? 0.0 : LapU(Iend, j, k);
        for (int j = JstrVm1; j <= Jendp1; j++) LapV(Iend + 1, j, k) = cv ? gamma2 * LapV(Iend, j, k) : 0.0;
      }
    }
  }
  if (!NSperiodic) {
    if (south_edge) {
      const int cu = o_lbc(p, LBS_SOUTH, LBV_U) == LBC_CLOSED, cv = o_lbc(p, LBS_SOUTH, LBV_V) == LBC_CLOSED;
      for (int k = 1; k <= N; k++) {
        for (int i = IstrUm1; i <= Iendp1; i++) LapU(i, Jstr - 1, k) = cu ? gamma2 * LapU(i, Jstr, k) : 0.0;
        for (int i = Istrm1; i <= Iendp1; i++) LapV(i, JstrV - 1, k) = cv ? 0.0 : LapV(i, JstrV, k);
      }
    }
    if (north_edge) {
      const int cu = o_lbc(p, LBS_NORTH, LBV_U) == LBC_CLOSED, cv = o_lbc(p, LBS_NORTH, LBV_V) == LBC_CLOSED;
      for (int k = 1; k <= N; k++) {
        for (int i = IstrUm1; i <= Iendp1; i++) LapU(i, Jend + 1, k) = cu ? gamma2 * LapU(i, Jend, k) : 0.0;
        for (int i = Istrm1; i <= Iendp1; i++) LapV(i, Jend + 1, k) = cv ? 0.0 : LapV(i, Jend, k);
      }
    }
  }
  if (!(NSperiodic || EWperiodic))                     /* corners, :930-976 */
    for (int k = 1; k <= N; k++) {
      if (south_edge && west_edge) {
        LapU(Istr, Jstr - 1, k) = 0.5 * (LapU(Istr + 1, Jstr - 1, k) + LapU(Istr, Jstr, k));
        LapV(Istr - 1, Jstr, k) = 0.5 * (LapV(Istr - 1, Jstr + 1, k) + LapV(Istr, Jstr, k));
      }
      if (south_edge && east_edge) {
        LapU(Iend + 1, Jstr - 1, k) = 0.5 * (LapU(Iend, Jstr - 1, k) + LapU(Iend + 1, Jstr, k));
        LapV(Iend + 1, Jstr, k) = 0.5 * (LapV(Iend, Jstr, k) + LapV(Iend + 1, Jstr + 1, k));
      }
      if (north_edge && west_edge) {
        LapU(Istr, Jend + 1, k) = 0.5 * (LapU(Istr + 1, Jend + 1, k) + LapU(Istr, Jend, k));
        LapV(Istr - 1, Jend + 1, k) = 0.5 * (LapV(Istr, Jend + 1, k) + LapV(Istr - 1, Jend, k));
      }
      if (north_edge && east_edge) {
        LapU(Iend + 1, Jend + 1, k) = 0.5 * (LapU(Iend, Jend + 1, k) + LapU(Iend + 1, Jend, k));
        LapV(Iend + 1, Jend + 1, k) = 0.5 * (LapV(Iend, Jend + 1, k) + LapV(Iend + 1, Jend, k));
      }
    }
  /* the second rotated harmonic operator, on LapU, LapV with Hz in the fluxes, and the time step, :981-1476 */
  geo_levels(b, p, s, F, LapU_, LapV_, F->visc4_r, F->visc4_p, &R2, GEO_SECOND, NULL, NULL);
  free(LapU_); free(LapV_);
  return 0;
}
