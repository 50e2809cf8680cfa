// k_step2d.hip -- split-explicit barotropic engine, step2d_tile
// (ROMS/Nonlinear/step2d_LF_AM3.h:137-2528: leap-frog predictor / Adams-Moulton
// corrector) and the LOOP_2D sequencing of main3d.F:592-700.
//
// Inside LOOP_2D, with closed or periodic edges and none of UV_VIS4, WET_DRY and point sources, a step2d call is ONE
// launch of the fused k2d_mom_lds<true> (k_step2d_mom.hip: free surface, fast-time averages and momentum together,
// zeta_new and zwrk kept in LDS) plus, on several tiles, one batched halo exchange.  The kernels of this file serve
// the other calls:
//   k2d_avg_last  the last predictor of the loop on one E-W periodic tile, which only finishes the fast-time averages
//   k2d_flux      DUon, DVom two points into the halo (:509-544)
//   k2d_zeta      fast-time averaging (:614-682) and the free-surface step (:770-868): zeta(knew), rzeta(krhs);
//                 zeta_new and zwrk go to device scratch on the extended range so that the momentum kernel can use
//                 them at i-1 / j-1 without another exchange
// the last two followed by k2d_mom_lds<false>, with the reference's boundary-condition and halo calls in between
// (step2d_impl).  The point formulas shared with the fused kernel are in step2d_common.h.  The reference's ~25 private
// (IminS:ImaxS,JminS:JmaxS) work arrays become registers / LDS; only DUon, DVom, zeta_new, zwrk live in device scratch.
#include "step2d_common.h"
#include <cstdlib>
#include <map>

int roms_launch_step2d_visc4(int krhs);      // k_uv3dmix2.hip
int roms_uv_adv_check(const char *where);    // k_rhs3d.hip

namespace {

__global__ void __launch_bounds__(BLK_X *BLK_Y)
k2d_flux(const RomsDev *__restrict__ c, S2 s, double *__restrict__ DUon, double *__restrict__ DVom)
{
  DEV_PROLOGUE(c)
  const int i = b.IstrU - 2 + blockIdx.x * BLK_X + threadIdx.x;
  const int j = b.JstrV - 2 + blockIdx.y * BLK_Y + threadIdx.y;
  if (i > b.Iendp2 || j > b.Jendp2) return;
  const gcd_t zeta = (gcd_t)(c->F.zeta + (long)(s.krhs - 1) * nij);
  const gcd_t h = (gcd_t)(c->F.h);
  const long a = I2(i, j);
  const double Drhs = zeta[a] + h[a];
  if (i >= b.IstrU - 1)
    DUon[a] = flux_u(GF(ubar)[a + (long)(s.krhs - 1) * nij], GF(on_u)[a], Drhs, zeta[a - 1] + h[a - 1]);
  if (j >= b.JstrV - 1)
    DVom[a] = flux_v(GF(vbar)[a + (long)(s.krhs - 1) * nij], GF(om_v)[a], Drhs, zeta[a - ni] + h[a - ni]);
}

__global__ void __launch_bounds__(BLK_X *BLK_Y)
k2d_zeta(const RomsDev *__restrict__ c, S2 s, const double *__restrict__ DUon, const double *__restrict__ DVom,
         double *__restrict__ zeta_new, double *__restrict__ zwrk)
{
  DEV_PROLOGUE(c)
  // thread range covers both the averaging range (IstrR:IendR,JstrR:JendR) and
  // the extended zeta range (IstrU-1:Iend, JstrV-1:Jend)
  const int i0 = min(b.IstrR, b.IstrU - 1), j0 = min(b.JstrR, b.JstrV - 1);
  const int i = i0 + blockIdx.x * BLK_X + threadIdx.x;
  const int j = j0 + blockIdx.y * BLK_Y + threadIdx.y;
  if (i > b.IendR || j > b.JendR) return;
  const roms_params_t &p = c->p;
  const long a = I2(i, j);
  // ---- fast-time averaging, :614-682 ----
  if (i >= b.IstrR && j >= b.JstrR) {
    const bool inU = i >= b.Istr, inV = j >= b.Jstr;
    average_point(c, s, a, inU, inV, inU ? DUon[a] : 0.0, inV ? DVom[a] : 0.0, nij);
  }
  if (s.iif > p.nfast) return;
  // ---- free surface, :770-868 ----
  // on the extended range: the low-side ghost values of zeta(knew) computed here are, bit for bit, what the exchange
  // delivers later; rzeta(krhs) on the owned points only
  if (i < b.IstrU - 1 || i > b.Iend || j < b.JstrV - 1 || j > b.Jend) return;
  const bool masking = p.masking != 0, am3z = !(s.iif == 1 || s.predictor);
  const double rhs = (DUon[a] - DUon[a + 1]) + (DVom[a] - DVom[a + ni]);
  const double rm = masking ? (double)GF(rmask)[a] : 1.0;
  double zn, zw;
  zeta_step(p, s, rhs, GF(pm)[a], GF(pn)[a], GF(zeta)[a + (long)(s.kstp - 1) * nij], GF(zeta)[a + (long)(s.krhs - 1) * nij],
            am3z ? (double)GF(rzeta)[a + (long)(s.kstp - 1) * nij] : 0.0,
            am3z ? (double)GF(rzeta)[a + (long)(3 - s.kstp - 1) * nij] : 0.0, rm, masking, zn, zw);
  zeta_new[a] = zn;
  zwrk[a] = zw;
  // WET_DRY && MASKING, :863-866: the shared array (not zeta_new) keeps the total depth of a land cell at Dcrit
  GF(zeta)[a + (long)(s.knew - 1) * nij] = (p.wet_dry && masking) ? zn + (p.Dcrit - GF(h)[a]) * (1.0 - rm) : zn;
  if (s.predictor && i >= b.Istr && j >= b.Jstr) GF(rzeta)[a + (long)(s.krhs - 1) * nij] = rhs;
}

// The last predictor of LOOP_2D (iif = nfast+1) on one E-W periodic tile: it only finishes the fast-time averages,
// with DUon / DVom evaluated in place.  (Not merged with the averaging half of k2d_zeta: that one reads exchanged
// fluxes from scratch, and choosing between the two sources would be a new branch per point in both.)
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k2d_avg_last(const RomsDev *__restrict__ c, S2 s)
{
  DEV_PROLOGUE(c)
  const int i = b.LBi + blockIdx.x * BLK_X + threadIdx.x;
  const int j = b.LBj + blockIdx.y * BLK_Y + threadIdx.y;
  if (i < b.IstrR || i > b.IendR || j < b.JstrR || j > b.JendR) return;
  const long a = I2(i, j);
  const gcd_t zk = (gcd_t)(c->F.zeta + (long)(s.krhs - 1) * nij);
  const gcd_t h = (gcd_t)(c->F.h);
  const bool inU = i >= b.Istr, inV = j >= b.Jstr;
  const double Drhs = zk[a] + h[a];
  const double du = inU ? flux_u(GF(ubar)[a + (long)(s.krhs - 1) * nij], GF(on_u)[a], Drhs, zk[a - 1] + h[a - 1]) : 0.0;
  const double dv = inV ? flux_v(GF(vbar)[a + (long)(s.krhs - 1) * nij], GF(om_v)[a], Drhs, zk[a - ni] + h[a - ni]) : 0.0;
  average_point(c, s, a, inU, inV, du, dv, nij);
}

// ---------------------------------------------------------------------------
// WET_DRY: wetdry_tile (wetdry.F:93-393), called by every step2d with zeta(:,:,kstp) after the fast-time averaging
// (step2d_LF_AM3.h:729-749), and wetdry_ini_tile (:395-561).  One thread per point of (IstrR:IendR,JstrR:JendR); the
// rho-point flag "sea and total depth above Dcrit" (:190-200) of the point and of its three lower neighbours is
// evaluated in registers (the reference's private array `wetdry`), so the masks need no second pass:
//   mode 0  a fast step (iif <= nfast): wetdry_mask_tile (:563-716) -- u / v masks 2 / 0 / +-1, and the running sum
//           rmask_wet_avg (:214-227; `first` = the first predictor of the loop: the sum starts)
//   mode 1  after the loop (iif = nfast+1): the flag is AINT(rmask_wet_avg / (2 nfast)), wetdry_avg_mask_tile
//           (:734-917) with DU_avg1, DV_avg1, and the full masks (:325-345)
//   mode 2  wetdry_ini_tile: the flag from zeta(Tindex), wetdry_avg_mask_tile with ubar, vbar(Tindex), full masks
// The caller exchanges the masks afterwards, as the reference does.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k2d_wetdry(const RomsDev *__restrict__ c, int mode, int first, int kstp)
{
  DEV_PROLOGUE(c)
  const int i = b.IstrR + blockIdx.x * BLK_X + threadIdx.x;
  const int j = b.JstrR + blockIdx.y * BLK_Y + threadIdx.y;
  if (i > b.IendR || j > b.JendR) return;
  const roms_params_t &p = c->p;
  const long a = I2(i, j);
  const gcd_t zk = (gcd_t)(c->F.zeta + (long)(kstp - 1) * nij);
  const gcd_t h = (gcd_t)c->F.h, rmask = (gcd_t)c->F.rmask, avg = (gcd_t)c->F.rmask_wet_avg;
  const double eps = 1.0E-10;
  const double cffa = 1.0 / (double)(2 * p.nfast);
  auto flag = [&](long q) -> double {
    if (mode == 1) return trunc(avg[q] * cffa);
    double w = 1.0;
    if (p.masking) w = w * rmask[q];
    if ((zk[q] + h[q]) <= (p.Dcrit + eps)) w = 0.0;
    return w;
  };
  const bool inU = i >= b.Istr, inV = j >= b.Jstr;       // i-1 / j-1 exist in the flag's range (Istr-1:IendR,Jstr-1:JendR)
  const double w0 = flag(a);
  const double wW = inU ? flag(a - 1) : 0.0, wS = inV ? flag(a - ni) : 0.0, wSW = (inU && inV) ? flag(a - 1 - ni) : 0.0;
  GF(rmask_wet)[a] = w0;
  if (mode == 0) GF(rmask_wet_avg)[a] = first ? w0 : GF(rmask_wet_avg)[a] + w0;
  double um = 0.0, vm = 0.0;
  if (inU) {
    double cff1 = wW + w0;
    if (cff1 == 1.0) cff1 = wW - w0;
    um = cff1;
    if (mode != 0) {
      const double DU = mode == 1 ? (double)GF(DU_avg1)[a] : (double)GF(ubar)[a + (long)(kstp - 1) * nij];
      const double cff5 = fabs(fabs(cff1) - 1.0);
      const double cff6 = 0.5 + copysign(0.5, DU) * cff1;
      um = 0.5 * cff1 * cff5 + cff6 * (1.0 - cff5);
      if (DU == 0.0 && (wW + w0) <= 1.0) um = 0.0;       // catch lone ponds
    }
    GF(umask_wet)[a] = um;
  }
  if (inV) {
    double cff1 = wS + w0;
    if (cff1 == 1.0) cff1 = wS - w0;
    vm = cff1;
    if (mode != 0) {
      const double DV = mode == 1 ? (double)GF(DV_avg1)[a] : (double)GF(vbar)[a + (long)(kstp - 1) * nij];
      const double cff5 = fabs(fabs(cff1) - 1.0);
      const double cff6 = 0.5 + copysign(0.5, DV) * cff1;
      vm = 0.5 * cff1 * cff5 + cff6 * (1.0 - cff5);
      if (DV == 0.0 && (wS + w0) <= 1.0) vm = 0.0;
    }
    GF(vmask_wet)[a] = vm;
  }
  double pw = 0.0;
  if (inU && inV) {
    // :631-683: 1 with four or three wet neighbours, 2 with two on the same side, 0 otherwise
    const bool A = wW > 0.5, B = w0 > 0.5, C = wSW > 0.5, D = wS > 0.5;      // (i-1,j) (i,j) (i-1,j-1) (i,j-1)
    const int n = (int)A + (int)B + (int)C + (int)D;
    if (n >= 3) pw = 1.0;
    else if (n == 2 && !((A && D) || (B && C))) pw = 2.0;
    GF(pmask_wet)[a] = pw;
  }
  if (mode != 0) {                                       // :325-345 / :478-498 (as written: pmask_full is never below 2)
    GF(rmask_full)[a] = w0 * rmask[a];
    // (LuvSrc, wetdry.F:307-320 / :511-524: the output masks count a source face as water; the source loop of the
    // reference runs over IstrR:IendR, JstrR:JendR, which holds every inU / inV point)
    const bool srcs = c->src.n > 0;
    if (inU) GF(umask_full)[a] = (srcs && c->src.umap[a] != 0) ? 1.0 : um * GF(umask)[a];
    if (inV) GF(vmask_full)[a] = (srcs && c->src.vmap[a] != 0) ? 1.0 : vm * GF(vmask)[a];
    if (inU && inV) GF(pmask_full)[a] = fmax(pw * GF(pmask)[a], 2.0);
  }
}

static int wetdry_launch(int mode, int first, int kstp)
{
  const roms_bounds_t &b = g_ctx.b;
  hipLaunchKernelGGL(k2d_wetdry, grid2d(b.IendR - b.IstrR + 1, b.JendR - b.JstrR + 1), block2d(), 0, g_ctx.stream,
                     g_ctx.devc, mode, first, kstp);
  KERNEL_CHECK("k2d_wetdry");
  halo_batch_begin();
  halo_exchange2d(GT_P, g_ctx.field[FID_pmask_wet].dev);
  halo_exchange2d(GT_R, g_ctx.field[FID_rmask_wet].dev);
  halo_exchange2d(GT_U, g_ctx.field[FID_umask_wet].dev);
  halo_exchange2d(GT_V, g_ctx.field[FID_vmask_wet].dev);
  if (mode == 0) halo_exchange2d(GT_R, g_ctx.field[FID_rmask_wet_avg].dev);
  else {
    halo_exchange2d(GT_P, g_ctx.field[FID_pmask_full].dev);
    halo_exchange2d(GT_R, g_ctx.field[FID_rmask_full].dev);
    halo_exchange2d(GT_U, g_ctx.field[FID_umask_full].dev);
    halo_exchange2d(GT_V, g_ctx.field[FID_vmask_full].dev);
  }
  return halo_batch_end();
}

// DUon/DVom scratch already holds the exchanged fluxes of barotropic level g_flux_lev (left there by the
// previous call of the same LOOP_2D)
bool g_flux_ready = false;
int g_flux_lev = 0;
int g_flux_buf = 0;       // which scratch pair holds them

// LuvSrc: ubar, vbar(knew) at the source faces = the source's transport over the face's new water column
// (step2d_LF_AM3.h:2484-2502; after the boundary conditions, before the exchange).  One thread per source; two sources
// on one face would race where the reference lets the later one win: the face map decides (its entry is that later one).
__global__ void k2d_src_bar(const RomsDev *__restrict__ c, int knew)
{
  DEV_PROLOGUE(c)
  const int is = blockIdx.x * blockDim.x + threadIdx.x;
  if (is >= c->src.n) return;
  const int i = c->src.I[is], j = c->src.J[is];
  if (!(b.IstrR <= i && i <= b.IendR && b.JstrR <= j && j <= b.JendR)) return;
  const long c0 = I2(i, j);
  const double *__restrict__ zeta = c->F.zeta + (long)(knew - 1) * nij;
  const double *__restrict__ h = c->F.h;
  if (c->src.D[is] == 0) {
    if (c->src.umap[c0] != is + 1) return;
    const double cff = 1.0 / (c->F.on_u[c0] * 0.5 * (zeta[c0 - 1] + h[c0 - 1] + zeta[c0] + h[c0]));
    c->F.ubar[c0 + (long)(knew - 1) * nij] = c->src.Qbar[is] * cff;
  } else if (c->src.D[is] == 1) {
    if (c->src.vmap[c0] != is + 1) return;
    const double cff = 1.0 / (c->F.om_v[c0] * 0.5 * (zeta[c0 - ni] + h[c0 - ni] + zeta[c0] + h[c0]));
    c->F.vbar[c0 + (long)(knew - 1) * nij] = c->src.Qbar[is] * cff;
  }
}

// LwSrc, step2d_LF_AM3.h:890-908: the new free surface of the cells with a cell-centred source rises by the source's
// volume over the cell's area (before zetabc).  ONE thread walks the table: sources sharing a cell add up in the
// table's order, as in the reference.
__global__ void k2d_src_zeta(const RomsDev *__restrict__ c, int knew)
{
  DEV_PROLOGUE(c)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double *__restrict__ zeta = c->F.zeta + (long)(knew - 1) * nij;
  for (int is = 0; is < c->src.n; is++) {
    if (c->src.D[is] != 2) continue;
    const int i = c->src.I[is], j = c->src.J[is];
    if (!(b.IstrR <= i && i <= b.IendR && b.JstrR <= j && j <= b.JendR)) continue;
    const long c0 = I2(i, j);
    zeta[c0] = zeta[c0] + c->src.Qbar[is] * c->F.pm[c0] * c->F.pn[c0] * c->p.dtfast;
  }
}

int step2d_impl(const roms_step_idx_t *si, bool in_loop)
{
  const roms_bounds_t &b = g_ctx.b;
  const roms_params_t &p = g_ctx.p;
  int rc;
  S2 s{si->krhs, si->kstp, si->knew, si->nstp, si->nnew, si->iif, si->iic, si->ntfirst, si->predictor_2d_step, 0};
  double *DUon = g_ctx.hostc.ws2[0], *DVom = g_ctx.hostc.ws2[1];
  double *zeta_new = g_ctx.hostc.ws2[2], *zwrk = g_ctx.hostc.ws2[3];
  const long nij = (long)(b.UBi - b.LBi + 1) * (b.UBj - b.LBj + 1);
  // The fused kernel (k2d_mom_lds<true>) applies the closed-wall conditions itself; open S/N edges take the split
  // path below, whose boundary conditions are separate launches.  So do
  //   UV_VIS4: the biharmonic term is a pass of its own in front of the momentum kernel
  //   WET_DRY: the masks are a pass of their own between the averages and the free surface
  //   LuvSrc / LwSrc: the source faces and cells are launches of their own
  const bool walls = lbc2d_all_closed();
  const bool srcs = (p.point_sources & 3) != 0;
  const bool fusable = walls && !p.uv_vis4 && !p.wet_dry && !srcs;
  // One tile, E-W periodic, closed N-S walls: the kernels store the periodic images and the wall rows themselves, so
  // that no boundary-condition, exchange or flux launch is needed
  if (fusable && b.ntileI * b.ntileJ == 1 && b.EWperiodic && !b.NSperiodic && !g_ctx.loopback) {
    s.ew_images = 1;
    if (s.iif <= p.nfast)     // ONE launch: free surface, fast-time averages and momentum
      return roms_launch_k2d_mom_lds(s, K2dLaunch::FusedOneTile, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    // the last predictor of the loop (iif = nfast+1) only finishes the fast-time averages (:614-682)
    hipLaunchKernelGGL(k2d_avg_last, grid2d(b.UBi - b.LBi + 1, b.UBj - b.LBj + 1), block2d(), 0, g_ctx.stream,
                       g_ctx.devc, s);
    KERNEL_CHECK("k2d_avg_last");
    if (s.predictor) {
      if ((rc = halo_exchange2d(GT_R, g_ctx.field[FID_Zt_avg1].dev))) return rc;
      if ((rc = halo_exchange2d(GT_U, g_ctx.field[FID_DU_avg1].dev))) return rc;
      if ((rc = halo_exchange2d(GT_V, g_ctx.field[FID_DV_avg1].dev))) return rc;
    }
    return 0;
  }
  // Every other configuration.  Messages per call: inside LOOP_2D on several tiles ONE fused exchange at the end
  // (rzeta, zeta, ubar, vbar of this call + DUon, DVom of the next one, whose krhs is this call's knew); any other
  // call exchanges its own fluxes first.
  const bool multi = b.ntileI * b.ntileJ > 1 || g_ctx.loopback;
  // DUon/DVom live in two scratch pairs: the fused kernel reads one (exchanged fluxes of this level)
  // while it writes the other (own-point fluxes of the next level)
  if (g_flux_buf) { DUon = g_ctx.hostc.ws2[4]; DVom = g_ctx.hostc.ws2[5]; }
  double *DUnext = g_flux_buf ? g_ctx.hostc.ws2[0] : g_ctx.hostc.ws2[4];
  double *DVnext = g_flux_buf ? g_ctx.hostc.ws2[1] : g_ctx.hostc.ws2[5];
  if (!(g_flux_ready && g_flux_lev == s.krhs)) {
    hipLaunchKernelGGL(k2d_flux, grid2d(b.Iendp2 - (b.IstrU - 2) + 1, b.Jendp2 - (b.JstrV - 2) + 1), block2d(), 0,
                       g_ctx.stream, g_ctx.devc, s, DUon, DVom);
    KERNEL_CHECK("k2d_flux");
    halo_batch_begin();
    halo_exchange2d(GT_U, DUon);
    halo_exchange2d(GT_V, DVom);
    if ((rc = halo_batch_end())) return rc;
  }
  g_flux_ready = false;
  if (in_loop && multi && fusable && s.iif <= p.nfast) {
    // ONE compute launch + ONE exchange per call
    if ((rc = roms_launch_k2d_mom_lds(s, K2dLaunch::FusedTiles, DUon, DVom, nullptr, nullptr, DUnext, DVnext))) return rc;
    halo_batch_begin();
    if (s.predictor) halo_exchange2d(GT_R, g_ctx.field[FID_rzeta].dev + (long)(s.krhs - 1) * nij);
    halo_exchange2d(GT_R, g_ctx.field[FID_zeta].dev + (long)(s.knew - 1) * nij);
    halo_exchange2d(GT_U, g_ctx.field[FID_ubar].dev + (long)(s.knew - 1) * nij);
    halo_exchange2d(GT_V, g_ctx.field[FID_vbar].dev + (long)(s.knew - 1) * nij);
    halo_exchange2d(GT_U, DUnext);
    halo_exchange2d(GT_V, DVnext);
    if ((rc = halo_batch_end())) return rc;
    g_flux_ready = true;
    g_flux_lev = s.knew;
    g_flux_buf ^= 1;
    return 0;
  }
  const int i0 = b.IstrR < b.IstrU - 1 ? b.IstrR : b.IstrU - 1, j0 = b.JstrR < b.JstrV - 1 ? b.JstrR : b.JstrV - 1;
  hipLaunchKernelGGL(k2d_zeta, grid2d(b.IendR - i0 + 1, b.JendR - j0 + 1), block2d(), 0, g_ctx.stream, g_ctx.devc, s,
                     (const double *)DUon, (const double *)DVom, zeta_new, zwrk);
  KERNEL_CHECK("k2d_zeta");
  if (s.iif == p.nfast + 1 && s.predictor) {
    halo_batch_begin();
    halo_exchange2d(GT_R, g_ctx.field[FID_Zt_avg1].dev);
    halo_exchange2d(GT_U, g_ctx.field[FID_DU_avg1].dev);
    halo_exchange2d(GT_V, g_ctx.field[FID_DV_avg1].dev);
    if ((rc = halo_batch_end())) return rc;
  }
  // WET_DRY: the new wet/dry masks, :729-749 (after the averages and their exchange, before the return below)
  if (p.wet_dry && (rc = wetdry_launch(s.iif <= p.nfast ? 0 : 1, s.iif == 1 && s.predictor, s.kstp))) return rc;
  if (s.iif > p.nfast) return 0;
  if ((p.point_sources & 2) && g_ctx.hostc.src.n > 0) {     // LwSrc, :890-908
    hipLaunchKernelGGL(k2d_src_zeta, dim3(1), dim3(64), 0, g_ctx.stream, g_ctx.devc, s.knew);
    KERNEL_CHECK("k2d_src_zeta");
  }
  if ((rc = bc_zeta(s.knew, si))) return rc;
  if (p.uv_vis4 && (rc = roms_launch_step2d_visc4(s.krhs))) return rc;
  if ((rc = roms_launch_k2d_mom_lds(s, K2dLaunch::Split, DUon, DVom, zeta_new, zwrk, nullptr, nullptr))) return rc;
  if ((rc = bc_u2d(s.knew, si))) return rc;
  if ((rc = bc_v2d(s.knew, si))) return rc;
  if ((p.point_sources & 1) && g_ctx.hostc.src.n > 0) {        // LuvSrc, step2d_LF_AM3.h:2484-2502
    hipLaunchKernelGGL(k2d_src_bar, dim3((g_ctx.hostc.src.n + 63) / 64), dim3(64), 0, g_ctx.stream, g_ctx.devc, s.knew);
    KERNEL_CHECK("k2d_src_bar");
  }
  halo_batch_begin();
  if (s.predictor) halo_exchange2d(GT_R, g_ctx.field[FID_rzeta].dev + (long)(s.krhs - 1) * nij);
  halo_exchange2d(GT_R, g_ctx.field[FID_zeta].dev + (long)(s.knew - 1) * nij);
  halo_exchange2d(GT_U, g_ctx.field[FID_ubar].dev + (long)(s.knew - 1) * nij);
  halo_exchange2d(GT_V, g_ctx.field[FID_vbar].dev + (long)(s.knew - 1) * nij);
  return halo_batch_end();
}

}  // namespace

// wetdry(ng, tile, Tindex, .TRUE.): the masks of the initial state (initial.F:438-466), Tindex = s->kstp
extern "C" int roms_hip_wetdry(const roms_step_idx_t *s)
{
  int rc = roms_entry_check("roms_hip_wetdry");
  if (rc) return rc;
  if (!g_ctx.p.wet_dry) return 0;
  if (s->kstp < 1 || s->kstp > 3) return roms_fail("roms_hip_wetdry", "kstp (the time index of the initial state) outside 1..3");
  ScopedTimer tm("wetdry");
  return wetdry_launch(2, 0, s->kstp);
}

extern "C" int roms_hip_step2d(const roms_step_idx_t *s)
{
  int rc = roms_entry_check("roms_hip_step2d");
  if (rc) return rc;
  if ((rc = roms_uv_adv_check("roms_hip_step2d"))) return rc;
  if ((rc = check_lbc())) return rc;
  if ((rc = roms_rowm_prepare())) return rc;
  ScopedTimer tm("step2d");
  g_flux_ready = false;
  return step2d_impl(s, false);
}

// LOOP_2D of main3d.F:592-700: the predictor/corrector sequencing, launches queued on the library's stream
static int step2d_loop_body(roms_step_idx_t *s, int *indx1)
{
  int rc;
  const int nfast = g_ctx.p.nfast;
  int predictor = 0;
  g_flux_ready = false;
  for (int my_iif = 1; my_iif <= nfast + 1; my_iif++) {
    const int next_indx1 = 3 - *indx1;
    if (!predictor && my_iif <= nfast + 1) {
      predictor = 1;
      s->iif = my_iif;
      s->kstp = (s->iif == 1) ? *indx1 : 3 - *indx1;
      s->knew = 3;
      s->krhs = *indx1;
    }
    s->predictor_2d_step = predictor;
    if ((rc = step2d_impl(s, true))) return rc;
    if (predictor) {
      predictor = 0;
      s->knew = next_indx1;
      s->kstp = 3 - s->knew;
      s->krhs = 3;
      if (s->iif < nfast + 1) *indx1 = next_indx1;
    }
    s->predictor_2d_step = predictor;
    if (s->iif < nfast + 1)
      if ((rc = step2d_impl(s, true))) return rc;
  }
  g_flux_ready = false;
  return 0;
}

// One tile: the 2*nfast+1 launches of the loop are captured once per (indx1, nstp, start-up phase) into a
// hipGraph and replayed -- the launch arguments of a replay are those of the capture, and so is the
// instantiation of the momentum kernel (row table, advection scheme); the graphs are dropped whenever bounds,
// parameters -- uv_adv among them -- or a field registration change (step2d_graphs_release).  On several
// tiles the loop contains host-side transport calls and runs eagerly.
struct LoopGraph { hipGraphExec_t exec; int indx1_out; roms_step_idx_t s_out; };
static std::map<int, LoopGraph> g_loop_graphs;
static int g_graph_exchanges = 0;            // roms_hip_graph_exchanges: 0 (default) never, 1 always, 2 in loopback only
static bool g_rccl_graph_failed = false;     // the capture of the transport failed once on this stack: stay eager
bool halo_rccl_capturable();                  // halo.hip: RCCL transport in use, message plan and buffers can be fixed
int halo_reserve_buffers();                   // halo.hip: allocate the message buffers for the largest exchange now

extern "C" int roms_hip_graph_exchanges(int on)
{
  g_graph_exchanges = on ? 1 : 0;
  step2d_graphs_release();
  return 0;
}
// 0 = LOOP_2D runs eagerly on several tiles, 1 = replayed as one hipGraph with the exchanges inside, -1 = the capture
// was tried and refused by this stack
extern "C" int roms_hip_graph_exchanges_state(void)
{
  if (g_rccl_graph_failed) return -1;
  return g_loop_graphs.empty() ? 0 : 1;
}

void step2d_graphs_release()
{
  g_rccl_graph_failed = false;
  for (auto &kv : g_loop_graphs)
    if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  g_loop_graphs.clear();
}

extern "C" int roms_hip_step2d_loop(roms_step_idx_t *s, int *indx1)
{
  int rc = roms_entry_check("roms_hip_step2d_loop");
  if (rc) return rc;
  if ((rc = roms_uv_adv_check("roms_hip_step2d_loop"))) return rc;
  if ((rc = check_lbc())) return rc;
  if ((rc = roms_rowm_prepare())) return rc;          // before any capture: it synchronises when it has work
  ScopedTimer tm("step2d_loop");
  const roms_bounds_t &b = g_ctx.b;
  const bool one_tile = b.ntileI * b.ntileJ == 1 && !g_ctx.loopback;
  // Several tiles over RCCL: the loop's launches AND its ncclSend / ncclRecv groups can be captured too (RCCL enqueues
  // its kernels on the capturing stream), so that a replay is one hipGraphLaunch for 59 compute launches, 59 packs,
  // 59 transport kernels and 59 unpacks.  Opt-in (roms_hip_graph_exchanges): measured in loopback on BENCHMARK1
  // (ROCm 7.2, RCCL of this image) the loop's device time drops from 1.85 to 1.65 ms but the step's wall time RISES
  // from 3.05 to 3.64 ms -- replaying what RCCL records besides its kernels costs more on the host than the eager
  // calls.  Every rank must capture and replay the same sequence.  If the capture fails the loop runs eagerly.
  const bool rccl_graph = !one_tile && halo_rccl_capturable() && !g_rccl_graph_failed &&
                          (g_graph_exchanges == 1 || (g_graph_exchanges == 2 && g_ctx.loopback));
  if (!one_tile && !rccl_graph) return step2d_loop_body(s, indx1);
  const int phase = s->iic == s->ntfirst ? 0 : (s->iic == s->ntfirst + 1 ? 1 : 2);
  const int key = ((*indx1 * 4 + s->nstp) * 4 + s->nnew) * 4 + phase;
  auto it = g_loop_graphs.find(key);
  if (it == g_loop_graphs.end()) {
    hipGraph_t graph = nullptr;
    const roms_step_idx_t s_in = *s;
    const int indx1_in = *indx1;
    if (rccl_graph && (rc = halo_reserve_buffers())) return rc;       // no allocation inside a capture
    HIP_TRY(hipStreamBeginCapture(g_ctx.stream, hipStreamCaptureModeThreadLocal));
    rc = step2d_loop_body(s, indx1);
    const hipError_t e = hipStreamEndCapture(g_ctx.stream, &graph);
    if (rccl_graph && (rc || e != hipSuccess)) {
      // this stack does not capture the transport: remember it and run the loop the ordinary way
      if (graph) (void)hipGraphDestroy(graph);
      (void)hipGetLastError();
      g_rccl_graph_failed = true;
      *s = s_in;
      *indx1 = indx1_in;
      return step2d_loop_body(s, indx1);
    }
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return roms_fail("roms_hip_step2d_loop: hipStreamEndCapture", hipGetErrorString(e));
    LoopGraph lg{nullptr, *indx1, *s};
    const hipError_t e2 = hipGraphInstantiate(&lg.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e2 != hipSuccess) return roms_fail("roms_hip_step2d_loop: hipGraphInstantiate", hipGetErrorString(e2));
    it = g_loop_graphs.emplace(key, lg).first;
  } else {
    // the sequencing of the loop does not depend on the data: indices as the capture left them
    const int iic = s->iic, ntfirst = s->ntfirst;
    *s = it->second.s_out;
    s->iic = iic;
    s->ntfirst = ntfirst;
    *indx1 = it->second.indx1_out;
  }
  HIP_TRY(hipGraphLaunch(it->second.exec, g_ctx.stream));
  return 0;
}
