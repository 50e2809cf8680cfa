// k_lmd.hip -- K-profile vertical mixing: roms_hip_lmd_vmix (k_lmd_vmix, k_lmd_bkpp, k_lmd_edges, described where they
// stand) and the switches and library-owned arrays of LMD_BKPP / LMD_DDMIX (roms_hip_set_kpp, roms_hip_set_ddmix,
// roms_hip_get_kpp).  The formulas the surface and the bottom layer share are in kpp.h.
#include "kpp.h"
#include <cmath>

// lmd_vmix = lmd_vmix_tile + lmd_skpp_tile + lmd_finish_tile (ROMS/Nonlinear/lmd_vmix.F:99/465,
// lmd_skpp.F:98, lmd_swfrac.F:6): K-profile vertical mixing with the BENCHMARK option set (LMD_RIMIX
// + RI_SPLINES, LMD_CONVEC, LMD_SKPP, LMD_NONLOCAL, SALINITY; uniform Jerlov water type).
// Column-local: one thread per (i,j), three sweeps.  Upward: the forward recurrences of the three splines
// (u, v, pden), of which only every sixth level is kept (registers).  Downward, segment by segment: the
// recurrences of a segment are re-run from its checkpoint (registers) and their back-substitution is fused with
// the Richardson-number mixing, the bulk Richardson function and the boundary-layer depth search, so no profile
// goes to device memory at all: the shear function nu_sx waits in LDS for the last sweep; the buoyancy-flux profile
// is recomputed (two exp) where used.  Upward again: the boundary-layer profiles, the convective adjustment, the
// final Akv, Akt.  Per column and level 4 + 4 + 2 + 2 array reads from memory (4 more from cache) and 5 writes -- the
// first version (forward values of all levels in scratch) read 18 and wrote 11.
namespace {

// LMD_DDMIX: the double-diffusive increments at a W-level from t, s of the rho-levels below (A) and above (B) and
// alfaobeta of the level below: lmd_vmix.F:371-419, constants of mod_scalars.F:1553-1577.  (A function, not a lambda of
// the kernel: the kernel's lambdas keep the numbering they have without the option.)
__device__ __forceinline__ void lmd_nu_dd(double tA, double tB, double sA, double sB, double aob, double &nu_ddt, double &nu_dds)
{
  const double lmd_Rrho0 = 1.9, lmd_nuf = 10.0E-4, lmd_fdd = 0.7, lmd_nu = 1.5E-6;
  const double lmd_tdd1 = 0.909, lmd_tdd2 = 4.6, lmd_tdd3 = 0.54, lmd_sdd1 = 0.15, lmd_sdd2 = 1.85, lmd_sdd3 = 0.85;
  const double ddDT = tB - tA;
  double ddDS = sB - sA;
  ddDS = copysign(1.0, ddDS) * fmax(fabs(ddDS), 1.0E-14);
  double Rrho = aob * ddDT / ddDS;
  if ((Rrho > 1.0) && (ddDS > 0.0)) {                          // salt fingering
    Rrho = fmin(Rrho, lmd_Rrho0);
    const double r = (Rrho - 1.0) / (lmd_Rrho0 - 1.0);
    nu_dds = 1.0 - r * r;
    nu_dds = lmd_nuf * nu_dds * nu_dds * nu_dds;
    nu_ddt = lmd_fdd * nu_dds;
  } else if ((0.0 < Rrho) && (Rrho < 1.0) && (ddDS < 0.0)) {   // diffusive convection
    nu_ddt = lmd_nu * lmd_tdd1 * exp(lmd_tdd2 * exp(-lmd_tdd3 * ((1.0 / Rrho) - 1.0)));
    if (Rrho < 0.5) nu_dds = nu_ddt * lmd_sdd1 * Rrho;
    else nu_dds = nu_ddt * (lmd_sdd2 * Rrho - lmd_sdd3);
  } else {
    nu_ddt = 0.0;
    nu_dds = 0.0;
  }
}

// The forward recurrences of the three splines are NOT stored per level: the upward sweep keeps only their values at
// every LMD_SEG-th level (checkpoints, in registers); the downward sweep takes the column segment by segment from the
// top, re-runs the recurrence of a segment from its checkpoint and consumes it in descending order.  Same operations
// in the same order as a single upward sweep, so the same bits -- without the 4 x (N-1) scratch stores and loads per
// column of the earlier version.  All three sweeps load a whole segment (LMD_SEG levels of every input) before they
// compute it: a wave has a dozen memory round trips per column instead of one per level and sweep (the kernel was
// waiting on memory for 72 % of its wave-cycles, SQ_WAIT_ANY, with one level's loads in flight).
#define LMD_SEG 5

// BKPP (LMD_BKPP, roms_hip_set_kpp): lmd_bkpp runs between lmd_skpp and lmd_finish (lmd_vmix.F:83-89), so the last sweep
// stores Akv / Akt without the lmd_finish increment -- k_lmd_bkpp adds it -- and ksbl goes to the library's array.
// DDMIX (LMD_DDMIX, roms_hip_set_ddmix): the double-diffusive increments nu_ddt / nu_dds of lmd_vmix.F:360-430 join the
// interior Akt(itemp) / Akt(isalt), which then differ.  They are never stored: the last sweep forms them from t, s(nstp)
// of the segment it loads anyway (LMD_SEG + 1 rho-levels per round trip) and alfaobeta of rho_eos, and the match at the
// boundary-layer depth recomputes them at its two levels.
template <int NMAX, bool BKPP = false, bool DDMIX = false>
__global__ void __launch_bounds__(BLK_X *BLK_Y, 2)
k_lmd_vmix(const RomsDev *__restrict__ c, int nstp, double lmd_Cg, double Vtc)
{
  DEV_PROLOGUE(c)
  const roms_params_t &p = c->p;
  constexpr int MS = (NMAX - 1 + LMD_SEG - 1) / LMD_SEG;        // segments of W-levels 1..NMAX-1
  const Blk XB = xcd_block();
  const int i = b.Istr + XB.x * BLK_X + threadIdx.x;
  const int j = b.Jstr + XB.y * BLK_Y + threadIdx.y;
  if (i > b.Iend || j > b.Jend) return;
  const long a = I2(i, j);
  const double g = p.g, vonKar = 0.41, eps = 1.0E-10;
  const double lmd_Ri0 = 0.7, lmd_nu0m = 10.0E-4, lmd_nu0s = 10.0E-4;
  const double lmd_cekman = 0.7, lmd_cmonob = 1.0, lmd_epsilon = 0.1;
  const double gorho0 = g / p.rho0;
  const gcd_t Hz = (gcd_t)c->F.Hz, pden = (gcd_t)c->F.pden, bvf = (gcd_t)c->F.bvf;
  const gcd_t z_w = (gcd_t)c->F.z_w;
  const gcd_t u = (gcd_t)(c->F.u + (long)(nstp - 1) * n3r), v = (gcd_t)(c->F.v + (long)(nstp - 1) * n3r);
  const gd_t Akv = (gd_t)c->F.Akv, AkT = (gd_t)c->F.Akt, AkS = (gd_t)(c->F.Akt + n3w);
  const gd_t ghT = (gd_t)c->F.ghats, ghS = (gd_t)(c->F.ghats + n3w);
  auto r3i = [&](int k) { return a + (long)(k - 1) * nij; };     // rho-type level k = 1..N
  auto w3i = [&](int k) { return a + (long)k * nij; };           // W-type level k = 0..N
  // DDMIX: t(:,:,:,nstp,itemp), t(:,:,:,nstp,isalt) and alfaobeta (0:N, the value of rho-level k at index k)
  const gcd_t ddT = DDMIX ? (gcd_t)(c->F.t + (long)(nstp - 1) * n3r) : nullptr;
  const gcd_t ddS = DDMIX ? (gcd_t)(c->F.t + ((long)(nstp - 1) + 3L) * n3r) : nullptr;
  const gcd_t ddA = DDMIX ? (gcd_t)c->ddmix.alfaobeta : nullptr;
  // the shear function nu_sx of W-levels 1..N-1 waits in LDS ([level][thread]) for the last sweep -- it used to be
  // parked in Akv: one field written and read back for nothing (0.13 GB each way on BENCHMARK3)
  constexpr int NTH = BLK_X * BLK_Y;
  __shared__ double s_nu[(NMAX - 1) * NTH];
  double *const nu_col = s_nu + threadIdx.y * BLK_X + threadIdx.x;        // nu_col[(k - 1) * NTH], k = 1..N-1

  // the inputs of rho-levels k0+1 .. k0+SEG+1 (clamped to N: the clamped ones are loaded but not used)
  struct Lev { double hz, ua, ub, va, vb, pd; };
  auto load_seg = [&](int k0, Lev (&L)[LMD_SEG + 1]) {
#pragma unroll
    for (int t = 0; t <= LMD_SEG; t++) {
      const long q = r3i(min(k0 + 1 + t, N));
      L[t].hz = Hz[q]; L[t].ua = u[q]; L[t].ub = u[q + 1]; L[t].va = v[q]; L[t].vb = v[q + ni]; L[t].pd = pden[q];
    }
  };
  // one level of the spline recurrences of u, v (lmd_vmix_tile :205-225 = lmd_skpp_tile :345-365) and of pden:
  // from the values of level k-1 and the inputs of rho-levels k (A) and k+1 (B)
  struct Fwd { double fc, du, dv, dr; };
  auto fwd = [](const Lev &A, const Lev &B, const Fwd &m) {
    const SplineCoef sc = spline_coef(A.hz, B.hz, m.fc);
    return Fwd{sc.FC, spline_fwd(sc.cff, 3.0 * (B.ua - A.ua + B.ub - A.ub), A.hz, m.du),
               spline_fwd(sc.cff, 3.0 * (B.va - A.va + B.vb - A.vb), A.hz, m.dv), spline_fwd(sc.cff, 6.0 * (B.pd - A.pd), A.hz, m.dr)};
  };

  // ---------- upward sweep: the recurrences, keeping their values at levels 0, SEG, 2 SEG ... only ----------
  double ckF[MS], ckU[MS], ckV[MS], ckR[MS];
  {
    Fwd f{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int m = 0; m < MS; m++) {
      ckF[m] = f.fc; ckU[m] = f.du; ckV[m] = f.dv; ckR[m] = f.dr;
      if (m * LMD_SEG + 1 <= N - 1) {
        Lev L[LMD_SEG + 1];
        load_seg(m * LMD_SEG, L);
#pragma unroll
        for (int t = 0; t < LMD_SEG; t++) {
          if (m * LMD_SEG + 1 + t <= N - 1) f = fwd(L[t], L[t + 1], f);
        }
      }
    }
  }

  // ---------- surface forcing of the boundary layer, lmd_skpp.F:300-340 ----------
  const double zwN = z_w[w3i(N)];
  double hsbl = GF(hsbl)[a];
  double sl_dpth = lmd_epsilon * (zwN - hsbl);
  const double su0 = GF(sustr)[a], su1 = GF(sustr)[a + 1], sv0 = GF(svstr)[a], sv1 = GF(svstr)[a + ni];
  // MASKING (lmd_skpp.F:272-866): mr = rmask, applied where the reference applies it
  const bool masking = p.masking != 0;
  const double mr = masking ? (double)GF(rmask)[a] : 1.0;
  const double Ustar = kpp_ustar(su0, su1, sv0, sv1, masking, mr);      // :272
  const double alpha = GF(alpha)[a], beta = GF(beta)[a], srflx = GF(srflx)[a];
  const double stT = GF(stflx)[a], stS = GF(stflx)[a + nij];
  const double Bo = g * (alpha * (stT - srflx) - beta * stS);
  const double Bosol = g * alpha * srflx;
  // buoyancy flux and the non-local flux shape at W-level k (:320-338); recomputed where needed
  // (two exp per call) instead of being stored and re-read
  auto bflux_z = [&](double zwk, double &gT, double &gS) {
    const double swdk = swfrac(p, zwN - zwk);
    const double bf = kpp_bflux(Bo, Bosol, swdk, masking, mr);    // :316
    const double cff = 1.0 - (0.5 + copysign(0.5, bf));
    gT = -cff * (stT - srflx + srflx * (1.0 - swdk));
    gS = cff * stS;
    return bf;
  };
  { double gT, gS; bflux_z(zwN, gT, gS); ghT[w3i(N)] = gT; ghS[w3i(N)] = gS; }

  // ---------- downward sweep, segment by segment: back-substitution of the three splines fused with (a) the shear /
  // Richardson-number mixing of lmd_vmix_tile (:240-300) and (b) the bulk Richardson function and the
  // boundary-layer depth search of lmd_skpp_tile (:380-470) ----------
  const double cff1 = 1.0 / 3.0, cff2 = 1.0 / 6.0;
  int ksbl = 1;
  {
    double Rref = 0.0, Uref = 0.0, Vref = 0.0;
    double dRk = 0.0, dUk = 0.0, dVk = 0.0;                      // final values at level k (k = N: 0)
    double FCk = 0.0;                                            // FC(i,N) = 0
    double bvk = 0.0, zwk = zwN;                                 // W-type level k (bvf(N) is not used)
    hsbl = z_w[w3i(1)];
    const int mtop = (N - 2) / LMD_SEG;                          // the segment of W-level N-1
    for (int m = mtop; m >= 0; m--) {
      const int k0 = m * LMD_SEG;                                // this segment: W-levels k0+1 .. min(k0+SEG, N-1)
      // everything the segment reads, in flight together: rho-levels k0+1 .. k0+SEG+1, bvf and z_w of W-levels
      // k0 .. k0+SEG (iteration k works on W-level k-1)
      double bvW[LMD_SEG + 1], zwW[LMD_SEG + 1];
#pragma unroll
      for (int t = 0; t <= LMD_SEG; t++) {
        const long qz = w3i(min(k0 + t, N - 1));
        bvW[t] = bvf[qz]; zwW[t] = z_w[qz];
      }
      // re-run the recurrences of the segment from its checkpoint
      double fF[LMD_SEG], fU[LMD_SEG], fV[LMD_SEG], fR[LMD_SEG];
      double hzA[LMD_SEG + 1], pdA[LMD_SEG + 1], umA[LMD_SEG + 1], vmA[LMD_SEG + 1];     // what the iterations need of L
      {
        Lev L[LMD_SEG + 1];
        load_seg(k0, L);
        Fwd f{ckF[0], ckU[0], ckV[0], ckR[0]};
#pragma unroll
        for (int t = 1; t < MS; t++)
          if (m == t) { f.fc = ckF[t]; f.du = ckU[t]; f.dv = ckV[t]; f.dr = ckR[t]; }
#pragma unroll
        for (int t = 0; t < LMD_SEG; t++) {
          fF[t] = 0.0; fU[t] = 0.0; fV[t] = 0.0; fR[t] = 0.0;
          if (k0 + 1 + t <= N - 1) {
            f = fwd(L[t], L[t + 1], f);
            fF[t] = f.fc; fU[t] = f.du; fV[t] = f.dv; fR[t] = f.dr;
          }
        }
#pragma unroll
        for (int t = 0; t <= LMD_SEG; t++) {
          hzA[t] = L[t].hz; pdA[t] = L[t].pd; umA[t] = 0.5 * (L[t].ua + L[t].ub); vmA[t] = 0.5 * (L[t].va + L[t].vb);
        }
      }
      // iteration k (rho-level k = L[k-k0-1], forward values and bvf / z_w of W-level k-1) for k = k0+SEG+1 .. k0+2;
      // the lowest segment also runs k = 1, which has no level below
#pragma unroll
      for (int t = LMD_SEG; t >= 0; t--) {
        const int k = k0 + 1 + t;
        if (k <= N && (t >= 1 || m == 0)) {
          const double hz = hzA[t], pd = pdA[t], um = umA[t], vm = vmA[t];
          const int tw = t >= 1 ? t - 1 : 0;                     // slot of the forward values of W-level k-1
          const double fc = fF[tw], du = fU[tw], dv = fV[tw], dr = fR[tw];
          const double bvm = bvW[t], zwm = zwW[t];
          if (k == N) {                                          // the reference values at the surface: x(N) = 0
            Rref = pd + hz * (cff1 * 0.0 + cff2 * dr);
            Uref = um + hz * (cff1 * 0.0 + cff2 * du);
            Vref = vm + hz * (cff1 * 0.0 + cff2 * dv);
          }
          // final spline derivatives at level k-1
          double dRm = 0.0, dUm = 0.0, dVm = 0.0;
          if (k - 1 >= 1) {
            dRm = spline_back(dr, fc, dRk);
            dUm = spline_back(du, fc, dUk);
            dVm = spline_back(dv, fc, dVk);
          }
          // (a) interior mixing at W-level k: only the shear function nu_sx is kept (in LDS); the last sweep forms
          // Akv and Akt from it and from bvf, which it reads anyway (lmd_vmix.F:286-297)
          if (k <= N - 1) {
            const double epsv = 1.0E-14;
            double shear2 = dUk * dUk + dVk * dVk;
            const double bv = bvk;
            const double Rig = bv / (shear2 + epsv);
            double cff = fmin(1.0, fmax(0.0, Rig) / lmd_Ri0);
            double nu_sx = 1.0 - cff * cff;
            nu_sx = nu_sx * nu_sx * nu_sx;
            shear2 = bv / (Rig + epsv);
            cff = shear2 * shear2 / (shear2 * shear2 + 16.0E-10);
            nu_sx = cff * nu_sx;
            nu_col[(k - 1) * NTH] = nu_sx;
          }
          // (b) bulk Richardson function at W-level k-1 -- until the boundary-layer depth is found: the levels below
          // it cannot change hsbl / ksbl any more (the search keeps the first crossing from the top)
          if (ksbl == 1) {
            const double depth = zwN - zwm;
            double gT, gS;
            const double bf = bflux_z(zwm, gT, gS);
            if (k - 1 == 0) { ghT[w3i(0)] = gT; ghS[w3i(0)] = gS; }
            double wmk, wsk;
            kpp_wscale(Ustar, bf, sl_dpth, depth, wmk, wsk);
            const double Rk = pd - hz * (cff1 * dRm + cff2 * dRk);
            const double Uk = um - hz * (cff1 * dUm + cff2 * dUk);
            const double Vk = vm - hz * (cff1 * dVm + cff2 * dVk);
            const double FCkm1 = kpp_critical(gorho0, Rref, Rk, Uref, Uk, Vref, Vk, depth, Vtc, wsk, bvm);
            // boundary-layer depth: first level (from the top, k = N..2) where the function turns positive
            if (k >= 2 && FCkm1 > 0.0) {
              hsbl = kpp_crossing(zwk, FCk, zwm, FCkm1);
              ksbl = k;
            }
            FCk = FCkm1;
          } else if (k - 1 == 0) {                               // the non-local flux shape at the bottom (:320-338)
            double gT, gS;
            bflux_z(zwm, gT, gS);
            ghT[w3i(0)] = gT; ghS[w3i(0)] = gS;
          }
          dRk = dRm; dUk = dUm; dVk = dVm;
          bvk = bvm; zwk = zwm;
        }
      }
    }
  }
  // the interior mixing coefficients of (a) at W-level k from the stored shear function: the same expressions
  // as lmd_vmix.F:286-297
  auto akv_a = [&](double nu_sx, double bv) { return 1.0E-6 * (1.0 / sqrt(fmax(bv, 1.0E-7))) + lmd_nu0m * nu_sx; };
  auto akt_a = [&](double nu_sx, double bv) { return 1.0E-7 * (1.0 / sqrt(fmax(bv, 1.0E-7))) + lmd_nu0s * nu_sx; };
  auto bfsfc_at = [&](double hs) { return kpp_bflux_at(p, Bo, Bosol, zwN - hs, masking, mr); };      // :562, :574 and :669, :681
  double Bfsfc = bfsfc_at(hsbl);
  if ((Ustar > 0.0) && (Bfsfc > 0.0)) {
    const double hekman = lmd_cekman * Ustar / fmax(fabs(GF(f)[a]), eps);
    const double hmonob = lmd_cmonob * Ustar * Ustar * Ustar / fmax(vonKar * Bfsfc, eps);
    hsbl = (zwN - fmin(fmin(hekman, hmonob), zwN - hsbl));
  }
  hsbl = fmin(hsbl, zwN);
  hsbl = fmax(hsbl, z_w[w3i(0)]);
  if (masking) hsbl = hsbl * mr;                                 // :595
  GF(hsbl)[a] = hsbl;
  kpp_wall_rows(b, GF(hsbl), a, ni, j, hsbl);                    // bc_r2d_tile: zero gradient at closed walls
  // ksbl = the first k from the top (N..2) with z_w(k-1) < hsbl (lmd_skpp.F:640-650); LMD_SEG levels per round trip
  ksbl = 1;
  for (int kt = N; kt >= 2 && ksbl == 1; kt -= LMD_SEG) {
    double zc[LMD_SEG];
#pragma unroll
    for (int t = 0; t < LMD_SEG; t++) zc[t] = z_w[w3i(max(kt - t - 1, 0))];
#pragma unroll
    for (int t = 0; t < LMD_SEG; t++)
      if ((ksbl == 1) && (kt - t >= 2) && (zc[t] < hsbl)) ksbl = kt - t;
  }
  Bfsfc = bfsfc_at(hsbl);
  sl_dpth = lmd_epsilon * (zwN - hsbl);
  const double zbl = zwN - hsbl;
  double wm, ws;
  const double f1 = kpp_scales_at(Ustar, Bfsfc, zbl, wm, ws);
  KppShape G;
  if (hsbl > z_w[w3i(1)]) {
    const int k = ksbl;
    const KppBracket B = kpp_bracket(z_w[w3i(k)], z_w[w3i(k - 1)], hsbl);
    // Akv / Akt of (a) at the two levels around the boundary-layer depth (level N keeps the array's own values)
    const double bv_k = bvf[w3i(k)], bv_m = bvf[w3i(k - 1)];
    const double nu_k = (k <= N - 1) ? nu_col[(k - 1) * NTH] : (double)Akv[w3i(k)], nu_m = nu_col[(k - 2) * NTH];
    const double akv_k = (k <= N - 1) ? akv_a(nu_k, bv_k) : nu_k, akv_m = akv_a(nu_m, bv_m);
    // DDMIX: the increments of the two levels, recomputed (level N keeps the array's own values)
    double ddt_k = 0.0, dds_k = 0.0, ddt_m = 0.0, dds_m = 0.0;
    if constexpr (DDMIX) {
      const long q0 = r3i(k - 1), q1 = r3i(k), q2 = r3i(min(k + 1, N));
      const double tt0 = ddT[q0], tt1 = ddT[q1], tt2 = ddT[q2], ts0 = ddS[q0], ts1 = ddS[q1], ts2 = ddS[q2];
      const double ab_m = ddA[w3i(k - 1)], ab_k = ddA[w3i(min(k, N - 1))];
      lmd_nu_dd(tt0, tt1, ts0, ts1, ab_m, ddt_m, dds_m);
      lmd_nu_dd(tt1, tt2, ts1, ts2, ab_k, ddt_k, dds_k);
    }
    const double akt_k = (k <= N - 1) ? (DDMIX ? akt_a(nu_k, bv_k) + ddt_k : akt_a(nu_k, bv_k)) : (double)AkT[w3i(k)],
                 akt_m = DDMIX ? akt_a(nu_m, bv_m) + ddt_m : akt_a(nu_m, bv_m);
    // salinity: Akt(isalt) = Akt(itemp) at the interior levels (lmd_vmix.F:296-297), with DDMIX plus its own increment;
    // level N was not touched
    const double aks_k = (k <= N - 1) ? (DDMIX ? akt_a(nu_k, bv_k) + dds_k : akt_k) : (double)AkS[w3i(k)],
                 aks_m = DDMIX ? akt_a(nu_m, bv_m) + dds_m : akt_m;
    G.m = kpp_match<false>(akv_k, akv_m, B, zbl, wm, f1, masking, mr);      // :754
    G.t = kpp_match<false>(akt_k, akt_m, B, zbl, ws, f1, masking, mr);      // :765
    G.s = kpp_match<false>(aks_k, aks_m, B, zbl, ws, f1, masking, mr);      // :777
  } else {
    ksbl = 0;
    const double dK_bl = vonKar * kpp_ustar(GF(bustr)[a], GF(bustr)[a + 1], GF(bvstr)[a], GF(bvstr)[a + ni], masking, mr);      // :793
    const double K_bl = dK_bl * (hsbl - z_w[w3i(0)]);
    G.m = kpp_match<false>(K_bl, dK_bl, zbl, wm, f1, masking, mr);          // :799
    G.t = kpp_match<false>(K_bl, dK_bl, zbl, ws, f1, masking, mr);          // :808
    G.s = G.t;
  }
  if constexpr (BKPP) c->kpp.ksbl[a] = ksbl;                      // lmd_skpp.F:653-658, :787
  // ---------- upward again, LMD_SEG levels at a time: boundary-layer profiles, convective adjustment, final values ----------
  for (int kb = 1; kb <= N - 1; kb += LMD_SEG) {
    double nuA[LMD_SEG], zwA[LMD_SEG], bvA[LMD_SEG];
#pragma unroll
    for (int t = 0; t < LMD_SEG; t++) {
      const long q3 = w3i(min(kb + t, N - 1));
      nuA[t] = nu_col[(min(kb + t, N - 1) - 1) * NTH]; zwA[t] = z_w[q3]; bvA[t] = bvf[q3];
    }
    // DDMIX: rho-levels kb .. kb+SEG, alfaobeta of kb .. kb+SEG-1, with the segment's other loads; the increments themselves
    // (two exp) are formed only at the levels the boundary layer leaves alone, k <= ksbl.  (Initialised, though every
    // element read is loaded first: with plain declarations the instantiations without the option lose their identity
    // with the code the kernel had before the option existed -- same instructions, other registers.)
    double ttA[LMD_SEG + 1] = {}, tsA[LMD_SEG + 1] = {}, abA[LMD_SEG] = {};
    if constexpr (DDMIX) {
#pragma unroll
      for (int t = 0; t <= LMD_SEG; t++) {
        const long q = r3i(min(kb + t, N));
        ttA[t] = ddT[q]; tsA[t] = ddS[q];
      }
#pragma unroll
      for (int t = 0; t < LMD_SEG; t++) abA[t] = ddA[w3i(min(kb + t, N - 1))];
    }
#pragma unroll
    for (int t = 0; t < LMD_SEG; t++) {
      const int k = kb + t;
      if (k <= N - 1) {
        const double zwk = zwA[t], bvk = bvA[t];
        double akv = akv_a(nuA[t], bvk), akt = akt_a(nuA[t], bvk), aks = akt;
        if constexpr (DDMIX) {
          if (k <= ksbl) {                     // (above ksbl the boundary-layer profile replaces akt / aks)
            double nut, nus;
            lmd_nu_dd(ttA[t], ttA[t + 1], tsA[t], tsA[t + 1], abA[t], nut, nus);
            akt = akt + nut;
            aks = aks + nus;
          }
        }
        if (k > ksbl) {
          const double depth = zwN - zwk;
          double gT, gS;
          const double bf = bflux_z(zwk, gT, gS);
          double wmk, wsk;
          kpp_wscale(Ustar, bf, sl_dpth, depth, wmk, wsk);
          const KppAk P = kpp_blend(depth, zbl, wmk, wsk, G, masking, mr);      // :866
          akv = P.akv; akt = P.akt; aks = P.aks;
          const double cff = lmd_Cg * (1.0 - (0.5 + copysign(0.5, bf))) / (zbl * wsk + eps);
          ghT[w3i(k)] = cff * gT;
          ghS[w3i(k)] = cff * gS;
        } else {
          ghT[w3i(k)] = 0.0;
          ghS[w3i(k)] = 0.0;
        }
        // lmd_finish_tile: convective mixing where the stratification is unstable (lmd_vmix.F:520-540)
        if constexpr (BKPP) {
          Akv[w3i(k)] = akv;
          AkT[w3i(k)] = akt;
          AkS[w3i(k)] = aks;
        } else {
          const double conv = kpp_convec(bvk);
          Akv[w3i(k)] = akv + conv;
          AkT[w3i(k)] = akt + conv;
          AkS[w3i(k)] = aks + conv;
        }
      }
    }
  }
}

// lmd_bkpp_tile (ROMS/Nonlinear/lmd_bkpp.F:233-804; LMD_BKPP with the file's own SASHA, RI_SPLINES, SALINITY, MASKING at
// run time, no LMD_SHAPIRO), then the lmd_finish increment (lmd_vmix.F:524-540).  Runs behind k_lmd_vmix<NMAX, true>,
// which left Akv / Akt without that increment and ksbl in the library's array.  Column-local, one thread per (i,j).
// The plain form: the critical function FC(k) needs the reference values at the bottom, which need the BACK-SUBSTITUTED
// derivative at level 1, so the descending sweep has to finish before the ascending one that searches; the three
// derivative profiles wait in the 3-D scratch slots ws3[0..2] (forward values from the first sweep, overwritten by the
// final ones in the second; every access is one double per lane along i) and the spline coefficient in LDS.  The
// buoyancy-flux profile is recomputed where used (two exp), as in k_lmd_vmix.
typedef int __attribute__((address_space(1))) *gi_t;

template <int NMAX>
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_lmd_bkpp(const RomsDev *__restrict__ c, int nstp, double Vtc)
{
  DEV_PROLOGUE(c)
  const roms_params_t &p = c->p;
  const Blk XB = xcd_block();
  const int i = b.Istr + XB.x * BLK_X + threadIdx.x;
  const int j = b.Jstr + XB.y * BLK_Y + threadIdx.y;
  if (i > b.Iend || j > b.Jend) return;
  const long a = I2(i, j);
  const double g = p.g, eps = 1.0E-10, lmd_cekman = 0.7, lmd_epsilon = 0.1;
  const double gorho0 = g / p.rho0;
  const gcd_t Hz = (gcd_t)c->F.Hz, pden = (gcd_t)c->F.pden, bvf = (gcd_t)c->F.bvf, z_w = (gcd_t)c->F.z_w;
  const gcd_t u = (gcd_t)(c->F.u + (long)(nstp - 1) * n3r), v = (gcd_t)(c->F.v + (long)(nstp - 1) * n3r);
  const gd_t Akv = (gd_t)c->F.Akv, AkT = (gd_t)c->F.Akt, AkS = (gd_t)(c->F.Akt + n3w);
  const gd_t dR = (gd_t)c->ws3[0], dU = (gd_t)c->ws3[1], dV = (gd_t)c->ws3[2];     // W-levels 1..N-1 of this column
  const gd_t hbbl_a = (gd_t)c->kpp.hbbl;
  auto r3i = [&](int k) { return a + (long)(k - 1) * nij; };     // rho-type level k = 1..N
  auto w3i = [&](int k) { return a + (long)k * nij; };           // W-type level k = 0..N
  constexpr int NTH = BLK_X * BLK_Y;
  __shared__ double s_fc[(NMAX - 1) * NTH];                      // the spline coefficient FC(k), k = 1..N-1
  double *const fc_col = s_fc + threadIdx.y * BLK_X + threadIdx.x;

  const bool masking = p.masking != 0;
  const double mr = masking ? (double)GF(rmask)[a] : 1.0;
  const double zw0 = z_w[w3i(0)], zwN = z_w[w3i(N)];
  // bl_dpth from the depth of the previous step (:243), Ustar from the bottom stress (:254)
  double hbbl = hbbl_a[a];
  double bl_dpth = lmd_epsilon * (hbbl - zw0);
  const double Ustar = kpp_ustar(GF(bustr)[a], GF(bustr)[a + 1], GF(bvstr)[a], GF(bvstr)[a + ni], masking, mr);      // :254-257
  // bottom turbulent and surface radiative buoyancy forcing (:272-277), total buoyancy flux at depth z (:288-300)
  const double alpha = GF(alpha)[a], beta = GF(beta)[a];
  const double Bo = g * (alpha * GF(btflx)[a] - beta * GF(btflx)[a + nij]);
  const double Bosol = g * alpha * GF(srflx)[a];
  auto bflux_z = [&](double zgrid) { return kpp_bflux(Bo, Bosol, swfrac(p, zgrid), masking, mr); };

  // ---------- the three parabolic splines, forward (:316-336) ----------
  {
    double FCm = 0.0, dRm = 0.0, dUm = 0.0, dVm = 0.0;
    long q = r3i(1);
    double hzA = Hz[q], pdA = pden[q], uaA = u[q], ubA = u[q + 1], vaA = v[q], vbA = v[q + ni];
    for (int k = 1; k <= N - 1; k++) {
      q = r3i(k + 1);
      const double hzB = Hz[q], pdB = pden[q], uaB = u[q], ubB = u[q + 1], vaB = v[q], vbB = v[q + ni];
      const SplineCoef sc = spline_coef(hzA, hzB, FCm);
      FCm = sc.FC;
      dRm = spline_fwd(sc.cff, 6.0 * (pdB - pdA), hzA, dRm);
      dUm = spline_fwd(sc.cff, 3.0 * (uaB - uaA + ubB - ubA), hzA, dUm);
      dVm = spline_fwd(sc.cff, 3.0 * (vaB - vaA + vbB - vbA), hzA, dVm);
      fc_col[(k - 1) * NTH] = FCm;
      dR[w3i(k)] = dRm; dU[w3i(k)] = dUm; dV[w3i(k)] = dVm;
      hzA = hzB; pdA = pdB; uaA = uaB; ubA = ubB; vaA = vaB; vbA = vbB;
    }
  }
  // ---------- back-substitution (:337-348); the values of level 1 stay in registers ----------
  double dR1 = 0.0, dU1 = 0.0, dV1 = 0.0;                        // x(N) = 0
  for (int k = N - 1; k >= 1; k--) {
    const double fc = fc_col[(k - 1) * NTH];
    dR1 = spline_back(dR[w3i(k)], fc, dR1);
    dU1 = spline_back(dU[w3i(k)], fc, dU1);
    dV1 = spline_back(dV[w3i(k)], fc, dV1);
    dR[w3i(k)] = dR1; dU[w3i(k)] = dU1; dV[w3i(k)] = dV1;
  }
  // ---------- the reference values at the bottom (:408-413): x(0) = 0 ----------
  const double cff1 = 1.0 / 3.0, cff2 = 1.0 / 6.0;
  double Rref, Uref, Vref;
  {
    const long q = r3i(1);
    const double hz = Hz[q];
    Rref = pden[q] - hz * (cff1 * 0.0 + cff2 * dR1);
    Uref = 0.5 * (u[q] + u[q + 1]) - hz * (cff1 * 0.0 + cff2 * dU1);
    Vref = 0.5 * (v[q] + v[q + ni]) - hz * (cff1 * 0.0 + cff2 * dV1);
  }
  // ---------- the critical function FC(k) (:419-465) and the first crossing from the bottom (:474-482), level by
  // level until it is found: the levels above it cannot change hbbl / kbbl any more ----------
  int kbbl = N;
  hbbl = zwN;
  {
    double FCkm = 0.0, zwm = zw0;                                // FC(i,0) = 0
    double dRm = 0.0, dUm = 0.0, dVm = 0.0;
    for (int k = 1; k <= N - 1 && kbbl == N; k++) {
      const long q = r3i(k), qw = w3i(k);
      const double zwk = z_w[qw];
      const double dRk = dR[qw], dUk = dU[qw], dVk = dV[qw];
      const double depth = zwk - zw0;
      const double bf = bflux_z(zwN - zwk);
      double wmk, wsk;
      kpp_wscale(Ustar, bf, bl_dpth, depth, wmk, wsk);
      const double hz = Hz[q];
      const double Rk = pden[q] + hz * (cff1 * dRk + cff2 * dRm);
      const double Uk = 0.5 * (u[q] + u[q + 1]) + hz * (cff1 * dUk + cff2 * dUm);
      const double Vk = 0.5 * (v[q] + v[q + ni]) + hz * (cff1 * dVk + cff2 * dVm);
      const double FCk = kpp_critical(gorho0, Rk, Rref, Uk, Uref, Vk, Vref, depth, Vtc, wsk, bvf[qw]);
      if (FCk > 0.0) {
        hbbl = kpp_crossing(zwk, FCk, zwm, FCkm);
        kbbl = k;
      }
      FCkm = FCk; zwm = zwk;
      dRm = dRk; dUm = dUk; dVm = dVk;
    }
  }
  // ---------- the Ekman limit, the clamps and the mask (:528-536) ----------
  if (Ustar >= 0.0) {
    const double hekman = lmd_cekman * Ustar / fmax(fabs(GF(f)[a]), eps) - GF(h)[a];
    hbbl = fmin(hekman, hbbl);
  }
  hbbl = fmin(hbbl, zwN);
  hbbl = fmax(hbbl, zw0);
  if (masking) hbbl = hbbl * mr;
  hbbl_a[a] = hbbl;
  kpp_wall_rows(b, hbbl_a, a, ni, j, hbbl);                      // bc_r2d_tile: zero gradient at closed walls
  // ---------- kbbl (:592-597) and the buoyancy flux at the final depth (:607-621) ----------
  kbbl = N;
  for (int k = 1; k <= N - 1 && kbbl == N; k++)
    if (z_w[w3i(k)] > hbbl) kbbl = k;
  ((gi_t)c->kpp.kbbl)[a] = kbbl;
  const double Bfbot = kpp_bflux_at(p, Bo, Bosol, zwN - hbbl, masking, mr);
  // ---------- velocity scales and shape functions at hbbl (:635-721) ----------
  bl_dpth = lmd_epsilon * (hbbl - zw0);
  const double zbl = hbbl - zw0;
  double wm, ws;
  const double f1 = kpp_scales_at(Ustar, Bfbot, zbl, wm, ws);
  KppShape G;
  {
    const int k = kbbl;
    const KppBracket B = kpp_bracket(z_w[w3i(k)], z_w[w3i(k - 1)], hbbl);
    G.m = kpp_match<true>(Akv[w3i(k)], Akv[w3i(k - 1)], B, zbl, wm, f1, masking, mr);      // :693
    G.t = kpp_match<true>(AkT[w3i(k)], AkT[w3i(k - 1)], B, zbl, ws, f1, masking, mr);      // :704
    G.s = kpp_match<true>(AkS[w3i(k)], AkS[w3i(k - 1)], B, zbl, ws, f1, masking, mr);      // :716
  }
  // ---------- the merged profile (:727-804), then the lmd_finish increment (lmd_vmix.F:524-540) ----------
  const int ksbl = ((gi_t)c->kpp.ksbl)[a];
  for (int k = 1; k <= N - 1; k++) {
    const long qw = w3i(k);
    const double zwk = z_w[qw];
    double akv = Akv[qw], akt = AkT[qw], aks = AkS[qw];
    if (zwk < hbbl) {
      const double depth = zwk - zw0;
      const double bf = bflux_z(zwN - zwk);
      double wmk, wsk;
      kpp_wscale(Ustar, bf, bl_dpth, depth, wmk, wsk);
      const KppAk P = kpp_blend(depth, zbl, wmk, wsk, G, masking, mr);      // :765
      // the maximum only where the two boundary layers overlap (:785)
      if (k > ksbl) { akv = fmax(akv, P.akv); akt = fmax(akt, P.akt); aks = fmax(aks, P.aks); }
      else { akv = P.akv; akt = P.akt; aks = P.aks; }
    }
    const double conv = kpp_convec(bvf[qw]);
    Akv[qw] = akv + conv;
    AkT[qw] = akt + conv;
    AkS[qw] = aks + conv;
  }
}

// the instantiation of k_lmd_vmix for a level rung and the run-time switches, one bool peeled per call
typedef void (*VmixKernel)(const RomsDev *, int, double, double);
template <int NMAX, bool... B> VmixKernel vmix_kernel() { return k_lmd_vmix<NMAX, B...>; }
template <int NMAX, bool... B, class... R> VmixKernel vmix_kernel(bool on, R... rest)
{
  return on ? vmix_kernel<NMAX, B..., true>(rest...) : vmix_kernel<NMAX, B..., false>(rest...);
}

// lmd_finish_tile boundary values exactly as written at lmd_vmix.F:545-640: W/E columns (note Iend-1 on
// the eastern edge, and no periodicity guard), then S/N rows, then the four corners.
__global__ void k_lmd_edges(const RomsDev *__restrict__ c, int phase)
{
  DEV_PROLOGUE(c)
  const int NAT = b.NAT;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;                                      // 0..N
  const gd_t Akv = (gd_t)(c->F.Akv + (long)k * nij);
  auto copy = [&](long dst, long src) {
    for (int it = 0; it < NAT; it++) GF(Akt)[dst + (long)k * nij + (long)it * n3w] = GF(Akt)[src + (long)k * nij + (long)it * n3w];
    Akv[dst] = Akv[src];
  };
  auto corner = [&](long dst, long s1, long s2) {
    for (int it = 0; it < NAT; it++) {
      const gd_t A = (gd_t)(c->F.Akt + (long)k * nij + (long)it * n3w);
      A[dst] = 0.5 * (A[s1] + A[s2]);
    }
    Akv[dst] = 0.5 * (Akv[s1] + Akv[s2]);
  };
  if (phase == 0) {
    const int j = b.Jstr + q;
    if (j > b.Jend) return;
    if (b.west_edge) copy(I2(b.Istr - 1, j), I2(b.Istr, j));
    if (b.east_edge) copy(I2(b.Iend - 1, j), I2(b.Iend, j));
  } else if (phase == 1) {
    const int i = b.Istr + q;
    if (i > b.Iend) return;
    if (b.south_edge) copy(I2(i, b.Jstr - 1), I2(i, b.Jstr));
    if (b.north_edge) copy(I2(i, b.Jend + 1), I2(i, b.Jend));
  } else if (q == 0) {
    if (b.south_edge && b.west_edge) corner(I2(b.Istr - 1, b.Jstr - 1), I2(b.Istr, b.Jstr - 1), I2(b.Istr - 1, b.Jstr));
    if (b.south_edge && b.east_edge) corner(I2(b.Iend + 1, b.Jstr - 1), I2(b.Iend, b.Jstr - 1), I2(b.Iend + 1, b.Jstr));
    if (b.north_edge && b.west_edge) corner(I2(b.Istr - 1, b.Jend + 1), I2(b.Istr, b.Jend + 1), I2(b.Istr - 1, b.Jend));
    if (b.north_edge && b.east_edge) corner(I2(b.Iend + 1, b.Jend + 1), I2(b.Iend, b.Jend + 1), I2(b.Iend + 1, b.Jend));
  }
}

}  // namespace

// ---- LMD_BKPP: the switch and hbbl, kbbl, ksbl of mod_mixing.F (roms_hip_set_kpp / roms_hip_get_kpp) ----
namespace {
const char *const k_kpp_name[3] = {"hbbl", "kbbl", "ksbl"};
struct KppStore {
  Guarded a[3];                                                  // (count: doubles of the allocation, two ints per double)
  long nij = 0;
} g_kpp;
}  // namespace

// (roms_hip_set_bounds: hbbl, kbbl, ksbl of the bottom boundary layer have the old extents)
void kpp_release()
{
  for (int q = 0; q < 3; q++) guarded_free(&g_kpp.a[q]);
  g_kpp.nij = 0;
  g_ctx.hostc.kpp = RomsKpp{};
  g_ctx.devc_dirty = true;
}

extern "C" int roms_hip_set_kpp(int lmd_bkpp, const double *hbbl)
{
  const char *me = "roms_hip_set_kpp";
  if (int rc = roms_setup_check(me)) return rc;
  if (lmd_bkpp != 0 && lmd_bkpp != 1) return roms_fail(me, "kpp: lmd_bkpp is 0 or 1");
  if (lmd_bkpp == 0) {
    if (g_kpp.a[0].dev) HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    kpp_release();
    return 0;
  }
  const roms_bounds_t &b = g_ctx.b;
  if (b.NAT < 2 || !g_ctx.p.salinity) return roms_fail(me, "kpp: LMD_BKPP is built for the SALINITY set-up (NAT = 2)");
  const long nij = (long)(b.UBi - b.LBi + 1) * (long)(b.UBj - b.LBj + 1);
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  if (!g_kpp.a[0].dev) {
    const long n[3] = {nij, (nij + 1) / 2, (nij + 1) / 2};
    for (int q = 0; q < 3; q++) {
      int rc = guarded_alloc(&g_kpp.a[q], k_kpp_name[q], -1, n[q]);
      if (rc) { kpp_release(); return rc; }
    }
    g_kpp.nij = nij;
  }
  // hbbl of the restart file, or zero as mod_mixing.F leaves it; kbbl and ksbl are outputs and start at zero
  if (hbbl) HIP_TRY(hipMemcpyAsync(g_kpp.a[0].dev, hbbl, sizeof(double) * nij, hipMemcpyHostToDevice, g_ctx.stream));
  else HIP_TRY(hipMemsetAsync(g_kpp.a[0].dev, 0, sizeof(double) * nij, g_ctx.stream));
  for (int q = 1; q < 3; q++) HIP_TRY(hipMemsetAsync(g_kpp.a[q].dev, 0, sizeof(double) * g_kpp.a[q].count, g_ctx.stream));
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  RomsKpp &K = g_ctx.hostc.kpp;
  K.bkpp = 1;
  K.hbbl = g_kpp.a[0].dev;
  K.kbbl = reinterpret_cast<int *>(g_kpp.a[1].dev);
  K.ksbl = reinterpret_cast<int *>(g_kpp.a[2].dev);
  g_ctx.devc_dirty = true;
  return 0;
}

// ---- LMD_DDMIX: the switch and alfaobeta of mod_mixing.F (roms_hip_set_ddmix; read through roms_hip_get_kpp) ----
namespace {
struct DdmixStore {
  Guarded a;                                                     // alfaobeta (LBi:UBi, LBj:UBj, 0:N)
  long n3w = 0;
} g_ddmix;
}  // namespace

// (roms_hip_set_bounds: alfaobeta has the old extents)
void ddmix_release()
{
  guarded_free(&g_ddmix.a);
  g_ddmix.n3w = 0;
  g_ctx.hostc.ddmix = RomsDdmix{};
  g_ctx.devc_dirty = true;
}

extern "C" int roms_hip_set_ddmix(int lmd_ddmix)
{
  const char *me = "roms_hip_set_ddmix";
  if (int rc = roms_setup_check(me)) return rc;
  if (lmd_ddmix != 0 && lmd_ddmix != 1) return roms_fail(me, "ddmix: lmd_ddmix is 0 or 1");
  if (lmd_ddmix == 0) {
    if (g_ddmix.a.dev) HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    ddmix_release();
    return 0;
  }
  const roms_bounds_t &b = g_ctx.b;
  // lmd_vmix.F:376 reads t(isalt) without a SALINITY guard
  if (b.NAT < 2 || !g_ctx.p.salinity) return roms_fail(me, "ddmix: LMD_DDMIX reads salinity: built for the SALINITY set-up (NAT = 2)");
  if (g_ddmix.a.dev) return 0;                                   // already on: alfaobeta stays what rho_eos left
  const long n3w = (long)(b.UBi - b.LBi + 1) * (long)(b.UBj - b.LBj + 1) * (long)(b.N + 1);
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  if (int rc = guarded_alloc(&g_ddmix.a, "alfaobeta", -1, n3w)) { ddmix_release(); return rc; }   // zeroed, as mod_mixing.F leaves it
  g_ddmix.n3w = n3w;
  g_ctx.hostc.ddmix.alfaobeta = g_ddmix.a.dev;
  g_ctx.devc_dirty = true;
  return 0;
}

extern "C" int roms_hip_get_kpp(const char *name, void *host, long n)
{
  const char *me = "roms_hip_get_kpp";
  if (!g_ctx.inited) return roms_fail(me, "library not initialised");
  if (!name || !host) return roms_fail(me, "kpp: null argument");
  if (!strcmp(name, "alfaobeta")) {
    if (!g_ddmix.a.dev) return roms_fail(me, "kpp: LMD_DDMIX is not switched on (roms_hip_set_ddmix)");
    return roms_copy_out(me, "kpp", name, g_ddmix.a.dev, g_ddmix.n3w, host, n);
  }
  for (int q = 0; q < 3; q++) {
    if (strcmp(name, k_kpp_name[q])) continue;
    if (!g_kpp.a[q].dev) return roms_fail(me, "kpp: LMD_BKPP is not switched on (roms_hip_set_kpp)");
    return roms_copy_out(me, "kpp", name, g_kpp.a[q].dev, g_kpp.nij, host, n, q == 0 ? sizeof(double) : sizeof(int), "elements");
  }
  return roms_fail(me, (std::string("kpp: unknown array ") + name).c_str());
}

extern "C" int roms_hip_lmd_vmix(const roms_step_idx_t *s)
{
  int rc = roms_entry_check("roms_hip_lmd_vmix");
  if (rc) return rc;
  if ((rc = check_lbc())) return rc;
  const roms_bounds_t &b = g_ctx.b;
  if (b.NAT < 2 || !g_ctx.p.salinity) return roms_fail("roms_hip_lmd_vmix", "built for the SALINITY set-up (NAT = 2)");
  const long nij = (long)(b.UBi - b.LBi + 1) * (b.UBj - b.LBj + 1);
  const long n3w = nij * (b.N + 1);
  const bool bkpp = g_ctx.hostc.kpp.bkpp != 0;
  const bool ddmix = g_ctx.hostc.ddmix.alfaobeta != nullptr;
  {
    ScopedTimer tm("lmd_vmix");
    // run-time constants of mod_scalars.F:4330 (lmd_Cg) and lmd_skpp.F:300 (Vtc), evaluated on the host
    const double vonKar = 0.41, lmd_Cstar = 10.0, lmd_Cv = 1.25, lmd_Ric = 0.3, lmd_betaT = -0.2, lmd_cs = 98.96,
                 lmd_epsilon = 0.1;
    const double lmd_Cg = lmd_Cstar * vonKar * pow(lmd_cs * vonKar * lmd_epsilon, 1.0 / 3.0);
    const double Vtc = lmd_Cv * sqrt(-lmd_betaT) / (sqrt(lmd_cs * lmd_epsilon) * lmd_Ric * vonKar * vonKar);
    const dim3 grid = grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1);
    if (b.N > ROMS_MAXN) return roms_fail("roms_hip_lmd_vmix", "N > 64 not instantiated");
    const bool n32 = b.N <= 32;                                  // <32 | ROMS_MAXN> x <BKPP> x <DDMIX>
    hipLaunchKernelGGL(n32 ? vmix_kernel<32>(bkpp, ddmix) : vmix_kernel<ROMS_MAXN>(bkpp, ddmix), grid, block2d(), 0, g_ctx.stream, g_ctx.devc, s->nstp, lmd_Cg, Vtc);
    KERNEL_CHECK("k_lmd_vmix");
    if (bkpp) {
      // LMD_BKPP, lmd_vmix.F:83-89: lmd_skpp without the lmd_finish increment, then lmd_bkpp, which adds it (the Vtc of
      // lmd_bkpp.F:233 is the expression of lmd_skpp.F:300); it reads AkT and AkS separately, LMD_DDMIX changes nothing in it
      hipLaunchKernelGGL(n32 ? k_lmd_bkpp<32> : k_lmd_bkpp<ROMS_MAXN>, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, s->nstp, Vtc);
      KERNEL_CHECK("k_lmd_bkpp");
    }
    const int nj = b.Jend - b.Jstr + 1, ni_ = b.Iend - b.Istr + 1;
    if (b.west_edge || b.east_edge)
      hipLaunchKernelGGL(k_lmd_edges, dim3((nj + 63) / 64, b.N + 1), dim3(64), 0, g_ctx.stream, g_ctx.devc, 0);
    if (b.south_edge || b.north_edge)
      hipLaunchKernelGGL(k_lmd_edges, dim3((ni_ + 63) / 64, b.N + 1), dim3(64), 0, g_ctx.stream, g_ctx.devc, 1);
    if ((b.south_edge || b.north_edge) && (b.west_edge || b.east_edge))
      hipLaunchKernelGGL(k_lmd_edges, dim3(1, b.N + 1), dim3(64), 0, g_ctx.stream, g_ctx.devc, 2);
    KERNEL_CHECK("k_lmd_edges");
  }
  // bc_r2d_tile(hsbl) (the kernel wrote the wall rows of a channel; western / eastern edges and corners through the
  // generic edge kernel) + exchange; bc_w3d_tile(Akv), bc_w3d_tile(Akt(:,:,:,itrc)): wall rows + exchange
  if (!b.EWperiodic && (rc = bc_generic(LBV_ZETA, LBV_ZETA, g_ctx.field[FID_hsbl].dev, 1))) return rc;
  if ((rc = halo_exchange2d(GT_R, g_ctx.field[FID_hsbl].dev))) return rc;
  if (bkpp) {                                                    // bc_r2d_tile(hbbl) + exchange, lmd_bkpp.F:577-586
    if (!b.EWperiodic && (rc = bc_generic(LBV_ZETA, LBV_ZETA, g_kpp.a[0].dev, 1))) return rc;
    if ((rc = halo_exchange2d(GT_R, g_kpp.a[0].dev))) return rc;
  }
  if ((rc = bc_w3d(g_ctx.field[FID_Akv].dev))) return rc;
  for (int it = 0; it < b.NAT; it++)
    if ((rc = bc_w3d(g_ctx.field[FID_Akt].dev + (long)it * n3w))) return rc;
  return 0;
}
