// k_biology.hip -- biology(ng,tile), ROMS/Nonlinear/biology.F:35 (main3d.F:795-797, between gls_corstep and step3d_t):
// the source and sink terms of the ecosystem model on t(:,:,:,nnew,idbio).  Built: NPZD_POWELL, npzd_powell_tile
// (ROMS/Nonlinear/Biology/npzd_Powell.h:91-661) -- nitrate, phytoplankton, zooplankton, detritus; the chained
// backward-implicit reaction sweeps inside the BioIter loop and the sinking of phytoplankton and detritus (bio_sink.h).
// The other models are refused by name.
#include "roms_dev.h"
#include "bio_sink.h"

namespace {

// Positive-definite concentrations, npzd_Powell.h:237-251 for one time level: v = the four pools in the order of idbio.
// The deficit below MinVal is summed, every pool is lifted to MinVal, and the deficit is taken from the largest pool
// (strict >: the first of equal pools wins; compared as the reference compares, the earlier pools already lifted) when
// that pool exceeds it.
__device__ __forceinline__ void bio_positive(double (&v)[4])
{
  const double MinVal = 1.0e-6;
  double cff1 = 0.0, vmax = 0.0;
  int imax = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    cff1 = cff1 + fmax(0.0, MinVal - v[q]);
    if (q > 0 && v[q] > vmax) imax = q;
    v[q] = fmax(MinVal, v[q]);
    if (imax == q) vmax = v[q];
  }
  if (vmax > cff1) {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (q == imax) v[q] = vmax - cff1;
  }
}

// =================================================================================================
// npzd_powell_tile, one thread per column (i, j) of Istr:Iend, Jstr:Jend, i fastest: every level access is one double
// per lane along i.  The reference's operation order throughout (the parity of tests/test_gpu_bio.py relies on the
// inverses of Hz being formed first and multiplied, :199-214).
//
// Where the column lives.  The reference keeps Bio, Bio_old (4 pools each), Light and the seven arrays of the sinking
// per column; whole, that is about 5 kB per thread at N = 64.  Here:
//   * light and the five reaction sweeps are one descending sweep: Light(k) needs the phytoplankton of the levels above
//     as the iteration found them, and every reaction is local to its cell, so cell k is attenuated, then reacted;
//   * the four pools wait between the sweeps in the 3-D scratch slots ws3[0..3] (private to the thread);
//   * the sinking column is in LDS and its bL, bR in ws3[4], ws3[5] (bio_sink.h); a constituent with w = 0 is skipped:
//     its flux is Hz * 0 * (...) and the column comes back unchanged;
//   * Bio_old is formed again from t(nstp) for the update instead of being kept.
// The positivity step of t(nnew) * Hz_inv (:232, itime = nnew) leaves no trace in the reference -- only BioTrc(:,nstp)
// goes on into Bio and Bio_old (:256-260) -- and is not evaluated.  rmask is never read (the reference does not); no
// point outside Istr:Iend, Jstr:Jend is touched.
// =================================================================================================
template <int NMAX>
__global__ void __launch_bounds__(BLK_X *BLK_Y)
k_npzd_powell(const RomsDev *__restrict__ c, int nstp, int nnew, double dtdays)
{
  DEV_PROLOGUE(c)
  const roms_bio_powell_t &P = c->bio.powell;
  const Blk XB = xcd_block();
  const int i = b.Istr + XB.x * BLK_X + threadIdx.x;
  const int j = b.Jstr + XB.y * BLK_Y + threadIdx.y;
  if (i > b.Iend || j > b.Jend) return;
  const long a = I2(i, j);
  constexpr int NTH = BLK_X * BLK_Y;
  __shared__ double s_q[NMAX * NTH];                             // the sinking column, level k at (k-1) * NTH
  double *const q_col = s_q + threadIdx.y * BLK_X + threadIdx.x;
  const gcd_t Hz = (gcd_t)c->F.Hz, z_w = (gcd_t)c->F.z_w;
  gcd_t tS[4];
  gd_t tN[4], B[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    tS[q] = (gcd_t)(c->F.t + ((long)(nstp - 1) + 3L * (P.idbio[q] - 1)) * n3r);
    tN[q] = (gd_t)(c->F.t + ((long)(nnew - 1) + 3L * (P.idbio[q] - 1)) * n3r);
    B[q] = (gd_t)c->ws3[q];
  }
  const gd_t bLa = (gd_t)c->ws3[4], bRa = (gd_t)c->ws3[5];
  auto r3i = [&](int k) { return a + (long)(k - 1) * nij; };     // rho-type level k = 1..N
  auto w3i = [&](int k) { return a + (long)k * nij; };           // W-type level k = 0..N
  enum { iNO3 = 0, iPhyt = 1, iZoop = 2, iSDet = 3 };

  // surface PAR, :268-277
  const double PARsur = P.const_par ? 158.075 : P.PARfrac * GF(srflx)[a] * c->p.rho0 * P.Cp;
  // the constants of the sweeps, :371-373, :391-392, :411-413, :427-429, :442-443
  const double up1 = dtdays * P.Vm_NO3 * P.PhyIS, up2 = P.Vm_NO3 * P.Vm_NO3, up3 = P.PhyIS * P.PhyIS;
  const double gr1 = dtdays * P.ZooGR, gr2 = 1.0 - P.ZooEEN - P.ZooEED;
  const double pm3 = dtdays * P.PhyMRD, pm2 = dtdays * P.PhyMRN, pm1 = 1.0 / (1.0 + pm2 + pm3);
  const double zm3 = dtdays * P.ZooMRD, zm2 = dtdays * P.ZooMRN, zm1 = 1.0 / (1.0 + zm2 + zm3);
  const double dr2 = dtdays * P.DetRR, dr1 = 1.0 / (1.0 + dr2);
  const double wsink[2] = {dtdays * fabs(P.wPhy), dtdays * fabs(P.wDet)};     // :589, in the order of idsink

#pragma unroll 1
  for (int Iter = 1; Iter <= P.BioIter; Iter++) {
    // ---------- light (:337-363) and the reactions (:371-450), surface to bottom ----------
    double PAR = PARsur;
    double zwt = z_w[w3i(N)];
#pragma unroll 1
    for (int k = N; k >= 1; k--) {
      double v[4];
      if (Iter == 1) {                                           // :229-260: Bio = the positive-definite t(nstp)
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = tS[q][r3i(k)];
        bio_positive(v);
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = B[q][r3i(k)];
      }
      const double zwb = z_w[w3i(k - 1)];
      double Light = 0.0;                                        // night time, :358-362
      if (PARsur > 0.0) {
        const double Att = (P.AttSW + P.AttPhy * v[iPhyt]) * (zwt - zwb);
        const double ExpAtt = exp(-Att);
        const double Itop = PAR;
        PAR = Itop * (1.0 - ExpAtt) / Att;                       // average at the cell centre
        Light = PAR;
        PAR = Itop * ExpAtt;                                     // at the bottom of the cell
      }
      zwt = zwb;
      {                                                          // nitrate uptake, :374-384
        const double cff4 = 1.0 / sqrt(up2 + up3 * Light * Light);
        const double cff = v[iPhyt] * up1 * cff4 * Light / (P.K_NO3 + v[iNO3]);
        v[iNO3] = v[iNO3] / (1.0 + cff);
        v[iPhyt] = v[iPhyt] + v[iNO3] * cff;
      }
      {                                                          // Ivlev grazing, :393-406
        const double cff = v[iZoop] * gr1 * (1.0 - exp(-P.Ivlev * v[iPhyt])) / v[iPhyt];
        v[iPhyt] = v[iPhyt] / (1.0 + cff);
        v[iZoop] = v[iZoop] + v[iPhyt] * gr2 * cff;
        v[iNO3] = v[iNO3] + v[iPhyt] * P.ZooEEN * cff;
        v[iSDet] = v[iSDet] + v[iPhyt] * P.ZooEED * cff;
      }
      v[iPhyt] = v[iPhyt] * pm1;                                 // phytoplankton mortality, :414-422
      v[iNO3] = v[iNO3] + v[iPhyt] * pm2;
      v[iSDet] = v[iSDet] + v[iPhyt] * pm3;
      v[iZoop] = v[iZoop] * zm1;                                 // zooplankton mortality, :430-438
      v[iNO3] = v[iNO3] + v[iZoop] * zm2;
      v[iSDet] = v[iSDet] + v[iZoop] * zm3;
      v[iSDet] = v[iSDet] * dr1;                                 // remineralisation, :444-450
      v[iNO3] = v[iNO3] + v[iSDet] * dr2;
#pragma unroll
      for (int q = 0; q < 4; q++) B[q][r3i(k)] = v[q];
    }
    // ---------- sinking of phytoplankton, then detritus (:460-630) ----------
#pragma unroll
    for (int isink = 0; isink < 2; isink++) {
      if (wsink[isink] == 0.0) continue;
      const gd_t Bs = B[isink == 0 ? iPhyt : iSDet];
#pragma unroll 1
      for (int k = 1; k <= N; k++) q_col[(k - 1) * NTH] = Bs[r3i(k)];
      (void)sink_column<NMAX, NTH>(Hz, z_w, a, nij, N, q_col, bLa, bRa, wsink[isink]);
#pragma unroll 1
      for (int k = 1; k <= N; k++) Bs[r3i(k)] = q_col[(k - 1) * NTH];
    }
  }
  // ---------- the increment in transport units, :648-656 ----------
#pragma unroll 1
  for (int k = 1; k <= N; k++) {
    double old[4];
#pragma unroll
    for (int q = 0; q < 4; q++) old[q] = tS[q][r3i(k)];
    bio_positive(old);                                           // Bio_old, as the first sweep formed it
    const double hz = Hz[r3i(k)];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const double cff = B[q][r3i(k)] - old[q];
      tN[q][r3i(k)] = tN[q][r3i(k)] + cff * hz;
    }
  }
}

const char *const k_bio_name[] = {"NONE", "NPZD_POWELL", "NPZD_FRANKS", "NPZD_IRON", "BIO_FENNEL", "NEMURO", "ECOSIM",
                                  "HYPOXIA_SRM", "RED_TIDE"};

}  // namespace

// (roms_hip_set_bounds: the tracer indices of the biology setting belong to the old NT)
void bio_release()
{
  g_ctx.hostc.bio = RomsBio{};
  g_ctx.devc_dirty = true;
}

extern "C" int roms_hip_set_biology(int model, const void *par, long nbytes)
{
  const char *me = "roms_hip_set_biology";
  if (int rc = roms_setup_check(me)) return rc;
  char msg[200];
  if (model < ROMS_BIO_NONE || model > ROMS_BIO_RED_TIDE) {
    snprintf(msg, sizeof msg, "biology: unknown model %d", model);
    return roms_fail(me, msg);
  }
  if (model == ROMS_BIO_NONE) {
    if (g_ctx.hostc.bio.model != ROMS_BIO_NONE) HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    bio_release();
    return 0;
  }
  if (model != ROMS_BIO_NPZD_POWELL) {
    snprintf(msg, sizeof msg, "biology: %s is not built (built: NPZD_POWELL)", k_bio_name[model]);
    return roms_fail(me, msg);
  }
  if (!par) return roms_fail(me, "biology: null parameter block");
  if (nbytes != (long)sizeof(roms_bio_powell_t)) {
    snprintf(msg, sizeof msg, "biology: nbytes = %ld, roms_bio_powell_t has %ld bytes", nbytes, (long)sizeof(roms_bio_powell_t));
    return roms_fail(me, msg);
  }
  roms_bio_powell_t P;
  memcpy(&P, par, sizeof P);
  const roms_bounds_t &b = g_ctx.b;
  for (int q = 0; q < 4; q++) {
    if (P.idbio[q] < b.NAT + 1 || P.idbio[q] > b.NT) {
      snprintf(msg, sizeof msg, "biology: idbio(%d) = %d lies outside NAT+1 .. NT = %d .. %d", q + 1, P.idbio[q], b.NAT + 1, b.NT);
      return roms_fail(me, msg);
    }
    for (int r = 0; r < q; r++)
      if (P.idbio[r] == P.idbio[q]) {
        snprintf(msg, sizeof msg, "biology: idbio(%d) = idbio(%d) = %d, a tracer is repeated", r + 1, q + 1, P.idbio[q]);
        return roms_fail(me, msg);
      }
  }
  if (P.BioIter < 0) return roms_fail(me, "biology: BioIter < 0");
  if (!(P.wPhy >= 0.0)) return roms_fail(me, "biology: sinking speed wPhy < 0");
  if (!(P.wDet >= 0.0)) return roms_fail(me, "biology: sinking speed wDet < 0");
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));      // a kernel in flight reads the block this replaces
  g_ctx.hostc.bio.model = model;
  g_ctx.hostc.bio.powell = P;
  g_ctx.devc_dirty = true;
  return 0;
}

extern "C" int roms_hip_biology(const roms_step_idx_t *s)
{
  const char *me = "roms_hip_biology";
  int rc = roms_entry_check(me);
  if (rc) return rc;
  if (g_ctx.hostc.bio.model == ROMS_BIO_NONE) return roms_fail(me, "biology is not switched on (roms_hip_set_biology)");
  const roms_bounds_t &b = g_ctx.b;
  if (b.N < 4) return roms_fail(me, "needs N >= 4 levels (the vertical stencils of the column read k-1 .. k+2)");
  if (b.N > ROMS_MAXN) return roms_fail(me, "N > 64 not instantiated");
  const roms_bio_powell_t &P = g_ctx.hostc.bio.powell;
  if (P.BioIter <= 0) return 0;                     // npzd_Powell.h:180
  ScopedTimer tm("biology");
  // the time step of one iteration in days, npzd_Powell.h:184 (sec2day = 1 / 86400, mod_scalars.F:792)
  const double sec2day = 1.0 / 86400.0;
  const double dtdays = g_ctx.p.dt * sec2day / (double)P.BioIter;
  const dim3 grid = grid2d(b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1);
  // the smallest instantiation that holds N (the level counts of the other column kernels)
  if (b.N <= 16) hipLaunchKernelGGL(k_npzd_powell<16>, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, s->nstp, s->nnew, dtdays);
  else if (b.N <= 32) hipLaunchKernelGGL(k_npzd_powell<32>, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, s->nstp, s->nnew, dtdays);
  else if (b.N <= 48) hipLaunchKernelGGL(k_npzd_powell<48>, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, s->nstp, s->nnew, dtdays);
  else hipLaunchKernelGGL(k_npzd_powell<ROMS_MAXN>, grid, block2d(), 0, g_ctx.stream, g_ctx.devc, s->nstp, s->nnew, dtdays);
  KERNEL_CHECK("k_npzd_powell");
  return 0;
}
