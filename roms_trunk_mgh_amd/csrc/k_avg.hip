// k_avg.hip -- set_avg(ng,tile), ROMS/Nonlinear/set_avg.F:28 (AVERAGES; main3d.F:493-495): initialise, accumulate
// and scale the time-averaged fields of include/roms_avg.def, and the WET_DRY counters of wet steps with
// set_avg_masks (ROMS/Utility/set_masks.F:412-517).
//
// ONE launch serves every selected average: the kernel-argument struct carries a table of descriptors (destination,
// sources, expression, loop ranges, mask and counter) and the grid is laid over (x-blocks, rows, descriptor x level),
// as k_periodic_multi / k_pack_multi of halo.hip do for the exchanges.  A launch per field would cost more than the
// traffic on the small configurations.  The kernel is pure streaming: per point one read of each source, one read
// (not on an initialising step) and one write of the sum.
//
// Operation order = the reference's, factor by factor from left to right:
//   initialise   avg = x [* mask]                                    set_avg.F:280-1256
//   accumulate   avg = avg + [mask *] x                              :1308-2288
//   scale        avg = fac * avg                                     :2340-3960
// On a step that closes the window the reference sweeps twice (accumulate, then scale); here the two are one pass,
// fac * (avg + [mask *] x): the same operations in the same order per point, and the build has -ffp-contract=off, so
// the result is bit-identical.  With nAVG = 1 every step is initialise + scale.
#include "roms_dev.h"
#include <algorithm>

// ---- the lines of roms_avg.def and the library-owned arrays (roms_hip_set_averages below) ----
struct AvgLine {
  const char *name, *why;     // why != nullptr: not built
  int gtype, shape, mask, range, expr, srcA, srcB, plane;
  int counter;                // 0..3 = p, r, u, v counter; -1 = an average
};
struct AvgArray {
  int id, itrc;               // line of the table, tracer (1-based; 0 = not per tracer)
  int nk;                     // planes: 1, N or N+1
  Guarded a;
};
#define ROMS_AVG_MAXARR (AVG_COUNT + ROMS_AVG_NTKINDS * ROMS_MAXNT)
struct AvgStore {
  int nAVG = 0, ntsAVG = 0, ntstart = 0, nrrec = 0;
  int n = 0;
  AvgArray arr[ROMS_AVG_MAXARR];
  Guarded cnt[4];             // pmask_avg, rmask_avg, umask_avg, vmask_avg
  long nij = 0;
};
enum { AVG_GT_r = GT_R, AVG_GT_u = GT_U, AVG_GT_v = GT_V, AVG_GT_w = GT_R, AVG_GT_p = GT_P };
enum { AVG_CNT_p = 0, AVG_CNT_r, AVG_CNT_u, AVG_CNT_v };
static const AvgLine k_avg_line[AVG_COUNT] = {
#define ROMS_AVG(name, aout, grid, shape, mask, range, expr, srcA, srcB, plane)                                       \
  {#name, nullptr, AVG_GT_##grid, shape, FID_##mask, range, expr, FID_##srcA, FID_##srcB, plane, -1},
#define ROMS_AVG_NOT_BUILT(name, aout, why) {#name, #aout ": " #why, 0, 0, 0, 0, 0, 0, 0, 0, -1},
#define ROMS_AVG_COUNTER(name, grid) {#name, nullptr, AVG_GT_##grid, AVS_2D, 0, 0, 0, 0, 0, 0, AVG_CNT_##grid},
#include "roms_avg.def"
#undef ROMS_AVG
#undef ROMS_AVG_NOT_BUILT
#undef ROMS_AVG_COUNTER
};
static AvgStore g_avg;

namespace {

const int k_kind[FID_COUNT] = {
#define ROMS_FIELD(name, kind, owner) kind,
#include "roms_fields.def"
#undef ROMS_FIELD
};

#define AVG_MAXDESC 48            // 48 descriptors of 64 B + the scalars stay below the 4 KB of kernel arguments
struct AvgDesc {
  double *dst;
  const double *a, *b;            // the sources, at the plane that goes with level 0 of the average
  const double *mask;             // WET_DRY: the *_full mask of the block
  const double *cnt;              // WET_DRY: the counter of wet steps of the grid type (closing factor)
  int expr, koff;                 // X_* of roms_avg.def; first plane of this descriptor in the launch
  int i0, i1, j0, j1;             // the loop ranges of the block
};
struct AvgArgs {
  AvgDesc d[AVG_MAXDESC];
  const double *pm, *pn;
  double fac;                     // 1 / nAVG (closing factor without WET_DRY)
  long ni, nij;
  int n, LBi, LBj;
};

enum { AVM_SET = 0, AVM_ADD = 1, AVM_SET_CLOSE = 2, AVM_ADD_CLOSE = 3 };

// the source expression x at point q of plane k; LEAD: m * x with m as the leftmost factor (accumulation under WET_DRY)
template <bool LEAD>
__device__ __forceinline__ double avg_term(const AvgDesc &d, const AvgArgs &a, long q2, long q, double m)
{
  gcd_t A = (gcd_t)d.a, B = (gcd_t)d.b;
  switch (d.expr) {
  case X_COPY: return LEAD ? m * A[q] : A[q];
  case X_SQ: return LEAD ? m * A[q] * A[q] : A[q] * A[q];
  case X_WPMPN: {
    const double pm = ((gcd_t)a.pm)[q2], pn = ((gcd_t)a.pn)[q2];
    return LEAD ? m * A[q] * pm * pn : A[q] * pm * pn;
  }
  case X_UV: {
    const double su = A[q] + A[q + 1], sv = B[q] + B[q + a.ni];
    return LEAD ? m * 0.25 * su * sv : 0.25 * su * sv;
  }
  case X_UT: {
    const double st = B[q - 1] + B[q];
    return LEAD ? m * 0.5 * A[q] * st : 0.5 * A[q] * st;
  }
  default: {  // X_VT
    const double st = B[q - a.ni] + B[q];
    return LEAD ? m * 0.5 * A[q] * st : 0.5 * A[q] * st;
  }
  }
}

// grid: x = blocks of BLK_X columns from LBi, y = groups of BLK_Y rows (capped: the rows are strided), z = plane
template <int MODE, bool WET>
__global__ void __launch_bounds__(BLK_X *BLK_Y) k_avg(const AvgArgs a)
{
  const int kk = blockIdx.z;
  int f = 0;
  while (f + 1 < a.n && kk >= a.d[f + 1].koff) f++;
  const AvgDesc &d = a.d[f];
  const int k = kk - d.koff;
  const int i = a.LBi + (int)(blockIdx.x * BLK_X + threadIdx.x);
  if (i < d.i0 || i > d.i1) return;
  gd_t dst = (gd_t)d.dst;
  for (int j = d.j0 + (int)(blockIdx.y * BLK_Y + threadIdx.y); j <= d.j1; j += (int)gridDim.y * BLK_Y) {
    const long q2 = (long)(i - a.LBi) + (long)(j - a.LBj) * a.ni;
    const long q = q2 + (long)k * a.nij;
    const double m = WET ? ((gcd_t)d.mask)[q2] : 1.0;
    double v;
    if (MODE == AVM_SET || MODE == AVM_SET_CLOSE) {
      v = avg_term<false>(d, a, q2, q, m);
      if (WET) v = v * m;
    } else {
      v = dst[q] + avg_term<WET>(d, a, q2, q, m);
    }
    if (MODE == AVM_SET_CLOSE || MODE == AVM_ADD_CLOSE) {
      const double fac = WET ? 1.0 / fmax(1.0, ((gcd_t)d.cnt)[q2]) : a.fac;      // set_avg.F:2317-2335
      v = fac * v;
    }
    dst[q] = v;
  }
}

// WET_DRY: the four counters pmask_avg, rmask_avg, umask_avg, vmask_avg (blockIdx.z).  mode 0: set_avg.F:248-275
// (= the clamped mask), 1: :1272-1303 (+ the clamped mask), 2: set_masks.F:470-489 (MIN(1, counter) after the close).
struct CntArgs {
  double *cnt[4];
  const double *full[4];
  int i0[4], i1[4], j0[4], j1[4];
  long ni;
  int LBi, LBj, mode;
};
__global__ void __launch_bounds__(BLK_X *BLK_Y) k_avg_counters(const CntArgs a)
{
  const int c = blockIdx.z;
  const int i = a.LBi + (int)(blockIdx.x * BLK_X + threadIdx.x);
  const int j = a.LBj + (int)(blockIdx.y * BLK_Y + threadIdx.y);
  if (i < a.i0[c] || i > a.i1[c] || j < a.j0[c] || j > a.j1[c]) return;
  const long q2 = (long)(i - a.LBi) + (long)(j - a.LBj) * a.ni;
  gd_t cnt = (gd_t)a.cnt[c];
  if (a.mode == 2) { cnt[q2] = fmin(1.0, cnt[q2]); return; }
  const double wet = fmax(0.0, fmin(((gcd_t)a.full[c])[q2], 1.0));
  cnt[q2] = a.mode == 0 ? wet : cnt[q2] + wet;
}

// the plane of a source that goes with level 0 (k = 1 of an N array, k = 0 of a 0:N array) of the average
const double *avg_source(int fid, const roms_step_idx_t *s, int itrc, int plane)
{
  const roms_bounds_t &b = g_ctx.b;
  const long nij = (long)(b.UBi - b.LBi + 1) * (long)(b.UBj - b.LBj + 1);
  const double *p = g_ctx.field[fid].dev;
  switch (k_kind[fid]) {
  case K_2D_T3: return p + (long)(s->kstp - 1) * nij;                                      // KOUT = kstp
  case K_3DR_T2: return p + (long)(s->nrhs - 1) * nij * b.N;                               // NOUT = nrhs
  case K_4DT: return p + ((long)(s->nrhs - 1) + 3L * (itrc - 1)) * nij * b.N;
  case K_3DW_NAT: return p + (long)plane * nij * (b.N + 1);
  case K_2D_NT: return p + (long)plane * nij;
  default: return p;
  }
}

void avg_range(int range, int *i0, int *i1, int *j0, int *j1)
{
  const roms_bounds_t &b = g_ctx.b;
  const bool iR = range == RNG_RR || range == RNG_VR || range == RNG_VI;                   // i = IstrR:IendR
  const bool jR = range == RNG_RR || range == RNG_UR || range == RNG_UI;                   // j = JstrR:JendR
  *i0 = iR ? b.IstrR : b.Istr;
  *i1 = (range == RNG_II || range == RNG_UI) ? b.Iend : b.IendR;
  *j0 = jR ? b.JstrR : b.Jstr;
  *j1 = (range == RNG_II || range == RNG_VI) ? b.Jend : b.JendR;
}

template <bool WET>
void avg_launch(int mode, dim3 grid, const AvgArgs &a)
{
  const dim3 blk = block2d();
  switch (mode) {
  case AVM_SET: hipLaunchKernelGGL((k_avg<AVM_SET, WET>), grid, blk, 0, g_ctx.stream, a); break;
  case AVM_ADD: hipLaunchKernelGGL((k_avg<AVM_ADD, WET>), grid, blk, 0, g_ctx.stream, a); break;
  case AVM_SET_CLOSE: hipLaunchKernelGGL((k_avg<AVM_SET_CLOSE, WET>), grid, blk, 0, g_ctx.stream, a); break;
  default: hipLaunchKernelGGL((k_avg<AVM_ADD_CLOSE, WET>), grid, blk, 0, g_ctx.stream, a); break;
  }
}

int avg_counters(int mode)
{
  const roms_bounds_t &b = g_ctx.b;
  CntArgs c;
  const double *full[4] = {g_ctx.field[FID_pmask_full].dev, g_ctx.field[FID_rmask_full].dev, g_ctx.field[FID_umask_full].dev,
                           g_ctx.field[FID_vmask_full].dev};
  // p, r, u, v: set_avg.F:248-275 / :1272-1303; after the close set_masks.F:470-489
  const int i0[2][4] = {{b.Istr, b.IstrR, b.Istr, b.IstrR}, {b.IstrP, b.IstrT, b.IstrP, b.IstrT}};
  const int i1[2][4] = {{b.IendR, b.IendR, b.IendR, b.IendR}, {b.IendP, b.IendT, b.IendT, b.IendT}};
  const int j0[2][4] = {{b.Jstr, b.JstrR, b.JstrR, b.Jstr}, {b.JstrP, b.JstrT, b.JstrT, b.JstrP}};
  const int j1[2][4] = {{b.JendR, b.JendR, b.JendR, b.JendR}, {b.JendP, b.JendT, b.JendT, b.JendT}};
  const int r = mode == 2;
  for (int q = 0; q < 4; q++) {
    c.cnt[q] = g_avg.cnt[q].dev;
    c.full[q] = full[q];
    // never outside the allocation, whatever the bounds say
    c.i0[q] = std::max(i0[r][q], b.LBi); c.i1[q] = std::min(i1[r][q], b.UBi);
    c.j0[q] = std::max(j0[r][q], b.LBj); c.j1[q] = std::min(j1[r][q], b.UBj);
  }
  c.ni = b.UBi - b.LBi + 1;
  c.LBi = b.LBi; c.LBj = b.LBj; c.mode = mode;
  dim3 grid = grid2d(b.UBi - b.LBi + 1, b.UBj - b.LBj + 1);
  grid.z = 4;
  hipLaunchKernelGGL(k_avg_counters, grid, block2d(), 0, g_ctx.stream, c);
  KERNEL_CHECK("k_avg_counters");
  return 0;
}

}  // namespace

// row of AoutT of a per-tracer line = its rank among the AVS_NT lines of the table; -1 otherwise
static int avg_tkind(int id)
{
  const AvgLine &L = k_avg_line[id];
  if (L.why || L.counter >= 0 || L.shape != AVS_NT) return -1;
  int r = 0;
  for (int q = 0; q < id; q++)
    if (!k_avg_line[q].why && k_avg_line[q].counter < 0 && k_avg_line[q].shape == AVS_NT) r++;
  return r;
}

// (roms_hip_set_bounds: the averages have the old extents)
void avg_release()
{
  for (int q = 0; q < g_avg.n; q++) guarded_free(&g_avg.arr[q].a);
  for (int q = 0; q < 4; q++) guarded_free(&g_avg.cnt[q]);
  g_avg = AvgStore{};
}

// The schedule of set_avg_tile and set_avg_masks, stated once (mirror: roms_trunk_mgh_amd/avg.py, phase()).
extern "C" int roms_hip_avg_phase(int iic, int nAVG, int ntsAVG, int ntstart, int nrrec)
{
  if (nAVG <= 0) return 0;                                                    // set_avg.F:189
  int ph = 0;
  const bool restart = nrrec > 0 && iic == ntstart;
  if ((iic > ntsAVG && (iic - 1) % nAVG == 1) || (iic >= ntsAVG && nAVG == 1) || restart) ph |= AVP_SET;   // :237-240
  else if (iic > ntsAVG) ph |= AVP_ADD;                                                                    // :1264
  const bool window_end = iic > ntsAVG && (iic - 1) % nAVG == 0 && !restart;
  if (window_end || (iic >= ntsAVG && nAVG == 1)) ph |= AVP_CLOSE;                                         // :2298-2301
  if (window_end) ph |= AVP_MASKS;                                                                // set_masks.F:466-468
  return ph;
}

extern "C" int roms_hip_set_averages(int nAVG, int ntsAVG, int ntstart, int nrrec, const int *Aout, const int *AoutT)
{
  const char *me = "roms_hip_set_averages";
  if (int rc = roms_setup_check(me)) return rc;
  if (nAVG < 0) return roms_fail(me, "averages: nAVG < 0");
  if (nAVG == 0) {
    if (g_avg.n || g_avg.cnt[0].dev) HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    avg_release();
    return 0;
  }
  if (!Aout) return roms_fail(me, "averages: Aout is NULL");
  const roms_bounds_t &b = g_ctx.b;
  const long nij = (long)(b.UBi - b.LBi + 1) * (long)(b.UBj - b.LBj + 1);
  // the selection; nothing is touched before all of it has been looked at
  AvgStore want;
  want.nAVG = nAVG; want.ntsAVG = ntsAVG; want.ntstart = ntstart; want.nrrec = nrrec; want.nij = nij;
  for (int id = 0; id < AVG_COUNT; id++) {
    const AvgLine &L = k_avg_line[id];
    if (L.counter >= 0) continue;
    const int tk = avg_tkind(id);
    for (int it = (tk >= 0 ? 1 : 0); it <= (tk >= 0 ? b.NT : 0); it++) {
      if (tk >= 0 ? !(AoutT && AoutT[tk * b.NT + it - 1]) : !Aout[id]) continue;
      if (L.why) {
        const std::string m = std::string("averages: ") + L.name + " is not built (" + L.why + ")";
        return roms_fail(me, m.c_str());
      }
      for (int fid : {L.srcA, L.srcB, L.expr == X_WPMPN ? (int)FID_pm : L.srcA, L.expr == X_WPMPN ? (int)FID_pn : L.srcA})
        if (!g_ctx.field[fid].dev) {
          const std::string m = std::string("averages: ") + L.name + " reads " + k_field_name[fid] + ", which is not registered";
          return roms_fail(me, m.c_str());
        }
      if (k_kind[L.srcA] == K_3DW_NAT && L.plane >= b.NAT) {
        const std::string m = std::string("averages: ") + L.name + " reads tracer " + std::to_string(L.plane + 1) + " of " +
                              k_field_name[L.srcA] + ", the tile has NAT = " + std::to_string(b.NAT);
        return roms_fail(me, m.c_str());
      }
      if (k_kind[L.srcA] == K_2D_NT && L.plane >= b.NT) {
        const std::string m = std::string("averages: ") + L.name + " reads tracer " + std::to_string(L.plane + 1) + " of " +
                              k_field_name[L.srcA] + ", the tile has NT = " + std::to_string(b.NT);
        return roms_fail(me, m.c_str());
      }
      AvgArray &a = want.arr[want.n++];
      a.id = id; a.itrc = it;
      a.nk = L.shape == AVS_2D ? 1 : L.shape == AVS_W ? b.N + 1 : b.N;
    }
  }
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  avg_release();
  g_avg = want;
  g_avg.n = 0;
  for (int q = 0; q < want.n; q++) {                   // zero-filled, as the reference's allocation leaves them
    AvgArray &a = g_avg.arr[q];
    int rc = guarded_alloc(&a.a, k_avg_line[a.id].name, -1, nij * a.nk);
    g_avg.n = q + 1;
    if (rc) { avg_release(); return rc; }
  }
  if (g_ctx.p.wet_dry)
    for (int q = 0; q < 4; q++) {
      int rc = guarded_alloc(&g_avg.cnt[q], k_avg_line[AVG_pmask_avg + q].name, -1, nij);
      if (rc) { avg_release(); return rc; }
    }
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  return 0;
}

// the array of (avg_id, itrc): an average or a counter; nullptr if it is not there
static const Guarded *avg_find(int id, int itrc)
{
  if (id < 0 || id >= AVG_COUNT) return nullptr;
  const AvgLine &L = k_avg_line[id];
  if (L.counter >= 0) return g_avg.cnt[L.counter].dev ? &g_avg.cnt[L.counter] : nullptr;
  const int want = avg_tkind(id) >= 0 ? itrc : 0;
  for (int q = 0; q < g_avg.n; q++)
    if (g_avg.arr[q].id == id && g_avg.arr[q].itrc == want) return &g_avg.arr[q].a;
  return nullptr;
}

extern "C" int roms_hip_get_average(int avg_id, int itrc, double *host, long n_doubles)
{
  const char *me = "roms_hip_get_average";
  if (!g_ctx.inited) return roms_fail(me, "library not initialised");
  if (avg_id < 0 || avg_id >= AVG_COUNT) return roms_fail(me, "averages: bad id");
  const Guarded *a = avg_find(avg_id, itrc);
  if (!a) {
    const std::string m = std::string("averages: ") + k_avg_line[avg_id].name + " is not selected (roms_hip_set_averages)";
    return roms_fail(me, m.c_str());
  }
  if (!host) return roms_fail(me, "averages: host array is NULL");
  return roms_copy_out(me, "averages", k_avg_line[avg_id].name, a->dev, a->count, host, n_doubles);
}

extern "C" double *roms_hip_average_device_ptr(int avg_id, int itrc)
{
  const Guarded *a = g_ctx.inited ? avg_find(avg_id, itrc) : nullptr;
  return a ? a->dev : nullptr;
}

extern "C" int roms_hip_set_avg(const roms_step_idx_t *s)
{
  const char *me = "roms_hip_set_avg";
  if (!g_ctx.inited) return roms_fail(me, "library not initialised");
  if (g_avg.nAVG == 0) return 0;                           // no roms_hip_set_averages, or nAVG = 0: set_avg.F:189
  int rc = roms_entry_check(me);
  if (rc) return rc;
  if (!s) return roms_fail(me, "null argument");
  const int phase = roms_hip_avg_phase(s->iic, g_avg.nAVG, g_avg.ntsAVG, g_avg.ntstart, g_avg.nrrec);
  if (!phase) return 0;
  if (s->kstp < 1 || s->kstp > 3 || s->nrhs < 1 || s->nrhs > 2) return roms_fail(me, "averages: kstp outside 1..3 or nrhs outside 1..2");
  const roms_bounds_t &b = g_ctx.b;
  const bool wet = g_ctx.p.wet_dry != 0;
  if (wet && !g_avg.cnt[0].dev)
    return roms_fail(me, "averages: wet_dry was switched on after roms_hip_set_averages; call it again");
  const long ni = b.UBi - b.LBi + 1, nj = b.UBj - b.LBj + 1, nij = ni * nj;
  if (nij != g_avg.nij) return roms_fail(me, "averages: the arrays have other extents than the bounds");
  ScopedTimer tm("set_avg");
  const bool set = (phase & AVP_SET) != 0, close = (phase & AVP_CLOSE) != 0;
  if (wet) {                                               // the counters first: the close divides by the new count
    rc = avg_counters(set ? 0 : 1);
    if (rc) return rc;
  }
  const int mode = set ? (close ? AVM_SET_CLOSE : AVM_SET) : (close ? AVM_ADD_CLOSE : AVM_ADD);
  // the second launch exists only for a selection whose descriptors outgrow the kernel-argument struct
  for (int f0 = 0; f0 < g_avg.n; f0 += AVG_MAXDESC) {
    AvgArgs a;
    a.n = std::min(g_avg.n - f0, AVG_MAXDESC);
    a.pm = g_ctx.field[FID_pm].dev; a.pn = g_ctx.field[FID_pn].dev;
    a.fac = 1.0 / (double)g_avg.nAVG;
    a.ni = ni; a.nij = nij; a.LBi = b.LBi; a.LBj = b.LBj;
    int nktot = 0;
    for (int f = 0; f < a.n; f++) {
      const AvgArray &A = g_avg.arr[f0 + f];
      const AvgLine &L = k_avg_line[A.id];
      AvgDesc &d = a.d[f];
      d.dst = A.a.dev;
      d.a = avg_source(L.srcA, s, A.itrc, L.plane);
      d.b = avg_source(L.srcB, s, A.itrc, L.plane);
      d.mask = wet ? g_ctx.field[L.mask].dev : nullptr;
      d.cnt = wet ? g_avg.cnt[L.mask == FID_rmask_full ? 1 : L.mask == FID_umask_full ? 2 : 3].dev : nullptr;
      d.expr = L.expr;
      d.koff = nktot;
      avg_range(L.range, &d.i0, &d.i1, &d.j0, &d.j1);
      nktot += A.nk;
    }
    // at most about 2048 workgroups: the rows beyond are strided
    const unsigned nbx = (unsigned)((ni + BLK_X - 1) / BLK_X), nby = (unsigned)((nj + BLK_Y - 1) / BLK_Y);
    const unsigned per_row = nbx * (unsigned)nktot;
    const unsigned gy = std::min(nby, std::max(1u, (2048u + per_row - 1) / per_row));
    const dim3 grid(nbx, gy, (unsigned)nktot);
    if (wet) avg_launch<true>(mode, grid, a);
    else avg_launch<false>(mode, grid, a);
    KERNEL_CHECK("k_avg");
  }
  // ghost points: where the reference fills them, i.e. with a periodic direction only (set_avg.F:2347-2358 and the
  // same after every field: exchange_*_tile, mp_exchange inside the same IF)
  if (close && (b.EWperiodic || b.NSperiodic) && g_avg.n) {
    halo_batch_begin();
    for (int q = 0; q < g_avg.n; q++) halo_exchange3d(k_avg_line[g_avg.arr[q].id].gtype, g_avg.arr[q].nk, g_avg.arr[q].a.dev);
    rc = halo_batch_end();
    if (rc) return rc;
  }
  // set_avg_masks (set_avg.F:92, set_masks.F:466-512): after the averages were scaled with the unclamped counts;
  // its mp_exchange2d is outside the periodic IF
  if (wet && (phase & AVP_MASKS)) {
    rc = avg_counters(2);
    if (rc) return rc;
    const int gt[4] = {GT_P, GT_R, GT_U, GT_V};
    halo_batch_begin();
    for (int q = 0; q < 4; q++) halo_exchange2d(gt[q], g_avg.cnt[q].dev);
    rc = halo_batch_end();
    if (rc) return rc;
  }
  return 0;
}
