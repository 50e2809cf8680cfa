// roms_dev.h -- internal header of libroms_hip.so (gfx950 / CDNA4 only).
//
// One process drives one GPU and one ROMS tile.  All module arrays of the tile
// live in HBM for the whole run (device mirrors of mod_ocean/mod_grid/
// mod_coupling/mod_mixing/mod_forces, same column-major i-fastest layout and
// the same LBi:UBi,LBj:UBj extents as the host arrays), so host and device
// index arithmetic is shared.  Kernels receive a pointer to one device-resident
// constant block (bounds + parameters + field pointers); wave-uniform reads of
// it compile to scalar loads.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include "roms_hip.h"

// The point-source table SOURCES(ng) (mod_sources.F:56-80) on the device, LuvSrc and LwSrc (roms_hip_set_sources).  The
// two face maps and the cell map (nij ints: 1 + the index of the source at the u- / v-face or the centre of the point,
// 0 elsewhere; the last source of a place wins, as the sequential loops of the reference leave it) let a kernel find
// "its" source without a search.
#define ROMS_NWS3 10   // 3-D scratch arrays (the _tile routines' automatic arrays; MPDATA holds Ta of three tracers at a time)

struct RomsSrc {
  int n;                      // Nsrc; 0 = no table
  int ltr[ROMS_MAXNT];        // LtracerSrc(itrc)
  const int *I, *J, *D;       // [n] Isrc, Jsrc, INT(Dsrc)
  const double *Qbar;         // [n]
  const double *Qsrc;         // [n * N]       is + n * (k-1)
  const double *Tsrc;         // [n * N * NT]  is + n * ((k-1) + N * (itrc-1))
  const int *umap, *vmap;     // [nij]  (LuvSrc; all zero without)
  const int *wmap;            // [nij]  LwSrc: 1 + the index of the last cell-centred source (Dsrc = 2) of the point
  // the interior cells (Istr:Iend, Jstr:Jend) with a source face or a cell-centred source, as indices into the 2-D
  // arrays: the software-pipelined tracer kernel leaves them to its SRC instantiation, which runs over this list
  const int *cells;
  int ncell;
  double *save;               // [n * N] the mass fluxes of the source faces across k_uv_column (k_step3d_uv.hip)
};

// The climatology CLIMA(ng) (mod_clima.F:190-261) with LnudgeM2CLM / LnudgeM3CLM / LnudgeTCLM (roms_hip_set_clima):
// device copies of the nudging coefficients and of the fields they relax towards, host extents (LBi:UBi, LBj:UBj
// [, N][, NTCLM]).  Every test of a flag is wave-uniform; with all flags zero no kernel reads a pointer.
struct RomsClima {
  int m2, m3, nt;             // LnudgeM2CLM, LnudgeM3CLM, NTCLM = number of nudged tracers
  int ic[ROMS_MAXNT];         // compact index ic (1-based) of tracer itrc, 0 = not nudged (step3d_t.F:1551-1560)
  int itrc[ROMS_MAXNT];       // tracer (1-based) of compact index ic
  double obcfac;              // obc_in = obcfac * obc_out on a RadNud edge (t3dbc_im.F:119-126)
  const double *M2nudgcof, *ubarclm, *vbarclm;   // [nij]
  const double *M3nudgcof, *uclm, *vclm;         // [nij * N]
  const double *Tnudgcof, *tclm;                 // [nij * N * nt]
};

// Tidal boundary forcing (set_tides.F, SSH_TIDES / UV_TIDES; roms_hip_set_tides, k_set_tides.hip).  The harmonic
// constants live on the device as STRIPS: per edge e (W, E, S, N) the two lines of rho-points the edge loads read --
// line 0 outside the edge (Istr-1, Iend+1, Jstr-1, Jend+1), line 1 the first one inside (Istr, Iend, Jstr, Jend) -- each
// over the whole allocated extent along the edge (LBj:UBj or LBi:UBi), so that consecutive threads read consecutive
// doubles on every edge.  Element (e, line, a) of a strip plane sits at off[e] + line * len[e] + (a - lb[e]); a
// constituent plane has `tot` doubles.  umask / vmask: one line per edge (the u- / v-points the edge vectors sit at),
// element (e, a) at off[e] / 2 + (a - lb[e]).
#define ROMS_MAXTC 32  // most tidal constituents (NTC) the constant block holds periods for
struct RomsTides {
  int ntc;                    // NTC; 0 = no tides
  int ssh, uv;                // SSH_TIDES, UV_TIDES
  int ssh_only;               // ssh && !uv: Flather / Shchepetkin take the reduced-physics bry_val (k_edge_bc)
  int ramp, add_fs, add_m2;   // RAMP_TIDES, ADD_FSOBC, ADD_M2OBC
  int lb[4], len[4];
  long off[4], tot;
  double tide_start, dstart;  // days
  double Tperiod[ROMS_MAXTC];
  const double *amp, *eph;                    // [ntc * tot] SSH_Tamp, SSH_Tphase
  const double *ang, *uph, *maj, *mnr;        // [ntc * tot] UV_Tangle, UV_Tphase, UV_Tmajor, UV_Tminor
  const double *angler;                       // [tot]
  const double *rmask;                        // [tot]; nullptr without MASKING
  const double *umask, *vmask;                // [tot / 2]
  const double *zeta_base, *ubar_base, *vbar_base;   // [nij] sub-tidal boundary data of the ADD options
};

// One device array between two guard bands (guarded_alloc, capi.hip): dev = the array the kernels see, base = the start
// of the allocation (the band in front of dev; nullptr = not allocated), count = its doubles.  name is a static string
// and q the index of an indexed scratch array (ws3[q], ws2[q]), -1 otherwise: what roms_hip_check_guards reports.
struct Guarded {
  double *dev = nullptr, *base = nullptr;
  long count = 0;
  const char *name = nullptr;
  int q = -1;
};

// AVERAGES (roms_hip_set_averages, roms_hip_set_avg; k_avg.hip): the columns of include/roms_avg.def.
enum { AVS_2D = 0, AVS_N, AVS_W, AVS_NT };
enum { RNG_RR = 0, RNG_UR, RNG_VR, RNG_II, RNG_UI, RNG_VI };
enum { X_COPY = 0, X_SQ, X_WPMPN, X_UV, X_UT, X_VT };
enum { AVP_SET = 1, AVP_ADD = 2, AVP_CLOSE = 4, AVP_MASKS = 8 };      // roms_hip_avg_phase

// DIAGNOSTICS_TS (roms_hip_set_diagnostics, k_set_diags.hip): DiaTwrk(LBi:UBi, LBj:UBj, N, NT, NDT) of mod_diags.F on
// the device, plane-major like the tracer itself (consecutive lanes along i store consecutive doubles of one term's
// plane), and the plane of every term of roms_dia.def: ix[id] = idiag - 1, or -1 where the term is not present.
// wrk == nullptr: diagnostics off, and no kernel reads this block.
struct RomsDia {
  double *wrk;
  int ndt;
  int ix[DIA_COUNT];
};
// DiaTwrk(:,:,:,itrc,idiag) of term `id` (device code; n3r = points of a rho-array)
#define DIA_PLANE(c, id, itrc, n3r) ((gd_t)((c)->dia.wrk + ((long)(c)->dia.ix[id] * (c)->b.NT + ((itrc) - 1)) * (n3r)))

// LMD_BKPP (roms_hip_set_kpp, k_lmd.hip): the switch and the library-owned arrays of mod_mixing.F the bottom
// boundary layer adds -- hbbl (double), kbbl and ksbl (int), all (LBi:UBi, LBj:UBj).  bkpp = 0: off, and no kernel reads
// this block.
struct RomsKpp {
  int bkpp;
  double *hbbl;
  int *kbbl, *ksbl;
};

// BIOLOGY (roms_hip_set_biology, k_biology.hip): the model and its parameters.  model = ROMS_BIO_NONE: off, and no
// kernel reads this block.
struct RomsBio {
  int model;
  roms_bio_powell_t powell;
};

// LMD_DDMIX (roms_hip_set_ddmix, k_lmd.hip): alfaobeta (LBi:UBi, LBj:UBj, 0:N) of mod_mixing.F, library-owned, written
// by rho_eos on IstrT:IendT, JstrT:JendT and read by lmd_vmix at interior points.  nullptr: off, and no kernel reads this
// block.  Last in RomsDev: the members before it keep their offsets.
struct RomsDdmix {
  double *alfaobeta;
};

struct RomsDev {
  roms_bounds_t b;
  roms_params_t p;
  roms_fields_t F;      // device pointers
  // device scratch = the _tile routines' automatic work arrays
  double *ws3[ROMS_NWS3];   // 3-D scratch, each nij*(N+1) doubles
  double *ws2[32];      // 2-D scratch, each nij doubles
  const double *rowm;   // row table of the i-uniform metric arrays (k_step2d_mom.hip), or nullptr
  RomsSrc src;          // point sources (LuvSrc), n = 0 without
  RomsClima clima;      // climatology nudging, all flags zero without
  RomsTides tides;      // tidal boundary forcing, ntc = 0 without
  RomsDia dia;          // tracer diagnostics, wrk = nullptr without
  RomsKpp kpp;          // KPP bottom boundary layer, bkpp = 0 without
  RomsBio bio;          // biology, model = ROMS_BIO_NONE without
  RomsDdmix ddmix;      // KPP double-diffusive mixing, alfaobeta = nullptr without
};

struct RomsCtx {
  bool inited = false;
  int rank = 0, ntileI = 1, ntileJ = 1, device = 0;
  hipStream_t stream = nullptr;
  roms_bounds_t b{};
  roms_params_t p{};
  bool have_bounds = false, have_params = false;
  double *host[FID_COUNT] = {nullptr};
  Guarded field[FID_COUNT];     // the device mirrors
  Guarded ws3[ROMS_NWS3], ws2[32];   // the scratch arrays behind hostc.ws3 / hostc.ws2
  long guard = 0;               // doubles of guard band on either side of every mirror / scratch array
  RomsDev hostc{};            // host copy of the constant block
  RomsDev *devc = nullptr;    // device copy
  bool devc_dirty = true;
  bool timing = false;
  std::string last_error;
  // halo exchange (RCCL) state lives in halo.hip
  void *nccl_comm = nullptr;
  unsigned char nccl_id[128];
  bool have_nccl_id = false;
  // ONE tile with an RCCL id: the periodic wrap of that tile travels through the transport to the tile
  // itself (W and E neighbour = own rank) instead of the local copy kernel, and every kernel takes its
  // multi-tile branch.  Same results; lets a one-GPU box execute the RCCL leg (tests/test_gpu_rccl.py).
  bool loopback = false;
  // row-uniform metrics (k_step2d_mom.hip): 0 = not examined since the last upload of a metric array,
  // 1 = all fifteen arrays are independent of i (table valid), 2 = not
  int rowm_state = 0;
  bool rowh = false;             // ... and h, visc2_r, visc2_p as well (second group of the table)
  double *rowm_dev = nullptr;
  long rowm_nj = 0;
};

extern RomsCtx g_ctx;

int  roms_fail(const char *where, const char *what);
int  roms_setup_check(const char *me);    // every roms_hip_set_* entry: init, set_bounds and set_params came first
// every roms_hip_get_* entry: `count` elements of `elem` bytes from the device to the host, refused where the host
// array has another size ("FAMILY: NAME has COUNT UNIT, the host array HOST_COUNT")
int  roms_copy_out(const char *me, const char *family, const char *name, const void *dev, long count, void *host,
                   long host_count, size_t elem = sizeof(double), const char *unit = "doubles");
int  roms_flush_consts();                 // upload hostc -> devc when dirty
int  roms_entry_check(const char *where); // every kernel entry calls this first
extern const char *const k_field_name[FID_COUNT];
long roms_field_count(int kind, const roms_bounds_t &b);

#define HIP_TRY(expr)                                                         \
  do {                                                                        \
    hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess) return roms_fail(#expr, hipGetErrorString(e_));     \
  } while (0)

#define KERNEL_CHECK(name)                                                    \
  do {                                                                        \
    hipError_t e_ = hipGetLastError();                                        \
    if (e_ != hipSuccess) return roms_fail(name, hipGetErrorString(e_));      \
  } while (0)

// ------------------------------------------------------------------------
// timing (hipEvents on the library stream) for bench.py's roofline object
// ------------------------------------------------------------------------
struct ScopedTimer {
  const char *name;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  explicit ScopedTimer(const char *n);
  ~ScopedTimer();
};

// ------------------------------------------------------------------------
// device-side index helpers
// ------------------------------------------------------------------------
// XCD-aware renumbering of a 2-D / 3-D grid, inside the kernel (the launch is unchanged): hardware
// deals workgroups to the 8 XCDs round-robin in linear order, so linear id L runs on XCD L % 8.  When
// the grid has a multiple of 8 tile columns each XCD is given a contiguous strip of columns, walked
// row by row with the z-index (component / level) fastest -- x-neighbours then share their boundary
// cache lines in one L2 and z-neighbours share the fields both read (see decode_tile_tracer).  A
// bijection on the same grid; placement only affects speed.
struct Blk { int x, y, z; };
#ifdef __HIPCC__
__device__ __forceinline__ Blk xcd_block()
{
  Blk r{(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
  const int nbx = gridDim.x, nby = gridDim.y, nz = gridDim.z;
  if ((nbx & 7) == 0) {
    const int L = r.x + nbx * (r.y + nby * r.z);
    const int xcd = L & 7, q = L >> 3, w = nbx >> 3;
    r.z = q % nz;
    const int t = q / nz;
    r.x = xcd * w + t % w;
    r.y = t / w;
  }
  return r;
}
#endif

#define DEV_PROLOGUE(c)                                                        \
  const roms_bounds_t &b = (c)->b;                                             \
  const int LBi = b.LBi, LBj = b.LBj;                                          \
  const int N = b.N;                                                           \
  const long ni = b.UBi - b.LBi + 1, nj = b.UBj - b.LBj + 1, nij = ni * nj;    \
  const long n3r = nij * N, n3w = nij * (N + 1);                               \
  (void)nj; (void)n3r; (void)n3w;

// Field pointers are read from the constant block, so the compiler only knows them as
// generic (flat) addresses.  Casting to the global address space turns flat_load/store
// into global_load/store: no LDS/scratch aperture check, and the loads stop counting
// against lgkmcnt, so LDS traffic and scalar loads no longer wait on them.
typedef const double __attribute__((address_space(1))) *gcd_t;
typedef double __attribute__((address_space(1))) *gd_t;
// field `name` of the constant block as a global-address-space pointer (device code with `c` in scope)
#define GF(name) ((gd_t)c->F.name)

// The predictor's start of u or v(nnew) at one point (pre_step3d.F:1040-1110; k_pre_uv, and k_prsgrd32<true> inside
// roms_hip_rhs3d).  stage: 0 = first step (forward Euler), 1 = second step (AB2), 2 = AB3.  vk: u or v(nstp); hzs: the sum
// of Hz over the face's two cells; r1, r2: ru or rv at nrhs and 3 - nrhs, read at q where the stage uses them;
// d: FC(k) - FC(k-1) of the explicit vertical viscous flux.
__device__ __forceinline__ double uv_start(int stage, double vk, double hzs, double DC0, gcd_t r1, gcd_t r2, long q, double d)
{
  double out;
  if (stage == 0) {
    const double a = vk * 0.5 * hzs;
    out = a + d;
  } else if (stage == 1) {
    const double a = vk * 0.5 * hzs;
    const double c3 = 0.5 * DC0;
    out = a - c3 * r2[q] + d;
  } else {
    const double a = vk * 0.5 * hzs;
    out = a + DC0 * ((5.0 / 12.0) * r1[q] - (16.0 / 12.0) * r2[q]) + d;
  }
  return out;
}

// WET_DRY: the land/sea mask of a point times its wet/dry mask.  Wherever the reference multiplies by the wet/dry mask
// directly after the land/sea mask (x = x*umask; x = x*umask_wet -- every WET_DRY block of the mixing, bulk-flux,
// MPDATA, step3d_uv and ini_fields files) the two small-integer factors combine exactly, signed zeros included:
// x*(m*w) == (x*m)*w bit for bit for m in {0,1}, w in {-1,0,1,2}.  Callers hold `c`; without WET_DRY this is the
// land/sea mask alone.
#define ROMS_MASKW(name)                                                                                  \
  __device__ __forceinline__ double name##w(const RomsDev *__restrict__ c, long q)                       \
  {                                                                                                       \
    double m = ((gcd_t)c->F.name)[q];                                                                     \
    if (c->p.wet_dry) m = m * ((gcd_t)c->F.name##_wet)[q];                                                \
    return m;                                                                                             \
  }
ROMS_MASKW(rmask)
ROMS_MASKW(umask)
ROMS_MASKW(vmask)
ROMS_MASKW(pmask)
#undef ROMS_MASKW
// the factor of the barotropic wet/dry rule (step2d_LF_AM3.h:2124-2126, u2dbc_im.F:1183-1187): 1 on a face between
// two wet cells (mask 2), 0 between two dry ones, and on a one-sided face (+-1) 1 only for flow out of the wet cell
__device__ __forceinline__ double wet_factor(double mask_wet, double vel)
{
  const double cff5 = fabs(fabs(mask_wet) - 1.0);
  const double cff6 = 0.5 + copysign(0.5, vel) * mask_wet;
  return 0.5 * mask_wet * cff5 + cff6 * (1.0 - cff5);
}

// LuvSrc: the horizontal advective tracer fluxes of the four faces of cell c0 at level k (ck = its 3-D index), replaced
// at source faces.  PRE = false: step3d_t.F:734-799 (Huon * Tsrc; without LtracerSrc and under MASKING the upstream value
// of the wet side, T = t(:,:,:,3,itrc)); PRE = true: pre_step3d.F:530-553 (Huon * Tsrc, or zero without LtracerSrc).
// The caller tests c->src.n (uniform) and src_cell_any() first: the body is the rare path.
__device__ __forceinline__ bool src_cell_any(const RomsDev *__restrict__ c, long c0, long ni)
{
  return (c->src.umap[c0] | c->src.umap[c0 + 1] | c->src.vmap[c0] | c->src.vmap[c0 + ni] | c->src.wmap[c0]) != 0;
}
// LwSrc, step3d_t.F:1136-1158 / :1331-1360: the tracer that comes with the volume of the cell-centred sources of point
// c0 at level k, added to tv (Ta before its vertical advection for MPDATA, t(nnew) after it otherwise); cff =
// dt * pm * pn (times oHz outside MPDATA), t3k = t(i,j,k,3,itrc), the value the inflow carries without LtracerSrc.
// Every source of the cell counts, in the order of the table (the sums of the reference's loop).
__device__ __forceinline__ double src_w_tracer(const RomsDev *__restrict__ c, long c0, int k, int itrc, double cff,
                                               double t3k, double tv)
{
  const RomsSrc &S = c->src;
  if (S.wmap[c0] == 0) return tv;
  const long ni = c->b.UBi - c->b.LBi + 1;
  for (int is = 0; is < S.n; is++) {
    if (S.D[is] != 2 || (long)(S.I[is] - c->b.LBi) + (long)(S.J[is] - c->b.LBj) * ni != c0) continue;
    const double cff3 = S.ltr[itrc - 1] ? S.Tsrc[is + (long)S.n * ((k - 1) + (long)c->b.N * (itrc - 1))] : t3k;
    tv = tv + cff * S.Qsrc[is + (long)S.n * (k - 1)] * cff3;
  }
  return tv;
}
template <bool PRE>
__device__ __forceinline__ void src_cell_fluxes(const RomsDev *__restrict__ c, long c0, long ck, long ni, int k, int itrc,
                                                const double *__restrict__ T, double &FXi, double &FXip1, double &FEj,
                                                double &FEjp1)
{
  const RomsSrc &S = c->src;
  const bool ltr = S.ltr[itrc - 1] != 0;
  const int N = c->b.N;
  auto face = [&](int m, long cf, long ckf, long off, const double *__restrict__ H, double &Fv) {
    if (!m) return;
    const int is = m - 1;
    if (ltr) Fv = H[ckf] * S.Tsrc[is + (long)S.n * ((k - 1) + (long)N * (itrc - 1))];
    else if (PRE) Fv = 0.0;
    else if (c->p.masking) {
      const double r1 = c->F.rmask[cf], r0 = c->F.rmask[cf - off];
      if (r1 == 0.0 && r0 == 1.0) Fv = H[ckf] * T[ckf - off];
      else if (r1 == 1.0 && r0 == 0.0) Fv = H[ckf] * T[ckf];
    }
  };
  face(S.umap[c0], c0, ck, 1, c->F.Huon, FXi);
  face(S.umap[c0 + 1], c0 + 1, ck + 1, 1, c->F.Huon, FXip1);
  face(S.vmap[c0], c0, ck, ni, c->F.Hvom, FEj);
  face(S.vmap[c0 + ni], c0 + ni, ck + ni, ni, c->F.Hvom, FEjp1);
}

#define I2(i,j)    ((long)((i) - LBi) + (long)((j) - LBj) * ni)
#define I3(i,j,k)  (I2(i,j) + (long)((k) - 1) * nij)
#define I3W(i,j,k) (I2(i,j) + (long)(k) * nij)

// grid-point type codes for the periodic exchange (exchange_2d.F / _3d.F)
enum { GT_R = 0, GT_U, GT_V, GT_P };

// thread (tx,ty) -> horizontal index; blocks are 64 x 4 so that one wavefront
// covers 64 consecutive i (one 512-byte line per k-level access).
#define BLK_X 64
#define BLK_Y 4
static inline dim3 grid2d(int nx, int ny) {
  return dim3((unsigned)((nx + BLK_X - 1) / BLK_X), (unsigned)((ny + BLK_Y - 1) / BLK_Y), 1);
}
static inline dim3 block2d() { return dim3(BLK_X, BLK_Y, 1); }
// LDS tile of a workgroup's points with their 2-point C-grid halo (k_rhs3d.hip, k_step2d_mom.hip), and the second
// differences of the 3rd / 4th-order advection at tile element a
#define TP (BLK_X + 4)       // tile pitch (i)
#define TJ (BLK_Y + 4)       // tile rows  (j)
__device__ __forceinline__ double d2x(const double *f, int a) { return f[a - 1] - 2.0 * f[a] + f[a + 1]; }
__device__ __forceinline__ double d2y(const double *f, int a) { return f[a - TP] - 2.0 * f[a] + f[a + TP]; }
// (tile, level) decode of a 1-D grid for kernels with one thread per cell: consecutive workgroups of an XCD take the
// SAME horizontal tile at consecutive levels, so the planes k-1, k, k+1 a vertical stencil reads meet in one L2
// (with the level in gridDim.z they are thousands of workgroups apart and on other XCDs); tiles are dealt to the
// XCDs round-robin, which balances any tile count.  Launch with grid_tile_level(); check .valid.
struct TileLv { int bx, by, k0; bool valid; };
#ifdef __HIPCC__
__device__ __forceinline__ TileLv decode_tile_level(int nx, int ny, int nz)
{
  const int nbx = (nx + BLK_X - 1) / BLK_X, nby = (ny + BLK_Y - 1) / BLK_Y;
  const int B = blockIdx.x, xcd = B & 7, q = B >> 3;
  TileLv r;
  r.k0 = q % nz;
  const int tl = (q / nz) * 8 + xcd;
  r.valid = tl < nbx * nby;
  r.bx = tl % nbx;
  r.by = tl / nbx;
  return r;
}
#endif
static inline dim3 grid_tile_level(int nx, int ny, int nz) {
  const int nbx = (nx + BLK_X - 1) / BLK_X, nby = (ny + BLK_Y - 1) / BLK_Y;
  return dim3((unsigned)(((nbx * nby + 7) / 8) * 8 * nz), 1, 1);
}

// XCD-aware (tile, tracer) decode of a 1-D grid.  Workgroups B and B+8 run on the same
// XCD (round-robin dispatch over the 8 XCDs, MI355X_MICROARCH.md); each XCD has its own
// 4 MB L2.  Two things are arranged through the order in which one XCD meets its tiles:
//  * consecutive workgroups of an XCD take the SAME horizontal tile for consecutive
//    tracers, so the tracer-independent fields (Huon, Hvom, W, Hz, z_r ...) one of them
//    streams are L2 hits for the other (measured on step3d_t: 2.9 -> 2.1 GB fetched);
//  * each XCD owns a contiguous strip of tile columns [x0,x1) and walks it row by row.
//    A 64-double row segment is not 128-B aligned (the reference's row pitch is odd), so
//    it shares its first and last cache line with the x-neighbours; inside a strip those
//    lines are fetched once per XCD instead of once per tile.
// With fewer than 8 tile columns the strips degenerate and tiles are dealt round-robin.
// Placement only affects speed, never results.
struct TileTr { int bx, by, itr; bool valid; };
#ifdef __HIPCC__
__device__ __forceinline__ TileTr decode_tile_tracer(int nx, int ny, int ntr, int ty = BLK_Y)
{
  const int nbx = (nx + BLK_X - 1) / BLK_X, nby = (ny + ty - 1) / ty;
  const int B = blockIdx.x, xcd = B & 7, q = B >> 3;
  TileTr r;
  r.itr = q % ntr;
  const int t = q / ntr;
  if (nbx < 8) {
    const int tl = t * 8 + xcd;
    r.valid = tl < nbx * nby;
    r.bx = tl % nbx;
    r.by = tl / nbx;
  } else {
    const int x0 = (xcd * nbx) >> 3, w = (((xcd + 1) * nbx) >> 3) - x0;
    r.bx = x0 + t % w;
    r.by = t / w;
    r.valid = r.by < nby;
  }
  return r;
}
#endif
static inline dim3 grid_tile_tracer(int nx, int ny, int ntr, int ty = BLK_Y) {
  const int nbx = (nx + BLK_X - 1) / BLK_X, nby = (ny + ty - 1) / ty;
  if (nbx < 8) return dim3((unsigned)(((nbx * nby + 7) / 8) * 8 * ntr), 1, 1);
  return dim3((unsigned)(8 * ((nbx + 7) / 8) * nby * ntr), 1, 1);
}

// ------------------------------------------------------------------------
// internal launchers shared between translation units
// ------------------------------------------------------------------------
int halo_exchange2d(int gtype, double *A, int nfields_stride_unused = 0);
int halo_exchange3d(int gtype, int nk, double *A);
void halo_batch_begin();                  // record the exchanges that follow ...
int halo_batch_end();                     // ... and run them as one message per neighbour and phase
int halo_allreduce_sum(double *A, long n); // mp_collect: SUM over all tiles of a device array, in place (halo.hip)
// capi.hip: n zeroed doubles between two guard bands, entered into the table roms_hip_check_guards walks, and out of it
int guarded_alloc(Guarded *a, const char *name, int q, long n);
void guarded_free(Guarded *a);
// the option stores (k_option_store, capi.hip): what roms_hip_finalize and roms_hip_set_bounds release, in this order
void sources_release();                   // sources.hip: frees what roms_hip_set_sources allocated
bool roms_sources_given();                // ... a table (Nsrc = 0 included) was handed over
void clima_release();                     // clima.hip: frees what roms_hip_set_clima allocated
void avg_release();                       // k_avg.hip: frees what roms_hip_set_averages allocated
void floats_release();                    // k_floats.hip: frees what roms_hip_set_floats allocated
void tides_release();                     // k_set_tides.hip: frees what roms_hip_set_tides allocated
void data_release();                      // k_set_data.hip: drops every record of roms_hip_set_data_record / _point
void dia_release();                       // k_set_diags.hip: frees what roms_hip_set_diagnostics allocated
bool dia_on();                            // ... diagnostics are switched on (the DIA instantiations run)
int dia_check(const char *where);         // ... and what they are not built with, refused by name (0 when off)
int dia_rate(int nnew);                   // ... step3d_t.F:1598-1611 on IstrR:IendR, JstrR:JendR (k_dia_rate)
void kpp_release();                       // k_lmd.hip: frees what roms_hip_set_kpp allocated
void bio_release();                       // k_biology.hip: drops the setting of roms_hip_set_biology
void ddmix_release();                     // k_lmd.hip: frees what roms_hip_set_ddmix allocated
// lateral boundary conditions on the S/N edges (k_base.hip); s = the barotropic time indices (Chapman, Flather),
// nstp = the time level the radiation condition compares with
int bc_zeta(int kout, const roms_step_idx_t *s);
int bc_u2d(int kout, const roms_step_idx_t *s);
int bc_v2d(int kout, const roms_step_idx_t *s);
int bc_u3d(int nout, int nstp);
int bc_v3d(int nout, int nstp);
int bc_t3d(int nout, int itrc, int nstp);   // the compact climatology index ic of itrc comes from the RomsClima block
bool lbc2d_all_closed();
int lbc_code(const roms_params_t &p, int sd, int v);   // effective enum roms_lbc of variable v on side sd
int bc_w3d(double *A);
int bc_generic(int gtype_var, int lbv, double *A, int nk);   // bc_2d.F / bc_3d.F rules for derived fields
void snapshot_release();                  // snapshot.hip: waits for and frees an in-flight snapshot
void snapshot_forget(int field_id);       // snapshot.hip: the same for one field (before it is re-registered)
void diag_release();                      // k_diag.hip: frees the buffers of roms_hip_diag
int check_lbc();
// roms_hip_pre_step3d / roms_hip_t3dmix2 as roms_hip_rhs3d runs them.  fused (k_rhs3d.hip: rhs3d_fuses_tstart()): the
// predictor leaves t(nnew) alone and the rotated mixing kernel stores Hz*t(nstp) + the explicit vertical flux
// divergence + its own term in one write; the two extern "C" entries pass false.
// uvstart (k_rhs3d.hip: rhs3d_fuses_uvstart()): the predictor leaves u, v(nnew) to the pressure-gradient kernel, which
// forms them at the point whose ru, rv(nrhs) it is about to overwrite.
int pre_step3d_entry(const roms_step_idx_t *s, bool fused, bool uvstart);   // k_pre_step3d.hip
int prsgrd_entry(const roms_step_idx_t *s, bool uvstart);     // k_prsgrd.hip
int t3dmix2_entry(const roms_step_idx_t *s, bool fused);      // k_mix.hip
int roms_rowm_prepare();               // k_step2d_mom.hip: examine the metric arrays if needed (synchronises once)
void roms_rowm_invalidate();            // a metric array may have changed
bool roms_rowm_is_table_field(int id);  // is field `id` one of the arrays the row table is built from?
void roms_rowm_release();
void step2d_graphs_release();           // k_step2d.hip: drop the captured LOOP_2D graphs (their launch arguments are stale)
