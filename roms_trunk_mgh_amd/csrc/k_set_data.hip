// k_set_data.hip -- time interpolation of the forcing, climatology and open-boundary snapshots: the calls of
// set_2dfld_tile (ROMS/Utility/set_2dfld.F:21), set_3dfld_tile (set_3dfld.F:21) and set_ngfld (set_ngfld.F:21) that
// set_data_tile (ROMS/Nonlinear/set_data.F:78-1390) makes for the targets of include/roms_data.def.  Not built: see the
// table's header.
//
// roms_hip_set_data_record / _point keep the two time records of a target on the device (a gridded record with the
// tile's extents, an edge record as an edge-major strip [along the edge][level]); roms_hip_set_data evaluates the
// interpolation weights on the host, term for term as set_2dfld.F:90-120 does (roms_hip_set_data_factors), and writes
// every target in ONE launch: a descriptor per target {rows of Finp(it1), Finp(it2), rows of Fout, their pitches, fac1,
// fac2, mode}, a prefix table from workgroups to descriptors, one workgroup per SD_SEG doubles of one row.  A row is a run
// of i at fixed (j, k) of a gridded target (IstrR:IendR only: what lies outside is not the routine's to write), the run
// along a southern / northern edge at one level, or -- element stride of one row of the field -- the run along a
// western / eastern edge.  Where the two source rows and the destination row share their 16-byte phase a lane moves two
// doubles per access (the phase differs from row to row with an odd row pitch, and between a plane of a field with a
// tracer dimension and its record: it is tested per row, a leading odd element and the tail go one by one); otherwise,
// and on strided rows, one double.  No LDS.  Fout = fac1*Finp(it1) + fac2*Finp(it2), the products and the sum in that order.
// Pure streaming: two loads and one store per point.
//
// The WET_DRY clip of the free-surface boundary data (set_data.F:928-1003) is carried by the edge rows of zeta_bry.
#include "roms_dev.h"
#include <cmath>
#include <cstdint>
#include <vector>

namespace {
enum { R_set_2dfld = 0, R_set_3dfld, R_set_ngfld };
enum { G_r = GT_R, G_u = GT_U, G_v = GT_V };
#define DATA_FID_DD_FIELD(name) FID_##name
#define DATA_FID_DD_BRY(name) FID_##name
#define DATA_FID_DD_CLIMA(name) (-1)
struct DataLine { const char *name; int routine, gtype, shape, dest, fid; };
const DataLine k_data_line[DATA_COUNT] = {
#define ROMS_DATA(name, routine, grid, shape, dest) {#name, R_##routine, G_##grid, shape, dest, DATA_FID_##dest(name)},
#include "roms_data.def"
#undef ROMS_DATA
};

// the records of one (target, index, side)
struct DataRec {
  int target = 0, index = 0, side = 0;
  double *slot[2] = {nullptr, nullptr};     // device: Finp(.., 1), Finp(.., 2)
  bool filled[2] = {false, false};
  double Tintrp[2] = {0.0, 0.0}, fpoint[2] = {0.0, 0.0};
  int tindex = 0, onerec = 0;               // Iinfo(8), Linfo(3) of the latest call
  bool point = false;                       // Linfo(1) = .FALSE.
  long n = 0;
};
std::vector<DataRec> g_recs;                // in the order (target, index, side)

enum { SDM_INTERP = 0, SDM_COPY, SDM_POINT };
struct DataDesc {
  const double *s1, *s2;      // row 0 of Finp(it1), Finp(it2); COPY reads s2 only, POINT none
  double *dst;                // row 0 of Fout
  const double *hclip;        // h at the points of row 0 (WET_DRY clip of zeta_bry), or nullptr
  double fac1, fac2;          // POINT: fac1 = Fval
  double dcrit;
  long spitch, splane;        // source: doubles from row to row of a plane, from plane to plane
  long dpitch, dplane, dstep; // destination: the same, and from element to element of a row
  int L, rpp, rows;           // elements of a row, rows of a plane, rows in all
  int segs;                   // workgroups per row
  int mode;
  int clip0, clip1;           // elements of a row the clip covers
};
// the descriptor table and the prefix table on the device; a pinned host image, reused once its copy has run
void *g_tab = nullptr, *g_tab_host = nullptr;
size_t g_tab_bytes = 0;
hipEvent_t g_tab_event = nullptr;

void tab_release()
{
  if (g_tab) (void)hipFree(g_tab);
  if (g_tab_host) (void)hipHostFree(g_tab_host);
  if (g_tab_event) (void)hipEventDestroy(g_tab_event);
  g_tab = g_tab_host = nullptr;
  g_tab_event = nullptr;
  g_tab_bytes = 0;
}
}  // namespace

// (roms_hip_set_bounds: the records of set_data have the old extents)
void data_release()
{
  for (DataRec &r : g_recs)
    for (int q = 0; q < 2; q++)
      if (r.slot[q]) (void)hipFree(r.slot[q]);
  g_recs.clear();
  tab_release();
}

// ------------------------------------------------------------------------------------------------- kernel --
#define SD_PAIRS 2                       // 16-byte accesses per lane
#define SD_SEG (256 * 2 * SD_PAIRS)      // doubles of a row per workgroup
typedef double v2d __attribute__((ext_vector_type(2)));
typedef const v2d __attribute__((address_space(1))) *gcv2_t;
typedef v2d __attribute__((address_space(1))) *gv2_t;

__global__ void __launch_bounds__(256) k_set_data(const DataDesc *__restrict__ D, const int *__restrict__ first, int nd)
{
  // first[d] <= blockIdx.x < first[d + 1]; wave-uniform
  int lo = 0, hi = nd;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  const DataDesc &T = D[lo];
  const int unit = (int)blockIdx.x - first[lo];
  const int row = unit / T.segs, seg = unit - row * T.segs;
  if (row >= T.rows) return;
  const int plane = row / T.rpp, r = row - plane * T.rpp;
  const long so = (long)plane * T.splane + (long)r * T.spitch, dof = (long)plane * T.dplane + (long)r * T.dpitch;
  const int mode = T.mode, L = T.L;
  const long dstep = T.dstep;
  const double fac1 = T.fac1, fac2 = T.fac2;
  gcd_t s1 = (gcd_t)(mode == SDM_INTERP ? T.s1 + so : nullptr);
  gcd_t s2 = (gcd_t)(mode != SDM_POINT ? T.s2 + so : nullptr);
  gd_t dst = (gd_t)(T.dst + dof);
  gcd_t hc = (gcd_t)(T.hclip ? T.hclip + dof : nullptr);
  const int clip0 = T.clip0, clip1 = T.clip1;
  const double dcrit = T.dcrit;
  auto one = [&](int e) {
    double x;
    if (mode == SDM_POINT) x = fac1;                                   // set_2dfld.F:127-133
    else if (mode == SDM_COPY) x = s2[e];                              // :98-104
    else x = fac1 * s1[e] + fac2 * s2[e];                              // :124
    if (hc && e >= clip0 && e <= clip1) {                              // set_data.F:935-940
      const double cff = dcrit - hc[(long)e * dstep];
      if (x <= cff) x = cff;
    }
    dst[(long)e * dstep] = x;
  };
  // 16-byte accesses where the rows in use share their phase; then `mis` = the odd element in front of the first pair
  const uintptr_t pd = (uintptr_t)(T.dst + dof) >> 3, p1 = s1 ? (uintptr_t)(T.s1 + so) >> 3 : pd,
                  p2 = s2 ? (uintptr_t)(T.s2 + so) >> 3 : pd;
  const bool vec = dstep == 1 && !hc && ((pd ^ p1) & 1) == 0 && ((pd ^ p2) & 1) == 0;
  const int mis = vec ? (int)(pd & 1) : 0;
  if (mis && seg == 0 && threadIdx.x == 0) one(0);
#pragma unroll
  for (int u = 0; u < SD_PAIRS; u++) {
    const int e = mis + seg * SD_SEG + 2 * (u * 256 + (int)threadIdx.x);
    if (vec && e + 1 < L) {
      v2d x;
      if (mode == SDM_POINT) { x.x = fac1; x.y = fac1; }
      else if (mode == SDM_COPY) x = *(gcv2_t)(s2 + e);
      else {
        const v2d a = *(gcv2_t)(s1 + e), c = *(gcv2_t)(s2 + e);
        x = fac1 * a + fac2 * c;
      }
      *(gv2_t)(dst + e) = x;
    } else {
      if (e < L) one(e);
      if (e + 1 < L) one(e + 1);
    }
  }
}

// -------------------------------------------------------------------------------------------- the weights --
// set_2dfld.F:90-94, :116-120, :139-141 (the same statements stand in set_3dfld.F:94-98 and set_ngfld.F:79-83), term for
// term in double.  ANINT rounds half away from zero: round(), not rint().
extern "C" int roms_hip_set_data_factors(double time, double dt, double T1, double T2, int Tindex, int onerec,
                                         double *fac1_out, double *fac2_out, int *synchro)
{
  const char *me = "roms_hip_set_data_factors";
  if (Tindex < 1 || Tindex > 2) return roms_fail(me, "set_data: Tindex outside 1..2");
  if (!fac1_out || !fac2_out) return roms_fail(me, "set_data: null argument");
  const double Tintrp[2] = {T1, T2};
  const double SecScale = 1000.0;
  const int it1 = 3 - Tindex, it2 = Tindex;
  double fac1 = round((Tintrp[it2 - 1] - time) * SecScale);
  double fac2 = round((time - Tintrp[it1 - 1]) * SecScale);
  if (onerec) {                                                        // :98: no interpolation, no test
    *fac1_out = 0.0;
    *fac2_out = 1.0;
    return 0;
  }
  if (fac1 * fac2 >= 0.0 && fac1 + fac2 > 0.0) {                       // :116-117
    const double fac = 1.0 / (fac1 + fac2);
    fac1 = fac * fac1;
    fac2 = fac * fac2;
    *fac1_out = fac1;
    *fac2_out = fac2;
    if (synchro && time + dt > Tintrp[it2 - 1]) *synchro = 1;          // :139-141
    return 0;
  }
  char msg[240];
  snprintf(msg, sizeof msg, "set_data: current model time exceeds ending value: time = %.6f s, TINTRP1 = %.6f s, TINTRP2 = %.6f s",
           time, Tintrp[it1 - 1], Tintrp[it2 - 1]);
  return roms_fail(me, msg);
}

// --------------------------------------------------------------------------------------------- the records --
namespace {
const char *const k_side_name[4] = {"west", "east", "south", "north"};

bool is_edge_shape(int shape) { return shape == DS_E || shape == DS_EN || shape == DS_ENT; }

// the library's climatology copy a DD_CLIMA target is written to (nullptr: roms_hip_set_clima has not made it)
double *clima_copy(int target, int index)
{
  const RomsClima &C = g_ctx.hostc.clima;
  const roms_bounds_t &b = g_ctx.b;
  const long nij = (long)(b.UBi - b.LBi + 1) * (long)(b.UBj - b.LBj + 1);
  switch (target) {
  case DATA_ubarclm: return C.m2 ? const_cast<double *>(C.ubarclm) : nullptr;
  case DATA_vbarclm: return C.m2 ? const_cast<double *>(C.vbarclm) : nullptr;
  case DATA_uclm: return C.m3 ? const_cast<double *>(C.uclm) : nullptr;
  case DATA_vclm: return C.m3 ? const_cast<double *>(C.vclm) : nullptr;
  case DATA_tclm: return C.tclm && index >= 1 && index <= C.nt ? const_cast<double *>(C.tclm) + (long)(index - 1) * nij * b.N : nullptr;
  }
  return nullptr;
}

// Everything a call says about its target, checked before anything is touched.  *n = the doubles of a record, *skip = an
// edge target on a side that is not a physical edge of this tile.
int data_validate(const char *me, int target, int index, int side, int slot, bool point, long *n, bool *skip)
{
  if (int rc = roms_setup_check(me)) return rc;
  if (target < 0 || target >= DATA_COUNT) return roms_fail(me, "set_data: unknown target (enum roms_data_id)");
  const DataLine &T = k_data_line[target];
  const roms_bounds_t &b = g_ctx.b;
  const long ni = b.UBi - b.LBi + 1, nj = b.UBj - b.LBj + 1, nij = ni * nj;
  auto fail = [&](const std::string &what) { return roms_fail(me, (std::string("set_data: ") + T.name + ": " + what).c_str()); };
  *skip = false;
  if ((T.shape == DS_2DT || T.shape == DS_ENT) && (index < 1 || index > b.NT))
    return fail("unknown index: tracer " + std::to_string(index) + " outside 1.." + std::to_string(b.NT));
  if (T.shape == DS_NC && index < 1) return fail("unknown index: ic = " + std::to_string(index) + " < 1");
  if (is_edge_shape(T.shape) && (side < LBS_WEST || side > LBS_NORTH))
    return fail("unknown side " + std::to_string(side) + " (enum roms_lbc_side)");
  if (slot < 1 || slot > 2) return fail("slot " + std::to_string(slot) + " outside 1..2");
  if (point && T.routine != R_set_2dfld) return fail("point data are read by set_2dfld only");
  switch (T.shape) {
  case DS_2D: case DS_2DT: *n = nij; break;
  case DS_N: case DS_NC: *n = nij * b.N; break;
  default: *n = (side <= LBS_EAST ? nj : ni) * (T.shape == DS_E ? 1 : b.N);
  }
  if (T.dest == DD_CLIMA && !clima_copy(target, index))
    return fail(std::string("the library has no device copy of it") + (T.shape == DS_NC ? " for ic = " + std::to_string(index) : std::string()) +
                ": hand the climatology over with roms_hip_set_clima first (its switch is off)");
  if ((T.dest == DD_FIELD || T.dest == DD_BRY) && !g_ctx.field[T.fid].dev) return fail("the field is not registered");
  if (is_edge_shape(T.shape)) {
    const bool edge = side == LBS_WEST ? b.west_edge : side == LBS_EAST ? b.east_edge : side == LBS_SOUTH ? b.south_edge : b.north_edge;
    const bool periodic = side <= LBS_EAST ? b.EWperiodic : b.NSperiodic;
    *skip = !edge || periodic;
  }
  return 0;
}

DataRec *data_find(int target, int index, int side, bool create)
{
  const DataLine &T = k_data_line[target];
  const int ix = (T.shape == DS_2DT || T.shape == DS_NC || T.shape == DS_ENT) ? index : 0, sd = is_edge_shape(T.shape) ? side : 0;
  size_t q = 0;
  for (; q < g_recs.size(); q++) {
    DataRec &r = g_recs[q];
    if (r.target == target && r.index == ix && r.side == sd) return &r;
    if (r.target > target || (r.target == target && (r.index > ix || (r.index == ix && r.side > sd)))) break;
  }
  if (!create) return nullptr;
  DataRec r;
  r.target = target; r.index = ix; r.side = sd;
  return &*g_recs.insert(g_recs.begin() + q, r);
}

void data_erase_if_empty(DataRec *r)
{
  if (r->filled[0] || r->filled[1]) return;
  for (int q = 0; q < 2; q++)
    if (r->slot[q]) (void)hipFree(r->slot[q]);
  g_recs.erase(g_recs.begin() + (r - g_recs.data()));
}
}  // namespace

extern "C" int roms_hip_set_data_record(int target, int index, int side, int slot, double Tintrp, int onerec,
                                        const double *rec, long n_doubles)
{
  const char *me = "roms_hip_set_data_record";
  long n = 0;
  bool skip = false;
  int rc = data_validate(me, target, index, side, slot, false, &n, &skip);
  if (rc) return rc;
  const DataLine &T = k_data_line[target];
  if (n_doubles != n) {
    char msg[200];
    snprintf(msg, sizeof msg, "set_data: %s: a record has %ld doubles, the host array %ld", T.name, n, n_doubles);
    return roms_fail(me, msg);
  }
  if (!rec) return roms_fail(me, (std::string("set_data: ") + T.name + ": the record is NULL").c_str());
  if (skip) return 0;                                // not an edge of this tile: nothing is kept
  DataRec *r = data_find(target, index, side, true);
  if (r->point) { r->point = false; r->filled[0] = r->filled[1] = false; }
  r->n = n;
  double *&dev = r->slot[slot - 1];
  if (!dev && hipMalloc(&dev, sizeof(double) * n) != hipSuccess) {
    (void)hipGetLastError();
    dev = nullptr;
    data_erase_if_empty(r);
    return roms_fail(me, "hipMalloc of a record failed");
  }
  // on the library's stream: behind the launches that read the slot's old contents; the wait makes the host buffer free
  hipError_t e = hipMemcpyAsync(dev, rec, sizeof(double) * n, hipMemcpyHostToDevice, g_ctx.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(g_ctx.stream);
  if (e != hipSuccess) {
    r->filled[slot - 1] = false;
    data_erase_if_empty(r);
    return roms_fail(me, hipGetErrorString(e));
  }
  r->filled[slot - 1] = true;
  r->Tintrp[slot - 1] = Tintrp;
  r->tindex = slot;
  r->onerec = onerec != 0;
  return 0;
}

extern "C" int roms_hip_set_data_point(int target, int index, int slot, double Tintrp, int onerec, double value)
{
  const char *me = "roms_hip_set_data_point";
  long n = 0;
  bool skip = false;
  int rc = data_validate(me, target, index, 0, slot, true, &n, &skip);
  if (rc) return rc;
  DataRec *r = data_find(target, index, 0, true);
  if (!r->point) { r->point = true; r->filled[0] = r->filled[1] = false; }
  r->n = n;
  r->filled[slot - 1] = true;
  r->Tintrp[slot - 1] = Tintrp;
  r->fpoint[slot - 1] = value;
  r->tindex = slot;
  r->onerec = onerec != 0;
  return 0;
}

// ------------------------------------------------------------------------------------------------ per step --
extern "C" int roms_hip_set_data(double time, double dt, int *synchro)
{
  const char *me = "roms_hip_set_data";
  if (int rc = roms_setup_check(me)) return rc;
  if (synchro) *synchro = 0;
  if (g_recs.empty()) return 0;
  const roms_bounds_t &b = g_ctx.b;
  const roms_params_t &p = g_ctx.p;
  const RomsTides &TD = g_ctx.hostc.tides;
  const long ni = b.UBi - b.LBi + 1, nj = b.UBj - b.LBj + 1, nij = ni * nj;
  const int N = b.N;
  auto i2 = [&](int i, int j) { return (long)(i - b.LBi) + (long)(j - b.LBj) * ni; };

  // every target is looked at before anything is launched
  std::vector<DataDesc> desc;
  struct Exch { int gtype, nk; double *A; };
  std::vector<Exch> exch;
  int syn = 0;
  for (const DataRec &r : g_recs) {
    const DataLine &T = k_data_line[r.target];
    auto fail = [&](const std::string &what) { return roms_fail(me, (std::string("set_data: ") + T.name + ": " + what).c_str()); };
    const int it2 = r.tindex, it1 = 3 - it2;
    if (!r.filled[it2 - 1] || (!r.onerec && !r.filled[it1 - 1]))
      return fail("slot " + std::to_string(r.filled[it2 - 1] ? it1 : it2) + " was never filled (roms_hip_set_data_record)");
    DataDesc d{};
    if (roms_hip_set_data_factors(time, dt, r.Tintrp[0], r.Tintrp[1], r.tindex, r.onerec, &d.fac1, &d.fac2, &syn)) {
      char msg[240];
      snprintf(msg, sizeof msg, "current model time exceeds ending value for variable: time = %.6f s, TINTRP1 = %.6f s, TINTRP2 = %.6f s",
               time, r.Tintrp[it1 - 1], r.Tintrp[it2 - 1]);
      return fail(msg);
    }
    d.mode = r.point ? SDM_POINT : r.onerec ? SDM_COPY : SDM_INTERP;
    if (r.point) d.fac1 = r.onerec ? r.fpoint[it2 - 1] : d.fac1 * r.fpoint[it1 - 1] + d.fac2 * r.fpoint[it2 - 1];   // Fval, :106, :128
    // the destination, as it stands now
    double *base = nullptr;
    if (T.dest == DD_CLIMA) {
      if (!(base = clima_copy(r.target, r.index)))
        return fail("the library has no device copy of it any more: hand the climatology over with roms_hip_set_clima");
    } else {
      if (!(base = g_ctx.field[T.fid].dev)) return fail("the field is not registered");
      if (T.shape == DS_2DT) base += (long)(r.index - 1) * nij;
      if (T.shape == DS_ENT) base += (long)(r.index - 1) * nij * N;
      if (TD.ntc > 0 && TD.add_fs && r.target == DATA_zeta_bry) base = const_cast<double *>(TD.zeta_base);
      if (TD.ntc > 0 && TD.add_m2 && r.target == DATA_ubar_bry) base = const_cast<double *>(TD.ubar_base);
      if (TD.ntc > 0 && TD.add_m2 && r.target == DATA_vbar_bry) base = const_cast<double *>(TD.vbar_base);
      if (!base) return fail("the tides hold no sub-tidal base to write to (roms_hip_set_tides)");
    }
    const double *s1 = r.slot[it1 - 1], *s2 = r.slot[it2 - 1];
    if (!is_edge_shape(T.shape)) {
      // set_2dfld.F:122-126, set_3dfld.F:132-138: IstrR:IendR, JstrR:JendR [, 1:N]
      const int nk = (T.shape == DS_N || T.shape == DS_NC) ? N : 1;
      const long o = i2(b.IstrR, b.JstrR);
      d.L = b.IendR - b.IstrR + 1;
      d.rpp = b.JendR - b.JstrR + 1;
      d.rows = d.rpp * nk;
      d.spitch = d.dpitch = ni;
      d.splane = d.dplane = nij;
      d.dstep = 1;
      d.s1 = s1 ? s1 + o : nullptr; d.s2 = s2 ? s2 + o : nullptr; d.dst = base + o;
      // the periodic images and the tile exchange (set_2dfld.F:170-201); with the extents of tclm's plane for DS_NC
      exch.push_back(Exch{T.gtype, nk, base});
    } else {
      // set_ngfld.F:100-104 over the reference's range (roms_data.def) within the allocated extent of this tile
      const bool we = r.side <= LBS_EAST, hi = r.side == LBS_EAST || r.side == LBS_NORTH;
      const int nk = T.shape == DS_E ? 1 : N;
      const int lb = we ? b.LBj : b.LBi, ub = we ? b.UBj : b.UBi, len = ub - lb + 1;
      const int first = we ? (T.gtype == GT_V ? 1 : 0) : (T.gtype == GT_U ? 1 : 0), last = we ? b.Mm + 1 : b.Lm + 1;
      int a0 = lb > first ? lb : first, a1 = ub < last ? ub : last;
      // the point of the *_bry field an edge value sits at (roms_fields.def; k_set_tides.hip)
      int fixed;
      if (we) fixed = hi ? b.Iend + 1 : (T.gtype == GT_U ? b.Istr : b.Istr - 1);
      else fixed = hi ? b.Jend + 1 : (T.gtype == GT_V ? b.Jstr : b.Jstr - 1);
      // The reference keeps four vectors; the one array here gives the last element of a western / eastern vector and
      // the first of a southern / northern one the same point (zeta_west(0) and zeta_south(0), ubar_west(0) and
      // ubar_south(1), vbar_west(1) and vbar_south(0) ...).  No condition reads either (the edge loops run over
      // Jstr:Jend / IstrU:Iend / JstrV:Jend, the corners are means of their neighbours, zetabc.F:699-731): the point is
      // the southern / northern vector's, so that one launch never stores two values to it.
      if (we) {
        const int jS = T.gtype == GT_V ? b.Jstr : b.Jstr - 1, jN = b.Jend + 1;
        if (b.south_edge && a0 <= jS) a0 = jS + 1;
        if (b.north_edge && a1 >= jN) a1 = jN - 1;
      }
      if (a1 < a0 || fixed < (we ? b.LBi : b.LBj) || fixed > (we ? b.UBi : b.UBj)) return fail("the bounds leave no point beside the edge");
      const long o = we ? i2(fixed, a0) : i2(a0, fixed);
      d.L = a1 - a0 + 1;
      d.rpp = d.rows = nk;
      d.spitch = len; d.splane = 0;
      d.dpitch = nij; d.dplane = 0;
      d.dstep = we ? ni : 1;
      d.s1 = s1 ? s1 + (a0 - lb) : nullptr; d.s2 = s2 ? s2 + (a0 - lb) : nullptr; d.dst = base + o;
      if (p.wet_dry && r.target == DATA_zeta_bry) {                      // set_data.F:928-1003
        if (!g_ctx.field[FID_h].dev) return fail("wet_dry: field not registered: h");
        d.hclip = g_ctx.field[FID_h].dev + o;
        d.dcrit = p.Dcrit;
        d.clip0 = (we ? b.JstrR : b.IstrR) - a0;
        d.clip1 = (we ? b.JendR : b.IendR) - a0;
      }
    }
    d.segs = (d.L + SD_SEG - 1) / SD_SEG;
    desc.push_back(d);
  }

  // the tables: descriptors, then first[nd + 1]
  const int nd = (int)desc.size();
  const size_t off_first = sizeof(DataDesc) * (size_t)nd, bytes = off_first + sizeof(int) * (size_t)(nd + 1);
  if (bytes > g_tab_bytes) {
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    tab_release();
    const size_t cap = bytes * 2;
    HIP_TRY(hipMalloc(&g_tab, cap));
    HIP_TRY(hipHostMalloc(&g_tab_host, cap, hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&g_tab_event, hipEventDisableTiming));
    g_tab_bytes = cap;
  } else {
    HIP_TRY(hipEventSynchronize(g_tab_event));     // the copy of the previous call has read the host image
  }
  memcpy(g_tab_host, desc.data(), off_first);
  int *first = reinterpret_cast<int *>(static_cast<char *>(g_tab_host) + off_first);
  long blocks = 0;
  for (int q = 0; q < nd; q++) {
    first[q] = (int)blocks;
    blocks += (long)desc[q].rows * desc[q].segs;
  }
  if (blocks > 0x7fffffffL) return roms_fail(me, "set_data: too many workgroups for one launch");
  first[nd] = (int)blocks;
  {
    const int rc = roms_flush_consts();            // the exchange kernels read the constant block
    if (rc) return rc;
  }
  {
    ScopedTimer tm("set_data");
    HIP_TRY(hipMemcpyAsync(g_tab, g_tab_host, bytes, hipMemcpyHostToDevice, g_ctx.stream));
    HIP_TRY(hipEventRecord(g_tab_event, g_ctx.stream));
    hipLaunchKernelGGL(k_set_data, dim3((unsigned)blocks), dim3(256), 0, g_ctx.stream,
                       reinterpret_cast<const DataDesc *>(g_tab),
                       reinterpret_cast<const int *>(static_cast<char *>(g_tab) + off_first), nd);
    KERNEL_CHECK("k_set_data");
    if (!exch.empty()) {
      halo_batch_begin();
      for (const Exch &x : exch) (void)halo_exchange3d(x.gtype, x.nk, x.A);
      const int rc = halo_batch_end();
      if (rc) return rc;
    }
  }
  if (synchro) *synchro = syn;
  return 0;
}
