// sources.hip -- point sources (mod_sources.F), LuvSrc / LwSrc: the table SOURCES(ng) on the device (RomsSrc,
// roms_dev.h) and roms_hip_set_sources.  Host code only: the kernels that read the table are the step kernels.
#include "roms_dev.h"
#include <algorithm>
#include <vector>

namespace {
struct SrcStore {
  int *geo = nullptr;        // device: I[n], J[n], D[n], umap[nij], vmap[nij]
  double *val = nullptr;     // device: Qbar[n], Qsrc[n*N], Tsrc[n*N*NT]
  int n = 0, N = 0, NT = 0;
  long nij = 0;
  std::vector<int> I, J, D;
  bool given = false;
} g_src;
}  // namespace

// (roms_hip_set_bounds: the face maps are in the old bounds' index space)
void sources_release()
{
  if (g_src.geo) (void)hipFree(g_src.geo);
  if (g_src.val) (void)hipFree(g_src.val);
  g_src = SrcStore{};
  g_ctx.hostc.src = RomsSrc{};
  g_ctx.devc_dirty = true;
}

bool roms_sources_given() { return g_src.given; }

extern "C" int roms_hip_set_sources(int Nsrc, const int *Isrc, const int *Jsrc, const double *Dsrc, const double *Qbar,
                                    const double *Qsrc, const double *Tsrc, const int *LtracerSrc)
{
  const char *me = "roms_hip_set_sources";
  if (int rc = roms_setup_check(me)) return rc;
  if (Nsrc < 0) return roms_fail(me, "Nsrc < 0");
  if (!(g_ctx.p.point_sources & 3))
    return roms_fail(me, "point sources: neither bit of roms_params_t.point_sources (LuvSrc, LwSrc) is set");
  const bool luv = (g_ctx.p.point_sources & 1) != 0, lw = (g_ctx.p.point_sources & 2) != 0;
  if (Nsrc == 0) {
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    step2d_graphs_release();               // captured source launches hold the freed table's size
    sources_release();
    g_src.given = true;
    return 0;
  }
  if (!Isrc || !Jsrc || !Dsrc || !Qbar || !Qsrc || !Tsrc || !LtracerSrc) return roms_fail(me, "null argument");
  const roms_bounds_t &b = g_ctx.b;
  const int N = b.N, NT = b.NT;
  const long ni = b.UBi - b.LBi + 1, nij = ni * (b.UBj - b.LBj + 1);
  std::vector<int> D(Nsrc);
  for (int is = 0; is < Nsrc; is++) {
    D[is] = (int)Dsrc[is];
    if (D[is] < 0 || D[is] > 2) return roms_fail(me, "point sources: Dsrc is 0 (u-face), 1 (v-face) or 2 (cell centre)");
  }
  const bool same = g_src.geo && g_src.n == Nsrc && g_src.N == N && g_src.NT == NT && g_src.nij == nij &&
                    std::equal(g_src.I.begin(), g_src.I.end(), Isrc) && std::equal(g_src.J.begin(), g_src.J.end(), Jsrc) &&
                    g_src.D == D;
  const size_t nval = (size_t)Nsrc * (1 + (size_t)N + (size_t)N * NT);
  if (!same) {
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    step2d_graphs_release();               // captured launches hold the old table's addresses
    sources_release();
    const size_t ngeo = 3 * (size_t)Nsrc + 3 * (size_t)nij + 2 * (size_t)Nsrc;
    std::vector<int> geo(ngeo, 0);
    int *umap = geo.data() + 3 * (size_t)Nsrc, *vmap = umap + nij, *wmap = vmap + nij, *cells = wmap + nij;
    int ncell = 0;
    for (int is = 0; is < Nsrc; is++) {
      geo[is] = Isrc[is]; geo[Nsrc + is] = Jsrc[is]; geo[2 * (size_t)Nsrc + is] = D[is];
      // a source of a kind the application has switched off is not looked at (IF (LuvSrc) / IF (LwSrc) in the reference)
      if (D[is] == 2 ? !lw : !luv) continue;
      // the face / cell maps: the last source of a face wins, as the sequential loops of the reference leave it
      if (Isrc[is] >= b.LBi && Isrc[is] <= b.UBi && Jsrc[is] >= b.LBj && Jsrc[is] <= b.UBj)
        (D[is] == 0 ? umap : D[is] == 1 ? vmap : wmap)[(long)(Isrc[is] - b.LBi) + (long)(Jsrc[is] - b.LBj) * ni] = is + 1;
      // the two cells of the face (the one cell of a cell-centred source), where they are interior cells of this tile
      // (each once)
      for (int side = 0; side < (D[is] == 2 ? 1 : 2); side++) {
        const int ci = Isrc[is] - (D[is] == 0 ? side : 0), cj = Jsrc[is] - (D[is] == 1 ? side : 0);
        if (ci < b.Istr || ci > b.Iend || cj < b.Jstr || cj > b.Jend) continue;
        const int cell = (int)((long)(ci - b.LBi) + (long)(cj - b.LBj) * ni);
        if (std::find(cells, cells + ncell, cell) == cells + ncell) cells[ncell++] = cell;
      }
    }
    HIP_TRY(hipMalloc(&g_src.geo, sizeof(int) * ngeo));
    HIP_TRY(hipMalloc(&g_src.val, sizeof(double) * (nval + (size_t)Nsrc * N)));
    HIP_TRY(hipMemcpy(g_src.geo, geo.data(), sizeof(int) * ngeo, hipMemcpyHostToDevice));
    g_src.n = Nsrc; g_src.N = N; g_src.NT = NT; g_src.nij = nij;
    g_src.I.assign(Isrc, Isrc + Nsrc); g_src.J.assign(Jsrc, Jsrc + Nsrc); g_src.D = D;
    RomsSrc &S = g_ctx.hostc.src;
    S.n = Nsrc;
    S.I = g_src.geo; S.J = g_src.geo + Nsrc; S.D = g_src.geo + 2 * (size_t)Nsrc;
    S.umap = g_src.geo + 3 * (size_t)Nsrc; S.vmap = S.umap + nij;
    S.wmap = S.vmap + nij;
    S.cells = S.wmap + nij; S.ncell = ncell;
    S.Qbar = g_src.val; S.Qsrc = g_src.val + Nsrc; S.Tsrc = g_src.val + Nsrc + (size_t)Nsrc * N;
    S.save = g_src.val + nval;
  }
  // the values change with every set_data: one staged copy (a few kB), in stream order after the kernels that read the old ones
  std::vector<double> val(nval);
  std::copy(Qbar, Qbar + Nsrc, val.begin());
  std::copy(Qsrc, Qsrc + (size_t)Nsrc * N, val.begin() + Nsrc);
  std::copy(Tsrc, Tsrc + (size_t)Nsrc * N * NT, val.begin() + Nsrc + (size_t)Nsrc * N);
  HIP_TRY(hipMemcpyAsync(g_src.val, val.data(), sizeof(double) * nval, hipMemcpyHostToDevice, g_ctx.stream));
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  for (int it = 0; it < ROMS_MAXNT; it++) g_ctx.hostc.src.ltr[it] = it < NT ? (LtracerSrc[it] != 0) : 0;
  g_src.given = true;
  g_ctx.devc_dirty = true;
  return 0;
}
