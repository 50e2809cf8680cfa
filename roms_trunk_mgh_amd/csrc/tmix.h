// tmix.h -- what the lateral tracer mixing kernels of k_mix.hip share: t3dmix2_s.h:89-306 and t3dmix4_s.h:100-480 along
// s-surfaces (k_t3dmix_s), t3dmix2_geo.h:90-424, t3dmix4_geo.h:104-784 and t3dmix2_iso.h / t3dmix4_iso.h rotated
// (k_t3dmix_geo).  The reference writes the same range, the same face coefficients and masks and the same vertical flux
// bracket in every one of them; here each is stated once: dmin0(), dmax0(), tdiff<STAB>(); Lap4, lap4_store();
// mix_column<MODE>(), mix_pointers<MODE, STAB>(); Face4, face_coef(), face_mask(); fs_bracket().
// MODE 0: the harmonic operator (all tracers of the launch).  MODE 1 / 2: first / second operator of the biharmonic one
// for tracer L.itrc.  Association stays with the caller: where a mask or a prefactor multiplies is the kernel's text.
#pragma once
#include "roms_dev.h"

__device__ __forceinline__ double dmin0(double a) { return a < 0.0 ? a : 0.0; }   // MIN(a,0)
__device__ __forceinline__ double dmax0(double a) { return a > 0.0 ? a : 0.0; }   // MAX(a,0)

// The tracer difference a - b of the operators' first application; STAB (TS_MIX_STABILITY, t3dmix2_s.h:212-218,
// t3dmix2_geo.h:236 / :268 / :301 and the like sites of t3dmix2_iso.h and of the first operator of t3dmix4_*.h): 3/4 of
// it plus 1/4 of the same difference a2 - b2 of t(nstp)
template <bool STAB>
__device__ __forceinline__ double tdiff(double a, double b, double a2, double b2)
{
  if constexpr (STAB) return 0.75 * (a - b) + 0.25 * (a2 - b2);
  else return a - b;
}

// The range and the edge rule of the first biharmonic operator (t3dmix4_s.h:262-275, :347-405): one point beyond the
// tile inside the grid; outside a physical edge LapT is zero where the tracer's condition is closed, a copy of the
// first inside value otherwise.  (The corner values the reference also sets are never read by the second operator.)
struct Lap4 {
  double *lap;                  // LapT of one tracer, module extents
  int i0, i1, j0, j1;           // Imin:Imax, Jmin:Jmax
  int closed[4];                // [LBS_WEST .. LBS_NORTH]
  int itrc;
  int nstp;                     // STAB kernels: the time level of the 1/4 part
};

__device__ __forceinline__ void lap4_store(const roms_bounds_t &b, const Lap4 &L, long ni, int i, int j, long a, double val)
{
  const gd_t lap = (gd_t)L.lap;
  lap[a] = val;
  if (!b.EWperiodic) {
    if (b.west_edge && i == b.Istr) lap[a - 1] = L.closed[LBS_WEST] ? 0.0 : val;
    if (b.east_edge && i == b.Iend) lap[a + 1] = L.closed[LBS_EAST] ? 0.0 : val;
  }
  if (!b.NSperiodic) {
    if (b.south_edge && j == b.Jstr) lap[a - ni] = L.closed[LBS_SOUTH] ? 0.0 : val;
    if (b.north_edge && j == b.Jend) lap[a + ni] = L.closed[LBS_NORTH] ? 0.0 : val;
  }
}

// The thread's column of a mixing launch (grid_tile_tracer): the tile, for MODE 1 the range L.i0:L.i1, L.j0:L.j1 one
// point wider; all tracers in the harmonic launch alone
struct MixCol { int i, j, itrc; bool valid; };
template <int MODE>
__device__ __forceinline__ MixCol mix_column(const roms_bounds_t &b, const Lap4 &L)
{
  const int ilo = MODE == 1 ? L.i0 : b.Istr, ihi = MODE == 1 ? L.i1 : b.Iend;
  const int jlo = MODE == 1 ? L.j0 : b.Jstr, jhi = MODE == 1 ? L.j1 : b.Jend;
  const TileTr tt = decode_tile_tracer(ihi - ilo + 1, jhi - jlo + 1, MODE == 0 ? b.NT : 1);
  const int i = ilo + tt.bx * BLK_X + threadIdx.x, j = jlo + tt.by * BLK_Y + threadIdx.y;
  return MixCol{i, j, MODE == 0 ? 1 + tt.itr : L.itrc, tt.valid && i <= ihi && j <= jhi};
}

// T: what the operator differences, t(nrhs) or LapT; S: t(nstp) of the 1/4 part (STAB; T otherwise); tn: t(nnew)
struct MixPtr { const double *T, *S; double *tn; };
template <int MODE, bool STAB>
__device__ __forceinline__ MixPtr mix_pointers(const RomsDev *__restrict__ c, int nrhs, int nnew, const Lap4 &L, int itrc, long n3r)
{
  static_assert(!(STAB && MODE == 2), "the second biharmonic operator acts on LapT alone");
  double *t = c->F.t + 3L * (itrc - 1) * n3r;
  const double *T = MODE == 2 ? L.lap : t + (long)(nrhs - 1) * n3r;
  return MixPtr{T, STAB ? t + (long)(L.nstp - 1) * n3r : T, t + (long)(nnew - 1) * n3r};
}

struct Face4 { double x0, x1, e0, e1; };        // values at the four faces of a cell: xi faces i, i+1, eta faces j, j+1
// 0.25 * (d + d of the neighbour) * metric: d = diff2 / diff4 of the tracer, (mu, mv) = (pmon_u, pnom_v) along
// s-surfaces (t3dmix2_s.h:209, :249), (on_u, om_v) in the rotated sweep (t3dmix2_geo.h:334, :354)
__device__ __forceinline__ Face4 face_coef(const double *__restrict__ d, const double *__restrict__ mu,
                                           const double *__restrict__ mv, long c0, long ni)
{
  return Face4{0.25 * (d[c0] + d[c0 - 1]) * mu[c0], 0.25 * (d[c0 + 1] + d[c0]) * mu[c0 + 1],
               0.25 * (d[c0] + d[c0 - ni]) * mv[c0], 0.25 * (d[c0 + ni] + d[c0]) * mv[c0 + ni]};
}
// MASKING (t3dmix2_s.h:235, :275; t3dmix2_geo.h:228, :260): umask / vmask of the face; WET_DRY: times its wet/dry mask,
// the block after each MASKING block.  1.0 without MASKING.
__device__ __forceinline__ Face4 face_mask(const RomsDev *__restrict__ c, long c0, long ni)
{
  if (!c->p.masking) return Face4{1.0, 1.0, 1.0, 1.0};
  return Face4{umaskw(c, c0), umaskw(c, c0 + 1), vmaskw(c, c0), vmaskw(c, c0 + ni)};
}

// One direction of the vertical flux of the rotated operators (t3dmix2_geo.h:376-394, t3dmix2_iso.h:395-417,
// t3dmix4_iso.h:443-480 and the like blocks of t3dmix4_geo.h): c1..c4 the MIN / MAX parts of the slopes at the two faces
// and two levels, dz = dTdz of the own column, t1..t4 the horizontal tracer differences that go with them
__device__ __forceinline__ double fs_bracket(double c1, double c2, double c3, double c4, double dz,
                                             double t1, double t2, double t3, double t4)
{
  return c1 * (c1 * dz - t1) + c2 * (c2 * dz - t2) + c3 * (c3 * dz - t3) + c4 * (c4 * dz - t4);
}
