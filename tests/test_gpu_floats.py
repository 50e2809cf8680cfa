"""-m gpu: Lagrangian floats on the device (FLOATS: roms_hip_set_floats, roms_hip_step_floats, csrc/k_floats.hip).

step_floats.F and interp_floats.F USE the I/O modules, so the reference cannot make a vector for them: the yardstick is
the numpy restatement tests/floats_util.py, whose known answers tests/test_floats.py checks without a GPU.  Bit for bit
throughout (np.array_equal on every entry of track and bounded): the kernel performs the reference's operations in the
reference's order and the build does not contract multiply-adds.
  1. per-call parity on a random state and a random track history, 197 floats placed at the seams, edges, land halo,
     surface and bottom
  2. seven whole steps through main3d; nothing else changes
  3. tiling invariance over the relay (2x2 closed, 4x1 E-W periodic with the collection in the middle of the routine),
     and one tile in RCCL loopback
  4. the refusals"""
import ctypes as C
import numpy as np
import pytest

import floats_util as fu
import tiling_util
import util
from roms_trunk_mgh_amd import ana, floats, hip, main3d
from test_gpu_wide import I0, LAND_ROW, SHAPES, seam_land

pytestmark = pytest.mark.gpu
NFLOATS = 197                                # more than one workgroup of 64, and no multiple of 64
FIELDS = ("u", "v", "W", "Hz", "z_w", "rho", "t", "pm", "pn")


def _state(shape, nghost, periodic, masked):
    ov = dict(SHAPES[shape])
    if nghost == 3:
        ov["uv_vis4"] = 1                                 # three ghost points (inp_par.F:264-278)
    if not periodic:
        ov["EWperiodic"] = False
    kw = dict(mask="island", land=seam_land(shape)) if masked else {}
    st = util.prepared_state("BENCHMARK_TINY", overrides=ov, **kw)
    assert st.b.NghostPoints == nghost and bool(st.b.EWperiodic) == periodic and st.p.masking == int(masked)
    return st


def _randomise(st, rng):
    """random fields with the scales of a model state: a float moves a fraction of a cell per step"""
    b, dt = st.b, st.p.dt
    sh2 = st["pm"].shape
    st["pm"][:] = 1.0e-3 * (1.0 + 0.2 * rng.random(sh2))
    st["pn"][:] = 1.0e-3 * (1.0 + 0.2 * rng.random(sh2))
    st["Hz"][:] = 5.0 + 10.0 * rng.random(st["Hz"].shape)
    st["z_w"][:, :, 0] = -10.0 * b.N - 5.0 * rng.random(sh2)
    st["z_w"][:, :, 1:] = st["z_w"][:, :, :1] + np.cumsum(st["Hz"], axis=2)
    vel = 0.3 / (1.0e-3 * dt)
    st["u"][:] = vel * rng.standard_normal(st["u"].shape)
    st["v"][:] = vel * rng.standard_normal(st["v"].shape)
    st["W"][:] = 0.2 * 10.0 / (1.0e-6 * dt) * rng.standard_normal(st["W"].shape)
    st["rho"][:] = rng.standard_normal(st["rho"].shape)
    st["t"][:] = rng.standard_normal(st["t"].shape)
    if st.p.masking:
        st["u"][:] *= st["umask"][:, :, None, None]
        st["v"][:] *= st["vmask"][:, :, None, None]
        st["rho"][:] *= st["rmask"][:, :, None]
        st["t"][:] *= st["rmask"][:, :, None, None, None]


def _placement(b, rng):
    """positions (level nf) of the 197 floats, their types, release times relative to `time` in steps, bounded"""
    n, Lm, Mm, N = NFLOATS, b.Lm, b.Mm, b.N
    x = 0.5 + Lm * rng.random(n)
    y = 0.5 + Mm * rng.random(n)
    z = N * rng.random(n)
    q = 0
    for sx in (I0 + 63.5, 0.5, Lm + 0.5):                  # the workgroup seam of the stencil kernels, the tile edges
        for off in (-0.49, -0.01, 0.0, 0.01, 0.49):
            x[q] = sx + off
            q += 1
    for sy in (0.5, Mm + 0.5):
        for off in (-0.3, 0.0, 0.3):
            y[q] = sy + off
            q += 1
    for il, jl in seam_land("w3"):                          # the nine land-halo cases around both land cells
        for ox in (-0.8, -0.3, 0.2, 0.7, 1.2):
            for oy in (-0.8, -0.3, 0.2, 0.7, 1.2):
                if q < n - 40:
                    x[q], y[q] = il + ox, jl + oy
                    q += 1
    x[q:q + 4] = [0.2, 0.49, Lm + 0.5, Lm + 0.9]            # x < 0.5 and x >= Lm + 0.5
    q += 4
    z[q:q + 4] = [N - 0.02, N - 0.3, 0.02, 0.3]             # within one step of the surface and of the bottom
    q += 4
    Ftype = 1 + np.arange(n) % 3
    rel = np.full(n, 1000.0)                                # after
    rel[0::5] = -1000.0                                     # before the start
    rel[1::5] = 0.0                                         # in the window
    rel[2::15] = 0.5                                        # the closed end of the window: time + dt/2 is outside
    rel[7::15] = -0.5                                       # time - dt/2 is inside
    bounded = np.ones(n, dtype=bool)
    bounded[1::5] = False
    bounded[3::10] = False
    return x, y, z, Ftype, rel, bounded


def _drifter(st, rng, time):
    b, dt = st.b, st.p.dt
    n = NFLOATS
    x, y, z, Ftype, rel, bounded = _placement(b, rng)
    T = np.zeros((10, n), order="F")
    T[floats.itstr] = time + rel * dt
    T[floats.ixgrd] = 0.5 + b.Lm * rng.random(n)
    T[floats.iygrd] = 0.5 + b.Mm * rng.random(n)
    T[floats.izgrd] = b.N * rng.random(n)
    T[floats.ixgrd, 1], T[floats.iygrd, 6] = -3.0, b.Mm + 0.75       # released outside the grid
    sh = st["pm"].shape
    fl = floats.Floats(b, Ftype, T, -5.0 - 30.0 * rng.random(n), 1.0e3 * rng.random(sh), 1.0e3 * rng.random(sh))
    track = rng.standard_normal((fl.NFV, floats.NFT + 1, n))
    for lev in range(floats.NFT + 1):
        track[floats.ixgrd - 1, lev] = x + (0.0 if lev == 0 else 0.2 * rng.standard_normal(n))
        track[floats.iygrd - 1, lev] = y + (0.0 if lev == 0 else 0.2 * rng.standard_normal(n))
        track[floats.izgrd - 1, lev] = z + (0.0 if lev == 0 else 0.1 * rng.standard_normal(n))
        for v in (floats.ixrhs, floats.iyrhs, floats.izrhs):
            track[v - 1, lev] = 0.3 / dt * rng.standard_normal(n)
    return fl, np.asfortranarray(track), bounded


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nghost", [2, 3])
@pytest.mark.parametrize("shape", ["w3", "thin"])
def test_every_call_equals_the_restatement(shape, nghost, periodic, masked):
    st = _state(shape, nghost, periodic, masked)
    rng = np.random.default_rng(17)
    _randomise(st, rng)
    be = hip.RomsHip(st)
    try:
        be.to_device()
        for k, shift in enumerate((0, 1, 3, 4)):
            nfl = tuple((v + shift) % 5 for v in (2, 3, 4, 0, 1))
            nnew = 1 + k % 2
            time = 40.0 * st.p.dt * k
            fl, track, bounded = _drifter(st, rng, time)
            # the history of level 0 of _drifter is the position at level nf
            track[:, [0, nfl[3]]] = track[:, [nfl[3], 0]]
            be.set_floats(fl)
            be.floats_put(track, bounded)
            s = util.step_idx(iic=3 + k, nnew=nnew)
            be.step_floats(s, time, nfl)
            got_t, got_b = be.floats_get()
            g = fu.grid_of_state(st, nnew, fl.xcoord, fl.ycoord)
            R = fu.one_tile(g, track, bounded)
            fu.step_floats(R, 1, nfl, time, fl.Ftype, fl.Tinfo, fl.Fz0)
            want_t, want_b = R[0].track, R[0].bounded
            bad = np.argwhere(~((got_t == want_t) | (np.isnan(got_t) & np.isnan(want_t))))
            assert np.array_equal(got_t, want_t, equal_nan=True), (shift, len(bad), bad[:5].tolist())
            assert np.array_equal(got_b, want_b), (shift, np.flatnonzero(got_b != want_b)[:5].tolist())
            # the case is not empty: floats moved, were lost or released, reflected, and the outputs were written
            moved = want_t[floats.ixgrd - 1, nfl[4]] != track[floats.ixgrd - 1, nfl[4]]
            assert moved.sum() > NFLOATS // 2 and (want_b & ~bounded).any()
            assert (want_t[floats.idpth - 1, nfl[4]] == 1.0e37).any() and (np.abs(want_t[floats.ifden - 1, nfl[4]]) < 10.0).any()
            assert periodic or (bounded & ~want_b).any()
        be.check_guards()
    finally:
        be.close()


# ------------------------------------------------------------------------------------------- 2. end to end --
class _Proxy:
    """forwards every call; after step_floats it pulls the state and feeds the restatement"""

    def __init__(self, be, fl):
        self._be, self._fl, self.ranks, self.steps = be, fl, None, 0

    def __getattr__(self, name):
        return getattr(self._be, name)

    def step_floats(self, s, time, nfl):
        be, fl = self._be, self._fl
        be.step_floats(s, time, nfl)
        be.to_host()
        g = fu.grid_of_state(be.st, s.nnew, fl.xcoord, fl.ycoord)
        if self.ranks is None:
            self.ranks = fu.one_tile(g, np.zeros(fl.track_shape()), np.zeros(fl.n, dtype=bool))
        self.ranks[0].g = g
        fu.step_floats(self.ranks, 1, nfl, time, fl.Ftype, fl.Tinfo, fl.Fz0)
        got_t, got_b = be.floats_get()
        assert np.array_equal(got_t, self.ranks[0].track, equal_nan=True), ("main3d", s.iic)
        assert np.array_equal(got_b, self.ranks[0].bounded), ("main3d", s.iic)
        self.steps += 1


PROGNOSTIC = ("zeta", "ubar", "vbar", "u", "v", "t", "Hz", "W", "Huon", "Hvom", "rho", "Zt_avg1", "DU_avg1", "DV_avg2")


def test_seven_steps_through_main3d():
    import mp_gpu_floats_worker as worker
    st0 = ana.make_tile("UPWELLING", perturb=1.0, overrides=SHAPES["w3"])
    out = {}
    for key in ("with", "without"):
        st = st0.copy()
        be = hip.RomsHip(st)
        try:
            if key == "with":
                fl = worker.drifter(st)
                fl.Tinfo[floats.itstr, 3::7] = 3.0 * st.p.dt          # some are released on the fourth step
                proxy = _Proxy(be, fl)
                m = main3d.Main3D(proxy, floats=fl)
            else:
                m = main3d.Main3D(be)
            m.initial()
            m.run(7)
            be.to_host()
            be.check_guards()
        finally:
            be.close()
        out[key] = st
    assert proxy.steps == 7 and fl.nfl() == tuple((v + 7) % 5 for v in (2, 3, 4, 0, 1))
    tr, bd = proxy.ranks[0].track, proxy.ranks[0].bounded
    assert bd.sum() > NFLOATS // 2 and not bd.all()
    assert np.abs(tr[floats.ixrhs - 1, fl.levels["nf"]][bd]).max() > 0.0
    for name in PROGNOSTIC:
        assert np.array_equal(out["with"][name], out["without"][name], equal_nan=True), name
    assert not np.array_equal(out["with"]["t"], st0["t"])


# ------------------------------------------------------------------------------------- 3. tiling invariance --
def _tiles_equal_single(tmp_path, world, ntI, ntJ, variant):
    import mp_gpu_floats_worker as worker
    st = worker.tiled_state(variant)
    be = hip.RomsHip(st)
    try:
        want_t, want_b = worker.run(be, st)
    finally:
        be.close()
    assert want_b.sum() > NFLOATS // 2 and not want_b.all()
    tiling_util.spawn_ranks("mp_gpu_floats_worker.py", world, [ntI, ntJ, tmp_path, variant], timeout=600)
    for r, d, _, _ in tiling_util.tiles(tmp_path, world, st.b):     # the tracks are not gridded: every rank holds them all
        assert np.array_equal(d["track"], want_t, equal_nan=True), (r, np.argwhere(d["track"] != want_t)[:5].tolist())
        assert np.array_equal(d["bounded"], want_b), r


@pytest.mark.parametrize("ntI,ntJ,variant", [(2, 2, "basin"), (4, 1, "")])
def test_tiled_floats_equal_the_single_tile_run(tmp_path, ntI, ntJ, variant):
    _tiles_equal_single(tmp_path, ntI * ntJ, ntI, ntJ, variant)


def test_rccl_loopback_equals_the_single_tile_run(tmp_path):
    _tiles_equal_single(tmp_path, 1, 1, 1, "rccl")


# ---------------------------------------------------------------------------------------------- 4. refusals --
def test_refusals_use_the_error_path_and_leave_the_library_usable():
    lib = hip.load()
    st = util.prepared_state("UPWELLING")
    rng = np.random.default_rng(3)
    fl, track, bounded = _drifter(st, rng, 0.0)
    s = util.step_idx(iic=2)
    nfl = (C.c_int * 5)(2, 3, 4, 0, 1)
    assert hip.RomsHip._live is None
    assert lib.roms_hip_init(0, 1, 1, 0, None) == 0
    try:                                                       # before bounds / params
        assert lib.roms_hip_set_floats(*fl.c_args()) != 0 and b"come first" in lib.roms_hip_last_error()
    finally:
        assert lib.roms_hip_finalize() == 0
    be = hip.RomsHip(st)
    try:
        be.step_floats(s, 0.0, (2, 3, 4, 0, 1))                # nothing configured: returns 0, does nothing
        with pytest.raises(RuntimeError, match="none set"):
            be.floats_put(track, bounded)
        be.set_floats(fl)
        be.floats_put(track, bounded)
        bad = floats.Floats(st.b, fl.Ftype.copy(), fl.Tinfo, fl.Fz0, fl.xcoord, fl.ycoord)
        for value in (0, 4):
            bad.Ftype[5] = value
            assert lib.roms_hip_set_floats(*bad.c_args()) != 0
            assert b"Ftype(6)" in lib.roms_hip_last_error() and b"outside 1..3" in lib.roms_hip_last_error()
        got_t, got_b = be.floats_get()                         # a refused call left the floats as they were
        assert np.array_equal(got_t, track) and np.array_equal(got_b, bounded)
        assert lib.roms_hip_step_floats(C.byref(s), 0.0, (C.c_int * 5)(0, 1, 2, 3, 3)) != 0
        assert b"permutation" in lib.roms_hip_last_error()
        buf = np.zeros(track.size + 1)
        ib = np.zeros(fl.n, dtype=np.int32)
        assert lib.roms_hip_floats_get(buf.ctypes.data, buf.size, ib.ctypes.data, ib.size) != 0
        assert b"doubles" in lib.roms_hip_last_error() and not buf.any()
        assert lib.roms_hip_step_floats(C.byref(s), 0.0, nfl) == 0
        be.set_floats(None)                                    # Nfloats = 0 releases everything
        with pytest.raises(RuntimeError, match="none set"):
            be.floats_put(track, bounded)
        be.step_floats(s, 0.0, (2, 3, 4, 0, 1))
        be.check_guards()
    finally:
        be.close()
    # N-S periodic bounds are refused
    st.b.NSperiodic = 1
    assert lib.roms_hip_init(0, 1, 1, 0, None) == 0
    try:
        assert lib.roms_hip_set_bounds(C.byref(st.b)) == 0 and lib.roms_hip_set_params(C.byref(st.p)) == 0
        assert lib.roms_hip_set_floats(*fl.c_args()) != 0 and b"N-S periodic" in lib.roms_hip_last_error()
    finally:
        st.b.NSperiodic = 0
        assert lib.roms_hip_finalize() == 0
