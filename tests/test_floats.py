"""CPU: Lagrangian floats (FLOATS; roms_hip_set_floats / roms_hip_step_floats) without a GPU.

Known answers that pin the numpy restatement tests/floats_util.py, which stands in for the reference vector these
routines cannot have; none of them depends on anyone's reading of the loops.  Then the ownership switch with the SUM
collection on 2x2 and 4x1 partitions against one tile, and the new entries of the ABI with the refusals that need no
device."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import floats_util as fu
from roms_trunk_mgh_amd import abi, floats, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NFT = fu.NFT


def make_grid(Lm=12, Mm=8, N=5, NT=2, ewp=False, masking=False, dt=2.0, seed=None, Istr=1, Iend=None, Jstr=1, Jend=None):
    """a uniform grid (pm = pn = 1/2, Hz = 1, z_w = k - N) with resting fields, or with random ones (seed)"""
    b = SimpleNamespace(LBi=-2, UBi=Lm + 2, LBj=-2, UBj=Mm + 2, Lm=Lm, Mm=Mm, N=N, NT=NT, EWperiodic=int(ewp),
                        Istr=Istr, Iend=Iend or Lm, Jstr=Jstr, Jend=Jend or Mm)
    ni, nj = b.UBi - b.LBi + 1, b.UBj - b.LBj + 1
    ii = np.arange(b.LBi, b.UBi + 1, dtype=float)[:, None] + np.zeros((1, nj))
    jj = np.arange(b.LBj, b.UBj + 1, dtype=float)[None, :] + np.zeros((ni, 1))
    z = lambda *s: np.zeros((ni, nj) + s)
    a = dict(pm=z() + 0.5, pn=z() + 0.5, rmask=z() + 1.0, xc=2.0 * ii, yc=2.0 * jj, Hz=z(N) + 1.0, rho=z(N),
             z_w=z(N + 1) + np.arange(N + 1, dtype=float) - N, W=z(N + 1), u=z(N), v=z(N), t=[z(N) for _ in range(NT)])
    if seed is not None:
        rng = np.random.default_rng(seed)
        a["pm"] = 0.5 + 0.1 * rng.random((ni, nj))
        a["pn"] = 0.5 + 0.1 * rng.random((ni, nj))
        a["Hz"] = 1.0 + rng.random((ni, nj, N))
        a["z_w"][:, :, 1:] = np.cumsum(a["Hz"], axis=2)
        a["z_w"] -= a["z_w"][:, :, -1:] - 0.1 * rng.random((ni, nj, 1))
        for k in ("rho", "W", "u", "v"):
            a[k] = 0.3 * rng.standard_normal(a[k].shape)
        a["W"] *= 0.2
        a["t"] = [rng.standard_normal((ni, nj, N)) for _ in range(NT)]
    g = fu.Grid(b, masking, dt, **a)
    if ewp:
        fill_periodic(g)
    return g


def fill_periodic(g):
    o = -g.LBi
    for A in [g.pm, g.pn, g.rmask, g.Hz, g.rho, g.z_w, g.W, g.u, g.v] + g.t:
        for i in range(g.LBi, 1):
            A[i + o] = A[i + g.Lm + o]
        for i in range(g.Lm + 1, g.UBi + 1):
            A[i + o] = A[i - g.Lm + o]


def blank(g, n):
    return np.zeros((g.NT + 10, NFT + 1, n), order="F"), np.zeros(n, dtype=bool)


def tinfo(n, tstr=1.0e30, x=1.0, y=1.0, z=1.0):
    T = np.zeros((10, n), order="F")
    T[fu.itstr], T[fu.ixgrd], T[fu.iygrd], T[fu.izgrd] = tstr, x, y, z
    return T


NFL0 = (2, 3, 4, 0, 1)                      # nfm3, nfm2, nfm1, nf, nfp1 of initial.F:146-149


def rot(nfl, k=1):
    return tuple((v + k) % (NFT + 1) for v in nfl)


# ------------------------------------------------------------------------------------------- interpolation --
def test_a_linear_field_is_reproduced_exactly():
    g = make_grid()
    g.pm[:] = 1.0
    g.pn[:] = 1.0
    o = 2
    i = np.arange(g.LBi, g.UBi + 1, dtype=float)[:, None, None]
    j = np.arange(g.LBj, g.UBj + 1, dtype=float)[None, :, None]
    kr = np.arange(1, g.N + 1, dtype=float)[None, None, :]
    kw = np.arange(0, g.N + 1, dtype=float)[None, None, :]
    f = lambda x, y, z: 3.0 * x - 2.0 * y + 5.0 * z + 1.0
    rho = f(i, j, kr - 0.5)
    u = f(i - 0.5, j, kr - 0.5)
    v = f(i, j - 0.5, kr - 0.5)
    w = f(i, j, kw)
    for x, y, z in [(3.25, 2.5, 1.75), (7.0, 4.125, 3.5), (10.875, 6.75, 2.0), (1.5, 1.5, 4.25)]:
        want = f(x, y, z)
        assert fu.interp(g, fu.r3dvar, True, rho, 1, x, y, z) == want
        assert fu.interp(g, -fu.u3dvar, True, u, 1, x, y, z) == want
        assert fu.interp(g, -fu.v3dvar, True, v, 1, x, y, z) == want
        assert fu.interp(g, fu.w3dvar, True, w, 0, x, y, z) == want
        assert fu.interp(g, -fu.w3dvar, True, w, 0, x, y, z) == want          # 2 pm pn / (Hz + Hz) = 1
        assert fu.interp(g, fu.r2dvar, False, rho[:, :, 0], 1, x, y, z) == f(x, y, 0.5)
    assert o == -g.LBi


def test_slope_multipliers():
    """u: the mean of pm over the two rho-points of the face; W: 2 pm pn / (Hz(khm) + Hz(khp))"""
    g = make_grid()
    g.pm[:] = 0.25
    g.pn[:] = 0.5
    g.Hz[:] = 4.0
    g.u[:] = 8.0
    g.v[:] = 8.0
    g.W[:] = 16.0
    assert fu.interp(g, -fu.u3dvar, True, g.u, 1, 4.3, 3.3, 2.2) == pytest.approx(2.0, abs=1e-15)
    assert fu.interp(g, -fu.v3dvar, True, g.v, 1, 4.3, 3.3, 2.2) == pytest.approx(4.0, abs=1e-15)
    assert fu.interp(g, -fu.w3dvar, True, g.W, 0, 4.25, 3.5, 2.5) == 16.0 * 2.0 * 0.25 * 0.5 / 8.0


def test_normal_velocity_is_zero_on_the_perimeter_of_a_land_cell_and_rho_ignores_land():
    g = make_grid(masking=True)
    o = 2
    il, jl = 5, 4
    g.rmask[il + o, jl + o] = 0.0
    g.u[:] = 1.0
    g.v[:] = 1.0
    g.u[il + o, jl + o] = g.u[il + 1 + o, jl + o] = 0.0                       # umask
    g.v[il + o, jl + o] = g.v[il + o, jl + 1 + o] = 0.0                       # vmask
    g.rho[:] = 7.0
    g.rho[il + o, jl + o] = 1.0e6
    for s in (0.0, 0.125, 0.5, 0.875):
        y = jl - 0.5 + s
        assert fu.interp(g, -fu.u3dvar, True, g.u, 1, il - 0.5, y, 2.5) == 0.0      # west side
        assert fu.interp(g, -fu.u3dvar, True, g.u, 1, il + 0.5, y, 2.5) == 0.0      # east side
        x = il - 0.5 + s
        assert fu.interp(g, -fu.v3dvar, True, g.v, 1, x, jl - 0.5, 2.5) == 0.0      # south side
        assert fu.interp(g, -fu.v3dvar, True, g.v, 1, x, jl + 0.5, 2.5) == 0.0      # north side
    # along the coast the tangential velocity is the water value, not diluted by the land point
    assert fu.interp(g, -fu.v3dvar, True, g.v, 1, il - 0.75, jl + 0.25, 2.5) == 0.5
    # without the halo rule the bilinear form leaks: the same point unmasked
    gu = make_grid(masking=False)
    gu.u[:] = g.u
    assert fu.interp(gu, -fu.u3dvar, True, gu.u, 1, il - 0.5, jl + 0.25, 2.5) == 0.25 * 0.5
    for x, y in [(il - 0.25, jl - 0.25), (il + 0.5, jl + 0.25), (il - 0.75, jl + 0.5)]:
        assert fu.interp(g, fu.r3dvar, True, g.rho, 1, x, y, 2.25) == 7.0
        assert fu.interp(g, fu.r3dvar, False, g.rho, 1, x, y, 2.25) > 7.0           # Gmask: not masked
    g.rmask[:] = 0.0
    assert fu.interp(g, fu.r3dvar, True, g.rho, 1, 3.5, 3.5, 2.25) == 0.0           # all land: :277-279


# ------------------------------------------------------------------------------------------------ the step --
def test_uniform_flow_moves_a_float_by_u_pm_dt_per_step():
    """A history consistent with uniform motion advances by exactly u pm dt grid units.  On the step after its release
    a float has all five positions equal to the release position (step_floats.F:719-725), so the Hamming corrector
    9/8 x(nf) - 1/8 x(nfm2) + dt (3/8 + 6/8 - 3/8) r gives 3/4 u pm dt there, and 27/32 + 3/4 on the one after."""
    g = make_grid()
    g.u[:] = 0.25
    d = 0.25 * 0.5 * 2.0
    T, bd = blank(g, 2)
    Ti = tinfo(2, tstr=[1e30, 0.0], x=3.0, y=4.0, z=2.5)
    nfl = NFL0
    nfm3, nfm2, nfm1, nf, nfp1 = nfl
    for lev, back in ((nfm3, 3), (nfm2, 2), (nfm1, 1), (nf, 0)):
        T[fu.ixgrd - 1, lev, 0], T[fu.iygrd - 1, lev, 0], T[fu.izgrd - 1, lev, 0] = 5.0 - back * d, 4.0, 2.5
        T[fu.ixrhs - 1, lev, 0] = 0.125
    bd[0] = True
    R = fu.one_tile(g, T, bd)
    Ft, Fz = np.array([1, 1]), np.zeros(2)
    xs = []
    for k in range(4):
        fu.step_floats(R, 1, nfl, k * g.dt, Ft, Ti, Fz)
        xs.append(R[0].track[fu.ixgrd - 1, nfl[4]].copy())
        assert R[0].track[fu.ixrhs - 1, nfl[4], 0] == 0.125
        nfl = rot(nfl)
    assert [x[0] for x in xs] == [5.0 + d, 5.0 + 2 * d, 5.0 + 3 * d, 5.0 + 4 * d]
    assert [x[1] for x in xs[:3]] == [3.0, 3.0 + 0.75 * d, 3.0 + (27.0 / 32.0 + 0.75) * d]
    assert R[0].bounded.all()
    # the outputs: 2-D coordinates xc = 2 i, yc = 2 j, depth from z_w = k - N
    tr = R[0].track
    assert tr[fu.iflon - 1, nfl[3], 0] == 2.0 * (5.0 + 4 * d) and tr[fu.iflat - 1, nfl[3], 0] == 8.0
    assert tr[fu.idpth - 1, nfl[3], 0] == 2.5 - g.N


def test_geopotential_float_sits_at_Fz0_and_isobaric_follows_the_surface():
    g = make_grid(N=5)
    g.z_w[:] = (-100.0 + 20.0 * np.arange(6))[None, None, :] + 2.0 * np.arange(6)[None, None, :] / 5.0   # surface at +2
    T, bd = blank(g, 3)
    Ti = tinfo(3, tstr=0.0, x=[3.5, 4.25, 6.0], y=[2.5, 3.0, 5.5], z=0.5)
    R = fu.one_tile(g, T, bd)
    Ft, Fz = np.array([3, 2, 1]), np.array([-50.0, -30.0, 0.0])
    nfl = NFL0
    for k in range(3):
        fu.step_floats(R, 1, nfl, k * g.dt, Ft, Ti, Fz)
        nfl = rot(nfl)
    tr, last = R[0].track, nfl[3]
    assert abs(tr[fu.idpth - 1, last, 0] - (-50.0)) < 1e-12
    assert abs(tr[fu.idpth - 1, last, 1] - (2.0 - 30.0)) < 1e-12
    assert tr[fu.izgrd - 1, last, 0] == pytest.approx((-50.0 + 100.0) / 20.4, abs=1e-12)
    assert tr[fu.izgrd - 1, last, 2] == 0.5                                   # Lagrangian in resting water
    # no level brackets the float: izgrd stays untouched
    Fz[0] = -500.0
    tr[fu.izgrd - 1, nfl[4], 0] = 1.25              # what the slot of nfp1 happens to hold
    fu.step_floats(R, 1, nfl, 3 * g.dt, Ft, Ti, Fz)
    assert R[0].track[fu.izgrd - 1, nfl[4], 0] == 1.25


def _history(g, n, x, y, z, nfl):
    T, bd = blank(g, n)
    for lev in range(NFT + 1):
        T[fu.ixgrd - 1, lev], T[fu.iygrd - 1, lev], T[fu.izgrd - 1, lev] = x, y, z
    bd[:] = True
    return T, bd


def test_reflection_at_the_surface_and_at_the_bottom():
    g = make_grid(N=5)
    g.W[:] = 1.0                                  # izrhs = W 2 pm pn / (Hz + Hz) = 0.25 per second
    nfl = NFL0
    T, bd = _history(g, 3, [4.0, 5.0, 6.0], 3.0, [4.875, 0.125, 2.0], nfl)
    T[fu.izrhs - 1, :, 0] = 0.25
    T[fu.izrhs - 1, :, 1] = -0.25
    T[fu.izgrd - 1, nfl[1], :] += 0.0625          # one level differs, to see that every level is reflected
    g.W[5 + 2] = -1.0                             # sinking in the column of the second float
    R = fu.one_tile(g, T, bd)
    fu.step_floats(R, 1, nfl, 0.0, np.array([1, 1, 1]), tinfo(3), np.zeros(3))
    tr = R[0].track
    for lev in nfl[:4]:
        assert tr[fu.izgrd - 1, lev, 0] == 10.0 - T[fu.izgrd - 1, lev, 0]
        assert tr[fu.izgrd - 1, lev, 1] == -T[fu.izgrd - 1, lev, 1]
        assert tr[fu.izgrd - 1, lev, 2] == T[fu.izgrd - 1, lev, 2]
    assert 0.0 < tr[fu.izgrd - 1, nfl[4], 1] < 1.0 and 4.0 < tr[fu.izgrd - 1, nfl[4], 0] < 5.0


@pytest.mark.parametrize("ewp", [True, False])
def test_periodic_shift_against_loss_at_a_closed_edge(ewp):
    g = make_grid(ewp=ewp)
    g.u[:] = 0.5
    g.u[: 6 + 2] = -0.5                            # westward in the western half
    nfl = NFL0
    T, bd = _history(g, 3, [12.375, 0.625, 6.0], 3.0, 2.5, nfl)
    T[fu.ixrhs - 1, :, 0] = T[fu.ixrhs - 1, :, 2] = 0.25
    T[fu.ixrhs - 1, :, 1] = -0.25
    R = fu.one_tile(g, T, bd)
    fu.step_floats(R, 1, nfl, 0.0, np.array([1, 1, 1]), tinfo(3), np.zeros(3))
    tr, b = R[0].track, R[0].bounded
    # all five positions equal: the corrector moves the float by 3/4 dt r = 0.375
    if ewp:
        assert b.all()
        assert tr[fu.ixgrd - 1, nfl[4], 0] == 12.75 - 12.0 and tr[fu.ixgrd - 1, nfl[4], 1] == 12.0 + 0.25
        for lev in nfl[:4]:                       # all five levels move with it
            assert tr[fu.ixgrd - 1, lev, 0] == 0.375 and tr[fu.ixgrd - 1, lev, 1] == 12.625
    else:
        assert list(b) == [False, False, True]
        assert tr[fu.ixgrd - 1, nfl[4], 0] == 12.75 and tr[fu.ixgrd - 1, nfl[4], 1] == 0.25
        for v in (fu.ixrhs, fu.iflon, fu.idpth, fu.ifden, fu.ifden + g.NT):
            assert tr[v - 1, nfl[4], 0] == 1.0e37 and tr[v - 1, nfl[4], 2] != 1.0e37
    assert tr[fu.ixgrd - 1, nfl[4], 2] == 6.375


def test_release_window_and_release_outside_the_grid():
    g = make_grid()
    time, h = 10.0, 0.5 * g.dt
    tstr = [time - h, np.nextafter(time - h, -1.0), time + h, np.nextafter(time + h, -1.0), time, time]
    Ti = tinfo(6, tstr=tstr, x=[3.0, 3.0, 3.0, 3.0, 12.75, 3.0], y=[2.0, 2.0, 2.0, 2.0, 2.0, 0.25], z=1.5)
    T, bd = blank(g, 6)
    R = fu.one_tile(g, T, bd)
    fu.step_floats(R, 1, NFL0, time, np.ones(6, dtype=int), Ti, np.zeros(6))
    assert list(R[0].bounded) == [True, False, False, True, False, False]
    tr = R[0].track
    assert (tr[fu.ixgrd - 1, :, 0] == 3.0).all() and (tr[fu.izgrd - 1, :, 3] == 1.5).all()
    assert not tr[:, :, 4].any() and not tr[:, :, 5].any()                    # out of the grid: :728-733
    assert tr[fu.ixrhs - 1, NFL0[4], 1] == 1.0e37                              # not yet released: spval


# ---------------------------------------------------------------------------------- ownership and collection --
def _drifting(g, n, seed):
    rng = np.random.default_rng(seed)
    x = 0.6 + (g.Lm - 0.2) * rng.random(n)
    y = 3.0 + (g.Mm - 5.5) * rng.random(n)
    z = 0.5 + (g.N - 1.0) * rng.random(n)
    Ft = 1 + np.arange(n) % 3
    Ti = tinfo(n, tstr=np.where(np.arange(n) % 4 == 3, 1.0e30, 0.0), x=x, y=y, z=z)
    return Ft, Ti, -5.0 * rng.random(n)


@pytest.mark.parametrize("ntI,ntJ,ewp", [(2, 2, False), (4, 1, True), (2, 2, True)])
def test_tiles_with_collection_equal_one_tile_bit_for_bit(ntI, ntJ, ewp):
    g = make_grid(Lm=16, Mm=8, ewp=ewp, seed=3)
    g.u += 0.35                                     # a drift to the east: floats cross the seams at i = 4.5, 8.5, 12.5
    g.v *= 0.5
    g.v += 0.1
    if ewp:
        fill_periodic(g)
    n = 40
    Ft, Ti, Fz = _drifting(g, n, 5)
    Ti[fu.ixgrd, 0], Ti[fu.iygrd, 0] = 8.4, 4.45       # next to both seams of the 2x2 split
    Ti[fu.ixgrd, 1], Ti[fu.ixgrd, 2] = 16.3, 0.7       # next to the periodic seam
    if not ewp:                                     # closed: keep the floats away from the edges they would be lost at
        Ti[fu.ixgrd] = 1.0 + 0.75 * (Ti[fu.ixgrd] - 0.6)
    T, bd = blank(g, n)
    one = fu.one_tile(g, T, bd)
    many = fu.split(g, ntI, ntJ, T, bd)
    assert len(many) == ntI * ntJ and many[-1].Xend == 16.5 and many[-1].Yend == 8.5
    nfl = NFL0
    owners = set()
    crossed_periodic = False
    for k in range(6):
        fu.step_floats(one, 1, nfl, k * g.dt, Ft, Ti, Fz)
        x_before = many[0].track[fu.ixgrd - 1, nfl[3]].copy()
        fu.step_floats(many, ntI, nfl, k * g.dt, Ft, Ti, Fz)
        for r, R in enumerate(many):
            assert np.array_equal(R.track, one[0].track), (k, r)
            assert np.array_equal(R.bounded, one[0].bounded), (k, r)
        x_after = one[0].track[fu.ixgrd - 1, nfl[4]]
        owners.add(int(x_after[0] + 0.5 - 1) // (16 // ntI))
        crossed_periodic |= bool(((x_before > 12.0) & (x_after < 4.0) & one[0].bounded).any())
        nfl = rot(nfl)
    assert one[0].bounded.sum() == n - n // 4 and len(owners) > 1    # nobody lost; float 0 changed its owner
    assert crossed_periodic == ewp
    assert np.abs(one[0].track[fu.ixrhs - 1]).max() > 0.0


# --------------------------------------------------------------------------------------------------- the ABI --
NAMES = ["roms_hip_set_floats", "roms_hip_floats_put", "roms_hip_floats_get", "roms_hip_step_floats"]


def test_entries_exist_in_header_library_fortran_module_and_python():
    lib = hip.load()
    header = open(os.path.join(ROOT, "include", "roms_hip.h")).read()
    fsrc = open(os.path.join(ROOT, "roms_trunk_mgh_amd", "fortran", "roms_hip_mod.F90")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in hip.DECLARED_SYMBOLS
        assert re.search(r"FUNCTION %s\b.*BIND\(C, name='%s'\)" % (name, name), fsrc, flags=re.S), name
        assert re.search(r"PUBLIC ::.*\b%s\b" % name, fsrc), name
    assert "step_floats.F:80-1053" in header and "interp_floats.F:56-541" in header
    assert (floats.itstr, floats.ixgrd, floats.izgrd, floats.idpth, floats.izrhs, floats.ifden) == (0, 1, 3, 6, 9, 10)
    assert floats.NFV(2) == 12 and floats.NFT == 4 and floats.ifTvar(1) == 11
    assert floats.INITIAL_LEVELS == dict(nfp1=1, nf=0, nfm1=4, nfm2=3, nfm3=2)
    f = floats.Floats(make_grid().b, [1], tinfo(1), [0.0], np.zeros((17, 13)), np.zeros((17, 13)))
    assert f.nfl() == NFL0
    f.rotate()
    assert f.nfl() == rot(NFL0) and f.track_shape() == (12, 5, 1)


def test_refusals_that_need_no_device():
    lib = hip.load()
    assert hip.RomsHip._live is None
    lib.roms_hip_finalize()
    s = abi.StepIdx(iic=1, ntfirst=1, nstp=1, nnew=2, nrhs=1, kstp=1, krhs=1, knew=2, iif=1, predictor_2d_step=0)
    one = np.zeros(1)
    ione = np.ones(1, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = lib.roms_hip_set_floats(1, ione.ctypes.data_as(ip), np.zeros(10).ctypes.data_as(dp), one.ctypes.data_as(dp),
                                 one.ctypes.data_as(dp), one.ctypes.data_as(dp))
    assert rc != 0 and b"come first" in lib.roms_hip_last_error()
    for bad in [(0, 1, 2, 3, 3), (1, 2, 3, 4, 5), (0, 1, 2, 3, -1)]:
        assert lib.roms_hip_step_floats(C.byref(s), 0.0, (C.c_int * 5)(*bad)) != 0
        assert b"not a permutation of 0..4" in lib.roms_hip_last_error()
    assert lib.roms_hip_step_floats(C.byref(s), 0.0, (C.c_int * 5)(*NFL0)) == 0        # no floats: nothing to do
    t = np.zeros(60)
    assert lib.roms_hip_floats_put(t.ctypes.data, t.size, ione.ctypes.data, 1) != 0
    assert b"not initialised" in lib.roms_hip_last_error() or b"none set" in lib.roms_hip_last_error()
    assert lib.roms_hip_floats_get(t.ctypes.data, t.size, ione.ctypes.data, 1) != 0
    assert b"not initialised" in lib.roms_hip_last_error() or b"none set" in lib.roms_hip_last_error()
