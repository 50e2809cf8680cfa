"""CPU: tidal boundary forcing (SSH_TIDES, UV_TIDES; roms_hip_set_tides / roms_hip_tides) without a GPU.

Known answers that pin the numpy restatement tests/tides_util.py, which stands in for the reference vector set_tides
cannot have (it USEs mod_tides and the netCDF layer); none of them depends on anyone's reading of the loops.  Then the
restatement on 2x2 and 4x1 partitions against one tile, the refusals that need no device, and a quasi-static run of the
CPU oracle under Main3D with the restated boundary arrays written before each step."""
import math

import numpy as np
import pytest

import tides_util as tu
from roms_trunk_mgh_amd import abi, ana, hip, main3d, tides

DIMS = dict(Lm=12, Mm=10, N=4, EWperiodic=False)
T0 = 44714.0


def basin(ntI=1, ntJ=1, tile=0, mask=None, table=tu.OPEN, **ov):
    st = ana.make_tile("UPWELLING", ntI, ntJ, tile, overrides=dict(DIMS, **ov), mask=mask)
    return tu.open_all(st, table)


def one(st, ssh=None, uv=None, T=T0, **kw):
    """one constituent from scalars: ssh = (amp, phase), uv = (angle, phase, major, minor)"""
    full = lambda v: np.full((st.ni, st.nj, 1), float(v), order="F")
    args = {}
    if ssh:
        args.update(SSH_Tamp=full(ssh[0]), SSH_Tphase=full(ssh[1]))
    if uv:
        args.update(UV_Tangle=full(uv[0]), UV_Tphase=full(uv[1]), UV_Tmajor=full(uv[2]), UV_Tminor=full(uv[3]))
    return tides.Tides(st.b, [T], **args, **kw)


def test_zero_phase_at_whole_periods_gives_the_amplitude():
    st = basin()
    b = st.b
    td = one(st, ssh=(0.7, 0.0), tide_start=2.0)
    for k in (0, 1, 5):
        E, _, _ = tu.harmonics(st, td, 2.0 * 86400.0 + k * T0)
        R = (st.I(b.IstrR, b.IendR), st.J(b.JstrR, b.JendR))
        assert np.allclose(E[R], 0.7, rtol=0, atol=1e-12 * (1 + k)) and (k or np.array_equal(E[R], np.full_like(E[R], 0.7)))
    tu.set_tides(st, td, 2.0 * 86400.0)
    w = tu.written_points(st, td)["zeta_bry"]
    assert np.array_equal(st["zeta_bry"][w], np.full(int(w.sum()), 0.7))
    assert w.sum() == 2 * (b.Lm + b.Mm) and not st["zeta_bry"][~w].any()          # four edges without the corners
    assert not st["ubar_bry"].any() and not st["vbar_bry"].any()                  # no UV_TIDES: currents untouched


def test_ellipse_along_the_grid_and_a_quarter_turn():
    st = basin()
    b = st.b
    ang = 0.3 + 0.01 * np.arange(st.ni)[:, None] * np.ones((1, st.nj))
    time = 0.4 * 86400.0
    cs = math.cos(2.0 * tu.PI * time / T0 - 0.25)
    U = (st.I(b.Istr, b.IendR), st.J(b.JstrR, b.JendR))
    V = (st.I(b.IstrR, b.IendR), st.J(b.Jstr, b.JendR))
    for turn, (uw, vw) in ((0.0, (0.2 * cs, 0.0)), (0.5 * math.pi, (0.0, 0.2 * cs))):
        td = one(st, uv=(0.0, 0.25, 0.2, 0.0), angler=ang)
        td.arr["UV_Tangle"][:, :, 0] = ang + turn                                 # angle = angler (+ a quarter turn)
        _, Ut, Vt = tu.harmonics(st, td, time)
        assert np.allclose(Ut[U], uw, rtol=0, atol=1e-16 + 2e-17 * (turn > 0)) and np.allclose(Vt[V], vw, rtol=0, atol=2e-17)
    # a minor axis alone: the current a quarter period later, turned by a quarter turn
    td = one(st, uv=(0.0, 0.25, 0.0, 0.1))
    _, Ut, Vt = tu.harmonics(st, td, time)
    assert np.allclose(Ut[U], 0.0, atol=1e-17) and np.allclose(Vt[V], 0.1 * math.sin(2.0 * tu.PI * time / T0 - 0.25), rtol=0, atol=1e-16)


def test_ramp_is_tanh_and_nonpositive_periods_are_skipped():
    st = basin()
    b = st.b
    R = (st.I(b.IstrR, b.IendR), st.J(b.JstrR, b.JendR))
    td = one(st, ssh=(1.0, 0.0), ramp=True, dstart=0.5)
    for days in (0.5, 0.75, 2.0):
        time = days * 86400.0
        E, _, _ = tu.harmonics(st, td, time)
        want = math.tanh(days - 0.5) * math.cos(2.0 * tu.PI * time / T0)
        assert np.allclose(E[R], want, rtol=0, atol=1e-15)
    full = lambda v: np.full((st.ni, st.nj, 3), float(v), order="F")
    td3 = tides.Tides(st.b, [T0, 0.0, -5.0], SSH_Tamp=full(0.3), SSH_Tphase=full(0.0))
    E, _, _ = tu.harmonics(st, td3, 0.0)
    assert np.array_equal(E[R], np.full_like(E[R], 0.3))                          # one of three counts
    td2 = tides.Tides(st.b, [T0, 43200.0, 43200.0], NTC=2, SSH_Tamp=full(0.3), SSH_Tphase=full(0.0))
    E, _, _ = tu.harmonics(st, td2, 0.0)
    assert np.array_equal(E[R], np.full_like(E[R], 0.6))                          # NTC of MTC


def test_land_points_are_zero():
    st = basin(mask="island")
    st["rmask"][:, st.J(0)] = st["rmask"][:, st.J(1)] = 1.0
    for i, j in ((0, 3), (1, 3), (5, 0), (5, 1), (13, 6), (12, 6), (7, 11), (7, 10)):       # land touching each edge
        st["rmask"][st.I(i), st.J(j)] = 0.0
    ana.set_masks(st, st["rmask"].copy())
    assert st.p.masking == 1
    td = ana.analytic_tides(st, ntc=3)
    for time in (0.3 * 86400.0, 200.25 * 86400.0):
        E, U, V = tu.harmonics(st, td, time)
        assert not E[st["rmask"] == 0.0].any() and not U[st["umask"] == 0.0].any() and not V[st["vmask"] == 0.0].any()
        assert np.abs(E).max() > 0.1 and np.abs(U).max() > 0.01 and np.abs(V).max() > 0.01
    tu.set_tides(st, td, 0.3 * 86400.0)
    b = st.b
    assert st["ubar_bry"][st.I(b.Istr), st.J(3)] == 0.0 and st["vbar_bry"][st.I(5), st.J(b.Jstr)] == 0.0
    assert st["zeta_bry"][st.I(b.Istr - 1), st.J(3)] == 0.0 and st["zeta_bry"][st.I(b.Istr - 1), st.J(5)] != 0.0


def test_add_options_write_base_plus_tide_without_accumulating():
    st = basin()
    rng = np.random.default_rng(2)
    base = {n: np.asfortranarray(rng.standard_normal((st.ni, st.nj))) for n in ("zeta_base", "ubar_base", "vbar_base")}
    plain = ana.analytic_tides(st, ntc=2)
    added = ana.analytic_tides(st, ntc=2, add_fsobc=True, add_m2obc=True, **base)
    ref = st.copy()
    time = 1.3 * 86400.0
    tu.set_tides(ref, plain, time)
    w = tu.written_points(st, plain)
    for _ in range(3):                                                            # repeated calls: no accumulation
        tu.set_tides(st, added, time)
        for name, bn in (("zeta_bry", "zeta_base"), ("ubar_bry", "ubar_base"), ("vbar_bry", "vbar_base")):
            assert np.array_equal(st[name][w[name]], (base[bn] + ref[name])[w[name]]) and not st[name][~w[name]].any()


@pytest.mark.parametrize("ntI,ntJ", [(2, 2), (4, 1)])
@pytest.mark.parametrize("masked", [False, True])
def test_tiled_restatement_equals_one_tile_on_every_written_point(ntI, ntJ, masked):
    kw = dict(mask="island") if masked else {}
    whole = basin(**kw)
    time = 200.25 * 86400.0
    tu.set_tides(whole, ana.analytic_tides(whole, ntc=3, ramp=True, dstart=199.0), time)
    gb = whole.b
    seen = {n: np.zeros((whole.ni, whole.nj), dtype=bool) for n in ("zeta_bry", "ubar_bry", "vbar_bry")}
    for tile in range(ntI * ntJ):
        st = basin(ntI, ntJ, tile, **kw)
        td = ana.analytic_tides(st, ntc=3, ramp=True, dstart=199.0)
        tu.set_tides(st, td, time)
        b = st.b
        for name, w in tu.written_points(st, td).items():
            ii, jj = np.nonzero(w)
            gi, gj = ii + b.LBi - gb.LBi, jj + b.LBj - gb.LBj
            assert np.array_equal(st[name][ii, jj], whole[name][gi, gj]), (name, tile)
            seen[name][gi, gj] = True
    for name, w in tu.written_points(whole, ana.analytic_tides(whole, ntc=3)).items():
        assert np.array_equal(seen[name], w), name                                # together they write what one tile writes


def test_conditions_follow_acquire_and_periodic_sides_are_skipped():
    table = dict(tu.OPEN, zeta="Cha", ubar="Fla", vbar="Gra")                     # vbar does not acquire: no currents
    st = basin(table=table)
    td = ana.analytic_tides(st, ntc=1)
    tu.set_tides(st, td, 5000.0)
    assert st["zeta_bry"].any() and not st["ubar_bry"].any() and not st["vbar_bry"].any()
    st = basin(table=dict(tu.OPEN, zeta="Cha", ubar="Red", vbar="Red"))           # Red acquires nothing (no FSOBC_REDUCED)
    tu.set_tides(st, td, 5000.0)
    assert not st["zeta_bry"].any()
    ch = ana.make_tile("UPWELLING", overrides=dict(DIMS, EWperiodic=True))
    tu.open_all(ch, sides=("south", "north"))
    tu.set_tides(ch, ana.analytic_tides(ch, ntc=1), 5000.0)
    b = ch.b
    own = ch.I(b.IstrR, b.IendR)
    assert ch["zeta_bry"][own, ch.J(b.Jstr - 1)].all() and not ch["zeta_bry"][:, ch.J(b.Jstr, b.Jend)].any()


def test_refusals_that_need_no_device():
    st = basin()
    with pytest.raises(ValueError, match="SSH_Tamp has shape"):
        tides.Tides(st.b, [T0, T0], SSH_Tamp=np.zeros((st.ni, st.nj, 1)), SSH_Tphase=np.zeros((st.ni, st.nj, 2)))
    with pytest.raises(ValueError, match="angler has shape"):
        tides.Tides(st.b, [T0], angler=np.zeros((st.ni, st.nj, 1)))
    lib = hip.load()
    assert hip.RomsHip._live is None
    td = ana.analytic_tides(st, ntc=1)
    assert lib.roms_hip_set_tides(*td.c_args()) != 0 and b"come first" in lib.roms_hip_last_error()
    assert lib.roms_hip_tides(0.0) != 0 and b"not initialised" in lib.roms_hip_last_error()
    assert {"roms_hip_set_tides", "roms_hip_tides"} <= set(hip.DECLARED_SYMBOLS)
    assert len(td.c_args()) == len(tides.NO_TIDES) == len(lib.roms_hip_set_tides.argtypes)


def test_quasi_static_basin_follows_the_imposed_elevation():
    """A flat basin without rotation, Cha / Fla on all four sides, one constituent of uniform amplitude whose period is
    long against the basin's seiche period, phase pi/2 so that the forcing starts at zero: at T/4 the interior mean free
    surface is the imposed amplitude, within (omega L / c)^2 (the inertia of the response) + T_seiche / T (what is left
    of the start-up seiche), both from the grid's own numbers."""
    import oracle
    st = ana.make_tile("UPWELLING", overrides=dict(EWperiodic=False, theta_s=0.0, theta_b=0.0))
    tu.open_all(st)
    H0, amp = 150.0, 0.05
    st["h"][:] = H0
    for name in ("f", "fomn", "sustr", "svstr", "bustr", "bvstr", "stflx", "btflx", "srflx", "ubar", "vbar", "u", "v", "zeta",
                 "Zt_avg1", "rdrag", "rdrag2"):
        st[name][:] = 0.0
    st["t"][:, :, :, :, 0] = 14.0
    st["t"][:, :, :, :, 1] = 35.0
    b, p = st.b, st.p
    L = max(float((1.0 / st["pm"][st.I(1, b.Lm), st.J(1)]).sum()), float((1.0 / st["pn"][st.I(1), st.J(1, b.Mm)]).sum()))
    c = math.sqrt(p.g * H0)
    Tseiche = 2.0 * L / c
    nsteps = int(round(6.0 * Tseiche / p.dt))                                     # T/4 = 6 seiche periods
    T = 4.0 * nsteps * p.dt
    bound = (2.0 * math.pi / T * L / c) ** 2 + Tseiche / T
    td = ana.analytic_tides(st, ntc=1, uv=False, periods=[T], amp=[amp])
    td.arr["SSH_Tphase"][:] = 0.5 * math.pi
    m = main3d.Main3D(tu.TidalOracle(oracle.Oracle(st)), tides=td)
    m.initial()
    m.run(nsteps)
    assert st["zeta_bry"][st.I(b.Istr - 1), st.J(5)] == pytest.approx(amp * math.sin(2.0 * math.pi * (nsteps - 1) * p.dt / T), abs=1e-15)
    mean = float(st.interior("zeta")[:, :, m.indx1 - 1].mean())
    print(f"quasi-static: mean {mean:.6f} of {amp}, error {abs(mean - amp) / amp:.4f}, bound {bound:.4f}, {nsteps} steps")
    assert np.isfinite(st["zeta"]).all() and bound < 0.1
    assert abs(mean - amp) <= bound * amp, (mean, amp, bound)
