"""-m gpu: tidal boundary forcing on the device (SSH_TIDES, UV_TIDES: roms_hip_set_tides, roms_hip_tides,
csrc/k_set_tides.hip) and the SSH_TIDES-without-UV_TIDES boundary value of the Flather / Shchepetkin conditions
(k_edge_bc).

set_tides.F needs mod_tides and the I/O layer, so the reference cannot make a vector for it: the yardstick is the numpy
restatement tests/tides_util.py, whose known answers tests/test_tides.py checks without a GPU.
  1. bit for bit where no transcendental differs (time = tide_start, zero phases, UV_Tangle = angler): all three
     boundary arrays on the whole allocated array, sentinel-filled, so that the corners and every non-edge point are
     seen unchanged
  2. general times and phases: |device - numpy| <= 1e-13 x the sum of the constituents' largest amplitudes (for the
     currents: major + minor), the margin tests/test_gpu_kernels.py::test_ana_srflux gives device sin / cos
  3. the SSH-only boundary value, one barotropic call, bit for bit against the oracle fed with the numpy value.  Only
     the branch with acquired free-surface data can be reached: Fla / Shc on ubar or vbar set the free surface's acquire
     themselves (inp_decode.F:1626-1629, :1652-1655), in the reference as here
  4. seven steps under Main3D(tides=) against the oracle fed by the restatement each step: 1e-10 on every field
  5. tilings 2x2 and 4x1 over the relay and one tile in RCCL loopback against one tile, bit for bit
  6. the refusals"""
import numpy as np
import pytest

import curv_util as cv
import tides_util as tu
import tiling_util
import util
from roms_trunk_mgh_amd import abi, ana, hip, main3d, tides
from test_gpu_kernels import _idx2d

pytestmark = pytest.mark.gpu
DIMS = dict(Lm=12, Mm=10, N=4, EWperiodic=False)
CURV = dict(Lm=66, Mm=9, N=5, EWperiodic=False)               # the shape of tests/test_gpu_curvilinear.py
BRY = ("zeta_bry", "ubar_bry", "vbar_bry")
SENTINEL = 777.25
DAY = 86400.0


def coast(st):
    """land touching each of the four edges (and the island of ana.island_mask)"""
    rm = st["rmask"].copy()
    b = st.b
    for i, j in ((0, 3), (1, 3), (5, 0), (5, 1), (b.Lm + 1, 6), (b.Lm, 6), (7, b.Mm + 1), (7, b.Mm)):
        rm[st.I(i), st.J(j)] = 0.0
    ana.set_masks(st, rm)
    assert st.p.masking == 1
    return st


def basin(kind="water", table=tu.OPEN):
    if kind == "curv":
        st = ana.make_tile("UPWELLING", perturb=1.0, overrides=dict(CURV))
        cv.curvilinear(st)
        st.angler = np.asfortranarray(0.4 * cv.wave(st, 2, 1.1, 0.7, 3, 0.9, 1.9))
    else:
        st = ana.make_tile("UPWELLING", perturb=1.0, overrides=dict(DIMS), mask="island" if kind == "land" else None)
        if kind == "land":
            coast(st)
        st.angler = None
    return tu.open_all(st, table)


def bases(st, add):
    rng = np.random.default_rng(3)
    mk = lambda: np.asfortranarray(rng.standard_normal((st.ni, st.nj)))
    kw = {}
    if add in ("fs", "both"):
        kw.update(add_fsobc=True, zeta_base=mk())
    if add in ("m2", "both"):
        kw.update(add_m2obc=True, ubar_base=mk(), vbar_base=mk())
    return kw


def device_bry(be, st, time):
    for name in BRY:
        st[name][:] = SENTINEL
    be.to_device(BRY)
    be.tides(time)
    be.to_host(BRY)
    return {name: st[name].copy() for name in BRY}


def numpy_bry(st, td, time):
    ref = st.copy()
    for name in BRY:
        ref[name][:] = SENTINEL
    tu.set_tides(ref, td, time)
    return ref


# ------------------------------------------------------------------------------------------ 1. bit for bit --
@pytest.mark.parametrize("add", [None, "fs", "m2"])
@pytest.mark.parametrize("kind", ["water", "land", "curv"])
@pytest.mark.parametrize("ntc", [1, 3])
def test_boundary_arrays_equal_the_restatement_bit_for_bit(ntc, kind, add):
    st = basin(kind)
    td = tu.exact_set(st, ntc, ntc + 1, angler=st.angler, **bases(st, add))
    assert td.MTC > td.NTC and (ntc == 1 or td.Tperiod[1] == 0.0)
    time = td.tide_start * DAY
    be = hip.RomsHip(st)
    try:
        be.set_tides(td)
        for _ in range(2):                                    # twice: base + tide, no accumulation
            got = device_bry(be, st, time)
        be.check_guards()
    finally:
        be.close()
    ref = numpy_bry(st, td, time)
    w = tu.written_points(st, td)
    b = st.b
    for name in BRY:
        assert np.array_equal(got[name], ref[name]), (name, float(np.abs(got[name] - ref[name]).max()))
        assert w[name].sum() >= 2 * (b.Lm + b.Mm) and (ref[name][~w[name]] == SENTINEL).all()
        # (with every sine zero Vwrk vanishes: vbar_bry is its base, or an exact zero)
        assert np.abs(ref[name][w[name]]).max() > 0.01 or (name == "vbar_bry" and add != "m2")
    for i, j in ((b.Istr - 1, b.Jstr - 1), (b.Iend + 1, b.Jstr - 1), (b.Istr - 1, b.Jend + 1), (b.Iend + 1, b.Jend + 1)):
        assert got["zeta_bry"][st.I(i), st.J(j)] == SENTINEL      # the four corner rho-points
    if kind == "land" and add is None:
        assert (ref["zeta_bry"][w["zeta_bry"]] == 0.0).any() and (ref["ubar_bry"][w["ubar_bry"]] == 0.0).any()


# ------------------------------------------------------------------------------ 2. general times and phases --
@pytest.mark.parametrize("kind", ["water", "land", "curv"])
def test_general_times_and_phases(kind):
    st = basin(kind)
    td = ana.analytic_tides(st, ntc=8, mtc=8, angler=st.angler, tide_start=0.1, ramp=True, dstart=0.0, **bases(st, "both"))
    td.Tperiod[5] = 0.0
    za, ua = tu.amp_bound(td)
    be = hip.RomsHip(st)
    worst = {}
    try:
        be.set_tides(td)
        for days in (0.3, 200.25):
            got = device_bry(be, st, days * DAY)
            ref = numpy_bry(st, td, days * DAY)
            w = tu.written_points(st, td)
            for name in BRY:
                d = float(np.abs(got[name] - ref[name]).max())
                worst[(name, days)] = d / (za if name == "zeta_bry" else ua)
                assert (got[name][~w[name]] == SENTINEL).all()
        be.check_guards()
    finally:
        be.close()
    print(kind, "largest |device - numpy| / sum of amplitudes:", worst)
    assert all(v <= 1e-13 for v in worst.values()), worst


# ------------------------------------------------------------------------------------ 3. SSH-only bry_val --
def _bc_state(code, uv_cor, kind):
    ov = dict(EWperiodic=False, Lm=12, Mm=10, N=4)
    st = util.prepared_state("UPWELLING", overrides=ov, mask="island" if kind != "water" else None, wet=kind == "wet")
    st.p = type(st.p).from_buffer_copy(st.p)
    st.p.uv_cor = uv_cor
    tu.open_all(st, dict(tu.OPEN, zeta="Che" if code == "Shc" else "Cha", ubar=code, vbar=code))
    rng = np.random.default_rng(4)
    for name in BRY:
        st[name][:] = 1.0e-2 * rng.standard_normal(st[name].shape)
    st["sustr"][:] = 1.0e-4 * rng.standard_normal(st["sustr"].shape)
    st["svstr"][:] = 1.0e-4 * rng.standard_normal(st["svstr"].shape)
    return st


@pytest.mark.parametrize("iif,pred", [(1, 1), (5, 1), (5, 0)])
@pytest.mark.parametrize("code,uv_cor,kind", [("Fla", 1, "water"), ("Fla", 0, "water"), ("Fla", 1, "land"), ("Shc", 1, "water"),
                                              ("Shc", 0, "land"), ("Shc", 1, "wet")])
def test_ssh_only_boundary_value(code, uv_cor, kind, iif, pred):
    import oracle
    st0 = _bc_state(code, uv_cor, kind)
    for sd in tu.SIDES:
        assert tu.acquire(st0.p, sd, "zeta")
    s = _idx2d(iif, pred, 7)
    know = s.krhs if (iif == 1 or pred) else s.kstp
    st_o, st_h, st_p, st_b = st0.copy(), st0.copy(), st0.copy(), st0.copy()
    ub, vb = tu.ssh_only_bry_val(st0, know)
    assert not np.array_equal(ub, st0["ubar_bry"]) and not np.array_equal(vb, st0["vbar_bry"])
    st_o["ubar_bry"][:] = ub
    st_o["vbar_bry"][:] = vb
    oracle.Oracle(st_o).call("step2d", s)
    oracle.Oracle(st_p).call("step2d", s)                     # the plain path: boundary data as they are
    td_ssh = ana.analytic_tides(st0, ntc=2, uv=False)
    td_both = ana.analytic_tides(st0, ntc=2)
    garbage = np.random.default_rng(9).standard_normal(st0["ubar_bry"].shape) * 1.0e3
    st_h["ubar_bry"][:] = garbage
    st_h["vbar_bry"][:] = -garbage
    for st, td in ((st_h, td_ssh), (st_b, td_both)):
        be = hip.RomsHip(st)
        try:
            be.set_tides(td)                                  # the switch alone: roms_hip_tides is not called
            be.call("step2d", s)
            be.to_host()
            be.check_guards()
        finally:
            be.close()
    for name in ("zeta", "ubar", "vbar"):
        assert np.array_equal(st_h[name], st_o[name]), (name, float(np.abs(st_h[name] - st_o[name]).max()))
    assert not np.array_equal(st_o["ubar"], st_p["ubar"]) and not np.array_equal(st_o["vbar"], st_p["vbar"])
    # with UV_TIDES also set the boundary data are taken as they are
    plain = hip.RomsHip(st0.copy())
    try:
        plain.call("step2d", s)
        st_n = plain.to_host()
    finally:
        plain.close()
    for name in ("zeta", "ubar", "vbar"):
        assert np.array_equal(st_b[name], st_n[name]), name


# ------------------------------------------------------------------------------------------ 4. seven steps --
def test_seven_steps_against_the_oracle_fed_by_the_restatement():
    import oracle
    st_o = basin("water")
    st_h = st_o.copy()
    mk = lambda st: ana.analytic_tides(st, ntc=3, mtc=4, tide_start=-0.2, ramp=True, dstart=-1.0)
    mo = main3d.Main3D(tu.TidalOracle(oracle.Oracle(st_o)), tides=mk(st_o))
    mo.initial()
    mo.run(7)
    be = hip.RomsHip(st_h)
    try:
        mh = main3d.Main3D(be, tides=mk(st_h))
        mh.initial()
        mh.run(7)
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    diffs = util.compare_states(st_h, st_o)
    print("seven steps, max relative differences:", diffs)
    assert all(v <= 1e-10 for v in diffs.values()), diffs
    assert np.abs(st_o["zeta_bry"]).max() > 0.05 and np.abs(st_o["ubar_bry"]).max() > 0.01
    # the tides reach the interior: a run without them differs
    st_n = basin("water")
    mn = main3d.Main3D(oracle.Oracle(st_n))
    mn.initial()
    mn.run(7)
    assert util.max_rel_diff(st_n["zeta"], st_o["zeta"]) > 1e-3


# ---------------------------------------------------------------------------------------------- 5. tiling --
def _tiles_equal_single(tmp_path, world, ntI, ntJ, variant):
    import mp_gpu_tides_worker as worker
    st, td = worker.tiled_state(variant)
    be = hip.RomsHip(st)
    try:
        want = worker.run(be, st, td)
    finally:
        be.close()
    assert np.abs(want["zeta_bry"]).max() > 0.05 and (("ssh" in variant) != bool(np.abs(want["ubar_bry"]).max() > 0.0))
    tiling_util.spawn_ranks("mp_gpu_tides_worker.py", world, [ntI, ntJ, tmp_path, variant], timeout=600)
    tiling_util.assert_tiles_equal(tmp_path, world, want, st.b, worker.FIELDS, owned="IstrR:IendR")


@pytest.mark.parametrize("variant", ["uv", "ssh"])
@pytest.mark.parametrize("ntI,ntJ", [(2, 2), (4, 1)])
def test_tiled_run_equals_the_single_tile_run(tmp_path, ntI, ntJ, variant):
    _tiles_equal_single(tmp_path, ntI * ntJ, ntI, ntJ, variant)


@pytest.mark.parametrize("variant", ["uv+rccl", "ssh+rccl"])
def test_rccl_loopback_equals_the_single_tile_run(tmp_path, variant):
    _tiles_equal_single(tmp_path, 1, 1, 1, variant)


# -------------------------------------------------------------------------------------------- 6. refusals --
def test_refusals_use_the_error_path_and_leave_the_library_usable():
    lib = hip.load()
    st = basin("water")
    td = ana.analytic_tides(st, ntc=2, mtc=3)
    time = 0.3 * DAY
    want = numpy_bry(st, td, time)

    def refused(text, **change):
        args = list(td.c_args())
        names = ("NTC", "MTC", "Tperiod", "SSH_Tamp", "SSH_Tphase", "UV_Tangle", "UV_Tphase", "UV_Tmajor", "UV_Tminor", "angler",
                 "tide_start", "ramp", "dstart", "add_fsobc", "zeta_base", "add_m2obc", "ubar_base", "vbar_base")
        for k, v in change.items():
            args[names.index(k)] = v
        assert lib.roms_hip_set_tides(*args) != 0
        assert text in lib.roms_hip_last_error(), lib.roms_hip_last_error()

    be = hip.RomsHip(st)
    try:
        be.set_tides(td)
        refused(b"NTC > MTC", NTC=4)
        refused(b"NTC < 0", NTC=-1)
        refused(b"come together", SSH_Tphase=None)
        refused(b"come together", UV_Tminor=None)
        refused(b"without zeta_base", add_fsobc=1)
        refused(b"without ubar_base", add_m2obc=1, ubar_base=st["h"].ctypes.data_as(tides._DP))
        refused(b"NTC = 0 with", NTC=0)
        got = device_bry(be, st, time)                        # every refusal left the configuration in force
        for name in BRY:
            assert np.abs(got[name] - want[name]).max() <= 1e-13 * max(tu.amp_bound(td)), name
        # add_m2obc while LnudgeM2CLM is on
        cl = ana.analytic_clima(st, sides=tu.SIDES, m3=False, tracers=[0] * st.b.NT)
        be.set_clima(cl)
        base = np.zeros((st.ni, st.nj), order="F")
        with pytest.raises(RuntimeError, match="LnudgeM2CLM"):
            be.set_tides(ana.analytic_tides(st, ntc=2, add_m2obc=True, ubar_base=base, vbar_base=base))
        be.set_clima(ana.analytic_clima(st, m2=False, m3=False, tracers=[0] * st.b.NT))
        # NULL bases keep the copy; a released context writes nothing
        add = ana.analytic_tides(st, ntc=2, mtc=3, add_fsobc=True, zeta_base=np.full((st.ni, st.nj), 2.0, order="F"))
        be.set_tides(add)
        be.set_tides(add, only=())
        got = device_bry(be, st, time)
        w = tu.written_points(st, td)["zeta_bry"]
        assert np.abs(got["zeta_bry"][w] - 2.0 - want["zeta_bry"][w]).max() <= 1e-12
        be.set_tides(None)
        got = device_bry(be, st, time)
        assert all((got[name] == SENTINEL).all() for name in BRY)
        with pytest.raises(RuntimeError, match="without zeta_base"):
            be.set_tides(add, only=())                        # released: nothing to keep
        be.check_guards()
        # a run afterwards equals a run without tides
        for name in BRY:
            st[name][:] = 0.0
        be.to_device(BRY)
        m = main3d.Main3D(be)
        m.initial()
        m.run(2)
        be.to_host()
    finally:
        be.close()
    st_n = basin("water")
    be = hip.RomsHip(st_n)
    try:
        m = main3d.Main3D(be)
        m.initial()
        m.run(2)
        be.to_host()
    finally:
        be.close()
    assert not util.compare_states(st, st_n)
