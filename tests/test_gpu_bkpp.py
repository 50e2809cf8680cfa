"""-m gpu: the KPP bottom boundary layer on the device (LMD_BKPP: roms_hip_set_kpp, k_lmd_bkpp inside roms_hip_lmd_vmix)
against the numpy restatement of lmd_bkpp.F (tests/bkpp_util.py) on the states whose branch census and decision
margins tests/test_bkpp.py asserts; the behaviour with the switch off; tiling; whole steps and the restart of hbbl; the
refusals.  Parity status: pinned -- the restatement equals the reference builds BENCHMARK_BKPP / BENCHMARK_MASK_BKPP
(tests/test_ref_pinning.py), and test_device_reproduces_reference_vectors compares the device with the reference's own
vectors (tests/golden/ref_bkpp.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

import bkpp_util as bk
import tiling_util
import util
from roms_trunk_mgh_amd import abi, hip, main3d

pytestmark = pytest.mark.gpu
TOL = 1e-10          # of each field's maximum: what tests/test_golden.py grants k_lmd_vmix for the device pow / exp
OUT = ("Akv", "Akt", "ghats", "hsbl")
S = util.step_idx()


def _fetch(be, sh, bkpp):
    be.to_host(list(OUT))
    out = {n: sh[n].copy() for n in OUT}
    if bkpp:
        out.update({n: be.get_kpp(n) for n in ("hbbl", "kbbl", "ksbl")})
    return out


def _device(st, bkpp, hprev=None):
    """roms_hip_lmd_vmix on a copy of st in a fresh context, the switch off (A) or on (B)"""
    sh = st.copy()
    be = hip.RomsHip(sh)
    try:
        if bkpp:
            be.set_kpp(True, hprev)
        be.call("lmd_vmix", S)
        out = _fetch(be, sh, bkpp)
        be.check_guards()
    finally:
        be.close()
    return out


def _close(a, want, what):
    scale = float(np.abs(want).max())
    err = float(np.abs(a - want).max())
    print(f"{what}: max |diff| {err:.3e}, field max {scale:.3e}")
    assert err <= TOL * scale, (what, err, scale)


# ------------------------------------------------------------------------------------- 1. device = restatement --
@pytest.mark.parametrize("case", bk.PARITY_CASES, ids=bk.case_id)
def test_device_equals_restatement(case):
    st, hprev = bk.bkpp_state(*case)
    b, N = st.b, st.b.N
    I = bk.interior(b)
    if not case[3]:
        assert st["bvf"].min() >= 0.0        # the lmd_finish increment is exactly zero: A is the pre-finish input
    A = _device(st, False)
    B = _device(st, True, hprev)
    r = bk.expected(st, A["Akv"], A["Akt"], A["hsbl"], hprev)
    assert np.array_equal(B["ksbl"][I], r["ksbl"][I]) and np.array_equal(B["kbbl"][I], r["kbbl"][I])
    D = bk.defined_points(b)
    _close(B["hbbl"][D], r["hbbl"][D], "hbbl")
    lev = slice(1, N)
    _close(B["Akv"][I][:, :, lev], r["Akv"][:, :, lev], "Akv")
    for it in range(2):
        _close(B["Akt"][I][:, :, lev, it], r["Akt"][:, :, lev, it], f"Akt {it + 1}")
    # the bottom layer leaves the surface layer's own outputs and the levels 0 and N alone
    assert np.array_equal(B["hsbl"], A["hsbl"]) and np.array_equal(B["ghats"], A["ghats"])
    for k in (0, N):
        assert np.array_equal(B["Akv"][I][:, :, k], A["Akv"][I][:, :, k]) and np.array_equal(B["Akt"][I][:, :, k], A["Akt"][I][:, :, k])
    # not vacuous: the bottom layer changed the profile of many columns, at several levels
    changed = (B["Akv"][I] != A["Akv"][I])
    assert changed.any(axis=2).sum() > 0.05 * changed.shape[0] * changed.shape[1] and r["kbbl"][I].max() > 2


# ------------------------------------------------------------------------------ 1b. device = reference vectors --
def _fixture_cases():
    return list(util.load_golden_maker("make_golden_bkpp").CASES)


@pytest.mark.parametrize("case", _fixture_cases())
def test_device_reproduces_reference_vectors(case):
    """tests/golden/ref_bkpp.npz: what the reference's own lmd_vmix(ng, tile) built with LMD_BKPP gives
    (BENCHMARK_BKPP / BENCHMARK_MASK_BKPP of oracle/build_ref.sh): kbbl and ksbl identical on every interior column,
    hbbl on every interior column, the Akv / Akt profiles at the stored columns and the column sums within TOL of each
    stored array's maximum; hbbl's boundary values are bc_r2d_tile of its interior.  The digest of the inputs asserts
    that the state is the one the reference ran."""
    mg = util.load_golden_maker("make_golden_bkpp")
    g = np.load(os.path.join(mg.HERE, "ref_bkpp.npz"))
    st, hprev = mg.prepare(case)
    B = _device(st, True, hprev)
    util.compare_packed(g, mg.pack(case, st, hprev, B, cols=g[f"{case}/cols"]), TOL)
    D = bk.defined_points(st.b)
    _close(B["hbbl"][D], bk.bc_hbbl(st.b, B["hbbl"].copy())[D], "hbbl boundary values")


# ----------------------------------------------------------------------------------------- 2. existing behaviour --
def test_zero_bottom_stress_equals_switch_off():
    """bustr = bvstr = 0: hbbl = z_w(0), no level lies inside the layer, and lmd_bkpp's own lmd_finish increment is the
    one k_lmd_vmix adds with the switch off: bit for bit.  With a mask on the water columns: on land hbbl = 0 lies above
    every level and lmd_bkpp.F:795-798 store zeros, as written."""
    for mask in (None, "island"):
        st, hprev = bk.bkpp_state("TINY", mask=mask, unstable=True, stress=False)
        A = _device(st, False)
        B = _device(st, True, hprev)
        water = st["rmask"] > 0.0 if mask else np.ones((st.ni, st.nj), dtype=bool)
        I = bk.interior(st.b)
        for name in OUT:
            assert np.array_equal(B[name][water], A[name][water]), (mask, name)
        assert np.array_equal(B["hbbl"][I], (st["z_w"][:, :, 0] * (st["rmask"] if mask else 1.0))[I])
        assert bk.finish_increment(st).max() > 0.0


def _reset(be, sh, st0):
    for name in OUT:
        sh[name][...] = st0[name]
    be.to_device(list(OUT))


def test_switch_off_and_on_again_in_one_context():
    """on -> off -> on in one context: each run equals the fresh context of its kind bit for bit, guards clean"""
    st, hprev = bk.bkpp_state("N33", "island", True, False)
    A, B = _device(st, False), _device(st, True, hprev)
    sh = st.copy()
    be = hip.RomsHip(sh)
    try:
        for bkpp, want in ((True, B), (False, A), (True, B), (False, A)):
            _reset(be, sh, st)
            be.set_kpp(bkpp, hprev if bkpp else None)
            be.call("lmd_vmix", S)
            got = _fetch(be, sh, bkpp)
            assert sorted(got) == sorted(want)
            for name in want:
                assert np.array_equal(got[name], want[name]), (bkpp, name)
            be.check_guards()
        with pytest.raises(RuntimeError, match="not switched on"):
            be.get_kpp("hbbl")
    finally:
        be.close()
    assert not np.array_equal(A["Akv"], B["Akv"])


# ---------------------------------------------------------------------------------------------------- 3. tiling --
@pytest.mark.parametrize("ntI,ntJ,variant", [(2, 1, ""), (1, 2, ""), (2, 2, ""), (2, 2, "basin")],
                         ids=["2x1", "1x2", "2x2", "2x2-basin"])
def test_tiles_equal_one_tile(tmp_path, ntI, ntJ, variant):
    import mp_gpu_bkpp_worker as worker
    world = ntI * ntJ
    st = worker.tiled_state(variant)
    be = hip.RomsHip(st)
    try:
        want = worker.run(be, st)
    finally:
        be.close()
    I = bk.interior(st.b)
    # not vacuous: in the channel layers of many depths that span levels.  In the basin run the layer stays at the bed
    # (hbbl = z_w(0), as deep as the water): it checks bc_r2d_tile(hbbl) and the exchange across tiles on four walls
    # and the corners; the basin's own profiles are compared in test_device_equals_restatement
    if variant == "basin":
        assert np.unique(want["hbbl"][I]).size > 10
    else:
        assert np.unique(want["hbbl"][I]).size > 100 and want["kbbl"][I].max() > 1
    tiling_util.spawn_ranks("mp_gpu_bkpp_worker.py", world, [ntI, ntJ, tmp_path, variant], timeout=600)
    tiling_util.assert_tiles_equal(tmp_path, world, want, st.b, ["hbbl", "kbbl", "ksbl", "Akv", "Akt", "hsbl"],
                                   rho_ghosts=("hbbl",))


# ----------------------------------------------------------------------------------------------- 4. whole steps --
def test_whole_steps_and_restart_of_hbbl():
    """10 steps of Main3D(physics=True, bkpp=True) on BENCHMARK_TINY: every field finite, hbbl between the bed and the
    free surface the levels were set from (z_w(0) = -h and z_w(N)); the run interrupted after 5 steps -- every field and
    hbbl fetched, a fresh context, hbbl handed over through set_kpp -- equals the uninterrupted one bit for bit."""
    import reuse_util as ru
    st0 = ru.clone(util.prepared_state("BENCHMARK_TINY"))
    # a weak stratification and a slow rotation: the Ekman limit decides and the bottom layer spans levels
    st0["t"][:, :, :, :, 0] = st0["t"][:, :, :1, :, 0] + 1.0e-3 * (st0["t"][:, :, :, :, 0] - st0["t"][:, :, :1, :, 0])
    st0["f"][:] = 5.0e-6

    def leg(st, nsteps, old=None, hbbl=None):
        be = hip.RomsHip(st)
        try:
            m = main3d.Main3D(be, physics=True, bkpp=True, hbbl=hbbl)
            if old is None:
                m.initial()
            else:
                ru.resume(m, old)
            m.run(nsteps)
            be.to_host()
            out = be.get_kpp("hbbl"), be.get_kpp("kbbl")
            be.check_guards()
        finally:
            be.close()
        return m, out

    full = ru.clone(st0)
    _, (h10, k10) = leg(full, 10)
    for name, _, _ in abi.FIELDS:
        assert np.isfinite(full[name]).all(), name
    I = bk.interior(full.b)
    assert np.all(h10[I] >= -full["h"][I]) and np.all(h10[I] <= full["z_w"][I][:, :, -1]) and np.isfinite(h10).all()
    assert k10[I].min() >= 1 and k10[I].max() <= full.b.N
    assert k10[I].max() > 1 and np.unique(h10[I]).size > 100          # not vacuous: layers of many depths
    part = ru.clone(st0)
    m5, (h5, _) = leg(part, 5)
    cont = ru.clone(part)
    _, (h10b, k10b) = leg(cont, 5, old=m5, hbbl=h5)
    assert not ru.differing(cont, full)
    assert np.array_equal(h10b, h10) and np.array_equal(k10b, k10)
    assert not np.array_equal(h5, h10)


# ------------------------------------------------------------------------------------------------- 5. refusals --
def test_refusals_leave_the_library_usable():
    st, hprev = bk.bkpp_state("PARTIAL")
    A = _device(st, False)
    sh = st.copy()
    sh.p = type(st.p).from_buffer_copy(st.p)
    be = hip.RomsHip(sh)
    lib = be.l
    try:
        def refused(rc, *words):
            msg = lib.roms_hip_last_error().decode()
            assert rc != 0 and all(w in msg for w in words), msg
        refused(lib.roms_hip_set_kpp(2, None), "roms_hip_set_kpp", "0 or 1")
        refused(lib.roms_hip_set_kpp(-1, None), "roms_hip_set_kpp", "0 or 1")
        buf = np.zeros((sh.ni, sh.nj), order="F")
        refused(lib.roms_hip_get_kpp(b"hbbl", buf.ctypes.data, buf.size), "roms_hip_get_kpp", "not switched on")
        sh.p.salinity = 0
        be._chk(lib.roms_hip_set_params(C.byref(sh.p)), "set_params")
        refused(lib.roms_hip_set_kpp(1, None), "roms_hip_set_kpp", "SALINITY")
        sh.p.salinity = 1
        be._chk(lib.roms_hip_set_params(C.byref(sh.p)), "set_params")
        # nothing was switched on by the refused calls: the run is A
        be.call("lmd_vmix", S)
        got = _fetch(be, sh, False)
        for name in OUT:
            assert np.array_equal(got[name], A[name]), name
        be.set_kpp(True, hprev)
        refused(lib.roms_hip_get_kpp(b"hsbl", buf.ctypes.data, buf.size), "roms_hip_get_kpp", "unknown array")
        refused(lib.roms_hip_get_kpp(b"hbbl", buf.ctypes.data, buf.size - 1), "roms_hip_get_kpp", "elements")
        refused(lib.roms_hip_set_kpp(3, None), "roms_hip_set_kpp", "0 or 1")
        assert np.array_equal(be.get_kpp("hbbl"), hprev)          # ... and the refused call left the switch and hbbl alone
        be.check_guards()
    finally:
        be.close()
