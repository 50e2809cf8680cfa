"""-m gpu: the KPP double-diffusive mixing on the device (LMD_DDMIX: roms_hip_set_ddmix, the DDMIX instantiations of
k_rho_eos_* and k_lmd_vmix) against the reference's own vectors (tests/golden/ref_ddmix.npz) and the numpy restatement
(tests/ddmix_util.py) on the states whose conditions tests/test_ddmix.py asserts; identities that need no reference;
tiling; the life cycle and the refusals.  Every case runs ddmix_util.run_device: rho_eos, then lmd_vmix on the builder's
density profiles."""
import ctypes as C
import os

import numpy as np
import pytest

import bkpp_util as bk
import ddmix_util as dd
import tiling_util
import util
from roms_trunk_mgh_amd import abi, hip, main3d

pytestmark = pytest.mark.gpu
TOL = 1e-10          # of each field's maximum: the project's bound for k_lmd_vmix (test_gpu_kernels.py::test_lmd_vmix)
EOS_TOL = 1e-12      # of the field's maximum: what test_gpu_kernels.py::test_rho_eos grants alpha / beta
S = util.step_idx()
_cache = {}


def _state(case):
    if case not in _cache:
        _cache[case] = dd.ddmix_state(*case)
    return _cache[case]


def _device(case, ddmix, bkpp=False):
    """run_device on a copy of the case's state in a fresh context; computed once per (case, switches)"""
    key = (case, ddmix, bkpp)
    if key not in _cache:
        st, hprev = _state(case)
        sh = st.copy()
        be = hip.RomsHip(sh)
        try:
            out = dd.run_device(be, sh, st, S, ddmix, bkpp, hprev)
            out["guarded"] = be.guarded_arrays()
            be.check_guards()
        finally:
            be.close()
        _cache[key] = out
    return _cache[key]


def _close(a, want, what, tol=TOL):
    scale = float(np.abs(want).max())
    err = float(np.abs(a - want).max())
    print(f"{what}: max |diff| {err:.3e}, field max {scale:.3e}")
    assert err <= tol * scale, (what, err, scale)


# ---------------------------------------------------------------------------------------------------- 1. parity --
@pytest.mark.parametrize("case", dd.CASES, ids=dd.case_id)
def test_rho_eos_stores_alfaobeta_and_changes_nothing_else(case):
    st, _ = _state(case)
    b = st.b
    A, B = _device(case, False), _device(case, True)
    for name in dd.RHO_EOS_OUT:
        assert np.array_equal(A["eos"][name], B["eos"][name]), name
    T = (slice(b.IstrT - b.LBi, b.IendT - b.LBi + 1), slice(b.JstrT - b.LBj, b.JendT - b.LBj + 1))
    want = dd.alfaobeta(st)
    got = B["alfaobeta"]
    _close(got[T][:, :, 1:], want[T][:, :, 1:], "alfaobeta against the restatement", EOS_TOL)
    assert not got[:, :, 0].any()                                  # level 0 is never written: zero, as allocated
    mg = util.load_golden_maker("make_golden_ddmix")
    g = np.load(os.path.join(mg.HERE, "ref_ddmix.npz"))
    name = f"{case[0]}-{'island' if case[1] else 'plain'}-skpp"
    cols = g[f"{name}/cols"]
    ref = g[f"{name}/prof/alfaobeta"]
    mine = got[dd.interior(b)][cols[:, 0], cols[:, 1], 1:]
    _close(mine, ref, "alfaobeta against the reference's vectors", EOS_TOL)


@pytest.mark.parametrize("bkpp", [False, True], ids=["skpp", "bkpp"])
@pytest.mark.parametrize("case", dd.CASES, ids=dd.case_id)
def test_lmd_vmix_reproduces_reference_vectors(case, bkpp):
    """tests/golden/ref_ddmix.npz: the reference's own rho_eos + lmd_vmix(ng, tile) built with LMD_DDMIX (and LMD_BKPP):
    every stored array within TOL of its maximum; the digest of the inputs asserts the state is the one the reference ran"""
    mg = util.load_golden_maker("make_golden_ddmix")
    g = np.load(os.path.join(mg.HERE, "ref_ddmix.npz"))
    name = f"{case[0]}-{'island' if case[1] else 'plain'}-{'bkpp' if bkpp else 'skpp'}"
    st, hprev = _state(case)
    B = _device(case, True, bkpp)
    plain = None if bkpp else _device(case, False)
    mine = mg.pack(name, st, hprev, B, plain, cols=g[f"{name}/cols"])
    assert sorted(mine) == sorted(k for k in g.files if k.startswith(name + "/"))
    # every field on its own, within the bound times its own maximum; alfaobeta at rho_eos's bound
    util.compare_packed(g, {k: v for k, v in mine.items() if k.endswith("/alfaobeta")}, EOS_TOL)
    util.compare_packed(g, {k: v for k, v in mine.items() if not k.endswith("/alfaobeta")}, TOL)


# ---------------------------------------------------------------------------- 2. identities without a reference --
@pytest.mark.parametrize("case", dd.CASES, ids=dd.case_id)
def test_only_akt_changes_and_by_the_restated_increment(case):
    st, _ = _state(case)
    b, N = st.b, st.b.N
    I = dd.interior(b)
    A, B = _device(case, False), _device(case, True)
    # lmd_skpp's depth search and momentum profile never read Akt
    for name in ("Akv", "hsbl", "ghats"):
        assert np.array_equal(A[name], B[name]), name
    ks = bk.ksbl_from_hsbl(st, B["hsbl"])[I]
    assert np.array_equal(ks, bk.ksbl_from_hsbl(st, A["hsbl"])[I])
    nt, ns, reg, _ = dd.state_increment(st, B["alfaobeta"])
    alone = np.arange(1, N)[None, None, :] <= ks[:, :, None]
    if b.east_edge:
        alone[-2] = False                    # column Iend-1 receives column Iend (lmd_vmix.F:560-575)
    scale = float(np.abs(B["Akt"]).max())
    d = [(B["Akt"][I][:, :, 1:N, it] - A["Akt"][I][:, :, 1:N, it]) for it in (0, 1)]
    for it, nu in ((0, nt), (1, ns)):
        err = float(np.abs(d[it] - nu[I])[alone].max())
        print(f"Akt {it + 1}: increment differs by {err:.3e}, field max {scale:.3e}")
        assert err <= TOL * scale
    active = alone & (reg[I] != dd.NONE) & (reg[I] != dd.CAPPED)
    assert active.sum() > 0.2 * alone.sum() and np.all(d[0][active] != d[1][active])
    # levels 0 and N are left alone
    for k in (0, N):
        assert np.array_equal(A["Akt"][:, :, k], B["Akt"][:, :, k])


@pytest.mark.parametrize("case", dd.CASES, ids=dd.case_id)
def test_rounding_of_t_moves_no_akt(case):
    """a 1e-13 relative change of t (the perturbation of tests/test_ddmix.py::test_sensitivity) moves no Akt out of
    lmd_vmix by 1e-10 of its maximum, the boundary-layer levels that match to the changed interior values included, with
    the bottom layer off and on; everything else lmd_vmix writes keeps its bits"""
    st, hprev = _state(case)
    for bkpp in (False, True):
        B = _device(case, True, bkpp)
        sp = st.copy()
        sp["t"][...] = st["t"] * (1.0 + 1e-13 * np.random.default_rng(5).uniform(0.5, 1.0, st["t"].shape))
        sh = sp.copy()
        be = hip.RomsHip(sh)
        try:
            P = dd.run_device(be, sh, sp, S, True, bkpp, hprev)
        finally:
            be.close()
        scale = float(np.abs(B["Akt"]).max())
        err = float(np.abs(P["Akt"] - B["Akt"]).max())
        print(f"bkpp {bkpp}: Akt moved by {err:.3e}, field max {scale:.3e}")
        assert err <= 1e-10 * scale
        for name in ("Akv", "hsbl", "ghats"):
            assert np.array_equal(P[name], B[name]), name


# ---------------------------------------------------------------------------------------------------- 3. tiling --
@pytest.mark.parametrize("ntI,ntJ,variant", [(2, 2, "kernels"), (4, 1, "kernels"), (2, 2, "steps")],
                         ids=["2x2", "4x1", "2x2-steps"])
def test_tiles_equal_one_tile(tmp_path, ntI, ntJ, variant):
    """rho_eos then lmd_vmix with the option on, and 10 whole steps of Main3D(physics, bkpp, ddmix) on BENCHMARK_TINY:
    every tiling gives the bits of one tile; the whole steps stay finite"""
    import mp_gpu_ddmix_worker as worker
    world = ntI * ntJ
    st = worker.tiled_state(variant)
    be = hip.RomsHip(st)
    try:
        want = worker.run(be, st, variant)
    finally:
        be.close()
    I = dd.interior(st.b)
    assert all(np.isfinite(want[n]).all() for n in want)
    assert np.unique(want["alfaobeta"][I][:, :, 1:]).size > 100
    if variant == "kernels":                  # not vacuous: every regime among the points
        reg = dd.state_increment(st)[2][I]
        assert all((reg == q).mean() > 0.1 for q in range(5))
    tiling_util.spawn_ranks("mp_gpu_ddmix_worker.py", world, [ntI, ntJ, tmp_path, variant], timeout=600)
    tiling_util.assert_tiles_equal(tmp_path, world, want, st.b, worker.NAMES + (["t"] if variant == "steps" else []))


# ------------------------------------------------------------------------------------------------ 4. life cycle --
def test_life_cycle_in_one_context():
    """on -> off equals a fresh context bit for bit (all four combinations with LMD_BKPP in turn); on -> set_bounds -> on;
    alfaobeta is a guarded array only while the option is on"""
    case = ("N33", "island")
    st, hprev = _state(case)
    order = ((True, False), (False, False), (True, True), (False, True), (True, False))
    fresh = {sw: _device(case, *sw) for sw in order}          # (one context at a time: before this one opens)
    sh = st.copy()
    be = hip.RomsHip(sh)
    try:
        base = be.guarded_arrays()
        assert "alfaobeta" not in base
        for ddmix, bkpp in order:
            want = fresh[(ddmix, bkpp)]
            got = dd.run_device(be, sh, st, S, ddmix, bkpp, hprev)
            for name in dd.OUT + (("alfaobeta",) if ddmix else ()) + (("hbbl", "kbbl", "ksbl") if bkpp else ()):
                assert np.array_equal(got[name], want[name]), (ddmix, bkpp, name)
            assert (be.guarded_arrays().count("alfaobeta") == 1) == ddmix
            be.check_guards()
        be.set_ddmix(False)
        with pytest.raises(RuntimeError, match="LMD_DDMIX is not switched on"):
            be.get_kpp("alfaobeta")
        assert sorted(be.guarded_arrays()) == sorted(base)
    finally:
        be.close()
    # on -> set_bounds (drops the store and every mirror) -> a new registration -> on
    sh = st.copy()
    be = hip.RomsHip(sh)
    try:
        be.set_ddmix(True)
        assert "alfaobeta" in be.guarded_arrays()
        be._chk(be.l.roms_hip_set_bounds(C.byref(sh.b)), "set_bounds")
        assert "alfaobeta" not in be.guarded_arrays()
        buf = np.zeros(sh.ni * sh.nj * (sh.b.N + 1))
        assert be.l.roms_hip_get_kpp(b"alfaobeta", buf.ctypes.data, buf.size) != 0
        assert b"LMD_DDMIX is not switched on" in be.l.roms_hip_last_error()
        be.check_guards()
    finally:
        be.close()
    sh = st.copy()
    be = hip.RomsHip(sh)
    try:
        be.set_ddmix(True)
        be.set_ddmix(True)                     # on twice: one array
        assert be.guarded_arrays().count("alfaobeta") == 1
        got = dd.run_device(be, sh, st, S, True)
        assert np.array_equal(got["Akt"], fresh[(True, False)]["Akt"])
    finally:
        be.close()


def test_refusals_leave_the_library_usable():
    case = ("PARTIAL", None)
    st, hprev = _state(case)
    A = _device(case, False)
    sh = st.copy()
    sh.p = type(st.p).from_buffer_copy(st.p)
    be = hip.RomsHip(sh)
    lib = be.l
    try:
        def refused(rc, *words):
            msg = lib.roms_hip_last_error().decode()
            assert rc != 0 and all(w in msg for w in words), msg
        refused(lib.roms_hip_set_ddmix(2), "roms_hip_set_ddmix", "0 or 1")
        refused(lib.roms_hip_set_ddmix(-1), "roms_hip_set_ddmix", "0 or 1")
        buf = np.zeros(sh.ni * sh.nj * (sh.b.N + 1))
        refused(lib.roms_hip_get_kpp(b"alfaobeta", buf.ctypes.data, buf.size), "roms_hip_get_kpp", "LMD_DDMIX is not switched on")
        sh.p.salinity = 0
        be._chk(lib.roms_hip_set_params(C.byref(sh.p)), "set_params")
        refused(lib.roms_hip_set_ddmix(1), "roms_hip_set_ddmix", "SALINITY")
        sh.p.salinity = 1
        be._chk(lib.roms_hip_set_params(C.byref(sh.p)), "set_params")
        assert "alfaobeta" not in be.guarded_arrays()
        for bad in (2, "on", 1.0, None):
            with pytest.raises(ValueError, match="lmd_ddmix"):
                be.set_ddmix(bad)
        # nothing was switched on by the refused calls: the run is A
        got = dd.run_device(be, sh, st, S, False)
        for name in dd.OUT:
            assert np.array_equal(got[name], A[name]), name
        be.set_ddmix(True)
        refused(lib.roms_hip_get_kpp(b"alfaobeta", buf.ctypes.data, buf.size - 1), "roms_hip_get_kpp", "doubles")
        refused(lib.roms_hip_set_ddmix(3), "roms_hip_set_ddmix", "0 or 1")
        assert "alfaobeta" in be.guarded_arrays()              # ... and the refused call left the switch alone
        be.check_guards()
    finally:
        be.close()
    # before bounds / params
    lib = hip.load()
    assert lib.roms_hip_init(0, 1, 1, 0, None) == 0, lib.roms_hip_last_error()
    try:
        assert lib.roms_hip_set_ddmix(1) != 0
        assert b"roms_hip_set_ddmix" in lib.roms_hip_last_error() and b"come first" in lib.roms_hip_last_error()
        # NAT < 2 (salinity = 1 in the parameters): refused as well, nothing allocated
        b1 = type(st.b).from_buffer_copy(st.b)
        b1.NAT = 1
        assert lib.roms_hip_set_bounds(C.byref(b1)) == 0, lib.roms_hip_last_error()
        assert lib.roms_hip_set_params(C.byref(st.p)) == 0, lib.roms_hip_last_error()
        n0 = lib.roms_hip_guarded_arrays(None, 0)
        assert st.p.salinity == 1 and lib.roms_hip_set_ddmix(1) != 0
        assert b"roms_hip_set_ddmix" in lib.roms_hip_last_error() and b"NAT = 2" in lib.roms_hip_last_error()
        assert lib.roms_hip_guarded_arrays(None, 0) == n0
        assert lib.roms_hip_set_ddmix(0) == 0
    finally:
        lib.roms_hip_finalize()
