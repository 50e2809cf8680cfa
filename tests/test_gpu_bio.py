"""-m gpu: the NPZD_POWELL biology on the device (roms_hip_set_biology, roms_hip_biology: k_npzd_powell) against the numpy
restatement of npzd_Powell.h (tests/bio_util.py) on the cases whose continuity tests/test_bio.py asserts; the identities
of the routine; whole steps against a host that does the biology itself; tiling; reuse of a context; the refusals.
Parity status: pinned -- the restatement equals the reference builds UPWELLING_BIO / UPWELLING_BIO_CPAR
(tests/test_ref_pinning.py), and test_device_reproduces_reference_vectors compares the device with the reference's own
vectors (tests/golden/ref_bio.npz).
Measured on the MI355X: see DESIGN.md section 8 (the largest difference of the parity cases is recorded there)."""
import ctypes as C
import os

import numpy as np
import pytest

import bio_util as bu
import tiling_util
import util
from roms_trunk_mgh_amd import abi, bio, hip, main3d

pytestmark = pytest.mark.gpu
TOL = 1e-10          # of each field's maximum: what tests/test_golden.py grants k_lmd_vmix for the device exp / pow
S = util.step_idx()  # nstp = 1, nnew = 2


def _device(st, par, calls=1):
    """roms_hip_biology on a copy of st in a fresh context; returns t"""
    sh = st.copy()
    be = hip.RomsHip(sh)
    try:
        be.set_biology("NPZD_POWELL", par)
        for _ in range(calls):
            be.call("biology", S)
        be.to_host(["t"])
        be.check_guards()
    finally:
        be.close()
    return sh["t"].copy()


def _close(a, want, what):
    scale = float(np.abs(want).max())
    err = float(np.abs(a - want).max())
    print(f"{what}: max |diff| {err:.3e}, field max {scale:.3e}, ratio {err / scale:.3e}")
    assert err <= TOL * scale, (what, err, scale)
    return err / scale


# ------------------------------------------------------------------------------------- 1. device = restatement --
@pytest.mark.parametrize("case", bu.PARITY_CASES, ids=bu.case_id)
def test_device_equals_restatement(case):
    grid, mask, pset = case
    st = bu.bio_state(grid, mask)
    par = bu.params(pset, st.p.dt)
    b, N = st.b, st.b.N
    info = {}
    want = bu.expected(st, par, info=info)
    got = _device(st, par)
    I = bu.interior(b)
    idbio = par.tracers(b)
    for q, itrc in enumerate(idbio):
        _close(got[I][:, :, :, 1, itrc - 1], want[I][:, :, :, 1, itrc - 1], f"t(nnew) {bio.POOLS[q]}")
    # t(nstp) and the third time level, the physical tracers, and every point outside Istr:Iend, Jstr:Jend: bit for bit
    assert np.array_equal(got[:, :, :, 0, :], st["t"][:, :, :, 0, :]) and np.array_equal(got[:, :, :, 2, :], st["t"][:, :, :, 2, :])
    assert np.array_equal(got[:, :, :, :, :b.NAT], st["t"][:, :, :, :, :b.NAT])
    outside = np.ones(got.shape[:2], dtype=bool)
    outside[I] = False
    assert np.array_equal(got[outside], st["t"][outside])
    # not vacuous: most cells moved, the night branch ran beside the day branch, and with sinking the departure point
    # lies more than one cell up somewhere and above the surface in the shallow columns
    inc = got[I][:, :, :, 1, idbio[0] - 1:idbio[0] + 3] - st["t"][I][:, :, :, 1, idbio[0] - 1:idbio[0] + 3]
    assert (inc != 0.0).mean() > 0.8
    if pset != "constpar":
        assert (~info["day"]).any() and info["day"].any()
    if pset == "sink":
        ks = info["ksource_SDet"]
        assert (ks > np.arange(1, N + 1) + 1).any() and (ks[..., 0] == N).any() and (ks[..., 0] < N).any()


# ------------------------------------------------------------------------------ 1b. device = reference vectors --
def _fixture_cases():
    return list(util.load_golden_maker("make_golden_bio").CASES)


@pytest.mark.parametrize("case", _fixture_cases())
def test_device_reproduces_reference_vectors(case):
    """tests/golden/ref_bio.npz: t(nnew) of the reference's own biology(ng, tile) (UPWELLING_BIO / UPWELLING_BIO_CPAR of
    oracle/build_ref.sh) at the stored columns and the column inventories, within TOL of each stored array's maximum; the
    digest of the inputs asserts that the state is the one the reference ran."""
    mg = util.load_golden_maker("make_golden_bio")
    g = np.load(os.path.join(mg.HERE, "ref_bio.npz"))
    st, par = mg.prepare(case)
    got = _device(st, par)
    util.compare_packed(g, mg.pack(case, st, par, got, cols=g[f"{case}/cols"]), TOL)


# ----------------------------------------------------------------------------------------------- 2. identities --
def test_no_iterations_change_nothing():
    st = bu.bio_state("TINY")
    got = _device(st, bio.PowellPar(BioIter=0))
    assert np.array_equal(got, st["t"])


@pytest.mark.parametrize("iters", [1, 3])
def test_reactions_conserve_nitrogen_on_the_device(iters):
    """w = 0: the four increments of a cell sum to rounding.  The bound: each pool's increment is the difference of two
    numbers of the size of the pool times Hz, rounded to 2^-53 relative; BioIter sweeps of about ten operations each."""
    st = bu.bio_state("N33", "island")
    par = bio.PowellPar(BioIter=iters, wPhy=0.0, wDet=0.0)
    got = _device(st, par)
    I = bu.interior(st.b)
    it0 = st.b.NAT
    inc = (got - st["t"])[I][:, :, :, 1, it0:it0 + 4]
    scale = (np.abs(bu.positive(st["t"][I][:, :, :, 0, it0:it0 + 4])).sum(axis=-1) * st["Hz"][I])
    resid = np.abs(inc.sum(axis=-1))
    print(f"largest residual / (sum of pools * Hz) = {(resid / scale).max():.3e}")
    assert (np.abs(inc) > 0.0).mean() > 0.8
    assert np.all(resid <= 64 * iters * 2.0 ** -53 * scale)


# ----------------------------------------------------------------------------------------------- 3. whole steps --
NSTEPS = 6


def _upwelling(mask):
    st = util.prepared_state("UPWELLING", NT=6, mask=mask)
    bio.analytic_biology(st)
    st["srflx"][:] = 5.0e-5 * (np.arange(st.ni) % 9 < 6)[:, None]        # day and night columns
    return st


class _HostBiology(main3d.Main3D):
    """Main3D whose biology is done by the host: before step3d_t it fetches t, Hz, z_w and srflx, applies the
    restatement and uploads t."""

    def __init__(self, be, par, **kw):
        super().__init__(be, **kw)
        self.par = par

    def step(self):
        be, par, call = self.be, self.par, self.be.call

        def hooked(kernel, s):
            if kernel == "step3d_t":
                st = be.to_host(["t", "Hz", "z_w", "srflx"])
                st["t"][...] = bu.expected(st, par, nstp=s.nstp, nnew=s.nnew)
                be.to_device(["t"])
            call(kernel, s)

        be.call = hooked
        try:
            super().step()
        finally:
            del be.call


def _run(st, make):
    sh = st.copy()
    be = hip.RomsHip(sh)
    try:
        m = make(be)
        m.initial()
        m.run(NSTEPS)
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    return sh


@pytest.mark.parametrize("mask", [None, "island"], ids=["plain", "masked"])
def test_whole_steps_equal_host_biology(mask):
    st = _upwelling(mask)
    par = bio.PowellPar()
    dev = _run(st, lambda be: main3d.Main3D(be, biology=par))
    host = _run(st, lambda be: _HostBiology(be, par))
    none = _run(st, lambda be: main3d.Main3D(be))
    it0 = st.b.NAT
    for q in range(4):
        _close(dev["t"][..., it0 + q], host["t"][..., it0 + q], f"t {bio.POOLS[q]} after {NSTEPS} steps")
    for name in ("u", "v", "zeta"):
        assert np.array_equal(dev[name], host[name]) and np.array_equal(dev[name], none[name]), name
    assert np.array_equal(dev["t"][..., :it0], none["t"][..., :it0])
    assert not np.array_equal(dev["t"][..., it0:it0 + 4], none["t"][..., it0:it0 + 4])      # the biology did something


def test_switch_off_is_todays_run():
    """Main3D(biology=None) issues exactly the calls it issued before: its result equals that of a driver that has
    never heard of biology (the step sequence with the new branch removed), bit for bit."""
    st = _upwelling(None)
    a = _run(st, lambda be: main3d.Main3D(be, biology=None))
    calls = []

    def spy(be):
        m = main3d.Main3D(be)
        real = be.call
        be.call = lambda kernel, s: (calls.append(kernel), real(kernel, s))[1]
        return m

    bq = _run(st, spy)
    assert "biology" not in calls and "step3d_t" in calls
    for name, _, _ in abi.FIELDS:
        assert np.array_equal(a[name], bq[name], equal_nan=True), name


# ---------------------------------------------------------------------------------------------------- 4. tiling --
@pytest.mark.parametrize("ntI,ntJ", [(2, 2), (4, 1)], ids=["2x2", "4x1"])
def test_tiles_equal_one_tile(tmp_path, ntI, ntJ):
    import mp_gpu_bio_worker as worker
    world = ntI * ntJ
    st = worker.tiled_state()
    be = hip.RomsHip(st)
    try:
        want = worker.run(be, st)
    finally:
        be.close()
    it0 = st.b.NAT
    assert np.unique(want["t"][..., it0:it0 + 4]).size > 1000
    tiling_util.spawn_ranks("mp_gpu_bio_worker.py", world, [ntI, ntJ, tmp_path], timeout=600)
    tiling_util.assert_tiles_equal(tmp_path, world, want, st.b, ["t"])


# ----------------------------------------------------------------------------------------------- 5. context reuse --
def test_on_off_on_with_changed_parameters_in_one_context():
    st = bu.bio_state("N17", "island")
    p1 = bu.params("sink", st.p.dt)
    p2 = bu.params("iter3", st.p.dt).replace(wDet=3.0, Ivlev=0.5)
    want1, want2 = _device(st, p1), _device(st, p2)
    assert not np.array_equal(want1, want2)
    sh = st.copy()
    be = hip.RomsHip(sh)
    try:
        for par, want in ((p1, want1), (None, st["t"]), (p2, want2), (p1, want1)):
            sh["t"][...] = st["t"]
            be.to_device(["t"])
            if par is None:
                be.set_biology(None)
                with pytest.raises(RuntimeError, match="biology is not switched on"):
                    be.call("biology", S)
            else:
                be.set_biology("NPZD_POWELL", par)
                be.call("biology", S)
            be.to_host(["t"])
            assert np.array_equal(sh["t"], want)
            be.check_guards()
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 6. refusals --
def test_refusals_leave_the_library_usable():
    st = bu.bio_state("PARTIAL")
    par = bu.params("sink", st.p.dt)
    want = _device(st, par)
    sh = st.copy()
    be = hip.RomsHip(sh)
    lib = be.l
    try:
        def refused(rc, *words):
            msg = lib.roms_hip_last_error().decode()
            assert rc != 0 and all(w in msg for w in words), msg

        def set_bio(model, blk, nbytes=None):
            return lib.roms_hip_set_biology(model, C.byref(blk), C.sizeof(blk) if nbytes is None else nbytes)

        refused(lib.roms_hip_biology(C.byref(S)), "roms_hip_biology", "biology is not switched on")
        be.set_biology("NPZD_POWELL", par)                       # the setting the refused calls must leave in force
        good = par.c_struct(sh.b)
        for name in ("NPZD_FRANKS", "NPZD_IRON", "FENNEL", "NEMURO", "ECOSIM", "HYPOXIA_SRM", "RED_TIDE"):
            refused(set_bio(abi.BIO_MODEL[name], good), "roms_hip_set_biology", name, "not built")
        refused(set_bio(99, good), "unknown model")
        refused(set_bio(1, good, C.sizeof(good) - 8), "nbytes")
        for q, value, word in ((0, sh.b.NAT, "outside"), (3, sh.b.NT + 1, "outside"), (2, good.idbio[1], "repeated")):
            bad = par.c_struct(sh.b)
            bad.idbio[q] = value
            refused(set_bio(1, bad), "idbio", word)
        for member, word in (("BioIter", "BioIter < 0"), ("wPhy", "wPhy < 0"), ("wDet", "wDet < 0")):
            bad = par.c_struct(sh.b)
            setattr(bad, member, -1)
            refused(set_bio(1, bad), word)
        be.call("biology", S)                                    # ... and the run is the one of the setting in force
        be.to_host(["t"])
        assert np.array_equal(sh["t"], want)
        be.check_guards()
    finally:
        be.close()
    # before bounds / params
    lib.roms_hip_finalize()
    rc = lib.roms_hip_set_biology(1, C.byref(good), C.sizeof(good))
    assert rc != 0 and b"come first" in lib.roms_hip_last_error()


def test_fewer_than_four_levels_is_refused():
    st = util.prepared_state("BENCHMARK_TINY", NT=6, overrides=dict(Lm=66, Mm=3, N=3))
    be = hip.RomsHip(st)
    try:
        be.set_biology("NPZD_POWELL")
        with pytest.raises(RuntimeError, match="needs N >= 4 levels"):
            be.call("biology", S)
    finally:
        be.close()
