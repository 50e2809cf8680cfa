"""-m gpu: climatology nudging of tracers and momentum on the device (roms_hip_set_clima; step3d_t.F:1551-1584,
rhs3d.F:567-594, step2d_LF_AM3.h:1818-1845 and the RadNud branches of the five boundary-condition routines).

The CPU oracle has no climatology and the reference cannot be built with one here, so nothing below compares against
either.  The evidence is of four exact kinds and one known answer, always against the HIP path WITHOUT climatology or
against closed forms:
  1. null cases, bit-equal to the run without set_clima (zero coefficients; climatology = the field the term reads)
  2. the term itself, mirrored operation for operation in numpy
  3. the edges, against the pinned route that takes tau from roms_params_t
  4. tiling invariance, owned and ghost points, over the gloo relay and once over RCCL in loopback
  5. exponential relaxation of a uniform tracer, 100 steps
and the error convention.  Every run ends with check_guards()."""
import numpy as np
import pytest

import clima_util as cu
import tiling_util
import util
from roms_trunk_mgh_amd import abi, ana, clima, hip, main3d

pytestmark = pytest.mark.gpu

S3D = util.step_idx(iic=5)
S_PRED = util.step_idx(iic=5, iif=3, pred=1, kstp=2, knew=3, krhs=1)
S_CORR = util.step_idx(iic=5, iif=3, pred=0, kstp=1, knew=2, krhs=3)
S_INI = util.step_idx(iic=1, iif=1, pred=0, kstp=1, krhs=1, knew=1)
ENTRIES = [("pre_step3d", S3D), ("rhs3d_tile", S3D), ("step2d", S_PRED), ("step2d", S_CORR), ("step3d_uv", S3D),
           ("step3d_t", S3D), ("ini_fields", S_INI)]
NULL_CASES = ["UPWELLING", "SEAMOUNT", "BENCHMARK_TINY", "basin"]


def _prepared(case, entry=None):
    if case == "basin":
        # the edges then read tau = 0 from the coefficient arrays: the run without gets obc_out = obc_in = 0 for the five
        # variables the switches cover (the free surface keeps its own)
        st = cu.radnud(util.prepared_state("UPWELLING", overrides={"EWperiodic": False}), others=(0.0, 0.0))
    else:
        st = util.prepared_state(case)
    if entry == "step3d_t":
        util.hz_weighted_tnew(st)
    return st


# ------------------------------------------------------------------ 1. null cases --
@pytest.mark.parametrize("case", NULL_CASES)
def test_zero_coefficients_change_nothing_in_any_entry(case):
    for entry, s in ENTRIES:
        st0 = _prepared(case, entry)
        a = cu.run_hip(st0, [(entry, s)])
        b = cu.run_hip(st0, [(entry, s)], cu.random_clima(st0, coef=0.0))
        assert cu.differing(a, b) == [], (case, entry)


@pytest.mark.parametrize("case", NULL_CASES)
def test_zero_coefficients_change_nothing_in_three_steps(case):
    if case == "basin":
        st0 = cu.radnud(ana.make_tile("UPWELLING", perturb=1.0, overrides={"EWperiodic": False}), others=(0.0, 0.0))
    else:
        st0 = ana.make_tile(case, perturb=1.0)
    a = cu.run_hip(st0, steps=3)
    b = cu.run_hip(st0, steps=3, clima_=cu.random_clima(st0, coef=0.0))
    assert cu.differing(a, b) == [], case
    assert np.isfinite(a["t"]).all()


@pytest.mark.parametrize("case", ["UPWELLING", "BENCHMARK_TINY", "basin"])
def test_climatology_equal_to_the_field_gives_no_momentum_term(case):
    """coefficients random and positive, uclm = u(nrhs) / ubarclm = ubar(krhs): the difference the term multiplies is
    exactly zero at every point, so any index slip between climatology, coefficient and field shows"""
    st0 = _prepared(case)
    if case == "basin":
        # the edges: coefficients equal to the parameters' on the two outermost points of every side, which is all an
        # edge reads (test 3 looks at the edges on their own); random inside
        st0 = cu.radnud(st0)
    for entry, s, lev2, lev3 in (("rhs3d_tile", S3D, None, S3D.nrhs - 1), ("step2d", S_PRED, S_PRED.krhs - 1, None),
                                 ("step2d", S_CORR, S_CORR.krhs - 1, None)):
        c = cu.random_clima(st0)
        if case == "basin":
            inner = (st0.I(2, st0.b.Lm - 1), st0.J(2, st0.b.Mm - 1))
            keep = c["M2nudgcof"][inner].copy()
            c["M2nudgcof"][:] = 2.0e-4
            c["M2nudgcof"][inner] = keep
        if lev3 is not None:
            c["uclm"][:] = st0["u"][:, :, :, lev3]
            c["vclm"][:] = st0["v"][:, :, :, lev3]
        else:
            c["ubarclm"][:] = st0["ubar"][:, :, lev2]
            c["vbarclm"][:] = st0["vbar"][:, :, lev2]
        a = cu.run_hip(st0, [(entry, s)])
        b = cu.run_hip(st0, [(entry, s)], c)
        assert cu.differing(a, b) == [], (case, entry, s.predictor_2d_step)


# ---------------------------------------------------------------- 2. the terms --
@pytest.mark.parametrize("flags,mask", [([1, 0], None), ([0, 1], None), ([1, 1], "island"), ([0, 1, 1], "island")])
def test_tracer_term_bit_for_bit(flags, mask):
    """t(nnew) with = mask(t0 + (dt c) (tclm - t0)), t0 = t(nnew) of the run without, on the whole R range; the ghost
    points of the periodic direction are the images; a tracer whose flag is off is untouched.  [0, 1]: ic = 1 <-> itrc = 2."""
    st0 = util.hz_weighted_tnew(util.prepared_state("UPWELLING", NT=len(flags), mask=mask))
    c = cu.random_clima(st0, tracers=flags)
    a = cu.run_hip(st0, [("step3d_t", S3D)])
    w = cu.run_hip(st0, [("step3d_t", S3D)], c)
    b, p, nnew = st0.b, st0.p, S3D.nnew - 1
    R = (st0.I(b.IstrR, b.IendR), st0.J(b.JstrR, b.JendR))
    assert cu.differing(a, w) == ["t"]
    for it in range(b.NT):
        ta, tw = a["t"][:, :, :, nnew, it], w["t"][:, :, :, nnew, it]
        for lev in range(3):
            if lev != nnew:
                assert cu.same(a["t"][:, :, :, lev, it], w["t"][:, :, :, lev, it])
        ic = c.ic(it + 1)
        if not ic:
            assert cu.same(ta, tw), it
            continue
        t0 = ta[R]
        want = t0 + (p.dt * c["Tnudgcof"][R + (slice(None), ic - 1)]) * (c["tclm"][R + (slice(None), ic - 1)] - t0)
        if mask:
            want = want * st0["rmask"][R][:, :, None]
        assert np.array_equal(tw[R], want), (it, float(np.abs(tw[R] - want).max()))
        assert not np.array_equal(tw[R], t0)
        for g in range(1, b.NghostPoints + 1):            # E-W periodic images
            assert np.array_equal(tw[st0.I(1 - g)], tw[st0.I(b.Lm + 1 - g)])
            assert np.array_equal(tw[st0.I(b.Lm + g)], tw[st0.I(g)])


@pytest.mark.parametrize("config", ["UPWELLING", "BENCHMARK_TINY"])
def test_rhs3d_term_bit_for_bit(config):
    """u = v = 0, no fluxes, no stresses, random ru / rv(nrhs) coming in: every other addition of rhs3d_tile is a zero, so
    ru with = ru without + the term in the order of rhs3d.F:574-580, and rufrc is its k-sum in the reference's order"""
    st0 = util.prepared_state(config)
    rng = np.random.default_rng(3)
    for name in ("u", "v", "W", "Huon", "Hvom", "sustr", "svstr", "bustr", "bvstr"):
        st0[name][:] = 0.0
    st0["ru"][:] = rng.standard_normal(st0["ru"].shape)
    st0["rv"][:] = rng.standard_normal(st0["rv"].shape)
    c = cu.random_clima(st0)
    a = cu.run_hip(st0, [("rhs3d_tile", S3D)])
    w = cu.run_hip(st0, [("rhs3d_tile", S3D)], c)
    b, nrhs, N = st0.b, S3D.nrhs - 1, st0.b.N
    assert sorted(cu.differing(a, w)) == ["ru", "rufrc", "rv", "rvfrc"]
    cof, Hz = c["M3nudgcof"], st0["Hz"]
    for comp, clm, frc, om, on, I, J, di, dj in (
            ("ru", "uclm", "rufrc", "om_u", "on_u", st0.I(b.IstrU, b.Iend), st0.J(b.Jstr, b.Jend), 1, 0),
            ("rv", "vclm", "rvfrc", "om_v", "on_v", st0.I(b.Istr, b.Iend), st0.J(b.JstrV, b.Jend), 0, 1)):
        Im, Jm = slice(I.start - di, I.stop - di), slice(J.start - dj, J.stop - dj)
        cff = 0.25 * (cof[Im, Jm] + cof[I, J]) * st0[om][I, J][:, :, None] * st0[on][I, J][:, :, None]
        term = cff * (Hz[Im, Jm] + Hz[I, J]) * (c[clm][I, J] - 0.0)
        want = a[comp][I, J, 1:, nrhs] + term
        got = w[comp][I, J, 1:, nrhs]
        assert np.array_equal(got, want), (comp, float(np.abs(got - want).max()))
        assert np.abs(term).max() > 0.0
        ksum = want[:, :, 0].copy()
        for k in range(1, N):
            ksum = ksum + want[:, :, k]
        # the surface and bottom stress follow as + 0.0 and + (-0.0): rhs3d.F:1560-1660 with zero stresses
        assert np.array_equal(w[frc][I, J], ksum), frc


def _flat_channel():
    """tests/test_known_answers.py::_channel: UPWELLING's periodic channel made flat and homogeneous, at rest"""
    st = ana.make_tile("UPWELLING", perturb=0.0, overrides=dict(dt=300.0, ndtfast=30, theta_s=0.0, theta_b=0.0, uv_vis2=0))
    st["h"][:] = 150.0
    st["f"][:] = 0.0
    st["fomn"][:] = 0.0
    st["t"][:, :, :, :, 0] = 14.0
    st["t"][:, :, :, :, 1] = 35.0
    for name in ("sustr", "svstr", "bustr", "bvstr", "stflx", "btflx", "srflx"):
        st[name][:] = 0.0
    st["Akv"][:] = 1.0e-5
    st["Akt"][:] = 1.0e-6
    for name in ("zeta", "ubar", "vbar", "u", "v", "Zt_avg1"):
        st[name][:] = 0.0
    return st


def test_step2d_term_closed_form():
    """flat bottom, everything at rest, rufrc = rvfrc = 0, f = 0, no stress, no viscosity; one corrector call with
    iif > 1: the only non-zero contribution to rhs_ubar is the nudging term and ubar(knew) is a closed form of it
    (step2d_LF_AM3.h:2150-2200 with ubar(kstp) = 0, rubar = 0), mirrored operation for operation.  The metrics of this
    grid come from the row table; the coefficient is a full 2-D array."""
    st0 = _flat_channel()
    c = cu.random_clima(st0)
    a = cu.run_hip(st0, [("step2d", S_CORR)])
    w = cu.run_hip(st0, [("step2d", S_CORR)], c)
    b, p = st0.b, st0.p
    h, pm, pn = st0["h"], st0["pm"], st0["pn"]
    a1 = 0.5 * p.dtfast * 5.0 / 12.0
    assert not a["ubar"].any() and not a["vbar"].any()
    for comp, clm, om, on, I, J, di, dj in (("ubar", "ubarclm", "om_u", "on_u", st0.I(b.IstrU, b.Iend), st0.J(b.Jstr, b.Jend), 1, 0),
                                            ("vbar", "vbarclm", "om_v", "on_v", st0.I(b.Istr, b.Iend), st0.J(b.JstrV, b.Jend), 0, 1)):
        Im, Jm = slice(I.start - di, I.stop - di), slice(J.start - dj, J.stop - dj)
        D0, Dm = 0.0 + h[I, J], 0.0 + h[Im, Jm]                             # Drhs = zeta(krhs) + h
        cff = 0.25 * (c["M2nudgcof"][Im, Jm] + c["M2nudgcof"][I, J]) * st0[om][I, J] * st0[on][I, J]
        rhs = cff * (Dm + D0) * (c[clm][I, J] - 0.0)
        cffm = (pm[I, J] + pm[Im, Jm]) * (pn[I, J] + pn[Im, Jm])
        fac = 1.0 / (D0 + Dm)                                               # 1 / (Dnew(i) + Dnew(i-1)), zeta(knew) = 0
        want = (0.0 + cffm * (a1 * rhs + 0.0 - 0.0)) * fac
        got = w[comp][I, J, S_CORR.knew - 1]
        assert np.array_equal(got, want), (comp, float(np.abs(got - want).max()))
        assert np.abs(want).max() > 0.0


# ---------------------------------------------------------------- 3. the edges --
X_OUT, FAC = 2.0e-4, 7.5


def _edge_pair(st0, entry, s, c):
    """run A: tau from roms_params_t (obc_out = X, obc_in = FAC * X); run B: the parameters of the five variables hold
    values that must not be used, tau comes from uniform coefficient arrays = X with obcfac = FAC"""
    sa = cu.radnud(st0.copy(), out=X_OUT, fac=FAC)
    sb = cu.radnud(st0.copy(), out=X_OUT, fac=FAC, others=(0.0123, 0.0456))
    for name in ("zeta_bry", "ubar_bry", "vbar_bry", "u_bry", "v_bry", "t_bry"):
        assert cu.same(sa[name], sb[name])
    return cu.run_hip(sa, [(entry, s)]), cu.run_hip(sb, [(entry, s)], c)


@pytest.mark.parametrize("config", ["UPWELLING", "BENCHMARK_TINY"])
def test_edges_take_tau_from_the_coefficient_arrays(config):
    st0 = util.prepared_state(config, overrides={"EWperiodic": False})
    b = st0.b

    def uniform():
        c = cu.random_clima(st0, obcfac=FAC)
        for name in ("M2nudgcof", "M3nudgcof", "Tnudgcof"):
            c[name][:] = X_OUT
        return c
    # ubar, vbar: one step2d call, predictor and corrector, climatology = ubar(krhs): no interior term
    for s in (S_PRED, S_CORR):
        c = uniform()
        c["ubarclm"][:] = st0["ubar"][:, :, s.krhs - 1]
        c["vbarclm"][:] = st0["vbar"][:, :, s.krhs - 1]
        a, w = _edge_pair(st0, "step2d", s, c)
        assert cu.differing(a, w) == [], ("step2d", s.predictor_2d_step)
    # u, v: step3d_uv applies u3dbc / v3dbc and has no interior term
    a, w = _edge_pair(st0, "step3d_uv", S3D, uniform())
    assert cu.differing(a, w) == []
    # t: coefficients non-zero on the boundary points only; there the numpy update of the term test applies
    c = uniform()
    I, J = st0.I(b.Istr, b.Iend), st0.J(b.Jstr, b.Jend)
    c["Tnudgcof"][I, J] = 0.0
    a, w = _edge_pair(util.hz_weighted_tnew(st0.copy()), "step3d_t", S3D, c)
    assert cu.differing(a, w) == ["t"]
    nnew = S3D.nnew - 1
    R = (st0.I(b.IstrR, b.IendR), st0.J(b.JstrR, b.JendR))
    for it in range(b.NT):
        t0 = a["t"][:, :, :, nnew, it][R]
        cc = c["Tnudgcof"][R + (slice(None), it)]
        want = t0 + (st0.p.dt * cc) * (c["tclm"][R + (slice(None), it)] - t0)
        got = w["t"][:, :, :, nnew, it][R]
        assert np.array_equal(got, want), (it, float(np.abs(got - want).max()))
        assert np.array_equal(got[1:-1, 1:-1], t0[1:-1, 1:-1]) and not np.array_equal(got, t0)
    # the coefficient really is read: another uniform value moves the edges
    c2 = uniform()
    c2["M3nudgcof"][:] = 3.0 * X_OUT
    a3, w3 = _edge_pair(st0, "step3d_uv", S3D, c2)
    assert {"u", "v"} <= set(cu.differing(a3, w3))


# ------------------------------------------------------- 4. tiling invariance --
def _tiles_equal_single(tmp_path, world, ntI, ntJ, config, variant, nsteps=3):
    import mp_gpu_clima_worker as worker
    st0 = worker.tiled_state(config, variant)
    ref = st0.copy()
    be = hip.RomsHip(ref)
    try:
        want = worker.run(be, ref, nsteps)
    finally:
        be.close()
    plain = cu.run_hip(st0, steps=nsteps)
    assert {"t", "u", "v", "ubar", "vbar"} <= set(cu.differing(ref, plain)), "the sponge made no difference"
    tiling_util.spawn_ranks("mp_gpu_clima_worker.py", world, [ntI, ntJ, tmp_path, config, nsteps, variant], timeout=600)
    tiling_util.assert_tiles_equal(tmp_path, world, want, ref.b, worker.FIELDS, owned="Istr:Iend",
                                   rho_ghosts=("zeta", "t", "Hz", "W"))


@pytest.mark.parametrize("ntI,ntJ,config,variant", [(2, 1, "BENCHMARK_TINY", ""), (1, 2, "UPWELLING", ""),
                                                    (2, 2, "UPWELLING", "basin")])
def test_tiled_runs_equal_the_single_tile_run(tmp_path, ntI, ntJ, config, variant):
    _tiles_equal_single(tmp_path, ntI * ntJ, ntI, ntJ, config, variant)


def test_rccl_loopback_equals_the_single_tile_run(tmp_path):
    _tiles_equal_single(tmp_path, 1, 1, 1, "UPWELLING", "rccl")


# ----------------------------------------------------------- 5. known answer --
def test_uniform_tracer_relaxes_exponentially():
    """flat, homogeneous channel at rest, uniform T0, tclm and c: T_n = tclm + (T0 - tclm) (1 - dt c)^n at every point and
    level after n = 100 steps; bound = the project's 1e-10 relative RMS for 100-step runs.  Salinity,
    not nudged, stays where the run without climatology has it."""
    st0 = _flat_channel()
    b, p, n = st0.b, st0.p, 100
    T0, tclm, cnud = 14.0, 9.0, 1.0 / (40.0 * p.dt)
    z = np.zeros((st0.ni, st0.nj, b.N, 1))
    c = clima.Clima(b, LnudgeTCLM=[1, 0], Tnudgcof=z + cnud, tclm=z + tclm)
    out = {}
    for key, cl in (("with", c), ("without", None)):
        st = st0.copy()
        st.clima = cl
        be = hip.RomsHip(st)
        try:
            m = main3d.Main3D(be)
            m.initial()
            m.run(n)
            be.to_host()
            be.check_guards()
        finally:
            be.close()
        out[key] = st["t"][:, :, :, m.s.nnew - 1, :][st0.I(b.IstrR, b.IendR), st0.J(b.JstrR, b.JendR)]
    want = tclm + (T0 - tclm) * (1.0 - p.dt * cnud) ** n
    T = out["with"][..., 0]
    err = float(np.sqrt(np.mean((T - want) ** 2))) / abs(want)
    print(f"relaxation after {n} steps: T = {float(T.mean())!r}, closed form {want!r}, relative RMS error {err:.3e}")
    assert abs(want - T0) > 1.0
    assert err <= 1.0e-10, err
    assert np.array_equal(out["with"][..., 1], out["without"][..., 1])


# ------------------------------------------------------------------ 6. errors --
def test_set_clima_refusals_leave_the_library_usable():
    st0 = util.prepared_state("UPWELLING")
    c = cu.random_clima(st0, tracers=[1, 0])
    want = cu.run_hip(st0, [("rhs3d_tile", S3D)], c)
    plain = cu.run_hip(st0, [("rhs3d_tile", S3D)])            # before `be` below: the library holds one context
    lib = hip.load()
    args = c.c_args()
    # wrong order of calls: before init, and before bounds / params
    assert hip.RomsHip._live is None
    assert lib.roms_hip_set_clima(*args) != 0 and b"come first" in lib.roms_hip_last_error()
    assert lib.roms_hip_init(0, 1, 1, 0, None) == 0
    try:
        assert lib.roms_hip_set_clima(*args) != 0 and b"come first" in lib.roms_hip_last_error()
    finally:
        assert lib.roms_hip_finalize() == 0
    st = st0.copy()
    be = hip.RomsHip(st)
    try:
        # NULL refresh before a first full call
        with pytest.raises(RuntimeError, match="never given"):
            be.set_clima(c, only=("tclm",))
        # a flag without its arrays
        bad = list(args)
        bad[6] = None                                          # LnudgeM3CLM = 1, uclm = NULL
        assert lib.roms_hip_set_clima(*bad) != 0
        msg = lib.roms_hip_last_error()
        assert b"uclm" in msg and b"never given" in msg
        with pytest.raises(RuntimeError, match="obcfac"):
            bad = list(args)
            bad[11] = -1.0
            be._chk(lib.roms_hip_set_clima(*bad), "set_clima")
        # after the refused calls nothing is switched on: the entry runs as without climatology ...
        be.call("rhs3d_tile", S3D)
        be.to_host()
        assert cu.differing(st, plain) == []
        # ... a full call works, a refresh of one array with the rest kept works, and a changed switch needs its arrays
        st.arr["ru"][:] = st0["ru"]
        st.arr["rufrc"][:] = st0["rufrc"]
        st.arr["rv"][:] = st0["rv"]
        st.arr["rvfrc"][:] = st0["rvfrc"]
        be.to_device(["ru", "rv", "rufrc", "rvfrc"])
        keep = c["uclm"].copy()
        c["uclm"][:] = 0.0
        be.set_clima(c)
        c["uclm"][:] = keep
        be.set_clima(c, only=("uclm",))
        be.call("rhs3d_tile", S3D)
        be.to_host()
        assert cu.differing(st, want) == []
        c2 = cu.random_clima(st0, tracers=[1, 1])
        with pytest.raises(RuntimeError, match="never given"):
            be.set_clima(c2, only=("uclm",))
        be.check_guards()
    finally:
        be.close()
