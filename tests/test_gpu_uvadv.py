"""-m gpu: the selectable momentum advection of roms_params_t.uv_adv (UV_C2ADVECTION, UV_C4ADVECTION, UV_SADVECTION;
k_rhs3d_lds<HADV, VADV>, k_rhs3d_vspline, k2d_mom_lds<..., C2>).

The CPU oracle and the reference builds only have the default pair, so the evidence is of the kinds of
tests/test_gpu_clima.py: the numpy mirror of tests/uvadv_util.py (pinned against the oracle for the default pair by
tests/test_uvadv.py), known answers where the schemes must coincide, the telescoping of the vertical fluxes, and the
error convention.  Every run ends with check_guards().
"""
import ctypes as C
import numpy as np
import pytest

import clima_util as cu
import tiling_util
import util
import uvadv_util as uv
from roms_trunk_mgh_amd import abi, ana, hip, main3d

pytestmark = pytest.mark.gpu

S3D = util.step_idx(iic=5)
S_PRED = util.step_idx(iic=5, iif=3, pred=1, kstp=2, knew=3, krhs=1)
S_CORR = util.step_idx(iic=5, iif=3, pred=0, kstp=1, knew=2, krhs=3)
NEW_PAIRS = [hv for hv in abi.UV_ADV_PAIRS if hv != ("U3", "C4W")]
# three workgroups in x with a partial last one, three in y; N = 6: the k = 2..N-2 loop of the fourth-order vertical
# flux has three levels, N = 4: one
GRID = dict(Lm=130, Mm=10)


def with_scheme(st0, h, v=None):
    st = st0.copy()
    st.p = type(st.p).from_buffer_copy(st.p)
    st.p.uv_adv = h if v is None else abi.uv_adv(h, v)
    return st


def random_state(case, N, seed=7):
    st = util.prepared_state("UPWELLING", overrides=dict(GRID, N=N, **({"EWperiodic": False} if case == "basin" else {})))
    assert (st.b.Lm, st.b.Mm, st.b.N) == (GRID["Lm"], GRID["Mm"], N) and bool(st.b.EWperiodic) == (case == "channel")
    rng = np.random.default_rng(seed)
    for name, amp in (("u", 0.3), ("v", 0.3), ("Huon", 4.0e3), ("Hvom", 4.0e3), ("W", 50.0), ("ru", 10.0), ("rv", 10.0)):
        st[name][:] = amp * rng.standard_normal(st[name].shape)
    return st


_default = {}


def default_run(case, N):
    if (case, N) not in _default:
        _default[case, N] = cu.run_hip(random_state(case, N), [("rhs3d_tile", S3D)])
    return _default[case, N]


# ------------------------------------------------------------ 1. the mirror --
@pytest.mark.parametrize("N", [6, 4])
@pytest.mark.parametrize("case", ["channel", "basin"])
def test_rhs3d_tile_equals_the_mirror_bit_for_bit(case, N):
    st0 = random_state(case, N)
    (IU, JU), (IV, JV) = uv.ranges(st0)
    n = S3D.nrhs - 1
    base = default_run(case, N)
    for h, v in NEW_PAIRS:
        got = cu.run_hip(with_scheme(st0, h, v), [("rhs3d_tile", S3D)])
        want = uv.rhs3d_tile(st0, S3D, h, v)
        for name, I, J in (("ru", IU, JU), ("rv", IV, JV)):
            a, w = got[name][I, J, 1:, n], want[name][I, J, 1:]
            assert np.array_equal(a, w), (h, v, name, float(np.abs(a - w).max()))
            assert not np.array_equal(a, base[name][I, J, 1:, n]), (h, v, name, "the scheme was ignored")
            assert cu.same(got[name][:, :, :, 1 - n], st0[name][:, :, :, 1 - n])
        for name, I, J in (("rufrc", IU, JU), ("rvfrc", IV, JV)):
            assert np.array_equal(got[name][I, J], want[name][I, J]), (h, v, name)
        assert sorted(cu.differing(got, st0)) == ["ru", "rufrc", "rv", "rvfrc"], (h, v)


@pytest.mark.parametrize("s", [S_PRED, S_CORR], ids=["predictor", "corrector"])
@pytest.mark.parametrize("case", ["channel", "basin"])
def test_step2d_c2_differs_from_the_default(case, s):
    st0 = random_state(case, 6)
    base = cu.run_hip(st0, [("step2d", s)])
    for v in ("C2", "SPLINES"):
        got = cu.run_hip(with_scheme(st0, "C2", v), [("step2d", s)])
        assert {"ubar", "vbar"} <= set(cu.differing(got, base)), v
        assert np.isfinite(got["ubar"]).all() and np.isfinite(got["vbar"]).all()
    for h, v in (("U3", "SPLINES"), ("C4", "C4"), ("C4", "SPLINES")):        # the 2-D step keeps the fourth-order form
        assert cu.differing(cu.run_hip(with_scheme(st0, h, v), [("step2d", s)]), base) == [], (h, v)


@pytest.mark.parametrize("s", [S_PRED, S_CORR], ids=["predictor", "corrector"])
@pytest.mark.parametrize("pair", [("C2", "C2"), ("C2", "SPLINES"), ("U3", "C4W")], ids=["C2-C2", "C2-SPLINES", "default"])
@pytest.mark.parametrize("case", ["channel", "basin"])
def test_step2d_equals_the_mirror_bit_for_bit(case, pair, s):
    """zero pressure gradient (uvadv_util.zero_pressure_gradient), a predictor and a corrector call with iif > 1: the
    right-hand side is 0 - (cff1 + cff2) of the advection (step2d_LF_AM3.h:1257-1283) with DUon, DVom of :509-544, so
    rubar / rvbar(krhs) of the predictor and ubar / vbar(knew) of the leap-frog and of the Adams-Moulton step (which
    reads rubar of two levels) follow from the mirror's term -- C2 under H = C2, the fourth-order form otherwise (that
    one is pinned against the oracle in tests/test_uvadv.py).  The channel takes the one-launch call, the basin the
    split sequence."""
    st0 = uv.zero_pressure_gradient(random_state(case, 6))
    got = cu.run_hip(with_scheme(st0, *pair), [("step2d", s)])
    want = uv.step2d_expected(st0, s, got["zeta"][:, :, s.knew - 1], c2=pair[0] == "C2")
    (IU, JU), (IV, JV) = uv.ranges(st0)
    for bar, rbar, I, J in (("ubar", "rubar", IU, JU), ("vbar", "rvbar", IV, JV)):
        a, w = got[bar][I, J, s.knew - 1], want[bar][I, J]
        assert np.array_equal(a, w), (bar, float(np.abs(a - w).max()))
        assert np.abs(want["rhs_" + bar][I, J]).max() > 0.0
        if s.predictor_2d_step:
            assert np.array_equal(got[rbar][I, J, s.krhs - 1], want["rhs_" + bar][I, J]), rbar


# -------------------------------------------------------- 2. known answer --
def test_schemes_coincide_on_linear_integer_fields():
    """basin; u, v, Huon, Hvom integer-valued and linear in i and j, constant in k, W a uniform integer: every second
    difference is an exact zero and the spline's CF is zero, so all horizontal and all vertical forms reduce to the same
    products of small integers -- ru, rv of the six pairs are bit-equal"""
    st0 = random_state("basin", 6)
    b = st0.b
    ii = np.arange(b.LBi, b.UBi + 1, dtype=np.float64)[:, None, None]
    jj = np.arange(b.LBj, b.UBj + 1, dtype=np.float64)[None, :, None]
    one = np.ones((1, 1, b.N))
    for lev in range(2):
        st0["u"][:, :, :, lev] = (2.0 * ii - 3.0 * jj + 5.0) * one
        st0["v"][:, :, :, lev] = (-1.0 * ii + 2.0 * jj - 7.0) * one
    st0["Huon"][:] = (3.0 * ii + 1.0 * jj + 11.0) * one
    st0["Hvom"][:] = (-2.0 * ii + 4.0 * jj + 3.0) * one
    st0["W"][:] = 3.0
    base = cu.run_hip(st0, [("rhs3d_tile", S3D)])
    assert not cu.same(base["ru"], st0["ru"])
    for h, v in NEW_PAIRS:
        got = cu.run_hip(with_scheme(st0, h, v), [("rhs3d_tile", S3D)])
        assert cu.differing(got, base) == [], (h, v)


# ------------------------------------------------------------ 3. refusals --
def test_other_values_are_refused_and_the_library_stays_usable():
    st0 = random_state("channel", 4)
    want = cu.run_hip(with_scheme(st0, "C4", "C4"), [("rhs3d_tile", S3D), ("step2d", S_PRED)])
    bad = [abi.uv_adv("U3", "C2"), abi.uv_adv("C2", "C4W"), 2, -1]
    st = with_scheme(st0, "C4", "C4")
    be = hip.RomsHip(st)
    try:
        for value in bad:
            st.p.uv_adv = value
            be._chk(be.l.roms_hip_set_params(C.byref(st.p)), "set_params")
            for entry, s in (("rhs3d_tile", S3D), ("rhs3d", S3D), ("step2d", S_PRED)):
                with pytest.raises(RuntimeError, match="uv_adv"):
                    be.call(entry, s)
            with pytest.raises(RuntimeError, match="uv_adv"):
                be.step2d_loop(util.step_idx(iic=5), 1)
        be.to_host()
        assert cu.differing(st, st0) == []                   # a refused call has changed nothing
        st.p.uv_adv = abi.uv_adv("C4", "C4")
        be._chk(be.l.roms_hip_set_params(C.byref(st.p)), "set_params")
        be.call("rhs3d_tile", S3D)
        be.call("step2d", S_PRED)
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    assert cu.differing(st, want) == []


# --------------------------------------------------------- 4. telescoping --
@pytest.mark.parametrize("case", ["channel", "basin"])
def test_vertical_fluxes_cancel_in_the_vertical_integral(case):
    """Coriolis off, zero stresses: rufrc is the k-sum of ru, and FC(0) = FC(N) = 0, so under every vertical scheme it
    equals the k-sum of the mirror's ru without the vertical term, up to rounding: 8 N 2^-52 (sum_k |ru_k| + 2 sum_k |FC_k|)
    per column, from the mirror's own terms"""
    st0 = random_state(case, 6)
    st0.p = type(st0.p).from_buffer_copy(st0.p)
    st0.p.uv_cor = 0
    for name in ("sustr", "svstr", "bustr", "bvstr"):
        st0[name][:] = 0.0
    N = st0.b.N
    (IU, JU), (IV, JV) = uv.ranges(st0)
    for h, v in abi.UV_ADV_PAIRS:
        got = cu.run_hip(with_scheme(st0, h, v), [("rhs3d_tile", S3D)])
        m = uv.rhs3d_tile(st0, S3D, h, v)
        for frc, r, FC, I, J in (("rufrc", "ru_h", "FCu", IU, JU), ("rvfrc", "rv_h", "FCv", IV, JV)):
            hsum = m[r][I, J, 1:].sum(axis=2)
            bound = 8.0 * N * 2.0 ** -52 * (np.abs(m[r][I, J, 1:]).sum(axis=2) + 2.0 * np.abs(m[FC][I, J]).sum(axis=2))
            err = np.abs(got[frc][I, J] - hsum)
            print(f"{case} ({h}, {v}) {frc}: largest error / bound = {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), (h, v, frc, float((err / bound).max()))
            assert np.abs(m[FC][I, J]).max() > 0.0


# -------------------------------------------------------------- 5. tiling --
@pytest.mark.parametrize("ntI,ntJ", [(2, 1), (1, 2)])
@pytest.mark.parametrize("h,v", [("C4", "SPLINES"), ("C2", "C2")])
def test_tiled_runs_equal_the_single_tile_run(tmp_path, ntI, ntJ, h, v):
    """three whole steps of BENCHMARK_TINY on two tiles over the gloo relay equal the one-tile run on owned and ghost
    points; (C2, C2) takes the deferred-flux 2-D call with the second-order form"""
    import mp_gpu_uvadv_worker as worker
    config, nsteps, world = "BENCHMARK_TINY", 3, ntI * ntJ
    ref = worker.tiled_state(config, h, v)
    assert ref.p.uv_adv == abi.uv_adv(h, v)
    be = hip.RomsHip(ref)
    try:
        want = worker.run(be, ref, nsteps)
    finally:
        be.close()
    plain = cu.run_hip(ana.make_tile(config, perturb=1.0), steps=nsteps)
    assert {"u", "v", "ubar", "vbar"} <= set(cu.differing(ref, plain)), "the scheme made no difference"
    tiling_util.spawn_ranks("mp_gpu_uvadv_worker.py", world, [ntI, ntJ, tmp_path, config, nsteps, h, v], timeout=600)
    tiling_util.assert_tiles_equal(tmp_path, world, want, ref.b, worker.FIELDS, owned="Istr:Iend",
                                   rho_ghosts=("zeta", "t", "Hz", "W"))


# --------------------------------------------------------------- 6. graph --
def test_loop_2d_graph_equals_the_eager_loop_under_c2():
    """20 steps of one-tile BENCHMARK_TINY under (C2, C2): LOOP_2D replayed as a hipGraph (roms_hip_step2d_loop) against
    the same sequence of single step2d calls driven from here (main3d.F:592-700), bit for bit; every field finite"""
    st0 = ana.make_tile("BENCHMARK_TINY", perturb=1.0, overrides={"uv_hadv": "C2", "uv_vadv": "C2"})
    out = {}
    for mode in ("graph", "eager"):
        st = st0.copy()
        be = hip.RomsHip(st)
        try:
            if mode == "eager":
                def loop(s, indx1, be=be, nfast=st.p.nfast):
                    predictor = 0
                    for my_iif in range(1, nfast + 2):
                        next_indx1 = 3 - indx1
                        if not predictor:
                            predictor = 1
                            s.iif = my_iif
                            s.kstp = indx1 if s.iif == 1 else 3 - indx1
                            s.knew, s.krhs = 3, indx1
                        s.predictor_2d_step = predictor
                        be.call("step2d", s)
                        if predictor:
                            predictor = 0
                            s.knew = next_indx1
                            s.kstp, s.krhs = 3 - s.knew, 3
                            if s.iif < nfast + 1:
                                indx1 = next_indx1
                        s.predictor_2d_step = predictor
                        if s.iif < nfast + 1:
                            be.call("step2d", s)
                    return indx1
                be.step2d_loop = loop
            m = main3d.Main3D(be)
            m.initial()
            m.run(20)
            be.to_host()
            be.check_guards()
        finally:
            be.close()
        out[mode] = st
    assert cu.differing(out["graph"], out["eager"]) == []
    for name in ("zeta", "ubar", "vbar", "u", "v", "t", "ru", "rv", "rufrc", "rvfrc"):
        assert np.isfinite(out["graph"][name]).all(), name
    plain = cu.run_hip(ana.make_tile("BENCHMARK_TINY", perturb=1.0), steps=20)
    assert {"u", "v", "ubar", "vbar"} <= set(cu.differing(out["graph"], plain))
