"""-m gpu: parity on a curvilinear grid -- metrics, Coriolis parameter and mixing coefficients varying in i and j.

On the analytic grids of roms_trunk_mgh_amd/ana.py pn is a constant, pm and f depend on j at most, dndx is zero and the
mixing coefficients are uniform, so a kernel that reads the western neighbour's metric, pm for pn, on_u for on_v or
visc2_r for visc2_p computes the same bits as a correct one, on every grid the other parity tests use.  Here every
state is passed through tests/curv_util.py::curvilinear first, on one shape -- 66 x 9 x 5: two workgroups in x with two
live columns in the second, three rows of workgroups with one live row in the last -- with the seam land, dry cells and
sources of tests/test_gpu_wide.py, whose state builders this module reuses.

  1. test_curv_kernels: single calls, HIP against the CPU oracle, for every kernel family (tw.FAMILIES) on the
     UPWELLING and the BENCHMARK_TINY configuration (CONFIGS_OF) in the four variants of tw.VARIANTS: 1e-12 of each
     field's maximum on every registered field, equal return values, guard bands, the oracle changed something; the
     barotropic entries also: the general kernel was chosen (row_metrics_state() == 2).
     test_curv_clima: the climatology terms against the mirrors of tests/clima_util.py, as tw.test_wide_clima.
     test_curv_set_avg: set_avg against the restatement of tests/avg_util.py (avgw3d reads pm, pn).
  2. test_row_table_detector: each of the eighteen arrays of k_rowm_build, one value changed at the western-most and
     at the eastern-most column the barotropic step reads (found with the oracle, edge_columns), with two and with
     three ghost points, on the channel and in a closed basin.  test_row_table_follows_uploads: the same within one
     context, through the upload of single fields.
  3. test_curv_runs: 10 whole steps with physics and diagnostics, 1e-10 relative RMS.

tests/test_curv_shapes.py checks the same states without a GPU: the grid varies between every pair of neighbours, the
oracle's result depends on every array a routine reads at the point it reads it (READS), the runs stay finite."""
import numpy as np
import pytest

import avg_util as au
import clima_util as cu
import curv_util as cv
import test_gpu_wide as tw
import util
from roms_trunk_mgh_amd import abi

pytestmark = pytest.mark.gpu
TOL = tw.TOL                            # 1e-12: the per-call bound of tests/test_basin.py and tests/test_gpu_wide.py
DIMS = dict(Lm=66, Mm=9, N=5)
CONFIGS = ("UPWELLING", "BENCHMARK_TINY")
# the builders of these labels choose the configuration themselves (tests/test_gpu_wide.py::_physics, _wet, _sources)
OWN_CONFIG = {"bulk_flux": "BENCHMARK_TINY", "lmd_vmix": "BENCHMARK_TINY"}
OWN_CONFIG_FAMILY = {"wet": "UPWELLING", "sources": "UPWELLING"}
BAROTROPIC = ("step2d", "step2d_loop")


def shape(config):
    """a shape for the builders of tests/test_gpu_wide.py (tw.shape_of)"""
    return DIMS, config


def configs_of(fam, label):
    own = OWN_CONFIG.get(label) or OWN_CONFIG_FAMILY.get(fam)
    return (own,) if own else CONFIGS


def check_geometry(b):
    """two workgroups over every x range, the second with two live columns; three rows of workgroups, the last with one
    live row"""
    assert (b.Lm, b.Mm, b.N) == (DIMS["Lm"], DIMS["Mm"], DIMS["N"]) and b.Istr == tw.I0
    nbx = {k: tw.nblk(*r) for k, r in tw.x_ranges(b).items()}
    nby = tw.nblk(b.Jstr, b.Jend, tw.BLK_Y)
    assert set(nbx.values()) == {2} and b.Iend - b.Istr + 1 - tw.BLK_X == 2
    assert nby == 3 and b.Jend - b.Jstr + 1 - 2 * tw.BLK_Y == 1
    return nbx


def kernel_cases():
    out = []
    for fam, (_, labels) in tw.FAMILIES.items():
        for label in labels:
            for config in configs_of(fam, label):
                for variant in tw.APPLIES.get(fam, tw.VARIANTS):
                    out.append(pytest.param(fam, label, config, variant, id=f"{label}-{config}-{variant}"))
    return out


def build(fam, label, config, variant):
    st0, calls = tw.FAMILIES[fam][0](label, shape(config), variant)
    check_geometry(st0.b)
    tw.check_seam(st0, variant, wet=bool(st0.p.wet_dry))
    cv.curvilinear(st0)
    assert st0.p.curvgrid == 1
    strengthen(st0, label, config)
    return st0, calls


# BENCHMARK_TINY at this size has cells of 600 km x 250 km, so dt pm pn is tiny and the terms pre_step3d and step3d_uv
# multiply by it vanish against Hz t and Hz u: the fluxes and right-hand sides those terms hold are scaled up (as
# tw._detune does for other entries) until a one-point shift of pm or pn moves the result by more than 100 x the bound
STRENGTHEN = {"pre_step3d": (("Huon", 300.0), ("Hvom", 300.0)), "step3d_uv": (("ru", 1.0e4), ("rv", 1.0e4))}


def strengthen(st, label, config):
    kernel = label.split(":")[0]
    if config == "BENCHMARK_TINY" and kernel in STRENGTHEN and label.split(":")[-1] not in ("wet", "src"):
        for name, factor in STRENGTHEN[kernel]:
            st[name] *= factor


def runs_barotropic(calls):
    return any(k in BAROTROPIC for k, _ in calls)


# ---------------------------------------------------------------------------- 1. single calls against the oracle --
@pytest.mark.parametrize("fam,label,config,variant", kernel_cases())
def test_curv_kernels(fam, label, config, variant):
    from roms_trunk_mgh_amd import hip
    st0, calls = build(fam, label, config, variant)
    st_h = st0.copy()
    h = hip.RomsHip(st_h)
    try:
        r_h = tw.run_calls(h, calls)
        state = h.row_metrics_state()
        h.to_host()
        h.check_guards()
    finally:
        h.close()
    st_o, r_o = tw.run_oracle(st0, calls)
    diffs = util.compare_states(st_h, st_o)
    print(label, config, variant, "max relative differences:", diffs)
    assert all(v <= TOL for v in diffs.values()), diffs
    assert len(r_h) == len(r_o)
    for a, o in zip(r_h, r_o):
        assert np.array_equal(a, o), (a, o)
    assert tw.vacuous_ok(label, variant) or util.compare_states(st_o, st0), "kernel did not modify anything: test is vacuous"
    if runs_barotropic(calls):
        assert state == 2, state


def clima_state(variant, entry):
    st0 = tw.prepared(shape("UPWELLING"), variant)
    if entry == "step3d_t":
        util.hz_weighted_tnew(st0)
    check_geometry(st0.b)
    tw.check_seam(st0, variant)
    return cv.curvilinear(st0)


@pytest.mark.parametrize("variant", tw.VARIANTS)
def test_curv_clima(variant):
    """tests/test_gpu_wide.py::test_wide_clima on the curvilinear grid.  Momentum: uclm = u(nrhs), ubarclm = ubar(krhs),
    so the term is zero at every point and the result equals the run without, bit for bit.  Tracers: t(nnew) =
    mask(t0 + (dt c)(tclm - t0)) on the whole R range, mirrored in numpy."""
    s3, sp, sc = util.step_idx(iic=5), util.step_idx(iic=5, iif=3, pred=1, kstp=2, knew=3, krhs=1), \
        util.step_idx(iic=5, iif=3, pred=0, kstp=1, knew=2, krhs=3)
    for entry, s in (("rhs3d_tile", s3), ("step2d", sp), ("step2d", sc)):
        st0 = clima_state(variant, entry)
        b = st0.b
        c = cu.random_clima(st0)
        if variant == "radnud":          # the edges read tau from the coefficients: those of the parameters there
            inner = (st0.I(2, b.Lm - 1), st0.J(2, b.Mm - 1))
            keep = c["M2nudgcof"][inner].copy()
            c["M2nudgcof"][:] = 2.0e-4
            c["M2nudgcof"][inner] = keep
            for sd in range(4):          # obc_in as the library computes it from obcfac
                for var in cu.NUDGED:
                    st0.p.obc_in[sd][abi.LBV[var]] = c.obcfac * 2.0e-4
        if entry == "rhs3d_tile":
            c["uclm"][:] = st0["u"][:, :, :, s.nrhs - 1]
            c["vclm"][:] = st0["v"][:, :, :, s.nrhs - 1]
        else:
            c["ubarclm"][:] = st0["ubar"][:, :, s.krhs - 1]
            c["vbarclm"][:] = st0["vbar"][:, :, s.krhs - 1]
        a = cu.run_hip(st0, [(entry, s)])
        w = cu.run_hip(st0, [(entry, s)], c)
        assert cu.differing(a, w) == [], (entry, s.predictor_2d_step)
        assert cu.differing(a, st0) != []
    if variant == "radnud":              # (RadNud edges: tau itself changes with the arrays)
        return
    st0 = clima_state(variant, "step3d_t")
    b, p, nnew = st0.b, st0.p, s3.nnew - 1
    c = cu.random_clima(st0, tracers=[0, 1])
    a = cu.run_hip(st0, [("step3d_t", s3)])
    w = cu.run_hip(st0, [("step3d_t", s3)], c)
    R = (st0.I(b.IstrR, b.IendR), st0.J(b.JstrR, b.JendR))
    assert cu.differing(a, w) == ["t"]
    assert cu.same(a["t"][:, :, :, nnew, 0], w["t"][:, :, :, nnew, 0])
    t0, tw_ = a["t"][:, :, :, nnew, 1][R], w["t"][:, :, :, nnew, 1][R]
    want = t0 + (p.dt * c["Tnudgcof"][R + (slice(None), 0)]) * (c["tclm"][R + (slice(None), 0)] - t0)
    if st0.p.masking:
        want = want * st0["rmask"][R][:, :, None]
    assert np.array_equal(tw_, want), float(np.abs(tw_ - want).max())
    assert not np.array_equal(tw_, t0)


def avg_state(periodic):
    ov = dict(DIMS) if periodic else dict(DIMS, EWperiodic=False)
    st = util.prepared_state("BENCHMARK_TINY", overrides=ov)
    check_geometry(st.b)
    return cv.curvilinear(st)


@pytest.mark.parametrize("periodic", [True, False])
def test_curv_set_avg(periodic):
    """tests/test_gpu_avg.py::test_every_call_equals_the_restatement (its first schedule with a window of three steps) on
    the curvilinear grid, a channel and a basin: avgw3d divides by pm pn at the point"""
    from roms_trunk_mgh_amd import hip
    from test_gpu_avg import SOURCES, _compare, _randomise
    st = avg_state(periodic)
    b = st.b
    sel = au.all_in_scope(b.NT)
    assert ("avgw3d", 0) in sel
    rng = np.random.default_rng(7)
    be = hip.RomsHip(st)
    try:
        kw = dict(nAVG=3, ntsAVG=1, ntstart=1, nrrec=0)
        be.set_averages(au.averages_of(b, sel, **kw))
        ref = au.AvgRef(b, False, 3, 1, 1, 0, sel)
        seen = 0
        for k, iic in enumerate(range(1, 1 + 2 * 3 + 2)):
            _randomise(st, rng)
            be.to_device(SOURCES)
            s = util.step_idx(iic=iic, kstp=1 + k % 3, nrhs=1 + k % 2)
            be.call("set_avg", s)
            ph = ref.set_avg(st, s)
            seen |= sum(1 << q for q in range(4) if ph[q])
            _compare(be, ref, (kw, iic))
        assert (seen & 7) == 7                          # initialised, accumulated and closed
        assert float(np.abs(ref.avg[("avgw3d", 0)]).max()) > 0.0
        be.check_guards()
    finally:
        be.close()


# ------------------------------------------------------------------------- 2. the row-table detector at its edges --
# the arrays of k_rowm_build (csrc/k_step2d_mom.hip): fifteen metrics (a difference: state 2, the general kernel), then
# the resting depth and the viscosity coefficients (a difference: state 1, metrics from the table, these from the arrays)
ROW_METRICS = ("pm", "pn", "on_u", "om_v", "fomn", "dndx", "dmde", "pmon_r", "pnom_r", "pmon_p", "pnom_p", "om_r", "on_r",
               "om_p", "on_p")
ROW_OTHERS = ("h", "visc2_r", "visc2_p")
ROW = 5                                 # the row of the changed value: water at both edges on the island grid
GHOSTS = {2: {}, 3: tw.DIF4["BENCHMARK_TINY"]}
S_LOOP = dict(iic=4)


def detector_state(nghost, variant):
    """BENCHMARK_TINY (CURVGRID, UV_VIS2, Coriolis): every array of the table independent of i; dndx, which is zero on the
    analytic grid, is given the values of dmde so that a factor changes it.  In a basin the u- and psi-type metrics have
    no column LBi (metrics.F leaves it zero; nothing reads it): it is given the row's value, so that the table is in use
    to begin with (asserted: state 3 before the change)"""
    st = tw.prepared(shape("BENCHMARK_TINY"), variant, GHOSTS[nghost])
    b = st.b
    assert b.NghostPoints == nghost and st.p.uv_vis4 == int(nghost == 3) and st.p.curvgrid == 1 and st.p.uv_vis2 == 1
    st["dndx"][:] = 0.7 * st["dmde"]
    for name in ROW_METRICS + ROW_OTHERS:
        if not b.EWperiodic and name.endswith(("_u", "_p")):
            st[name][0] = st[name][1]
        a = st[name][st.I(max(b.Istr - nghost, b.LBi), min(b.Iend + nghost, b.UBi))]
        assert a.shape[0] >= b.Lm + 2 and (a == a[:1]).all() and float(np.abs(a[:, st.J(ROW)]).min()) > 0.0, name
    return st


def perturbed(st0, name, i, images=False):
    """one value of the array times 1.5; images = True: with its periodic images among the allocated columns"""
    st = st0.copy()
    for q in (util._cells(st, [(i, ROW)]) if images else [(st.I(i), st.J(ROW))]):
        st[name][q] *= 1.5
    return st


def loop_oracle(st0):
    import oracle
    st = st0.copy()
    r = oracle.Oracle(st).step2d_loop(util.step_idx(**S_LOOP), 1)
    return st, r


def edge_columns(st0, name, base=None):
    """(western-most, eastern-most) column of the array that the oracle's step2d_loop reads in row ROW: the outermost of
    Istr-3 .. Istr+2 and of Iend-2 .. Iend+3 (inside the allocated range; om_p in a basin has no psi point west of
    Istr+1) at which that one changed element changes the result"""
    b = st0.b
    base = base or loop_oracle(st0)[0]
    others = [n for n, _, _ in abi.FIELDS if n != name]

    def read(i):
        return b.LBi <= i <= b.UBi and bool(util.compare_states(loop_oracle(perturbed(st0, name, i))[0], base, others))
    west = [i for i in range(b.Istr - 3, b.Istr + 3) if read(i)]
    east = [i for i in range(b.Iend - 2, b.Iend + 4) if read(i)]
    assert west and east, (name, west, east)
    return west[0], east[-1]


def run_loop_hip(st0):
    from roms_trunk_mgh_amd import hip
    st_h = st0.copy()
    h = hip.RomsHip(st_h)
    try:
        r = h.step2d_loop(util.step_idx(**S_LOOP), 1)
        state = h.row_metrics_state()
        h.to_host()
        h.check_guards()
    finally:
        h.close()
    return st_h, r, state


_base_state = {}


def base_state(nghost, variant):
    """row_metrics_state() of the unchanged detector state: 3"""
    if (nghost, variant) not in _base_state:
        _base_state[nghost, variant] = run_loop_hip(detector_state(nghost, variant))[2]
    return _base_state[nghost, variant]


@pytest.mark.parametrize("variant", ["island", "closed"])
@pytest.mark.parametrize("nghost", [2, 3])
@pytest.mark.parametrize("name", ROW_METRICS + ROW_OTHERS)
def test_row_table_detector(name, nghost, variant):
    """The unchanged state uses the table (3).  One element is changed at the outermost column the oracle reads, west
    and east.  In the basin that is the element itself, ghost column or not.  On the one-tile channel the library takes
    a ghost column from its periodic image (the exchange keeps them equal), so the change is made at the column and its
    images, as a grid file holds them; a ghost column that differs from every interior one exists only on several
    tiles (tests/test_gpu_multitile.py, the `edge` variants)."""
    assert base_state(nghost, variant) == 3
    st0 = detector_state(nghost, variant)
    periodic = bool(st0.b.EWperiodic)
    for i in edge_columns(st0, name):
        st = perturbed(st0, name, i, images=periodic)
        st_o, r_o = loop_oracle(st)
        st_h, r_h, state = run_loop_hip(st)
        assert state == (2 if name in ROW_METRICS else 1), (name, i, state)
        diffs = util.compare_states(st_h, st_o)
        assert all(v <= TOL for v in diffs.values()), (name, i, diffs)
        assert r_h == r_o
        assert util.compare_states(st_o, loop_oracle(st0)[0], [n for n, _, _ in abi.FIELDS if n != name])


@pytest.mark.parametrize("name", ["pm", "on_p", "visc2_p"])
def test_row_table_follows_uploads(name):
    """one context: independent of i (3) -> one value changed and that array uploaded (2, or 1 for the second group) ->
    restored and uploaded (3); the oracle's result after every change"""
    from roms_trunk_mgh_amd import hip
    st0 = detector_state(2, "closed")
    i = edge_columns(st0, name)[0]
    st_h = st0.copy()
    names = [n for n, _, _ in abi.FIELDS]
    h = hip.RomsHip(st_h)
    try:
        for phase, src in enumerate((st0, perturbed(st0, name, i), st0)):
            for n in names:
                st_h[n][...] = src[n]
            h.to_device([n for n in names if n != name])
            h.to_device([name])
            r_h = h.step2d_loop(util.step_idx(**S_LOOP), 1)
            state = h.row_metrics_state()
            h.to_host()
            want = 3 if phase != 1 else (2 if name in ROW_METRICS else 1)
            assert state == want, (phase, state)
            st_o, r_o = loop_oracle(src)
            diffs = util.compare_states(st_h, st_o)
            assert all(v <= TOL for v in diffs.values()), (phase, diffs)
            assert r_h == r_o and util.compare_states(st_o, src)
        h.check_guards()
    finally:
        h.close()


# ------------------------------------------------------------------- 2b. the selectable momentum advection --
UVADV_PAIRS = [("C2", "C2"), ("C2", "SPLINES"), ("C4", "SPLINES")]


def uvadv_state(case):
    """tests/test_gpu_uvadv.py::random_state at 66 x 9 x 5 on the curvilinear grid"""
    st = util.prepared_state("UPWELLING", overrides=dict(DIMS, **({"EWperiodic": False} if case == "basin" else {})))
    check_geometry(st.b)
    rng = np.random.default_rng(7)
    for name, amp in (("u", 0.3), ("v", 0.3), ("Huon", 4.0e3), ("Hvom", 4.0e3), ("W", 50.0), ("ru", 10.0), ("rv", 10.0)):
        st[name][:] = amp * rng.standard_normal(st[name].shape)
    return cv.curvilinear(st)


@pytest.mark.parametrize("pair", UVADV_PAIRS, ids=["C2-C2", "C2-SPLINES", "C4-SPLINES"])
@pytest.mark.parametrize("case", ["channel", "basin"])
def test_curv_uvadv_rhs3d_tile(case, pair):
    """tests/test_gpu_uvadv.py::test_rhs3d_tile_equals_the_mirror_bit_for_bit with dndx, dmde, fomn and the metrics of the
    stresses varying in i and j"""
    import uvadv_util as uv
    from test_gpu_uvadv import S3D, with_scheme
    st0 = uvadv_state(case)
    (IU, JU), (IV, JV) = uv.ranges(st0)
    n = S3D.nrhs - 1
    got = cu.run_hip(with_scheme(st0, *pair), [("rhs3d_tile", S3D)])
    with np.errstate(all="ignore"):
        want = uv.rhs3d_tile(st0, S3D, *pair)
        flat = uv.rhs3d_tile(cv.rolled(st0, "dmde", 0), S3D, *pair)
    for name, I, J in (("ru", IU, JU), ("rv", IV, JV)):
        a, w = got[name][I, J, 1:, n], want[name][I, J, 1:]
        assert np.array_equal(a, w), (pair, name, float(np.abs(a - w).max()))
        assert not np.array_equal(flat[name][I, J, 1:], w), "the curvilinear term does not show"
    for name, I, J in (("rufrc", IU, JU), ("rvfrc", IV, JV)):
        assert np.array_equal(got[name][I, J], want[name][I, J]), (pair, name)


@pytest.mark.parametrize("s", ["predictor", "corrector"])
@pytest.mark.parametrize("pair", UVADV_PAIRS, ids=["C2-C2", "C2-SPLINES", "C4-SPLINES"])
@pytest.mark.parametrize("case", ["channel", "basin"])
def test_curv_uvadv_step2d(case, pair, s):
    """tests/test_gpu_uvadv.py::test_step2d_equals_the_mirror_bit_for_bit on the curvilinear grid: the right-hand side
    is 0 - advection + the curvilinear term (the mirror's, pinned against the oracle for the default pair in
    tests/test_curv_shapes.py)"""
    import uvadv_util as uv
    from test_gpu_uvadv import S_CORR, S_PRED, with_scheme
    s = S_PRED if s == "predictor" else S_CORR
    st0 = uv.zero_pressure_gradient(uvadv_state(case))
    assert st0.p.curvgrid == 1
    got = cu.run_hip(with_scheme(st0, *pair), [("step2d", s)])
    assert got is not None
    want = uv.step2d_expected(st0, s, got["zeta"][:, :, s.knew - 1], c2=pair[0] == "C2")
    (IU, JU), (IV, JV) = uv.ranges(st0)
    for bar, rbar, I, J in (("ubar", "rubar", IU, JU), ("vbar", "rvbar", IV, JV)):
        a, w = got[bar][I, J, s.knew - 1], want[bar][I, J]
        assert np.array_equal(a, w), (bar, float(np.abs(a - w).max()))
        assert np.abs(want["rhs_" + bar][I, J]).max() > 0.0
        if s.predictor_2d_step:
            assert np.array_equal(got[rbar][I, J, s.krhs - 1], want["rhs_" + bar][I, J]), rbar


# ------------------------------------------------------------------------------------------- 3. whole steps --
RUNS = {"BENCHMARK_TINY-island": ("BENCHMARK_TINY", "island"), "UPWELLING-open": ("UPWELLING", "open_island"),
        # the seamount's sloping levels with both viscosities rotated to geopotentials (uv_vis2 = uv_vis4 = 2; the
        # viscosities of tests/test_gpu_uvgeo4.py)
        "SEAMOUNT-geo4-closed": ("SEAMOUNT", "closed")}
SEAMOUNT_GEO4 = {"uv_vis2": 2, "uv_vis4": 2, "visc2": 50.0, "visc4": 1.0e8}


def run_state(name):
    config, variant = RUNS[name]
    geo4 = "geo4" in name
    st = tw.tile(shape(config), variant, ov=SEAMOUNT_GEO4 if geo4 else None)
    check_geometry(st.b)
    tw.check_seam(st, variant)
    if geo4:
        tw.check_geo4_run(st)
        assert float(np.ptp(st.interior("h"))) > 100.0            # sloping levels: the rotation acts
    return cv.curvilinear(st)


@pytest.mark.parametrize("name", list(RUNS))
def test_curv_runs(name):
    import oracle
    from roms_trunk_mgh_amd import hip
    from test_gpu_fullsize import _check_prognostic
    st_o = run_state(name)
    st_h = st_o.copy()
    be = hip.RomsHip(st_h)
    try:
        tw.run_steps(be)
        state = be.row_metrics_state()
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    mo = tw.run_steps(oracle.Oracle(st_o))
    _check_prognostic(st_h, st_o, mo)
    assert state == 2
