"""-m gpu: biharmonic viscosity rotated to geopotential surfaces (UV_VIS4 with MIX_GEO_UV, uv3dmix4_geo.h:262-1478;
roms_params_t.uv_vis4 = 2).  k_uv4_geo_first / k_uv4_geo_second through the C ABI against two yardsticks written
separately, both pinned bit for bit to the reference built with the option (tests/test_ref_pinning.py,
tests/test_golden.py): the numpy restatement of tests/uvgeo4_util.py and the CPU oracle's uv3dmix4_geo
(oracle/oracle_uvmix_geo.c).  The kernels evaluate the reference's expressions in the reference's order: the comparisons
with the restatement and with the oracle's uv3dmix4 are for identical bits; the oracle's whole rhs3d at the per-call bound of
tests/test_gpu_wide.py.  Whole steps against the oracle: tests/test_gpu_wide.py, test_gpu_levels.py,
test_gpu_curvilinear.py (10 steps) and tests/test_gpu_main3d.py (100 steps)."""
import numpy as np
import pytest

import curv_util as cv
import reuse_util as ru
import test_gpu_wide as wide
import tiling_util
import util
import uvgeo4_util as G
from roms_trunk_mgh_amd import abi, ana, hip

pytestmark = pytest.mark.gpu
# the viscosities of tests/test_gpu_biharmonic.py; MIX_GEO_UV is one switch for both operators: uv_vis2 = 2 as well
VIS4 = {"UPWELLING": {"uv_vis2": 2, "uv_vis4": 2, "visc4": 4.0e7},
        "SEAMOUNT": {"uv_vis2": 2, "uv_vis4": 2, "visc2": 50.0, "visc4": 1.0e8},
        "BENCHMARK_TINY": {"uv_vis2": 2, "uv_vis4": 2, "visc4": 2.0e10}}
OUT = ("u", "v", "rufrc", "rvfrc")


def _idx():
    return util.step_idx(iic=5, iif=1, pred=0, knew=2, krhs=3)


def _open(st):
    for sd in ("west", "east", "south", "north"):
        for var in ("ubar", "vbar", "u", "v", "t"):
            st.p.lbc[abi.LBS[sd]][abi.LBV[var]] = abi.LBC["Gra"]


def _state(config, variant):
    ov = dict(VIS4[config])
    if variant in ("closed", "open", "mask_closed"):
        ov["EWperiodic"] = False
    st = ru.clone(util.prepared_state(config, overrides=ov, mask="island" if variant.startswith("mask") else None,
                                      wet=(variant == "wet") or None))
    if variant == "open":
        _open(st)
    assert st.b.NghostPoints == 3 and st.p.uv_vis4 == 2
    return st


def _device(st, kernel, s):
    h = hip.RomsHip(st)
    try:
        h.call(kernel, s)
        h.to_host()
    finally:
        h.close()
    return st


def _oracle(st0, kernel, s):
    """the oracle's entry, uv_vis2 = uv_vis4 = 2"""
    import oracle
    st = ru.clone(st0)
    oracle.Oracle(st).call(kernel, s)
    return st


def _expected(st0, kernel, s):
    """the cross-check.  uv3dmix4: the restatement.  rhs3d: the oracle's rhs3d without UV_VIS4 (uv3dmix2_geo for
    uv_vis2 = 2), then the restatement -- the operator reads u, v(nrhs) only and adds to u, v(nnew), rufrc, rvfrc."""
    import oracle
    st = ru.clone(st0)
    if kernel == "rhs3d":
        st.p.uv_vis4 = 0
        oracle.Oracle(st).call("rhs3d", s)
        st.p.uv_vis4 = 2
    return G.uv3dmix4_geo(st, s)


def _same(st_h, st_n, st0):
    for name in OUT:
        assert np.array_equal(st_h[name], st_n[name]), (name, float(np.abs(st_h[name] - st_n[name]).max()))
    assert not np.array_equal(st_n["u"], st0["u"]) and not np.array_equal(st_n["rvfrc"], st0["rvfrc"])


@pytest.mark.parametrize("config", ["UPWELLING", "SEAMOUNT", "BENCHMARK_TINY"])
@pytest.mark.parametrize("variant", ["periodic", "closed", "open", "mask", "mask_closed", "wet"])
@pytest.mark.parametrize("kernel", ["uv3dmix4", "rhs3d"])
def test_uv3dmix4_geo_kernel(config, variant, kernel):
    st0 = _state(config, variant)
    s = _idx()
    st_o = _oracle(st0, kernel, s)
    st_n = _expected(st0, kernel, s)
    for name in OUT:                               # the two yardsticks agree on what they both compute, bit for bit
        assert np.array_equal(st_o[name], st_n[name]), (name, float(np.abs(st_o[name] - st_n[name]).max()))
    st_h = _device(ru.clone(st0), kernel, s)
    _same(st_h, st_n, st0)
    _same(st_h, st_o, st0)
    if kernel == "uv3dmix4":                       # the other registered fields are left alone
        assert sorted(util.compare_states(st_h, st0)) == sorted(OUT)
        assert util.compare_states(st_h, st_o) == {}
    else:                                          # every registered field of the whole rhs3d against the oracle's
        diffs = util.compare_states(st_h, st_o)
        print(config, variant, "rhs3d max relative differences:", diffs)
        assert all(v <= wide.TOL for v in diffs.values()), diffs


@pytest.mark.parametrize("variant,wet,curv", [("island", False, False), ("island", True, False), ("closed", False, False),
                                              ("island", False, True), ("closed", False, True)])
def test_workgroup_seams(variant, wet, curv):
    """130 x 9 x 5: three workgroups in x with two live columns in the last, three in y with one live row; land (and a
    dry cell) on the first seam; again on the curvilinear grid of tests/curv_util.py"""
    st0 = ru.clone(wide.prepared("w3", variant, VIS4["UPWELLING"], wet=wet))
    wide.check_geometry("w3", st0.b)
    wide.check_seam(st0, variant, wet)
    if curv:
        cv.curvilinear(st0)
    s = _idx()
    st_n = G.uv3dmix4_geo(ru.clone(st0), s)
    st_h = _device(ru.clone(st0), "uv3dmix4", s)
    _same(st_h, st_n, st0)
    _same(st_h, _oracle(st0, "uv3dmix4", s), st0)


@pytest.mark.parametrize("ntI,ntJ", [(2, 1), (1, 2)])
def test_tilings(tmp_path, ntI, ntJ):
    """five whole steps with uv_vis2 = 2, uv_vis4 = 2 on masked BENCHMARK_TINY as a closed basin: two tiles against one,
    owned points bit for bit, every field finite"""
    import mp_gpu_uvgeo4_worker as worker
    nsteps = 5
    ref = worker.tiled_state()
    assert ref.p.uv_vis2 == 2 and ref.p.uv_vis4 == 2 and ref.p.masking == 1 and not ref.b.EWperiodic
    be = hip.RomsHip(ref)
    try:
        want = worker.run(be, ref, nsteps)
    finally:
        be.close()
    tiling_util.spawn_ranks("mp_gpu_uvgeo4_worker.py", 2, [ntI, ntJ, tmp_path, nsteps], timeout=300)
    for r, d, _, _ in tiling_util.tiles(tmp_path, 2, ref.b):
        for name in worker.FIELDS:
            assert np.isfinite(d[name]).all() and np.isfinite(want[name]).all(), name
    tiling_util.assert_tiles_equal(tmp_path, 2, want, ref.b, worker.FIELDS, owned="Istr:Iend")


def test_the_switch_acts():
    """on the sloping levels of SEAMOUNT uv_vis4 = 2 gives another u than uv_vis4 = 1; the 2-D operator of step2d has no
    rotation (nor has the reference's): identical bits for the two values"""
    out, bar = [], []
    for vis in (1, 2):
        st = ru.clone(util.prepared_state("SEAMOUNT", overrides={"uv_vis2": 0, "uv_vis4": vis, "visc4": 1.0e8}))
        s = _idx()
        _device(st, "uv3dmix4", s)
        out.append(st["u"][:, :, :, s.nnew - 1].copy())
        st = ru.clone(util.prepared_state("SEAMOUNT", overrides={"uv_vis2": 0, "uv_vis4": vis, "visc4": 1.0e8}))
        st0 = st.copy()
        _device(st, "step2d", util.step_idx(iic=5, iif=2, pred=1, knew=3, krhs=1))
        assert not np.array_equal(st["ubar"], st0["ubar"])
        bar.append(st)
    assert util.max_rel_diff(out[1], out[0]) > 1e-9
    assert util.compare_states(bar[1], bar[0]) == {}


@pytest.mark.parametrize("pair", [(2, 1), (1, 2)])
@pytest.mark.parametrize("kernel", ["uv3dmix2", "uv3dmix4", "rhs3d"])
def test_mixed_pair_is_refused(pair, kernel):
    """MIX_GEO_UV is one switch for both operators: (uv_vis2, uv_vis4) = (2, 1) or (1, 2) is refused by name, nothing is
    changed, and a fresh context works afterwards"""
    st = _state("UPWELLING", "periodic")
    st.p.uv_vis2, st.p.uv_vis4 = pair
    st0 = st.copy()
    s = _idx()
    h = hip.RomsHip(st)
    try:
        with pytest.raises(RuntimeError) as e:
            h.call(kernel, s)
        assert "MIX_GEO_UV" in str(e.value)
        h.to_host()
    finally:
        h.close()
    assert util.compare_states(st, st0) == {}
    good = _state("UPWELLING", "periodic")
    st_n = G.uv3dmix4_geo(ru.clone(good), s)
    _same(_device(ru.clone(good), "uv3dmix4", s), st_n, good)


def test_rotated_uv_vis4_needs_three_ghost_points():
    st = ru.clone(ana.make_tile("UPWELLING", perturb=1.0, overrides={"uv_vis2": 2}))           # two ghost points
    assert st.b.NghostPoints == 2
    st.p.uv_vis4 = 2
    h = hip.RomsHip(st)
    try:
        with pytest.raises(RuntimeError) as e:
            h.call("uv3dmix4", util.step_idx())
        assert "NghostPoints = 3" in str(e.value)
    finally:
        h.close()
    good = _state("UPWELLING", "periodic")
    s = _idx()
    _same(_device(ru.clone(good), "uv3dmix4", s), G.uv3dmix4_geo(ru.clone(good), s), good)


def _m_mix(v):
    """both operators along s-surfaces (1) or rotated to geopotentials (2): one CPP switch"""
    def change(st, be):
        st.p.uv_vis2 = st.p.uv_vis4 = v
        ru.push_params(st, be)
    return change


@pytest.mark.parametrize("app", ru.APPS)
def test_context_reuse(app):
    """one context switched uv_vis4 (with uv_vis2) 1 -> 2 -> 1 through roms_hip_set_params between steps equals fresh
    contexts bit for bit on every registered field, and the switch is felt"""
    st0 = ru.tile(app, dict(ru.DIF4[app], uv_vis2=1))
    changes = [(_m_mix(2), ru.M_STEPS), (_m_mix(1), ru.M_STEPS)]
    st_c, m_c, _, snap = ru.run_continued(st0, changes, True)
    st_f, _ = ru.run_fresh(snap, changes)
    assert ru.differing(st_c, st_f) == []
    st_s, m_s, _, _ = ru.run_continued(st0, [(ru.m_none, ru.M_STEPS), (ru.m_none, ru.M_STEPS)], True)
    assert np.isfinite(st_c["u"]).all()
    assert not np.array_equal(st_c["u"][:, :, :, m_c.s.nnew - 1], st_s["u"][:, :, :, m_s.s.nnew - 1])
