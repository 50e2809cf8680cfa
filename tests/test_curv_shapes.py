"""The inputs of tests/test_gpu_curvilinear.py checked without a GPU, so that no GPU case there can pass vacuously.

  * test_grid_varies_everywhere: every array curvilinear() fills differs between every pair of adjacent columns and of
    adjacent rows, over the range on which the array is defined (curv_util.defined).
  * test_reads: READS lists, per kernel label, the grid and coefficient arrays the routine reads: those read on both
    configurations, then those read on one of them only (MIX_S_TS reads pmon_u / pnom_v where MIX_GEO_TS reads on_u /
    om_v).  For every array of READS the oracle's result must change, on some field, by more than 100 x the parity
    bound of the GPU case (1e-12 of the field's maximum) when that array alone is replaced by its copy rolled one
    column, and separately one row: a kernel reading the array one point off fails its parity case.  For every array
    NOT in READS the rolled copy must leave the oracle's result unchanged bit for bit -- which is what shows that the
    routine does not read it, for each label and array, rather than a list of source lines.  Where the BENCHMARK_TINY
    state was too weak for a pair (pm, pn in pre_step3d and step3d_uv: cells of 600 km, dt pm pn is tiny) the GPU
    module scales the fluxes and right-hand sides up (test_gpu_curvilinear.STRENGTHEN) until the pair clears the bound.
  * the geometry and seam conditions (build() asserts them), the oracle finite and not trivial on every state, the
    edge columns of the detector cases found, the 10-step runs finite and moving."""
import numpy as np
import pytest

import curv_util as cv
import test_gpu_curvilinear as tc
import test_gpu_wide as tw
import util
from roms_trunk_mgh_amd import abi

BOUND = 100.0 * tc.TOL
# the variants the sensitivities are taken over (the larger of the two counts): the periodic island grid and a basin
# with open edges (RadNud; GLS: the gradient edges APPLIES allows)
SENS_VARIANTS = {"gls": ("island", "open_island")}

# label: (read on both configurations, {configuration: read there only})
READS = {
    'set_depth': ((), {}),
    'set_massflux': (('on_u', 'om_v'), {}),
    'omega': ((), {}),
    'set_zeta': ((), {}),
    'rho_eos': ((), {}),
    'prsgrd': (('on_u', 'om_v'), {}),
    't3dmix2': (('pm', 'pn', 'diff2'), {'UPWELLING': ('pmon_u', 'pnom_v'), 'BENCHMARK_TINY': ('on_u', 'om_v')}),
    'uv3dmix2': (('pm', 'pn', 'om_r', 'on_r', 'pnom_r', 'pmon_r', 'pnom_p', 'pmon_p', 'om_p', 'on_p', 'visc2_r', 'visc2_p'), {}),
    'rhs3d_tile': (('fomn', 'om_u', 'on_u', 'om_v', 'on_v', 'dndx', 'dmde'), {}),
    'pre_step3d': (('pm', 'pn'), {}),
    'rhs3d': (('pm', 'pn', 'om_r', 'on_r', 'fomn', 'pnom_r', 'pmon_r', 'om_u', 'on_u', 'om_v', 'on_v', 'pnom_p', 'pmon_p', 'om_p', 'on_p', 'dndx', 'dmde', 'visc2_r', 'visc2_p', 'diff2'), {'UPWELLING': ('pmon_u', 'pnom_v')}),
    'step2d': (('pm', 'pn', 'om_r', 'on_r', 'fomn', 'pnom_r', 'pmon_r', 'on_u', 'om_v', 'pnom_p', 'pmon_p', 'om_p', 'on_p', 'dndx', 'dmde', 'visc2_r', 'visc2_p'), {}),
    'step3d_uv': (('pm', 'pn', 'on_u', 'om_v'), {}),
    'step3d_t': (('pm', 'pn'), {}),
    'set_vbc': ((), {}),
    'wvelocity': (('pm', 'pn'), {}),
    'ini_zeta': ((), {}),
    'ini_fields': ((), {}),
    'step2d_loop': (('pm', 'pn', 'om_r', 'on_r', 'fomn', 'pnom_r', 'pmon_r', 'on_u', 'om_v', 'pnom_p', 'pmon_p', 'om_p', 'on_p', 'dndx', 'dmde', 'visc2_r', 'visc2_p'), {}),
    'prsgrd:STANDARD': (('on_u', 'om_v'), {}),
    'prsgrd:WJ_GRADP': (('on_u', 'om_v'), {}),
    'prsgrd:PJ_GRADP': (('on_u', 'om_v'), {}),
    't3dmix4:dif4': (('pm', 'pn', 'diff4'), {'UPWELLING': ('pmon_u', 'pnom_v'), 'BENCHMARK_TINY': ('on_u', 'om_v')}),
    'uv3dmix4:dif4': (('pm', 'pn', 'om_r', 'on_r', 'pnom_r', 'pmon_r', 'pnom_p', 'pmon_p', 'om_p', 'on_p', 'visc4_r', 'visc4_p'), {}),
    'step2d:dif4': (('pm', 'pn', 'om_r', 'on_r', 'fomn', 'pnom_r', 'pmon_r', 'on_u', 'om_v', 'pnom_p', 'pmon_p', 'om_p', 'on_p', 'dndx', 'dmde', 'visc2_r', 'visc2_p', 'visc4_r', 'visc4_p'), {}),
    'uv3dmix2:geo': (('pm', 'pn', 'om_r', 'on_r', 'om_u', 'on_u', 'om_v', 'on_v', 'om_p', 'on_p', 'visc2_r', 'visc2_p'), {}),
    'rhs3d:geo': (('pm', 'pn', 'om_r', 'on_r', 'fomn', 'om_u', 'on_u', 'om_v', 'on_v', 'om_p', 'on_p', 'dndx', 'dmde', 'visc2_r', 'visc2_p', 'diff2'), {'UPWELLING': ('pmon_u', 'pnom_v')}),
    'uv3dmix4:geo': (('pm', 'pn', 'om_r', 'on_r', 'om_u', 'on_u', 'om_v', 'on_v', 'om_p', 'on_p', 'visc4_r', 'visc4_p'), {}),
    'rhs3d:geo4': (('pm', 'pn', 'om_r', 'on_r', 'fomn', 'om_u', 'on_u', 'om_v', 'on_v', 'om_p', 'on_p', 'dndx', 'dmde', 'visc2_r', 'visc2_p', 'visc4_r', 'visc4_p', 'diff2'), {'UPWELLING': ('pmon_u', 'pnom_v')}),
    't3dmix2:iso': (('pm', 'pn', 'on_u', 'om_v', 'diff2'), {}),
    't3dmix4:iso': (('pm', 'pn', 'on_u', 'om_v', 'diff4'), {}),
    'gls_prestep:k-epsilon': (('pm', 'pn'), {}),
    'gls_corstep:k-epsilon': (('pm', 'pn'), {}),
    'gls_prestep:my25': (('pm', 'pn'), {}),
    'gls_corstep:my25': (('pm', 'pn'), {}),
    'pre_step3d:MPDATA': (('pm', 'pn'), {}),
    'step3d_t:MPDATA': (('pm', 'pn', 'omn', 'om_u', 'on_u', 'om_v', 'on_v'), {}),
    'pre_step3d:HSIMT': (('pm', 'pn'), {}),
    'step3d_t:HSIMT': (('pm', 'pn'), {}),
    'pre_step3d:MIXED': (('pm', 'pn'), {}),
    'step3d_t:MIXED': (('pm', 'pn', 'omn', 'om_u', 'on_u', 'om_v', 'on_v'), {}),
    'step3d_uv:classic': (('pm', 'pn', 'on_u', 'om_v'), {}),
    'step3d_t:classic': (('pm', 'pn'), {}),
    'set_vbc:1': ((), {}),
    'set_vbc:2': ((), {}),
    'set_vbc:3': ((), {}),
    'bulk_flux': ((), {}),
    'lmd_vmix': ((), {}),
    'wvelocity+diag': (('pm', 'pn'), {}),
    'set_depth:wet': ((), {}),
    'prsgrd:wet': (('on_u', 'om_v'), {}),
    't3dmix2:wet': (('pm', 'pn', 'pmon_u', 'pnom_v', 'diff2'), {}),
    'uv3dmix2:wet': (('pm', 'pn', 'om_r', 'on_r', 'pnom_r', 'pmon_r', 'pnom_p', 'pmon_p', 'om_p', 'on_p', 'visc2_r', 'visc2_p'), {}),
    'pre_step3d:wet': (('pm', 'pn'), {}),
    'rhs3d:wet': (('pm', 'pn', 'om_r', 'on_r', 'fomn', 'pnom_r', 'pmon_r', 'pmon_u', 'om_u', 'on_u', 'pnom_v', 'om_v', 'on_v', 'pnom_p', 'pmon_p', 'om_p', 'on_p', 'dndx', 'dmde', 'visc2_r', 'visc2_p', 'diff2'), {}),
    'step3d_uv:wet': (('pm', 'pn', 'on_u', 'om_v'), {}),
    'ini_zeta:wet': ((), {}),
    'ini_fields:wet': ((), {}),
    'wetdry:wet': ((), {}),
    'step2d:wet': (('pm', 'pn', 'om_r', 'on_r', 'fomn', 'pnom_r', 'pmon_r', 'on_u', 'om_v', 'pnom_p', 'pmon_p', 'om_p', 'on_p', 'dndx', 'dmde', 'visc2_r', 'visc2_p'), {}),
    'step2d:src': (('pm', 'pn', 'om_r', 'on_r', 'fomn', 'pnom_r', 'pmon_r', 'on_u', 'om_v', 'pnom_p', 'pmon_p', 'om_p', 'on_p', 'dndx', 'dmde', 'visc2_r', 'visc2_p'), {}),
    'step3d_uv:src': (('pm', 'pn', 'on_u', 'om_v'), {}),
    'pre_step3d:src': (('pm', 'pn'), {}),
    'step3d_t:src': (('pm', 'pn'), {}),
    'rhs3d:src': (('pm', 'pn', 'om_r', 'on_r', 'fomn', 'pnom_r', 'pmon_r', 'pmon_u', 'om_u', 'on_u', 'pnom_v', 'om_v', 'on_v', 'pnom_p', 'pmon_p', 'om_p', 'on_p', 'dndx', 'dmde', 'visc2_r', 'visc2_p', 'diff2'), {}),
    'omega:src': ((), {}),
    'wetdry:src': ((), {}),
}


def _finite(st):
    return all(np.isfinite(st[name]).all() for name, _, _ in abi.FIELDS)


def reads(label, config):
    common, only = READS[label]
    return set(common) | set(only.get(config, ()))


def label_cases():
    seen = []
    for p in tc.kernel_cases():
        fam, label, config, _ = p.values
        if (fam, label, config) not in seen:
            seen.append((fam, label, config))
    return [pytest.param(*c, id=f"{c[1]}-{c[2]}") for c in seen]


def test_reads_covers_every_label():
    assert set(READS) == {label for _, labels in tw.FAMILIES.values() for label in labels}


@pytest.mark.parametrize("config", tc.CONFIGS)
@pytest.mark.parametrize("variant", ["island", "closed"])
def test_grid_varies_everywhere(config, variant):
    for ov in (None, tw.DIF4[config]):
        st = cv.curvilinear(tw.prepared(tc.shape(config), variant, ov))
        tc.check_geometry(st.b)
        assert _finite(st)
        pm0 = tw.prepared(tc.shape(config), variant, ov)["pm"]
        ratio = st["pm"] / pm0
        assert 1.0 - cv.AMP <= ratio.min() < 0.9 and 1.1 < ratio.max() <= 1.0 + cv.AMP
        assert not np.array_equal(st["pm"] / pm0, st["pn"] / tw.prepared(tc.shape(config), variant, ov)["pn"])
        for name in cv.ARRAYS:
            a = st[name][cv.defined(st, name)]
            a = a.reshape(a.shape[0], a.shape[1], -1)
            assert (a[1:] != a[:-1]).all() and (a[:, 1:] != a[:, :-1]).all(), name
            if name in cv.COEFFICIENTS:
                assert (a > 0.0).all(), name
        assert not np.array_equal(st["visc2_r"], st["visc2_p"]) and not np.array_equal(st["visc4_r"], st["visc4_p"])
        b = st.b
        if b.EWperiodic:                                     # period Lm
            for name in ("pm", "pn", "f", "visc2_r", "diff4"):
                assert np.allclose(st[name][st.I(0)], st[name][st.I(b.Lm)], rtol=1e-13, atol=0.0), name


@pytest.mark.parametrize("fam,label,config", label_cases())
def test_reads(fam, label, config):
    variants = SENS_VARIANTS.get(fam, ("island", "radnud"))
    sens = {}
    for variant in variants:
        st0, calls = tc.build(fam, label, config, variant)     # asserts geometry and seam conditions
        assert _finite(st0)
        st_o, _ = tw.run_oracle(st0, calls)
        assert _finite(st_o), [n for n, _, _ in abi.FIELDS if not np.isfinite(st_o[n]).all()]
        assert tw.vacuous_ok(label, variant) or util.compare_states(st_o, st0)
        for name in cv.ARRAYS:
            others = [n for n, _, _ in abi.FIELDS if n != name]
            for axis in (0, 1):
                st_r, _ = tw.run_oracle(cv.rolled(st0, name, axis), calls)
                assert _finite(st_r), (name, axis)
                d = util.compare_states(st_r, st_o, others)
                sens[name, axis] = max(sens.get((name, axis), 0.0), max(d.values()) if d else 0.0)
    want = reads(label, config)
    for (name, axis), v in sens.items():
        if name in want:
            assert v > BOUND, (name, axis, v)
        else:
            assert v == 0.0, (name, axis, v, "read, but not in READS")


@pytest.mark.parametrize("fam,label,config,variant", [p for p in tc.kernel_cases() if p.values[3] in ("closed", "open_island")])
def test_oracle_on_the_other_variants(fam, label, config, variant):
    st0, calls = tc.build(fam, label, config, variant)
    st_o, _ = tw.run_oracle(st0, calls)
    assert _finite(st0) and _finite(st_o)
    assert tw.vacuous_ok(label, variant) or util.compare_states(st_o, st0)


@pytest.mark.parametrize("variant", ["island", "closed"])
@pytest.mark.parametrize("nghost", [2, 3])
def test_detector_edge_columns(nghost, variant):
    """every array of the table is read by the oracle's step2d_loop near both edges; with three ghost points on the
    channel some are read three columns out (pn at Istr-3), which is why k_rowm_build examines NghostPoints columns"""
    st0 = tc.detector_state(nghost, variant)
    base = tc.loop_oracle(st0)[0]
    b = st0.b
    cols = {name: tc.edge_columns(st0, name, base) for name in tc.ROW_METRICS + tc.ROW_OTHERS}
    assert all(b.Istr - nghost <= w and e <= b.Iend + nghost for w, e in cols.values()), cols
    if nghost == 3 and variant == "island":
        assert cols["pn"][0] == b.Istr - 3


@pytest.mark.parametrize("name", list(tc.RUNS))
def test_oracle_runs_on_the_curvilinear_states(name):
    import oracle
    st = tc.run_state(name)
    m = tw.run_steps(oracle.Oracle(st), 10)
    assert np.isfinite(st["t"]).all() and np.isfinite(st["u"]).all()
    assert float(np.abs(st["u"]).max()) > 1e-6 and m.last_diag is not None


def _geo4_run_states():
    import test_gpu_levels as tl
    return ([("wide", n) for n in tw.RUNS if "geo4" in n] + [("levels", n) for n in tl.RUNS if "geo4" in n] +
            [("curv", n) for n in tc.RUNS if "geo4" in n])


@pytest.mark.parametrize("where,name", _geo4_run_states())
def test_the_rotation_acts_in_the_whole_step_runs(where, name):
    """the 10-step runs with uv_vis2 = uv_vis4 = 2 (w3 island and open_island, UPWELLING N = 33, SEAMOUNT curvilinear
    closed): the oracle's run with both operators along s-surfaces instead ends with another u, so a device that ran
    the s-surface operator would miss the run bound"""
    import oracle
    import test_gpu_levels as tl
    mod = {"wide": tw, "levels": tl, "curv": tc}[where]
    st_g, st_s = mod.run_state(name), mod.run_state(name)
    st_s.p.uv_vis2 = st_s.p.uv_vis4 = 1
    mg = tw.run_steps(oracle.Oracle(st_g), 10)
    tw.run_steps(oracle.Oracle(st_s), 10)
    u_g, u_s = st_g.interior("u")[..., mg.s.nnew - 1], st_s.interior("u")[..., mg.s.nnew - 1]
    assert np.isfinite(u_g).all() and np.isfinite(st_g["t"]).all()
    d = float(np.sqrt(np.mean((u_g - u_s) ** 2)) / np.sqrt(np.mean(u_s ** 2)))
    print(where, name, "relative RMS distance of the s-surface run", d)
    assert d > 100.0 * 1e-10


def test_geo4_run_states_are_listed():
    assert len(_geo4_run_states()) == 4


@pytest.mark.parametrize("s", ["predictor", "corrector"])
@pytest.mark.parametrize("case", ["channel", "basin"])
def test_2d_mirror_with_the_curvilinear_term_equals_the_oracle(case, s):
    """tests/test_uvadv.py::test_default_2d_mirror_equals_oracle_step2d_bit_for_bit on the state of
    test_curv_uvadv_step2d: the mirror's curvilinear term (uvadv_util.step2d_expected) against the oracle's, bit for
    bit; without the term the mirror gives another velocity"""
    import oracle
    import uvadv_util as uv
    from test_gpu_uvadv import S_CORR, S_PRED
    s = S_PRED if s == "predictor" else S_CORR
    st0 = uv.zero_pressure_gradient(tc.uvadv_state(case))
    want = st0.copy()
    oracle.Oracle(want).call("step2d", s)
    got = uv.step2d_expected(st0, s, want["zeta"][:, :, s.knew - 1], c2=False)
    flat = st0.copy()
    flat.p = type(flat.p).from_buffer_copy(flat.p)
    flat.p.curvgrid = 0
    without = uv.step2d_expected(flat, s, want["zeta"][:, :, s.knew - 1], c2=False)
    (IU, JU), (IV, JV) = uv.ranges(st0)
    for bar, rbar, I, J in (("ubar", "rubar", IU, JU), ("vbar", "rvbar", IV, JV)):
        assert np.array_equal(got[bar][I, J], want[bar][I, J, s.knew - 1]), bar
        assert not np.array_equal(without[bar][I, J], want[bar][I, J, s.knew - 1]), bar
        if s.predictor_2d_step:
            assert np.array_equal(got["rhs_" + bar][I, J], want[rbar][I, J, s.krhs - 1]), rbar


@pytest.mark.parametrize("case", ["channel", "basin"])
def test_3d_mirror_equals_the_oracle_on_the_curvilinear_state(case):
    import oracle
    import uvadv_util as uv
    from test_gpu_uvadv import S3D
    st0 = tc.uvadv_state(case)
    want = st0.copy()
    oracle.Oracle(want).call("rhs3d_tile", S3D)
    with np.errstate(all="ignore"):
        got = uv.rhs3d_tile(st0, S3D)
    (IU, JU), (IV, JV) = uv.ranges(st0)
    n = S3D.nrhs - 1
    assert np.array_equal(got["ru"][IU, JU, 1:], want["ru"][IU, JU, 1:, n])
    assert np.array_equal(got["rv"][IV, JV, 1:], want["rv"][IV, JV, 1:, n])
    assert np.array_equal(got["rufrc"][IU, JU], want["rufrc"][IU, JU]) and np.array_equal(got["rvfrc"][IV, JV], want["rvfrc"][IV, JV])
