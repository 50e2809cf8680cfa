"""-m gpu: parity at the level-count boundaries of every column kernel, across the option families.

The column kernels are ladders of instantiations picked from N at launch (RUNGS restates the `if (b.N <= ...)` ladders
of csrc/), with fully unrolled `k <= NMAX` loops guarded by `k <= N`, per-thread arrays of NMAX + 1 or NMAX + 2
entries and LDS columns of NMAX levels.  The other parity tests run the level axis in the default configuration only
(tests/test_gpu_kernels.py::test_more_than_32_levels: N = 40 and 64, unmasked periodic UPWELLING).  Here, on one shape
that is tiny otherwise -- 66 x 5: two workgroups in x with two live columns in the second, two in y with one live row,
with the seam land, dry cells and sources of tests/test_gpu_wide.py (whose state builders this module reuses) -- every
kernel with a ladder or a whole-column array runs at LEVELS: each rung's N == NMAX and the first N of the next rung
(N = 16 is the everyday UPWELLING), on the periodic island grid (every MASK = true instantiation) and in a closed
unmasked basin (every MASK = false one).  The level loops without a ladder run at N = 33 and 64.

  1. test_levels_kernels: single calls, HIP against the CPU oracle (the momentum-advection schemes the oracle does not
     have: against the numpy mirror of tests/uvadv_util.py), 1e-12 of each field's maximum on every registered field,
     equal return values, guard bands, and the top level changed by the reference (top_level_changed) -- which is what
     makes a column truncated to the rung below, or a dropped top level, a failure rather than "some field changed".
  2. test_levels_runs: 10 whole steps with physics and diagnostics, 1e-10 relative RMS.
  3. test_more_than_64_levels_are_refused_and_the_library_stays_usable.

tests/test_levels_shapes.py checks the same states without a GPU: the coverage of RUNGS by the case list, geometry,
seam conditions, the oracle's calls finite with a changed top level, the oracle's runs finite and moving."""
import numpy as np
import pytest

import test_gpu_wide as tw
import util
import uvadv_util as uv
from roms_trunk_mgh_amd import abi
from test_gpu_kernels import SCHEME_PAIRS

pytestmark = pytest.mark.gpu
TOL = tw.TOL                            # 1e-12: the per-call bound of tests/test_basin.py and tests/test_gpu_wide.py
LM, MM = 66, 5
LEVELS = (17, 32, 33, 48, 49, 64)       # N == NMAX of the rungs 32, 48, 64 and the first N above the rungs 16, 32, 48
PLAIN_LEVELS = (33, 64)                 # for the level loops without a ladder
VARIANTS = ("island", "closed")         # periodic and masked, land on both sides of the seam | an unmasked basin
MASKED = {"island": True, "closed": False}          # the MASK template parameter of the kernels in the variant

# The instantiations of each column kernel, as the host code selects them from N (roms_trunk_mgh_amd/csrc/):
RUNGS = {
    "k_uv_column": (16, 32, 48, 64),                 # k_step3d_uv.hip:432-436
    "k_rhs3d_vspline": (16, 32, 48, 64),             # k_rhs3d.hip:466-469
    "k_step3d_t_pipe:unmasked": (16, 32, 48, 64),    # k_step3d_t.hip:452-453, kernel_for_n<true> advect.h:273-281
    "k_step3d_t_pipe:masked": (16, 32, 64),          # k_step3d_t.hip:450-451, kernel_for_n advect.h:273-281
    "k_pre_t": (16, 32, 64),                         # k_pre_step3d.hip:214-217
    "k_step3d_t_hsimt": (16, 32, 64),                # k_step3d_t.hip:432
    "k_omega": (16, 32, 64),                         # k_base.hip:600-602
    "k_uv_couple": (16, 32, 64),                     # k_step3d_uv.hip:446-448
    # the whole-column vertical schemes of advect.h take the NMAX of the tracer kernel around them (k_pre_t, the masked
    # k_step3d_t_pipe: 16 / 32 / 64; in the unmasked k_step3d_t_pipe they also meet its rung 48)
    "a4_slopes": (16, 32, 64),
    "spline_w": (16, 32, 64),
    "k_lmd_vmix": (32, 64),                          # k_lmd.hip, roms_hip_lmd_vmix: n32
    "k_uv_column_classic": (32, 64),                 # k_step3d_uv.hip:429-430
    "k_step3d_t_pipe:src": (64,),                    # k_step3d_t.hip:460-463: one instantiation for every N
    "k_step3d_t_pipe:classic": (64,),                # k_step3d_t.hip:447-449: one instantiation for every N
}


def nmax(family, N):
    """NMAX of the instantiation of `family` that a grid of N levels is handed"""
    return min(r for r in RUNGS[family] if N <= r)


_T = ("pre_step3d", "step3d_t")
PAIR_LABELS = [f"{k}:{h}+{v}" for h, v in SCHEME_PAIRS for k in _T] + ["pre_step3d:A4+SPLINES:first"]
UVADV_PAIRS = [("U3", "SPLINES"), ("C2", "SPLINES"), ("C4", "SPLINES"), ("C4", "C4")]
UVADV_LABELS = [f"rhs3d_tile:{h}+{v}" for h, v in UVADV_PAIRS]
_A4 = [f"{k}:A4+{v}" for v in ("A4", "SPLINES") for k in _T]
_SPL = [f"{k}:{h}+SPLINES" for h in ("U3", "A4", "C4") for k in _T] + ["pre_step3d:A4+SPLINES:first"]
_STEP_T = ["step3d_t"] + [lb for lb in PAIR_LABELS if lb.startswith("step3d_t")]
# the labels (of LADDER below) that launch each family, and the variants in which they do
LAUNCHED_BY = {
    "k_uv_column": (["step3d_uv", "step3d_uv:wet", "step3d_uv:src"], VARIANTS),
    "k_rhs3d_vspline": ([lb for lb in UVADV_LABELS if lb.endswith("SPLINES")], VARIANTS),
    "k_step3d_t_pipe:unmasked": (_STEP_T + ["step3d_t:MIXED"], ("closed",)),
    "k_step3d_t_pipe:masked": (_STEP_T + ["step3d_t:MIXED"], ("island",)),
    "k_pre_t": (["pre_step3d", "pre_step3d:wet", "pre_step3d:src", "pre_step3d:MPDATA", "pre_step3d:HSIMT",
                 "pre_step3d:MIXED"] + [lb for lb in PAIR_LABELS if lb.startswith("pre_step3d")], VARIANTS),
    "k_step3d_t_hsimt": (["step3d_t:HSIMT"], VARIANTS),
    "k_omega": (["omega", "omega:src"], VARIANTS),
    "k_uv_couple": (["step3d_uv", "step3d_uv:wet", "step3d_uv:src", "step3d_uv:classic"], VARIANTS),
    "a4_slopes": (_A4, VARIANTS),
    "spline_w": (_SPL, VARIANTS),
    "k_lmd_vmix": (["lmd_vmix"], VARIANTS),
    "k_uv_column_classic": (["step3d_uv:classic"], VARIANTS),
    "k_step3d_t_pipe:src": (["step3d_t:src"], VARIANTS),
    "k_step3d_t_pipe:classic": (["step3d_t:classic"], VARIANTS),
}


def shape(N, config="UPWELLING"):
    """a shape for the builders of tests/test_gpu_wide.py (tw.shape_of)"""
    return dict(Lm=LM, Mm=MM, N=N), config


def check_geometry(b, N):
    """two workgroups over every x range, the second with two live columns; two rows of workgroups, the second with
    one live row"""
    assert (b.Lm, b.Mm, b.N) == (LM, MM, N) and b.Istr == tw.I0
    nbx = {k: tw.nblk(*r) for k, r in tw.x_ranges(b).items()}
    nby = tw.nblk(b.Jstr, b.Jend, tw.BLK_Y)
    assert set(nbx.values()) == {2} and b.Iend - b.Istr + 1 - tw.BLK_X == 2
    assert nby == 2 and b.Jend - b.Jstr + 1 - tw.BLK_Y == 1
    return nbx


# ---------------------------------------------------------------------------------------------- the states --
def _pairs(label, sh, variant):
    """the tracer scheme pairs of tests/test_gpu_kernels.py; ':first' = iic = 1, where the weights of the predictor
    differ"""
    kernel, pair, *first = label.split(":")
    h, v = pair.split("+")
    st = tw.prepared(sh, variant, {"Hadv": h, "Vadv": v})
    if kernel == "step3d_t":
        util.hz_weighted_tnew(st)
    return st, [(kernel, tw._s(iic=1 if first else 5))]


def _uvadv(label, sh, variant):
    """the momentum advection schemes, by the overrides of tests/test_gpu_uvadv.py"""
    h, v = label.split(":")[1].split("+")
    st = tw.prepared(sh, variant, {"uv_hadv": h, "uv_vadv": v})
    assert st.p.uv_adv == abi.uv_adv(h, v)
    return st, [("rhs3d_tile", tw._s())]


def _wide(fam):
    return tw.FAMILIES[fam][0]


# family -> (builder, labels): the kernels with a ladder or a whole-column array, at every N of LEVELS ...
LADDER = {
    "base": (_wide("base"), ["omega", "pre_step3d", "rhs3d", "step3d_uv", "step3d_t"]),
    "pairs": (_pairs, PAIR_LABELS),
    "adv3": (_wide("adv3"), tw.FAMILIES["adv3"][1]),
    "classic": (_wide("classic"), tw.FAMILIES["classic"][1]),
    "uvadv": (_uvadv, UVADV_LABELS),
    "wet": (_wide("wet"), ["pre_step3d:wet", "rhs3d:wet", "step3d_uv:wet"]),
    "sources": (_wide("sources"), ["omega:src", "pre_step3d:src", "step3d_uv:src", "step3d_t:src"]),
    "physics": (_wide("physics"), ["lmd_vmix", "wvelocity+diag"]),
}
# ... and the level loops without one (one level per launch, or N + 1 in gridDim), at PLAIN_LEVELS
PLAIN = {
    "base": (_wide("base"), ["rho_eos", "set_depth", "set_massflux", "t3dmix2", "uv3dmix2", "ini_fields"]),
    "prsgrd": (_wide("prsgrd"), tw.FAMILIES["prsgrd"][1]),
    "dif4": (_wide("dif4"), [lb for lb in tw.FAMILIES["dif4"][1] if not lb.startswith("step2d")]),    # step2d: no level axis
    "geo": (_wide("geo"), tw.FAMILIES["geo"][1]),
    "iso": (_wide("iso"), tw.FAMILIES["iso"][1]),
    "gls": (_wide("gls"), tw.FAMILIES["gls"][1]),
}
assert all(set(VARIANTS) <= set(tw.APPLIES.get(fam, tw.VARIANTS)) for fam in PLAIN)      # the APPLIES rule of test_gpu_wide


def kernel_cases():
    out = []
    for table, levels in ((LADDER, LEVELS), (PLAIN, PLAIN_LEVELS)):
        for fam, (_, labels) in table.items():
            for N in levels:
                for variant in VARIANTS:
                    for label in labels:
                        out.append(pytest.param(fam, label, N, variant, id=f"{label}-N{N}-{variant}"))
    return out


def build(fam, label, N, variant):
    table = LADDER if label in LADDER.get(fam, (None, ()))[1] else PLAIN
    st0, calls = table[fam][0](label, shape(N), variant)
    check_geometry(st0.b, N)
    tw.check_seam(st0, variant, wet=bool(st0.p.wet_dry))
    return st0, calls


def run_reference(fam, st0, calls):
    """the oracle on a copy of the state; the momentum-advection schemes (the oracle has the default pair only): the
    mirror of tests/uvadv_util.py on the ranges rhs3d_tile writes"""
    if fam != "uvadv":
        return tw.run_oracle(st0, calls)
    (kernel, s), = calls
    st_r = st0.copy()
    h, v = next(hv for hv in UVADV_PAIRS if abi.uv_adv(*hv) == st0.p.uv_adv)
    with np.errstate(all="ignore"):                          # the mirror's padding points, which no used range holds
        m = uv.rhs3d_tile(st0, s, h, v)
    (IU, JU), (IV, JV) = uv.ranges(st0)
    for name, frc, I, J in (("ru", "rufrc", IU, JU), ("rv", "rvfrc", IV, JV)):
        st_r[name][I, J, 1:, s.nrhs - 1] = m[name][I, J, 1:]
        st_r[frc][I, J] = m[frc][I, J]
    return st_r, []


# lmd_vmix leaves the levels 0 and N of Akv / Akt alone by design (lmd_vmix.F; util.kpp_state), omega sets W(N) = 0 (and
# finds it so in the input): the highest level they write is N - 1 of their w-level fields
BELOW_TOP = ("lmd_vmix", "omega")


def top_level_changed(label, st_r, st0):
    """names of the fields with a level axis whose top level -- index N - 1 of rho-level fields, N of w-level fields --
    the reference has changed (BELOW_TOP: the level under it)"""
    k = -2 if label.split(":")[0] in BELOW_TOP else -1
    return [n for n, kind, _ in abi.FIELDS if kind.startswith(("K_3D", "K_4D"))
            and not np.array_equal(st_r[n][:, :, k], st0[n][:, :, k])]


# ---------------------------------------------------------------------------- 1. single calls against the oracle --
@pytest.mark.parametrize("fam,label,N,variant", kernel_cases())
def test_levels_kernels(fam, label, N, variant):
    from roms_trunk_mgh_amd import hip
    st0, calls = build(fam, label, N, variant)
    st_h = st0.copy()
    h = hip.RomsHip(st_h)
    try:
        r_h = tw.run_calls(h, calls)
        h.to_host()
        h.check_guards()
    finally:
        h.close()
    st_r, r_r = run_reference(fam, st0, calls)
    diffs = util.compare_states(st_h, st_r)
    print(label, N, variant, "max relative differences:", diffs)
    assert all(v <= TOL for v in diffs.values()), diffs
    assert len(r_h) == len(r_r)
    for a, o in zip(r_h, r_r):
        assert np.array_equal(a, o), (a, o)
    assert top_level_changed(label, st_r, st0), "the reference left the top level alone: the case cannot see a truncated column"


# ------------------------------------------------------------------------------------------- 2. whole steps --
RUNS = {f"{cfg}-N{N}-{v}": (cfg, N, variant, {}) for cfg in ("BENCHMARK_TINY", "UPWELLING") for N in PLAIN_LEVELS
        for v, variant in (("island", "island"), ("open", "open_island"))}
RUNS["BENCHMARK_TINY-N33-mpdata6"] = ("BENCHMARK_TINY", 33, "island", dict(ov=tw.SCHEMES["MPDATA"], NT=6))
RUNS["UPWELLING-N49-beach"] = ("UPWELLING", 49, "island", dict(ov=tw.BEACH))
RUNS["UPWELLING-N33-geo4"] = ("UPWELLING", 33, "island", dict(ov=tw.GEO4_RUN))      # uv_vis2 = uv_vis4 = 2 in whole steps


def run_state(name):
    config, N, variant, kw = RUNS[name]
    st = tw.tile(shape(N, config), variant, **kw)
    check_geometry(st.b, N)
    tw.check_seam(st, variant)
    if name.endswith("geo4"):
        tw.check_geo4_run(st)
    return st


@pytest.mark.parametrize("name", list(RUNS))
def test_levels_runs(name):
    """BENCHMARK_TINY: the first whole steps with k_lmd_vmix<64> in them"""
    import oracle
    from roms_trunk_mgh_amd import hip
    from test_gpu_fullsize import _check_prognostic
    st_o = run_state(name)
    st_h = st_o.copy()
    be = hip.RomsHip(st_h)
    try:
        tw.run_steps(be)
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    mo = tw.run_steps(oracle.Oracle(st_o))
    _check_prognostic(st_h, st_o, mo)
    if name.endswith("beach"):
        assert 0 < st_o["rmask_wet"].sum() < st_o["rmask_wet"].size
        for n in ("rmask_wet", "umask_wet", "vmask_wet", "pmask_wet"):
            assert np.array_equal(st_h[n], st_o[n]), n


# ----------------------------------------------------------------------------------------------- 3. refusal --
def test_more_than_64_levels_are_refused_and_the_library_stays_usable():
    """N = 65: roms_hip_set_bounds refuses the bounds, so the refusal surfaces where the context is made, before any
    entry; a fresh context afterwards gives the oracle's omega bit for bit
    (tests/test_gpu_errors.py::test_unsupported_advection_pair_is_refused_and_library_stays_usable)"""
    import oracle
    from roms_trunk_mgh_amd import hip
    st = tw.prepared(shape(64), "closed")
    st.b = type(st.b).from_buffer_copy(st.b)                 # the s-coordinate tables of the parameters hold ROMS_MAXN + 1
    st.b.N = 65                                              # levels, so no state of 65 can be made: the bounds say 65
    assert st.b.N == abi.ROMS_MAXN + 1
    with pytest.raises(RuntimeError, match="N or NT too large"):
        hip.RomsHip(st)
    st0, _ = build("base", "omega", 64, "closed")
    st_o, st_h = st0.copy(), st0.copy()
    oracle.Oracle(st_o).call("omega", util.step_idx())
    h = hip.RomsHip(st_h)
    try:
        h.call("omega", util.step_idx())
        h.to_host()
        h.check_guards()
    finally:
        h.close()
    assert np.array_equal(st_h["W"], st_o["W"]) and not np.array_equal(st_o["W"], st0["W"])
