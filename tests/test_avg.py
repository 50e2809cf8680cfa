"""CPU: the time-averaged fields (AVERAGES; roms_hip_set_averages / roms_hip_set_avg) without a GPU.

  * the schedule of set_avg_tile and set_avg_masks: the library's roms_hip_avg_phase, its Python mirror avg.phase and
    the numpy restatement's own reading of the IF conditions (tests/avg_util.py), each against a table written out by
    hand;
  * known answers on the numpy restatement, which stands in for the reference vector this routine cannot have: they do
    not depend on anyone's reading of the loops;
  * the table include/roms_avg.def against the Fortran constants and the restatement's hand-written blocks."""
import os
import re

import numpy as np
import pytest

import avg_util as au
import util
from roms_trunk_mgh_amd import abi, ana, avg, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, A, C, M = avg.SET, avg.ADD, avg.CLOSE, avg.MASKS

# (nAVG, ntsAVG, ntstart, nrrec) -> {iic: phase}, three windows, every iic not listed = nothing happens
BY_HAND = {
    (3, 1, 1, 0): (range(1, 12), {2: S, 3: A, 4: A | C | M, 5: S, 6: A, 7: A | C | M, 8: S, 9: A, 10: A | C | M, 11: S}),
    # nAVG = 1: set + close on every step from ntsAVG on; MOD(iic-1, 1) = 0 also closes the masks from ntsAVG + 1 on
    (1, 1, 1, 0): (range(1, 5), {1: S | C, 2: S | C | M, 3: S | C | M, 4: S | C | M}),
    # ntsAVG = 3: nothing before iic = 4; (iic-1) % 4 == 1 first holds at 6, so 4 accumulates into the zero arrays and
    # 5 closes that first, short window, as the reference does
    (4, 3, 1, 0): (range(1, 15), {4: A, 5: A | C | M, 6: S, 7: A, 8: A, 9: A | C | M, 10: S, 11: A, 12: A, 13: A | C | M,
                                  14: S}),
    # restart at iic = 7: (7-1) % 3 == 0 would close, but the restart step initialises instead and closes nothing
    (3, 1, 7, 1): (range(7, 18), {7: S, 8: S, 9: A, 10: A | C | M, 11: S, 12: A, 13: A | C | M, 14: S, 15: A,
                                  16: A | C | M, 17: S}),
}


@pytest.mark.parametrize("key", list(BY_HAND))
def test_schedule_equals_the_table_written_by_hand(key):
    lib = hip.load()
    steps, table = BY_HAND[key]
    for iic in steps:
        want = table.get(iic, 0)
        assert avg.phase(iic, *key) == want, ("avg.py", key, iic)
        assert lib.roms_hip_avg_phase(iic, *key) == want, ("k_avg.hip", key, iic)
        ini, acc, close, masks = au.schedule(iic, *key)
        assert (S * ini) | (A * acc) | (C * close) | (M * masks) == want, ("avg_util", key, iic)
    assert avg.phase(5, 0, 1, 1, 0) == lib.roms_hip_avg_phase(5, 0, 1, 1, 0) == 0          # nAVG = 0: set_avg.F:189


def test_schedule_of_the_first_case_in_words():
    """(3,1,1,0): nothing at 1; set at 2, 5, 8; add at 3, 6; add + close at 4, 7."""
    ph = {iic: avg.phase(iic, 3, 1, 1, 0) for iic in range(1, 9)}
    assert ph[1] == 0
    assert [i for i in ph if ph[i] & S] == [2, 5, 8]
    assert [i for i in ph if ph[i] & A and not ph[i] & C] == [3, 6]
    assert [i for i in ph if ph[i] & A and ph[i] & C] == [4, 7]
    assert all(avg.phase(i, 1, 2, 1, 0) == (0 if i < 2 else S | C | (M if i > 2 else 0)) for i in range(1, 7))


# ------------------------------------------------------------------------------------------------ the table --
def test_table_agrees_with_the_fortran_constants_and_the_restatement():
    src = open(os.path.join(ROOT, "roms_trunk_mgh_amd", "fortran", "roms_hip_mod.F90")).read()
    pairs = dict((n, int(v)) for n, v in re.findall(r"\bAVG_(\w+)=(\d+)", src))
    assert pairs.pop("COUNT") == avg.AVG_COUNT == len(avg.AVG_ID)
    assert pairs == avg.AVG_ID
    assert set(avg.BUILT) == set(au.BLOCKS) and len(avg.BUILT) == 42
    assert avg.TRACER_KINDS == ["avgt", "avgTT", "avgUT", "avgVT", "avgHuonT", "avgHvomT"]
    assert avg.COUNTERS == list(au.COUNTERS)
    for name in ("avgu2dE", "avgv3dN", "avgpvor2d", "avgrvor3d", "avghbbl", "avgu2Sd", "avgSxx3d", "avgbedldu", "avgDU_avg1"):
        assert name in avg.NOT_BUILT
    rng = {"RNG_RR": au.RR, "RNG_UR": au.UR, "RNG_VR": au.VR, "RNG_II": au.II, "RNG_UI": au.UI, "RNG_VI": au.VI}
    for d in avg.LINES:
        if d["kind"] != "avg":
            continue
        cite, ranges, mask, three_d, per_tracer, _ = au.BLOCKS[d["name"]]
        assert rng[d["range"]] == ranges and d["mask"] == mask, d["name"]
        assert (d["shape"] != "AVS_2D") == three_d and (d["shape"] == "AVS_NT") == per_tracer, d["name"]
        assert d["srcA"] in abi.FIELD_ID and d["srcB"] in abi.FIELD_ID and d["mask"] in abi.FIELD_ID
    with pytest.raises(ValueError):
        avg.Averages(ana.make_tile("UPWELLING").b, 3, select=["avgt"])


# ------------------------------------------------------------------------------------------ known answers --
SMALL = dict(Lm=12, Mm=7, N=4)


def _state(wet=False, **ov):
    kw = dict(overrides=dict(SMALL, **ov))
    if wet:
        kw.update(mask="island", wet=True)
    return util.prepared_state("BENCHMARK_TINY", **kw)


def _run(st, select, nAVG, steps, ntsAVG=1, ntstart=1, nrrec=0, before=None):
    ref = au.AvgRef(st.b, st.p.wet_dry, nAVG, ntsAVG, ntstart, nrrec, select)
    for n, iic in enumerate(steps):
        if before:
            before(n, iic)
        ref.set_avg(st, util.step_idx(iic=iic, kstp=1 + n % 3, nrhs=1 + n % 2))
    return ref


def _fill_all_time_levels(st):
    for name in ("zeta", "ubar", "vbar"):
        st[name][:] = st[name][:, :, :1]
    for name in ("u", "v"):
        st[name][:] = st[name][:, :, :, :1]
    st["t"][:] = st["t"][:, :, :, :1, :]
    rng = np.random.default_rng(2)
    for name in ("wvel", "Akv", "Akt", "hsbl", "Pair", "Tair", "Uwind", "Vwind", "lhflx", "lrflx", "shflx", "evap", "rain",
                 "stflx", "srflx", "sustr", "svstr"):
        st[name][:] = rng.standard_normal(st[name].shape)


@pytest.mark.parametrize("periodic", [True, False])
def test_a_constant_state_returns_itself_and_zero_outside_the_ranges(periodic):
    """nAVG = 4, the state held over the window (whatever time level KOUT / NOUT point at): every average of a field is
    the field, every quadratic term the product of the face means, on the block's ranges; outside them 0 -- but for the
    periodic images, which equal their originals."""
    st = _state(EWperiodic=periodic)
    _fill_all_time_levels(st)
    b = st.b
    sel = au.all_in_scope(b.NT)
    ref = _run(st, sel, 4, range(1, 6))
    R = (st.I(b.IstrR, b.IendR), st.J(b.JstrR, b.JendR))
    s0 = util.step_idx(kstp=1, nrhs=1)
    for (name, it), a in ref.avg.items():
        _, rng, _, three_d, _, fn = au.BLOCKS[name]
        I, J = ref._ij(rng)
        x = au._prod(fn(au._Pt(st, s0, I, J, it, three_d)))
        # four equal addends and a division by four are exact
        assert np.array_equal(a[I, J], x), name
        assert np.abs(x).max() > 0.0, name
        outside = a.copy()
        outside[I, J] = 0.0
        if periodic:
            for g in range(1, b.NghostPoints + 1):
                assert np.array_equal(a[st.I(b.Lm + g)], a[st.I(g)]), name
            for g in range(3):
                assert np.array_equal(a[st.I(-g)], a[st.I(b.Lm - g)]), name
            outside[:st.I(1)] = 0.0
            outside[st.I(b.Lm + 1):] = 0.0
        assert not outside.any(), name
    u, v = st["u"][:, :, :, 0], st["v"][:, :, :, 0]
    I, J = st.I(b.Istr, b.Iend), st.J(b.Jstr, b.Jend)
    Ip, Jp = slice(I.start + 1, I.stop + 1), slice(J.start + 1, J.stop + 1)
    assert np.allclose(ref.avg[("avgUV", 0)][I, J], (0.5 * (u[I, J] + u[Ip, J])) * (0.5 * (v[I, J] + v[I, Jp])), rtol=1e-14, atol=0)
    Im = slice(I.start - 1, I.stop - 1)
    t2 = st["t"][:, :, :, 0, 1]
    assert np.allclose(ref.avg[("avgUT", 2)][I, st.J(b.JstrR, b.JendR)],
                       u[I, st.J(b.JstrR, b.JendR)] * 0.5 * (t2[Im, st.J(b.JstrR, b.JendR)] + t2[I, st.J(b.JstrR, b.JendR)]),
                       rtol=1e-14, atol=0)
    assert np.array_equal(ref.avg[("avgw3d", 0)][R], st["W"][R] * st["pm"][R][:, :, None] * st["pn"][R][:, :, None])


def test_a_linear_ramp_returns_its_midpoint():
    """zeta = z0 + c * step over n = 5 steps -> z0 + c (n + 1) / 2, with c a power of two so that every sum is exact"""
    st = _state()
    b = st.b
    z0 = np.round(st["zeta"][:, :, 0] * 64.0) / 64.0
    c, n = 0.25, 5

    def ramp(k, iic):
        st["zeta"][:] = (z0 + c * (k + 1))[:, :, None]
    ref = _run(st, [("avgzeta", 0)], n, range(2, 2 + n), before=ramp)
    R = (st.I(b.IstrR, b.IendR), st.J(b.JstrR, b.JendR))
    want = z0 + c * (n + 1) / 2.0
    got = ref.avg[("avgzeta", 0)]
    assert np.allclose(got[R], want[R], rtol=1e-15, atol=0) and np.abs(got[R] - z0[R]).min() > 0.7


def test_nAVG_1_returns_the_instantaneous_field():
    st = _state()
    b = st.b
    sel = [("avgzeta", 0), ("avgw3d", 0), ("avgt", 2), ("avgUT", 1)]
    ref = au.AvgRef(b, 0, 1, 1, 1, 0, sel)
    R = (st.I(b.IstrR, b.IendR), st.J(b.JstrR, b.JendR))
    for iic in (1, 2, 3):
        s = util.step_idx(iic=iic, kstp=1 + iic % 3, nrhs=1 + iic % 2)
        st["W"][:] = st["W"] * 1.5
        assert ref.set_avg(st, s)[:3] == (True, False, True)
        assert np.array_equal(ref.avg[("avgzeta", 0)][R], st["zeta"][:, :, s.kstp - 1][R])
        assert np.array_equal(ref.avg[("avgt", 2)][R], st["t"][:, :, :, s.nrhs - 1, 1][R])
        assert np.array_equal(ref.avg[("avgw3d", 0)][R], st["W"][R] * st["pm"][R][:, :, None] * st["pn"][R][:, :, None])


def test_wet_dry_divides_by_the_wet_steps():
    """nAVG = 5, one rho point wet on steps 1, 3, 4 of the window, one never: the sum over the wet steps / 3, and 0; the
    counters come out 0 or 1 (set_avg_masks) although the division used the counts."""
    st = _state(wet=True)
    b = st.b
    full0 = st["rmask_full"].copy()
    wet_pts = np.argwhere(full0[st.I(b.Istr, b.Iend), st.J(b.Jstr, b.Jend)] == 1.0)
    assert len(wet_pts) >= 3
    ia, ja = int(wet_pts[0][0]) + st.I(b.Istr), int(wet_pts[0][1]) + st.J(b.Jstr)
    ib, jb = int(wet_pts[-1][0]) + st.I(b.Istr), int(wet_pts[-1][1]) + st.J(b.Jstr)
    zs = []

    def weather(k, iic):
        st["rmask_full"][:] = full0
        st["rmask_full"][ia, ja] = 1.0 if k in (0, 2, 3) else 0.0
        st["rmask_full"][ib, jb] = 0.0
        st["zeta"][:] = np.round(64.0 * (1.0 + k) * (0.5 + st["h"] / st["h"].max())[:, :, None]) / 64.0
        zs.append(st["zeta"][:, :, 0].copy())
    ref = au.AvgRef(b, 1, 5, 1, 1, 0, [("avgzeta", 0), ("avgZZ", 0)])
    for k, iic in enumerate(range(2, 7)):
        weather(k, iic)
        out = ref.set_avg(st, util.step_idx(iic=iic, kstp=1))
    assert out == (False, True, True, True)
    got = ref.avg[("avgzeta", 0)]
    # rfac = 1 / MAX(1, count) multiplies the sum (set_avg.F:2321, :2343)
    assert got[ia, ja] == (1.0 / 3.0) * (zs[0][ia, ja] + zs[2][ia, ja] + zs[3][ia, ja]) and got[ia, ja] != 0.0
    assert got[ib, jb] == 0.0 and ref.avg[("avgZZ", 0)][ib, jb] == 0.0
    i, j = int(wet_pts[1][0]) + st.I(b.Istr), int(wet_pts[1][1]) + st.J(b.Jstr)      # wet throughout
    assert got[i, j] == (1.0 / 5.0) * sum(z[i, j] for z in zs)
    for k, c in ref.cnt.items():
        assert set(np.unique(c)) <= {0.0, 1.0}, k
    assert ref.cnt["rmask_avg"][ia, ja] == 1.0 and ref.cnt["rmask_avg"][ib, jb] == 0.0
    # one step earlier the counter held the count itself
    ref2 = au.AvgRef(b, 1, 5, 1, 1, 0, [("avgzeta", 0)])
    for k, iic in enumerate(range(2, 6)):
        weather(k, iic)
        ref2.set_avg(st, util.step_idx(iic=iic, kstp=1))
    assert ref2.cnt["rmask_avg"][ia, ja] == 3.0 and ref2.cnt["rmask_avg"][ib, jb] == 0.0
