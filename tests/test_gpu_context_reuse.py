"""-m gpu: parity of a REUSED context -- replays of the captured LOOP_2D graphs, changes made through the C ABI between
steps, and exact restart.  Every other GPU parity test builds a fresh context and runs it to the end with one
configuration; here one context is kept over a change M and compared, bit for bit on every registered field, with a
fresh context that continues from the host copy of its fields (tests/reuse_util.py), and at the whole-step bound
(1e-10 relative RMS, the FLOOR table of tests/test_gpu_main3d.py) with the oracle taken through the same sequence.

Grid 66 x 9 x 5.  k = 6 steps before the change and m = 4 after it: the graph key is computed as
roms_hip_step2d_loop does and the test asserts that a key repeated before the change and, for either nstp, after it.
tests/test_context_reuse.py shows on the oracle that every change is one the model feels; for the options the oracle
lacks (uv_adv, climatology) that is checked here against the run without the change.

Scenarios: 1 plain restart (the registered fields are the whole state), 2 ntstart = 5, 3 set_params mid-run (ndtfast,
uv_adv, drag law, dt, one edge of a basin opened, and the other members the host code of the barotropic path reads
when it decides what to launch: wet_dry switched on, uv_vis4 off and on, the point_sources bits 1 -> 2 -> 0; Dcrit;
the biharmonic coefficient by upload), 4 set_sources (0 -> 3, values, a face moved, 3 -> 5, 5 -> 0), 5 set_clima (on,
coefficients only, obcfac, switches, off), 6 pn changed along a column and put back (row table <-> arrays), 7 fields
registered again at new addresses, 8 averages and floats switched on after step k and off again, 9 masks switched on
over the library's defaults, 10 a second set_bounds in one context (also in RCCL loopback, in a child process),
11 LOOP_2D by single roms_hip_step2d calls (also in RCCL loopback with graph_exchanges(1)), 12 a context after one with
graph_exchanges(1), sources and climatology (child process).

Members of roms_params.def that decide launches and are NOT changed mid-run: masking (scenario 9 switches it on; off
again would leave land values in the fields), uv_vis4 / the advection schemes from two to three ghost points (the
ghost-point count belongs to the bounds: scenario 10), lbc_west / lbc_east to or from periodic (EWperiodic is a member
of the bounds too), gls_mixing / ts_dif4 / the other 3-D switches (no launch of the barotropic path depends on them)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import reuse_util as ru
from roms_trunk_mgh_amd import abi, ana, hip, main3d

pytestmark = pytest.mark.gpu
SCEN = ru.scenarios()
HERE = os.path.dirname(os.path.abspath(__file__))


def _same_returns(a, b):
    assert (a.iic, a.indx1, a.ntfirst) == (b.iic, b.indx1, b.ntfirst) and bytes(a.s) == bytes(b.s)
    assert (a.last_diag is None) == (b.last_diag is None)
    if a.last_diag is not None:
        assert np.array_equal(a.last_diag, b.last_diag)


def _felt_stage_by_stage(st0, changes, mkw, st_c):
    """non-vacuity on the device, for the options the oracle lacks: the run that stops changing after the first q
    changes ends elsewhere than the one that stops after q - 1"""
    total = sum(steps for _, steps in changes)
    prev = None
    for q in range(len(changes) + 1):
        done = changes[:q]
        rest = total - sum(steps for _, steps in done)
        st_q, m_q, _, _ = ru.run_continued(st0, done + ([(ru.m_none, rest)] if rest else []), True, mkw=mkw)
        if prev is not None:
            assert ru.felt(st_q, prev, m_q), ("change", q, ru.parity(st_q, prev, m_q))
        prev = st_q
    assert ru.differing(prev, st_c) == []


@pytest.mark.parametrize("name", list(SCEN))
def test_scenario(name):
    sc = SCEN[name]
    st0 = sc["state"]()
    mkw, changes = sc.get("mkw"), sc["changes"]
    seen = []                                                    # row_metrics_state() after step k and after each change
    probe = (lambda be, m: seen.append(be.row_metrics_state())) if name.startswith("pn-") else None
    st_c, m_c, keys, snap = ru.run_continued(st0, changes, True, mkw=mkw, probe=probe)
    k = ru.K
    for _, steps in changes:
        ru.assert_replays(keys[:k + steps], k)
        k += steps
    st_f, m_f = ru.run_fresh(snap, changes, mkw=mkw)
    assert ru.differing(st_c, st_f) == []                       # every registered field
    _same_returns(m_c, m_f)
    assert np.isfinite(st_c["t"]).all() and float(np.abs(st_c["u"]).max()) > 1e-6
    if name.startswith("pn-"):
        # roms_hip_row_metrics_state: the channel's metrics and depth are independent of i (3: row table), the changed
        # column sends the kernel to the arrays (2), the restored one back; a basin's metric arrays differ in the
        # columns beside its walls, so it reads the arrays throughout (the upload still drops the graphs)
        assert seen == ([3, 2, 3] if name.endswith("channel") else [2, 2, 2]), seen
    if sc.get("oracle") is not False:
        st_o, m_o, keys_o, _ = ru.run_continued(st0, changes, False, mkw=mkw)
        assert keys_o == keys
        out = ru.parity(st_c, st_o, m_o)
        assert all(v <= ru.TOL for v in out.values()), out
        if m_o.last_diag is not None:
            assert all(abs(m_c.last_diag[q] - m_o.last_diag[q]) <= 1e-9 * abs(m_o.last_diag[q]) for q in range(6))
    else:                                                        # the oracle lacks the option: the change is felt
        _felt_stage_by_stage(st0, changes, mkw, st_c)


@pytest.mark.parametrize("app", ru.APPS)
def test_ntstart_5(app):
    """scenario 2: the oracle with ntstart = 5 is the oracle with ntstart = 1 bit for bit (tests/test_context_reuse.py),
    so the same is asserted for the library; phases 0, 1 and 2 of the key all occur with ntfirst = 5"""
    st0 = ru.restart_state(app)
    st_5, m_5, keys, _ = ru.run_continued(st0, [], True, k=8, ntstart=5)
    assert {q % 4 for q, _ in keys} == {0, 1, 2} and m_5.ntfirst == 5 and m_5.iic == 13
    st_1, m_1, _, _ = ru.run_continued(st0, [], True, k=8, ntstart=1)
    assert ru.differing(st_5, st_1) == []
    st_o, m_o, _, _ = ru.run_continued(st0, [], False, k=8, ntstart=5)
    out = ru.parity(st_5, st_o, m_o)
    assert all(v <= ru.TOL for v in out.values()), out
    assert ru.differing(st_5, st0) != []


# ------------------------------------------------------------------------------------------ 5. set_clima --
def _m_clima(kind):
    def change(st, be):
        st_run, st = st, ru.clone(st)          # the climatology of a resting ocean, whatever the run's state is
        st["t"][:, :, :, :, 0] = st.p.T0
        st["t"][:, :, :, :, 1] = st.p.S0
        st.clima = st_run.clima
        if kind == "on":
            flags = np.zeros(st.b.NT, dtype=np.int32)
            flags[0] = 1
            ana.analytic_clima(st, tracers=flags, obcfac=3.0)
            only = None
        elif kind == "coefficients":
            ana.analytic_clima(st, tracers=st.clima.LnudgeTCLM, obcfac=3.0, tnudg=4.0 * st.p.dt)
            only = ("M2nudgcof", "M3nudgcof", "Tnudgcof")
        elif kind == "obcfac":
            ana.analytic_clima(st, tracers=st.clima.LnudgeTCLM, obcfac=0.5, tnudg=4.0 * st.p.dt)
            only = None
        elif kind == "switches":
            flags = np.zeros(st.b.NT, dtype=np.int32)
            flags[1] = 1
            ana.analytic_clima(st, tracers=flags, obcfac=0.5, m2=False, tnudg=4.0 * st.p.dt)
            only = None
        else:
            st.clima = None
        st_run.clima = st.clima
        st = st_run
        if be is None or be.name != "hip":
            return
        if st.clima is None:
            be._chk(be.l.roms_hip_set_clima(0, None, None, None, 0, None, None, None, None, None, None, 1.0), "set_clima")
        else:
            be.set_clima(st.clima, only=only)
    return change


@pytest.mark.parametrize("app", ru.APPS)
def test_set_clima_mid_run(app):
    """scenario 5 on a basin whose western edge is RadNud (obcfac is read there).  The oracle has no climatology: every
    stage is compared with the fresh contexts, and with the run that leaves the stage out"""
    import test_basin

    def state():
        st = ru.tile(app, {"EWperiodic": False})
        sd = abi.LBS["west"]
        for var in test_basin.RADNUD:
            st.p.lbc[sd][abi.LBV[var]] = abi.LBC["RadNud"]
            st.p.obc_out[sd][abi.LBV[var]] = 2.0e-4
            st.p.obc_in[sd][abi.LBV[var]] = 1.5e-3
        rng = np.random.default_rng(5)
        for name in ("zeta_bry", "ubar_bry", "vbar_bry", "u_bry", "v_bry"):
            st[name][:] = 1.0e-2 * rng.standard_normal(st[name].shape)
        st["t_bry"][:] = st["t"][:, :, :, 0, :]
        return st
    st0 = state()
    kinds = ["on", "coefficients", "obcfac", "switches", "off"]
    changes = [(_m_clima(q), ru.M_STEPS) for q in kinds]
    st_c, m_c, keys, snap = ru.run_continued(st0, changes, True)
    k = ru.K
    for _, steps in changes:
        ru.assert_replays(keys[:k + steps], k)
        k += steps
    st_f, m_f = ru.run_fresh(snap, changes)
    assert ru.differing(st_c, st_f) == []
    _same_returns(m_c, m_f)
    assert np.isfinite(st_c["t"]).all()
    _felt_stage_by_stage(st0, changes, None, st_c)               # each stage is felt


# ------------------------------------------------------------------------------------ 7. re-registration --
def _m_register_again(names):
    def change(st, be):
        if be is None or be.name != "hip":
            return
        for n in names:
            new = st.arr[n].copy(order="F")
            assert new.ctypes.data != st.arr[n].ctypes.data
            st.arr[n] = new
            be._chk(be.l.roms_hip_register_field(abi.FIELD_ID[n], new.ctypes.data, new.size), "register_field " + n)
        be.to_device(names)
    return change


@pytest.mark.parametrize("app", ru.APPS)
@pytest.mark.parametrize("variant", ["channel", "basin"])
def test_fields_registered_again(app, variant):
    """scenario 7: zeta, ubar and t registered again from other host arrays with the same contents -- new device
    addresses under the captured graphs.  Equal to the fresh contexts and to the run that registers nothing again."""
    st0 = ru.tile(app, {} if variant == "channel" else {"EWperiodic": False})
    changes = [(_m_register_again(["zeta", "ubar", "t"]), ru.M_STEPS)]
    st_c, m_c, keys, snap = ru.run_continued(st0, changes, True)
    ru.assert_replays(keys, ru.K)
    st_f, m_f = ru.run_fresh(snap, changes)
    st_n, m_n, _, _ = ru.run_continued(st0, [(ru.m_none, ru.M_STEPS)], True)
    assert ru.differing(st_c, st_f) == [] and ru.differing(st_c, st_n) == []
    _same_returns(m_c, m_f)
    _same_returns(m_c, m_n)
    st_o, m_o, _, _ = ru.run_continued(st0, [(ru.m_none, ru.M_STEPS)], False)      # (nothing changes for the oracle)
    out = ru.parity(st_c, st_o, m_o)
    assert all(v <= ru.TOL for v in out.values()), out


# ------------------------------------------------------------------------------------ 9. library defaults --
MASKS = ("rmask", "umask", "vmask", "pmask")


def _m_masking_on(st, be):
    ana.set_masks(st, ana.island_mask(st.cfg, st.b))             # sets p.masking
    if be is not None and be.name == "hip":
        ru.push_params(st, be)
        for n in MASKS:
            a = st.arr[n]
            be._chk(be.l.roms_hip_register_field(abi.FIELD_ID[n], a.ctypes.data, a.size), "register_field " + n)
        be.to_device(MASKS)


@pytest.mark.parametrize("app", ru.APPS)
def test_masks_over_the_library_defaults(app):
    """scenario 9: k steps without MASKING on the all-water masks the library keeps, then masking = 1 with the masks
    registered and uploaded"""
    st0 = ru.tile(app)
    changes = [(_m_masking_on, ru.M_STEPS)]
    st_c, m_c, keys, snap = ru.run_continued(st0, changes, True, be_kw=dict(leave_unregistered=MASKS))
    ru.assert_replays(keys, ru.K)
    st_f, m_f = ru.run_fresh(snap, changes)
    assert ru.differing(st_c, st_f) == []
    _same_returns(m_c, m_f)
    st_o, m_o, _, _ = ru.run_continued(st0, changes, False)
    out = ru.parity(st_c, st_o, m_o)
    assert all(v <= ru.TOL for v in out.values()), out
    st_n, m_n, _, _ = ru.run_continued(st0, [(ru.m_none, ru.M_STEPS)], False)
    assert ru.felt(st_o, st_n, m_n)


# ------------------------------------------------------------------------------------- 10. second bounds --
@pytest.mark.parametrize("app", ru.APPS)
def test_second_set_bounds(app):
    st_b, m_b, keys = ru.second_bounds_run(app)
    seen = [q for q, _ in keys]
    assert len(set(seen)) < len(seen)
    st_f, m_f = ru.plain_second_run(app)
    assert ru.differing(st_b, st_f) == []
    _same_returns(m_b, m_f)
    st_o, m_o, _, _ = ru.run_continued(ru.tile(app, dict(ru.DIF4[app], N=6)), [], False)
    out = ru.parity(st_b, st_o, m_o)
    assert all(v <= ru.TOL for v in out.values()), out


# ------------------------------------------------------------------------------ 11. LOOP_2D by single calls --
def _single_call_state(form):
    app = "BENCHMARK_TINY" if form == "channel_benchmark" else "UPWELLING"
    if form.startswith("channel"):
        return ru.tile(app)
    if form == "basin":
        return ru.tile(app, {"EWperiodic": False})
    if form == "beach":
        return ru.family_tile(app, "beach")[0]
    if form == "vis4":
        return ru.tile(app, ru.DIF4[app])
    st = ru.source_tile(app, "river")
    st.sources = ru.source_table(st, 3, "river")
    return st


@pytest.mark.parametrize("form", ["channel", "channel_benchmark", "basin", "beach", "sources", "vis4"])
def test_loop_by_single_calls(form):
    """scenario 11: the fused channel, split basin, WET_DRY, sources and UV_VIS4 forms; all by single calls, and
    interleaved -- 3 loop steps, one by single calls, 3 loop steps (the deferred-flux hand-over between the two entries,
    a replay after an eager loop)"""
    st0 = _single_call_state(form)
    st_l, m_l, _ = ru.mixed_run(st0, "LLLLLLL")
    for pattern in ("SSSSSSS", "LLLSLLL"):
        st_s, m_s, _ = ru.mixed_run(st0, pattern)
        assert ru.differing(st_l, st_s) == [], pattern
        _same_returns(m_l, m_s)
    assert float(np.abs(st_l["u"]).max()) > 1e-6


# ---------------------------------------------------------------------------------------- child processes --
def _child(tmp_path, mode, app):
    out = os.path.join(str(tmp_path), f"{mode}.npz")
    p = subprocess.Popen([sys.executable, os.path.join(HERE, "mp_gpu_reuse_worker.py"), mode, app, out],
                         env=dict(os.environ, OMP_NUM_THREADS="1"))
    try:
        assert p.wait(timeout=120) == 0
    finally:
        if p.poll() is None:
            p.kill()
    return np.load(out)


def _equal_fields(d, st):
    return [name for name, _, _ in abi.FIELDS if not np.array_equal(d[name], st[name], equal_nan=True)]


class _Fields:
    """the fields a child process saved, with TileState's interior()"""

    def __init__(self, d, like):
        self.d, self.like, self.b = d, like, like.b

    def interior(self, name):
        b = self.b
        return self.d[name][self.like.I(b.Istr, b.Iend), self.like.J(b.Jstr, b.Jend)]


def test_second_set_bounds_in_rccl_loopback(tmp_path):
    """scenario 10 with the halo plan in use: one rank with an RCCL id is its own W / E neighbour, its message plan is
    built from the bounds at the first exchange -- and must be rebuilt for the second bounds (three ghost points)"""
    app = "UPWELLING"
    d = _child(tmp_path, "bounds", app)
    st_f, _ = ru.plain_second_run(app)
    assert _equal_fields(d, st_f) == []
    st_o, m_o = ru.plain_second_run(app, hip_backend=False)
    out = ru.parity(_Fields(d, st_o), st_o, m_o)
    assert all(v <= ru.TOL for v in out.values()), out


def test_context_after_one_with_graphed_exchanges(tmp_path):
    """scenario 12: a loopback context with graph_exchanges(1), sources and climatology is closed; the next context of
    the process, which asks for nothing, runs LOOP_2D eagerly (graph_exchanges_state() == 0) and equals a plain run.
    The second context is a loopback context too, not a plain one-tile context: on one tile without an RCCL id
    graph_exchanges_state() is 1 from the ordinary one-tile graphs whatever the switch says, so only a context that
    has exchanges to capture can show that the switch is back at its default.  The plain run it is compared with is
    made in another process than the two contexts: this one (the two contexts live in the child)."""
    app = "UPWELLING"
    d = _child(tmp_path, "two_ctx", app)
    if int(d["first_state"]) == -1:
        pytest.skip("this stack refused to capture the RCCL transport in the first context (graph_exchanges_state() == -1)")
    assert int(d["first_state"]) == 1
    assert int(d["second_state"]) == 0
    st_f, _, _, _ = ru.run_continued(ru.tile(app), [], True)
    assert _equal_fields(d, st_f) == []


@pytest.mark.parametrize("app", ru.APPS)
def test_loop_by_single_calls_in_rccl_loopback(tmp_path, app):
    """scenario 11 where the deferred-flux state is in use: in loopback the channel takes the several-tiles fused call,
    whose launch leaves the next call's exchanged fluxes in the other scratch pair (g_flux_ready / g_flux_lev /
    g_flux_buf); single roms_hip_step2d calls take the general sequence.  With graph_exchanges(1): all by the loop
    (replayed graphs with the exchanges inside), all by single calls, and 3 loop steps, one by single calls, 3 loop steps
    -- each equal to the plain one-tile run, bit for bit"""
    d = _child(tmp_path, "single", app)
    if -1 in [int(v) for v in d["states"]]:
        pytest.skip("this stack refused to capture the RCCL transport (graph_exchanges_state() == -1)")
    assert [int(v) for v in d["states"]] == [1, 0, 1]            # graphs live after L.., none after S.. (never captured)
    st_l, m_l, _ = ru.mixed_run(ru.tile(app), "LLLLLLL")
    for q, pattern in enumerate(("LLLLLLL", "SSSSSSS", "LLLSLLL")):
        bad = [name for name, _, _ in abi.FIELDS if not np.array_equal(d[f"{pattern}:{name}"], st_l[name], equal_nan=True)]
        assert bad == [], (pattern, bad)
        assert int(d["indx1"][q]) == m_l.indx1


# ------------------------------------------------------------------------- 8. averages and floats mid-run --
def _switched_run(st0, on, off, fetch, half=None):
    """k steps, on(be, m), m steps (half(be, m, st) after the first two of them), fetch(be) -> kept, off(be, m), m steps"""
    st = ru.clone(st0)
    be = hip.RomsHip(st)
    try:
        m = main3d.Main3D(be)
        m.initial()
        m.run(ru.K)
        be.to_host()
        snap = (ru.clone(st), ru.resume(main3d.Main3D.__new__(main3d.Main3D), m))
        on(be, m)
        m.run(2)
        mid = half(be, m, st) if half else None
        m.run(ru.M_STEPS - 2)
        kept = fetch(be)
        off(be, m)
        m.run(ru.M_STEPS)
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    return st, m, snap, kept, mid


def _plain(st0):
    return ru.run_continued(st0, [(ru.m_none, 2 * ru.M_STEPS)], True)[:2]


@pytest.mark.parametrize("app", ru.APPS)
def test_averages_switched_on_and_off(app):
    """scenario 8: set_averages after step k, off again after m steps.  Every registered field equals the run without
    averages bit for bit; the accumulators equal those of a fresh context that starts from the host copy of step k"""
    import avg_util as au
    st0 = ru.tile(app)
    sel = au.all_in_scope(st0.b.NT)

    def averages():
        return au.averages_of(st0.b, sel, nAVG=3)

    def on(be, m):
        m.averages = averages()
        be.set_averages(m.averages)

    def off(be, m):
        m.averages = None
        be.set_averages(None)

    def fetch(be):
        return {q: be.get_average(*q) for q in sel}
    st_c, m_c, snap, got, _ = _switched_run(st0, on, off, fetch)
    st_n, m_n = _plain(st0)
    assert ru.differing(st_c, st_n) == []
    _same_returns(m_c, m_n)
    st = ru.clone(snap[0])
    be = hip.RomsHip(st)
    try:
        m = ru.resume(main3d.Main3D(be, averages=averages()), snap[1])
        m.run(ru.M_STEPS)
        want = fetch(be)
        be.check_guards()
    finally:
        be.close()
    assert all(np.array_equal(got[q], want[q], equal_nan=True) for q in sel), [q for q in sel if not np.array_equal(got[q], want[q])]
    assert all(np.isfinite(v).all() for v in got.values())
    assert float(np.abs(got[("avgzeta", 0)]).max()) > 0.0 and not np.array_equal(got[("avgzeta", 0)], st_c["zeta"][:, :, 0])


def test_floats_switched_on_and_off():
    """scenario 8: set_floats after step k, off again after m steps.  Every registered field equals the run without
    floats bit for bit; floats_get after two of the m steps -> a fresh context from the host copy -> set_floats +
    floats_put continues to the same tracks, bit for bit"""
    import mp_gpu_floats_worker as worker
    from roms_trunk_mgh_amd import floats
    app = "UPWELLING"
    st0 = ru.tile(app)

    def drifter(st):
        fl = worker.drifter(st)
        fl.Tinfo[floats.itstr] += ru.K * st.p.dt                  # released on the step the floats are switched on
        fl.Tinfo[floats.itstr, 3::7] += 3.0 * st.p.dt             # ... some on the fourth step after it
        return fl

    def on(be, m):
        m.floats = drifter(st0)
        be.set_floats(m.floats)

    def off(be, m):
        m.floats = None
        be.set_floats(None)

    def half(be, m, st):
        be.to_host()
        return ru.clone(st), ru.resume(main3d.Main3D.__new__(main3d.Main3D), m), be.floats_get(), dict(m.floats.levels)
    st_c, m_c, _, got, mid = _switched_run(st0, on, off, lambda be: be.floats_get(), half)
    st_n, m_n = _plain(st0)
    assert ru.differing(st_c, st_n) == []
    _same_returns(m_c, m_n)
    tr, bd = got
    assert bd.sum() > bd.size // 2 and not bd.all()
    st, old, (track, bounded), levels = mid
    assert not np.array_equal(track, tr, equal_nan=True)        # the floats moved on in the last two steps
    fl = drifter(st)
    fl.levels = dict(levels)
    be = hip.RomsHip(st)
    try:
        m = ru.resume(main3d.Main3D(be, floats=fl), old)
        be.floats_put(track, bounded)
        m.run(ru.M_STEPS - 2)
        want_t, want_b = be.floats_get()
        be.check_guards()
    finally:
        be.close()
    assert np.array_equal(tr, want_t, equal_nan=True) and np.array_equal(bd, want_b)
