"""Helpers of tests/test_gpu_context_reuse.py and tests/test_context_reuse.py: one context kept over a change.

A scenario is (state A, k steps, a change M, m steps).  It is run three ways:

  continued   one context: initial(), k steps under A, M through the C ABI, m steps
  fresh       every registered field of the continued run after step k (to_host), the host side of M applied to that
              copy, a NEW context from it, the step counters taken over (resume: no start-up branch), m steps
  oracle      the same sequence on oracle.Oracle, M applied to st.p / st.sources

continued == fresh bit for bit on every registered field; continued against the oracle at the whole-step bound.

A change is a function M(st, be): it edits the host side (st.p, st.sources, st.clima, host arrays) and, where `be` is
not None, hands the edit to the backend the way a ROMS host would (set_params, set_sources, set_clima, sync_to_device).
With be = None it only prepares the host copy a fresh context is then built from.  It must be a function of `st` alone.

The shape is 66 x 9 x 5: two workgroups in x with two live columns in the second, three workgroup rows."""
import ctypes as C

import numpy as np

import util
from roms_trunk_mgh_amd import abi, ana, main3d
from roms_trunk_mgh_amd.state import rel_rms

SHAPE = dict(Lm=66, Mm=9, N=5)
APPS = ["UPWELLING", "BENCHMARK_TINY"]
TOL = 1e-10                                        # the whole-step bound (tests/test_gpu_main3d.py)
K, M_STEPS = 6, 4
DIF4 = {"UPWELLING": {"uv_vis4": 1, "visc4": 4.0e7}, "BENCHMARK_TINY": {"uv_vis4": 1, "visc4": 2.0e10}}
VIS4_SWITCH = {"UPWELLING": 4.0e7, "BENCHMARK_TINY": 2.0e11}
# the option families of scenario 1: overrides, mask, NT, physics
FAMILIES = {
    "channel": dict(ov={}, mask=None),
    "basin": dict(ov={"EWperiodic": False}, mask=None),
    "beach": dict(ov={"EWperiodic": False, "wet_dry": 1, "beach": 1, "zeta_amp": 0.3}, mask="island"),
    "mpdata6": dict(ov={"Hadv": "MPDATA", "Vadv": "MPDATA"}, mask=None, NT=6),
    "gls": dict(ov={"gls": "k-epsilon"}, mask=None),
    "physics": dict(ov={}, mask=None, physics=True),
}


def floor_table():
    import test_gpu_main3d
    return test_gpu_main3d.FLOOR


def clone(st):
    """a copy with its own parameter block (TileState.copy shares it)"""
    other = st.copy()
    other.p = type(st.p).from_buffer_copy(st.p)
    return other


def tile(app, ov=None, mask=None, NT=None):
    o = dict(SHAPE, **(ov or {}))
    if o.get("gls"):
        o = dict(util.GLS_BUILDS[ana.CONFIGS[app]["app"]], **o)
    st = ana.make_tile(app, perturb=1.0, NT=NT, overrides=o, mask=mask)
    st.p = type(st.p).from_buffer_copy(st.p)
    # the fixed KPP stand-in of ana.make_tile divides by the bed's depth: 0 / 0 where the beach crosses the resting level
    st["ghats"][~np.isfinite(st["ghats"])] = 0.0
    b = st.b
    assert (b.Lm, b.Mm, b.N) == (66, 9, o["N"])
    assert (b.Iend - b.Istr + 1) - 64 == 2 and (b.Jend - b.Jstr + 1 + 3) // 4 == 3
    return st


def family_tile(app, family):
    f = FAMILIES[family]
    return tile(app, f["ov"], f["mask"], f.get("NT")), dict(physics=bool(f.get("physics")), diagnostics=bool(f.get("physics")))


def restart_state(app):
    """a prepared state (every time level filled) for the runs that begin at ntstart = 5"""
    st = clone(util.prepared_state(app, overrides=dict(SHAPE)))
    assert (st.b.Lm, st.b.Mm, st.b.N) == (66, 9, 5)
    return st


# --------------------------------------------------------------------------------------------- graph keys --
def graph_key(indx1, s):
    """the key of roms_hip_step2d_loop (csrc/k_step2d.hip)"""
    phase = 0 if s.iic == s.ntfirst else (1 if s.iic == s.ntfirst + 1 else 2)
    return ((indx1 * 4 + s.nstp) * 4 + s.nnew) * 4 + phase


class Recorder:
    """Main3D whose LOOP_2D calls are noted: keys[n] = the graph key of step n + 1"""

    def __init__(self, m):
        self.m, self.keys = m, []
        loop = m.be.step2d_loop

        def noted(s, indx1):
            self.keys.append((graph_key(indx1, s), s.nstp))
            return loop(s, indx1)
        self._loop = noted

    def run(self, n):
        m = self.m
        for _ in range(n):
            inner, m.be.step2d_loop = m.be.step2d_loop, self._loop
            try:
                m.step()
            finally:
                m.be.step2d_loop = inner


def assert_replays(keys, k):
    """a cached graph is replayed before the change (some key of steps 1..k occurs twice), and after it -- the change
    drops the cache -- a key of either nstp parity occurs twice"""
    before, after = keys[:k], keys[k:]
    seen = [q for q, _ in before]
    assert len(set(seen)) < len(seen), ("no replay before the change", before)
    for nstp in (1, 2):
        mine = [q for q, n in after if n == nstp]
        assert len(mine) >= 2 and len(set(mine)) < len(mine), ("no replay after the change", nstp, after)


def resume(new, old):
    """continue `old`'s run in the Main3D `new`: the same iic, ntfirst, indx1 and roms_step_idx_t -- not a new
    ntstart, so that no start-up branch is taken"""
    new.iic, new.ntstart, new.ntfirst, new.indx1 = old.iic, old.ntstart, old.ntfirst, old.indx1
    new.s = abi.StepIdx.from_buffer_copy(old.s)
    new.last_diag = None if old.last_diag is None else old.last_diag.copy()
    return new


# ------------------------------------------------------------------------------------------------ changes --
def push_params(st, be):
    if be is not None and be.name == "hip":
        be._chk(be.l.roms_hip_set_params(C.byref(st.p)), "set_params")


def upload(be, names):
    if be is not None and be.name == "hip":
        be.to_device(names)


def push_sources(st, be):
    if be is None:
        return
    if st.sources is not None and st.sources.n > 0:
        be.set_sources(st.sources)
    elif be.name == "hip":
        be._chk(be.l.roms_hip_set_sources(0, None, None, None, None, None, None, None), "set_sources")
    else:                                  # (0, arrays): an application without sources; (0, NULL) would forget the table
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        i0, d0 = (C.c_int * 1)(), (C.c_double * 1)()
        ci, cd = C.cast(i0, ip), C.cast(d0, dp)
        assert be.l.oracle_set_sources(0, ci, ci, cd, cd, cd, cd, ci, st.b.N, st.b.NT) == 0


def m_none(st, be):
    pass


def m_ndtfast(st, be):
    """ndtfast / nfast and the weights of set_weights: another number of launches in LOOP_2D"""
    nd = st.p.ndtfast + 7
    nfast, w1, w2 = ana.set_weights(nd)
    st.p.ndtfast, st.p.nfast, st.p.dtfast = nd, nfast, st.p.dt / nd
    for q in range(2 * nd):
        st.p.weight1[q], st.p.weight2[q] = w1[q], w2[q]
    push_params(st, be)


def m_uvadv(scheme):
    def change(st, be):
        st.p.uv_adv = abi.uv_adv(*scheme) if scheme else 1
        push_params(st, be)
    return change


def m_drag(st, be):
    """the drag law (linear <-> quadratic) and its coefficient"""
    st.p.uv_drag = 1 if st.p.uv_drag == 2 else 2
    st["rdrag"][:] = 3.0e-2
    st["rdrag2"][:] = 3.0e-1
    push_params(st, be)
    upload(be, ["rdrag", "rdrag2"])


def m_dt(st, be):
    st.p.dt = 0.5 * st.p.dt
    st.p.dtfast = st.p.dt / st.p.ndtfast
    push_params(st, be)


def m_open_west(st, be):
    """one edge of a basin: closed -> Chapman / Flather (all-closed selects the fused barotropic kernel's wall code)"""
    sd = abi.LBS["west"]
    for var, code in (("zeta", "Cha"), ("ubar", "Fla"), ("vbar", "Fla")):
        st.p.lbc[sd][abi.LBV[var]] = abi.LBC[code]
    push_params(st, be)


def m_vis4_coefficient(st, be):
    st["visc4_r"][:] *= 3.0
    st["visc4_p"][:] *= 3.0
    upload(be, ["visc4_r", "visc4_p"])


def m_wetdry_dcrit(st, be):
    st.p.Dcrit = 3.0 * st.p.Dcrit
    push_params(st, be)


def m_wet_dry_on(st, be):
    """WET_DRY switched on over registered masks (all wet): the fused one-launch barotropic form gives way to the
    general sequence with the mask launches.  Dcrit above the shallowest water, so that cells fall dry and the model
    feels it"""
    water = st["rmask"] > 0.5
    st.p.wet_dry = 1
    st.p.Dcrit = 1.1 * float(st["h"][water].min())
    push_params(st, be)


def m_uv_vis4(on):
    """the biharmonic pass of step2d (a launch of its own in front of the momentum kernel) taken out / put back"""
    def change(st, be):
        st.p.uv_vis4 = int(on)
        push_params(st, be)
    return change


def m_source_bits(bits, kind=None):
    """roms_params_t.point_sources changed in a live context: set_params drops the source store (the maps were built
    for the old switches), the new kind's table is handed over again; bits = 0: the application has no sources"""
    def change(st, be):
        st.p.point_sources = bits
        st.sources = source_table(st, 3, kind) if bits else None
        push_params(st, be)
        if bits:
            push_sources(st, be)
    return change


def source_table(st, n, kind, moved=False, scale=1.0):
    """the first n sources of a fixed list of five: rivers through the southern wall (v-faces; `moved`: the second one
    a column further east), or wells (Dsrc = 2)"""
    from roms_trunk_mgh_amd import sources
    b = st.b
    q0 = {"UPWELLING": 1.3e3 * 41 * 80, "BENCHMARK": 1.0e9 * 64 * 32}[st.cfg["app"]] / (b.Lm * b.Mm)
    if kind == "river":
        I = [5, 63 + int(moved), 65, 30, 66]             # beside and across the workgroup seam, the last live column
        J = [1, 1, 1, 1, 1]
        D = [1.0] * 5
    else:
        I = [5, 63 + int(moved), 65, 30, 66]
        J = [2, 5, 9, 4, 1]
        D = [2.0] * 5
    Q = [q0, 0.6 * q0, 0.8 * q0, 0.5 * q0, 0.7 * q0]
    I, J, D, Q = I[:n], J[:n], D[:n], [scale * q for q in Q[:n]]
    w = np.linspace(1.0, 3.0, b.N)
    Tsrc = np.zeros((n, b.N, b.NT))
    for it in range(b.NT):
        Tsrc[:, :, it] = 4.0 + 2.0 * it + 0.1 * np.arange(n)[:, None] + 0.01 * scale
    ltr = np.array([1] + [0] * (b.NT - 1), dtype=np.int32)
    return sources.Sources(I, J, D, Q, np.tile(w / w.sum(), (n, 1)), Tsrc, ltr)


def m_sources(kind, n, moved=False, scale=1.0):
    def change(st, be):
        st.sources = source_table(st, n, kind, moved, scale) if n else None
        push_sources(st, be)
    return change


def source_tile(app, kind):
    """point_sources set from the start, Nsrc = 0 given"""
    st = tile(app, {"EWperiodic": False})
    st.p.point_sources = 1 if kind == "river" else 2
    st.sources = None
    return st


def m_pn_column(restore):
    """pn changed along one column (the row table must give way to the arrays), or put back"""
    def change(st, be):
        col = st.I(40)
        if restore:
            st["pn"][col, :] = st["pn"][col - 1, :]
        else:
            st["pn"][col, :] *= 1.25
        upload(be, ["pn"])
    return change


# --------------------------------------------------------------------------------------------------- runs --
def open_backend(st, hip_backend, **kw):
    import oracle
    if hip_backend:
        from roms_trunk_mgh_amd import hip
        be = hip.RomsHip(st, **kw)
    else:
        be = oracle.Oracle(st)
    if st.p.point_sources and getattr(st, "sources", None) is None:
        push_sources(st, be)
    return be


def run_continued(st0, changes, hip_backend, k=K, m=M_STEPS, mkw=None, ntstart=1, on_step_k=None, initial=True, be_kw=None, probe=None):
    """changes: a list of (M, steps after it).  Returns (final state, Main3D, keys, snapshot): snapshot = (host copy of
    every registered field after step k, the Main3D's counters then) for the fresh run."""
    st = clone(st0)
    be = open_backend(st, hip_backend, **(be_kw or {}))
    try:
        mm = main3d.Main3D(be, ntstart=ntstart, **(mkw or {}))
        rec = Recorder(mm)
        if initial:
            mm.initial()
        rec.run(k)
        be.to_host()
        snap = (clone(st), resume(main3d.Main3D.__new__(main3d.Main3D), mm))
        if on_step_k:
            on_step_k(be, mm)
        if probe:
            probe(be, mm)
        for change, steps in changes:
            be.to_host()                   # the host arrays are current whenever a change reads them
            change(st, be)
            rec.run(steps)
            if probe:
                probe(be, mm)
        be.to_host()
        if hip_backend:
            be.check_guards()
    finally:
        if hip_backend:
            be.close()
    return st, mm, rec.keys, snap


def run_fresh(snap, changes, mkw=None, be_kw=None):
    """the run continued in NEW contexts: one per change, each built from the host copy of the one before"""
    from roms_trunk_mgh_amd import hip
    st, old = clone(snap[0]), snap[1]
    for change, steps in changes:
        change(st, None)
        be = hip.RomsHip(st, **(be_kw or {}))
        try:
            if st.p.point_sources and getattr(st, "sources", None) is None:
                push_sources(st, be)
            mm = resume(main3d.Main3D(be, **(mkw or {})), old)
            mm.run(steps)
            be.to_host()
            be.check_guards()
        finally:
            be.close()
        old = mm
    return st, old


def differing(a, b):
    """names of the registered fields that are not bit-equal"""
    return [name for name, _, _ in abi.FIELDS if not np.array_equal(a[name], b[name], equal_nan=True)]


def parity(st_h, st_o, m):
    """relative RMS of the compared fields (zeta, ubar, vbar, u, v and each tracer) with the FLOOR table"""
    F = floor_table()
    s = m.s
    out = {"zeta": rel_rms(st_h.interior("zeta")[..., m.indx1 - 1], st_o.interior("zeta")[..., m.indx1 - 1], F["zeta"])}
    for name in ("ubar", "vbar"):
        out[name] = rel_rms(st_h.interior(name)[..., m.indx1 - 1], st_o.interior(name)[..., m.indx1 - 1], F[name])
    for name in ("u", "v"):
        out[name] = rel_rms(st_h.interior(name)[..., s.nnew - 1], st_o.interior(name)[..., s.nnew - 1], F[name])
    for it in range(st_o.b.NT):
        out[f"t{it + 1}"] = rel_rms(st_h.interior("t")[..., s.nnew - 1, it], st_o.interior("t")[..., s.nnew - 1, it], F["t"])
    return out


def felt(st_with, st_without, m):
    """non-vacuity: the change moved a compared field by more than 100 x the parity bound"""
    return max(parity(st_with, st_without, m).values()) > 100.0 * TOL


# --------------------------------------------------------------------------------------- LOOP_2D by hand --
def loop_by_single_calls(be, s, indx1):
    """LOOP_2D of main3d.F:592-700 as 2 nfast + 1 step2d calls (the sequencing of step2d_loop_body, csrc/k_step2d.hip)"""
    nfast = be.st.p.nfast
    predictor = 0
    for my_iif in range(1, nfast + 2):
        next_indx1 = 3 - indx1
        if not predictor:
            predictor = 1
            s.iif = my_iif
            s.kstp = indx1 if s.iif == 1 else 3 - indx1
            s.knew = 3
            s.krhs = indx1
        s.predictor_2d_step = predictor
        be.call("step2d", s)
        if predictor:
            predictor = 0
            s.knew = next_indx1
            s.kstp = 3 - s.knew
            s.krhs = 3
            if s.iif < nfast + 1:
                indx1 = next_indx1
        s.predictor_2d_step = predictor
        if s.iif < nfast + 1:
            be.call("step2d", s)
    return indx1


def mixed_run(st0, pattern, be_kw=None, graph_exchanges=False):
    """pattern: per step "L" (roms_hip_step2d_loop) or "S" (the 2 nfast + 1 single roms_hip_step2d calls).  Returns
    (state, Main3D, graph_exchanges_state() after the run)"""
    from roms_trunk_mgh_amd import hip
    st = clone(st0)
    be = hip.RomsHip(st, **(be_kw or {}))
    try:
        if graph_exchanges:
            be.graph_exchanges(1)
        m = main3d.Main3D(be)
        m.initial()
        loop = be.step2d_loop
        for how in pattern:
            be.step2d_loop = loop if how == "L" else (lambda s, indx1: loop_by_single_calls(be, s, indx1))
            m.step()
        be.step2d_loop = loop
        state = be.graph_exchanges_state()
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    return st, m, state


def second_bounds_run(app, be_kw=None):
    """66 x 9 x 5 with two ghost points for k steps, then roms_hip_set_bounds to 66 x 9 x 6 with UV_VIS4 (three ghost
    points) in the SAME context: parameters, registration, upload, k steps.  Returns the second state."""
    from roms_trunk_mgh_amd import hip
    st_a = tile(app)
    st_b = tile(app, dict(DIF4[app], N=6))
    assert st_a.b.NghostPoints == 2 and st_b.b.NghostPoints == 3 and st_b.p.uv_vis4 == 1
    be = hip.RomsHip(st_a, **(be_kw or {}))
    try:
        m = main3d.Main3D(be)
        m.initial()
        m.run(K)
        be._chk(be.l.roms_hip_set_bounds(C.byref(st_b.b)), "set_bounds")
        be._chk(be.l.roms_hip_set_params(C.byref(st_b.p)), "set_params")
        for name, _, _ in abi.FIELDS:
            a = st_b.arr[name]
            be._chk(be.l.roms_hip_register_field(abi.FIELD_ID[name], a.ctypes.data, a.size), "register_field " + name)
        be.st = st_b
        be.to_device()
        m = main3d.Main3D(be)
        rec = Recorder(m)
        m.initial()
        rec.run(K)
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    return st_b, m, rec.keys


def plain_second_run(app, hip_backend=True):
    st = tile(app, dict(DIF4[app], N=6))
    return run_continued(st, [], hip_backend)[:2]


# ---------------------------------------------------------------------------------------------- scenarios --
def scenarios():
    """name -> dict(state = () -> st0, changes = [(M, steps)], mkw, oracle = the oracle has the options,
    none = the changes that leave the model alone (for the non-vacuity run))"""
    S = {}
    for app in APPS:
        for fam in FAMILIES:
            def state(app=app, fam=fam):
                return family_tile(app, fam)[0]
            S[f"restart-{app}-{fam}"] = dict(state=state, changes=[(m_none, M_STEPS)], mkw=family_tile(app, fam)[1], vacuous=True)
        chan = lambda app=app: tile(app)
        basin = lambda app=app: tile(app, {"EWperiodic": False})
        for vname, v in (("channel", chan), ("basin", basin)):
            S[f"ndtfast-{app}-{vname}"] = dict(state=v, changes=[(m_ndtfast, M_STEPS)])
            # (the oracle has the default momentum advection only)
            S[f"uvadv-{app}-{vname}"] = dict(state=v, changes=[(m_uvadv(("C2", "C2")), M_STEPS), (m_uvadv(None), M_STEPS)],
                                             oracle=False)
            S[f"pn-{app}-{vname}"] = dict(state=v, changes=[(m_pn_column(False), M_STEPS), (m_pn_column(True), M_STEPS)])
        S[f"drag-{app}"] = dict(state=chan, changes=[(m_drag, M_STEPS)], mkw=dict(physics=True))
        S[f"dt-{app}"] = dict(state=chan, changes=[(m_dt, M_STEPS)])
        S[f"lbc-{app}"] = dict(state=basin, changes=[(m_open_west, M_STEPS)])
        S[f"visc4-{app}"] = dict(state=lambda app=app: tile(app, DIF4[app]), changes=[(m_vis4_coefficient, M_STEPS)])
        for kind in ("river", "well"):
            S[f"sources-{app}-{kind}"] = dict(
                state=lambda app=app, kind=kind: source_tile(app, kind),
                changes=[(m_sources(kind, 3), M_STEPS), (m_sources(kind, 3, scale=1.5), M_STEPS),
                         (m_sources(kind, 3, moved=True, scale=1.5), M_STEPS), (m_sources(kind, 5, moved=True, scale=1.5), M_STEPS),
                         (m_sources(kind, 0), M_STEPS)])
        S[f"wetdry_on-{app}"] = dict(state=lambda app=app: tile(app, mask="island"), changes=[(m_wet_dry_on, M_STEPS)])
        # (BENCHMARK: a coefficient ten times DIF4's, so that four steps with the operator back on move ubar by more
        # than 1e-8; UPWELLING's is felt as it is and unstable at ten times)
        S[f"vis4_switch-{app}"] = dict(state=lambda app=app: tile(app, dict(DIF4[app], visc4=VIS4_SWITCH[app])),
                                       changes=[(m_uv_vis4(False), M_STEPS), (m_uv_vis4(True), M_STEPS)])

        def rivers(app=app):
            st = source_tile(app, "river")
            st.sources = source_table(st, 3, "river")
            return st
        S[f"source_bits-{app}"] = dict(state=rivers, changes=[(m_source_bits(2, "well"), M_STEPS), (m_source_bits(0), M_STEPS)])
    S["dcrit-UPWELLING-beach"] = dict(state=lambda: family_tile("UPWELLING", "beach")[0], changes=[(m_wetdry_dcrit, M_STEPS)])
    return S
