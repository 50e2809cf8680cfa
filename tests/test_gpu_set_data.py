"""GPU: set_data on the device (roms_hip_set_data_record / _point / roms_hip_set_data, csrc/k_set_data.hip) against the numpy
statement of set_2dfld.F:90-134 and of set_data.F's destinations (tests/set_data_util.py), bit for bit.

Shapes: UPWELLING tiles (41 x 80 x 16) as a periodic channel (3818 doubles per plane) and as a closed-off basin
(43 x 83 = 3569 doubles per plane, odd: the second plane of a field with a tracer dimension is 16-byte misaligned
against its record), so that one call holds rows that take the 16-byte path, rows with a leading odd element, rows
whose sources and destination differ in phase, the strided columns of the western / eastern edges and tails."""
import copy
import ctypes as C

import numpy as np
import pytest

import clima_util as cu
import set_data_util as su
import tides_util as tu
import util
from roms_trunk_mgh_amd import abi, ana, clima, data, hip, main3d

pytestmark = pytest.mark.gpu
TA, TB = 86400.0, 97200.0
TIMES = (TA, TB, 0.5 * (TA + TB), TA + 0.0625, TA + 1234.567)
GRID = ("sustr", "svstr", "srflx", "stflux", "btflux", "Tair")
CLIM = ("ubarclm", "vbarclm", "uclm", "vclm", "tclm")
BRY = data.BOUNDARY
SENTINEL = 777.25
same = cu.same


def state(kind, **kw):
    ov = {"EWperiodic": False} if kind == "basin" else {}
    return util.prepared_state("UPWELLING", NT=3, overrides=ov, **kw)


def all_keys(st):
    """every family: 2-D rho-, u- and v-type fields, one plane of two K_2D_NT fields (the other planes left alone), the
    climatology with tclm of flags [0, 1, 1], every boundary variable on every side"""
    keys = [("sustr", 0, None), ("svstr", 0, None), ("srflx", 0, None), ("stflux", 2, None), ("btflux", 1, None), ("Tair", 0, None)]
    keys += [("ubarclm", 0, None), ("vbarclm", 0, None), ("uclm", 0, None), ("vclm", 0, None), ("tclm", 1, None), ("tclm", 2, None)]
    for side in su.SIDES:
        keys += [(n, 0, side) for n in BRY[:5]] + [("t_bry", 1, side), ("t_bry", 3, side)]
    return keys


def fetch(be, st, cl):
    be.to_host(GRID + tuple(BRY))
    out = {n: st[n].copy() for n in GRID + tuple(BRY)}
    if cl is not None:
        out.update({n: be.get_clima(cl, n) for n in CLIM})
    return out


def expected(ref, cl):
    out = {n: ref[n] for n in GRID + tuple(BRY)}
    if cl is not None:
        out.update({n: cl.arr[n] for n in CLIM})
    return out


def assert_same(got, want, what):
    for n in want:
        assert same(got[n], want[n]), (what, n, int((got[n] != want[n]).sum()))


# ---------------------------------------------------------------------------- 4. every family, one call --
@pytest.mark.parametrize("kind", ["channel", "basin"])
def test_every_target_family_in_one_call_bit_for_bit(kind):
    st = state(kind)
    b = st.b
    assert ((st.ni * st.nj) % 2 == 1) == (kind == "basin")
    rng = np.random.default_rng(7)
    for n in GRID + tuple(BRY):
        st[n][:] = rng.standard_normal(st[n].shape)
    cl = cu.random_clima(st, tracers=[0, 1, 1])
    assert cl.ic(2) == 1 and cl.ic(3) == 2
    st.clima = cl
    ref, cl_ref = st.copy(), copy.deepcopy(cl)
    be = hip.RomsHip(st)
    try:
        ncall = 0
        for Tindex in (1, 2):
            for onerec in (False, True):
                D = su.random_data(b, all_keys(st), T=(TA, TB), Tindex=Tindex, seed=10 * Tindex + onerec, onerec=onerec)
                D.attach(be)
                for time in (TIMES if not onerec else (TA + 7.0,)):
                    syn = be.set_data(time, 300.0)
                    want_syn = su.apply(ref, D, time, 300.0, clima=cl_ref)
                    assert syn == want_syn
                    assert_same(fetch(be, st, cl), expected(ref, cl_ref), (Tindex, onerec, time))
                    ncall += 1
        assert ncall == 12
        # the planes no record names and the points outside the routines' ranges kept what they had
        assert same(st["stflux"][:, :, 0], ref["stflux"][:, :, 0]) and same(st["t_bry"][:, :, :, 1], ref["t_bry"][:, :, :, 1])
        be.check_guards()
    finally:
        be.close()
    # the statement itself left the padding column / the corner-free rows alone, so "unchanged" above means something
    st0 = state(kind)
    assert not same(ref["srflx"], st0["srflx"])
    if kind == "channel":                                  # a record for a periodic side keeps nothing
        assert su.edge_points(b, "zeta_bry", "west") is None and su.edge_points(b, "zeta_bry", "south") is not None


# ------------------------------------------------------------------------------------------ 5. point data --
def test_point_data_give_the_uniform_field():
    st = state("channel")
    b = st.b
    st["Pair"][:] = SENTINEL
    st["stflux"][:] = SENTINEL
    be = hip.RomsHip(st)
    try:
        D = data.Data(b)
        D.load("Pair", 1, TA, 1013.25, point=True)
        D.load("Pair", 2, TB, 1009.5, point=True)
        D.load("stflux", 2, TB, -3.0e-6, index=2, point=True)
        D.load("stflux", 1, TA, 2.0e-6, index=2, point=True)             # Tindex = 1 holds the EARLIER time: refused below
        D.attach(be)
        with pytest.raises(RuntimeError, match="stflux.*exceeds ending value"):
            be.set_data(TA + 100.0, 60.0)
        be.to_host(["Pair", "stflux"])
        assert (st["Pair"] == SENTINEL).all() and (st["stflux"] == SENTINEL).all()
        D.load("stflux", 2, TB, -3.0e-6, index=2, point=True)
        ref = st.copy()
        for time in (TA, TA + 0.0625, TB):
            assert be.set_data(time, 60.0) == su.apply(ref, D, time, 60.0)
            be.to_host(["Pair", "stflux"])
            assert same(st["Pair"], ref["Pair"]) and same(st["stflux"], ref["stflux"])
        f1, f2, _ = su.factors(TB, 60.0, TA, TB, 2)
        inner = st["Pair"][st.I(b.IstrR):st.I(b.IendR) + 1, st.J(b.JstrR):st.J(b.JendR) + 1]
        assert (inner == f1 * 1013.25 + f2 * 1009.5).all() and (st["stflux"][:, :, 0] == SENTINEL).all()
        with pytest.raises(RuntimeError, match="point data"):
            be.set_data_point("uclm", 1, TA, 1.0)
        be.check_guards()
    finally:
        be.close()


# -------------------------------------------------------------------------------------- 6. boundary strips --
@pytest.mark.parametrize("wet", [False, True])
def test_boundary_strips_land_on_the_rows_and_columns_of_the_convention(wet):
    st = state("basin", mask="island", wet=True) if wet else state("basin")
    b = st.b
    for n in BRY:
        st[n][:] = SENTINEL
    I, J = st.I, st.J
    be = hip.RomsHip(st)
    try:
        D = data.Data(b)
        for side in su.SIDES:
            for n in BRY:
                sh = data.record_shape(b, n, side)
                for slot, T, v in ((1, TA, 1.0), (2, TB, 3.0)):
                    val = -1.0e4 if (wet and n == "zeta_bry") else v * (1 + su.SIDES.index(side)) + 0.001 * np.arange(np.prod(sh)).reshape(sh, order="F")
                    D.load(n, slot, T, np.full(sh, val) if np.isscalar(val) else val, index=2 if n == "t_bry" else 0, side=side)
        D.attach(be)
        be.set_data(0.5 * (TA + TB), 60.0)
        be.to_host(BRY)
        be.check_guards()
    finally:
        be.close()
    f1, f2, _ = su.factors(0.5 * (TA + TB), 60.0, TA, TB, 2)

    def mid(side, n):
        r = D.rec[(n, 2 if n == "t_bry" else 0, side)]
        return f1 * r["slot"][1] + f2 * r["slot"][2]
    Lm, Mm = b.Lm, b.Mm
    # v-type south = row Jstr, north = row Jend+1, from i = 0; u-type west = column Istr, east = column Iend+1; a column
    # leaves the points it shares with the southern / northern rows to them (no condition reads those)
    v = st["vbar_bry"]
    assert same(v[I(0):I(Lm + 1) + 1, J(b.Jstr)], mid("south", "vbar_bry")[I(0):I(Lm + 1) + 1]) and b.Jstr == 1
    assert same(v[I(0):I(Lm + 1) + 1, J(Mm + 1)], mid("north", "vbar_bry")[I(0):I(Lm + 1) + 1])
    u = st["ubar_bry"]
    assert same(u[I(b.Istr), J(1):J(Mm) + 1], mid("west", "ubar_bry")[J(1):J(Mm) + 1]) and b.Istr == 1
    assert same(u[I(Lm + 1), J(1):J(Mm) + 1], mid("east", "ubar_bry")[J(1):J(Mm) + 1])
    # the tangential components sit on the outer line and start at 1 (set_data.F:1023, :1050)
    assert same(v[I(0), J(2):J(Mm) + 1], mid("west", "vbar_bry")[J(2):J(Mm) + 1]) and v[I(0), J(0)] == SENTINEL
    assert same(u[I(1):I(Lm + 1) + 1, J(0)], mid("south", "ubar_bry")[I(1):I(Lm + 1) + 1]) and u[I(0), J(0)] == SENTINEL
    u3 = st["u_bry"]
    assert same(u3[I(b.Istr), J(1):J(Mm) + 1, :], mid("west", "u_bry")[J(1):J(Mm) + 1, :])
    t3 = st["t_bry"]
    assert same(t3[I(0):I(Lm + 1) + 1, J(Mm + 1), :, 1], mid("north", "t_bry")[I(0):I(Lm + 1) + 1, :])
    assert (t3[:, :, :, 0] == SENTINEL).all() and (t3[:, :, :, 2] == SENTINEL).all()
    # every other point is unchanged: interior points, and the padding beyond Lm+1 / Mm+1
    for n in BRY:
        a = st[n]
        assert (a[I(2):I(Lm - 1) + 1, J(2):J(Mm - 1) + 1] == SENTINEL).all(), n
        assert (a[I(Lm + 1) + 1:] == SENTINEL).all() and (a[:, J(Mm + 1) + 1:] == SENTINEL).all(), n
    z = st["zeta_bry"]
    if wet:        # the record lies below the bed: Dcrit - h exactly, on JstrR:JendR / IstrR:IendR of each edge
        assert st.p.wet_dry == 1
        assert same(z[I(0), J(0):J(Mm + 1) + 1], st.p.Dcrit - st["h"][I(0), J(0):J(Mm + 1) + 1])
        assert same(z[I(Lm + 1), J(0):J(Mm + 1) + 1], st.p.Dcrit - st["h"][I(Lm + 1), J(0):J(Mm + 1) + 1])
        assert same(z[I(0):I(Lm + 1) + 1, J(0)], st.p.Dcrit - st["h"][I(0):I(Lm + 1) + 1, J(0)])
        assert same(z[I(0):I(Lm + 1) + 1, J(Mm + 1)], st.p.Dcrit - st["h"][I(0):I(Lm + 1) + 1, J(Mm + 1)])
    else:
        assert same(z[I(0), J(1):J(Mm) + 1], mid("west", "zeta_bry")[J(1):J(Mm) + 1])
    ref = st.copy()
    for n in BRY:
        ref[n][:] = SENTINEL
    su.apply(ref, D, 0.5 * (TA + TB), 60.0)
    for n in BRY:
        assert same(st[n], ref[n]), n


# ------------------------------------------------------------------------------------------------ 7. tides --
def _tidal_basin():
    st = ana.make_tile("UPWELLING", perturb=1.0, overrides=dict(Lm=12, Mm=10, N=4, EWperiodic=False))
    return tu.open_all(st)


@pytest.mark.parametrize("add", [True, False])
def test_set_data_then_tides_gives_base_plus_tide(add):
    time = 3.3 * 86400.0
    Tr = (3.25 * 86400.0, 3.5 * 86400.0)
    st = _tidal_basin()
    b = st.b
    keys = [("zeta_bry", 0, side) for side in su.SIDES]
    D = su.random_data(b, keys, T=Tr, Tindex=1, seed=4, scale=0.3)
    zero = np.zeros((st.ni, st.nj), order="F")
    kw = dict(add_fsobc=True, zeta_base=zero) if add else {}
    st["zeta_bry"][:] = SENTINEL
    be = hip.RomsHip(st)
    try:
        be.set_tides(tu.general_set(st, **kw))
        D.attach(be)
        be.set_data(time, 60.0)
        be.to_host(["zeta_bry"])
        after_data = st["zeta_bry"].copy()
        be.tides(time)
        be.to_host(["zeta_bry"])
        got = st["zeta_bry"].copy()
        be.check_guards()
    finally:
        be.close()
    ref = _tidal_basin()
    ref["zeta_bry"][:] = SENTINEL
    if not add:                      # without the ADD option the record goes to zeta_bry
        su.apply(ref, D, time, 60.0)
        assert same(after_data, ref["zeta_bry"]) and (after_data != SENTINEL).sum() >= 2 * (b.Lm + b.Mm)
        return
    assert (after_data == SENTINEL).all()
    base = zero.copy(order="F")
    su.apply(ref, D, time, 60.0, bases={"zeta_bry": base})
    assert np.abs(base).max() > 0.1
    be = hip.RomsHip(ref)
    try:
        be.set_tides(tu.general_set(ref, add_fsobc=True, zeta_base=base))
        be.tides(time)
        be.to_host(["zeta_bry"])
    finally:
        be.close()
    assert same(got, ref["zeta_bry"]) and (got != SENTINEL).sum() >= 2 * (b.Lm + b.Mm)


# ------------------------------------------------------------------------- 8. all or nothing and refusals --
def test_all_or_nothing_and_refusals_by_name():
    st = state("channel")
    b = st.b
    names = ("srflx", "sustr", "Tair")
    for n in names:
        st[n][:] = SENTINEL
    be = hip.RomsHip(st)
    lib = be.l
    try:
        assert be.set_data(TA, 60.0) == 0                                # no records: a no-op
        D = su.random_data(b, [(n, 0, None) for n in names], T=(TA, TB))
        D.load("sustr", 2, TA + 50.0, D.rec[("sustr", 0, None)]["slot"][2])     # ends before the time asked for below
        D.attach(be)
        with pytest.raises(RuntimeError) as e:
            be.set_data(TA + 100.0, 60.0)
        msg = str(e.value)
        assert "sustr" in msg and "exceeds ending value" in msg and "%.6f" % TA in msg and "%.6f" % (TA + 50.0) in msg
        be.to_host(names)
        assert all((st[n] == SENTINEL).all() for n in names)
        D.load("sustr", 2, TB, D.rec[("sustr", 0, None)]["slot"][2])
        ref = st.copy()
        assert be.set_data(TA + 100.0, 60.0) == su.apply(ref, D, TA + 100.0, 60.0) == 0
        be.to_host(names)
        assert all(same(st[n], ref[n]) and not (st[n] == SENTINEL).all() for n in names)

        def refused(pattern, *args):
            assert lib.roms_hip_set_data_record(*args) != 0
            msg = lib.roms_hip_last_error().decode()
            assert pattern in msg, msg
        rec = np.zeros(st.ni * st.nj * b.N)
        p = rec.ctypes.data
        nij = st.ni * st.nj
        refused("a record has %d doubles" % nij, data.DATA_ID["Pair"], 0, 0, 1, TA, 0, p, nij + 1)
        refused("unknown target", data.DATA_COUNT, 0, 0, 1, TA, 0, p, nij)
        refused("unknown target", -1, 0, 0, 1, TA, 0, p, nij)
        refused("slot 3 outside 1..2", data.DATA_ID["Pair"], 0, 0, 3, TA, 0, p, nij)
        refused("stflux: unknown index", data.DATA_ID["stflux"], b.NT + 1, 0, 1, TA, 0, p, nij)
        refused("zeta_bry: unknown side", data.DATA_ID["zeta_bry"], 0, 4, 1, TA, 0, p, st.ni)
        refused("roms_hip_set_clima", data.DATA_ID["uclm"], 0, 0, 1, TA, 0, p, nij * b.N)
        refused("roms_hip_set_clima", data.DATA_ID["tclm"], 1, 0, 1, TA, 0, p, nij * b.N)
        # a side that is no physical edge of the tile: accepted, nothing kept
        assert lib.roms_hip_set_data_record(data.DATA_ID["zeta_bry"], 0, 0, 1, TA, 0, p, st.nj) == 0
        # the refused calls left the records alone
        assert be.set_data(TA + 100.0, 60.0) == 0
        # a slot never filled
        be.set_data_record("Pair", 2, TB, rec[:nij].reshape((st.ni, st.nj), order="F"))
        with pytest.raises(RuntimeError, match="Pair: slot 1 was never filled"):
            be.set_data(TA + 100.0, 60.0)
        be.set_data_record("Pair", 2, TB, rec[:nij].reshape((st.ni, st.nj), order="F"), onerec=True)      # ... unless onerec
        assert be.set_data(TA + 100.0, 60.0) == 0
        be.check_guards()
    finally:
        be.close()


# ------------------------------------------------------------------------------------------ 9. whole steps --
def _forcing_case():
    st = util.prepared_state("UPWELLING")
    keys = [("sustr", 0, None), ("svstr", 0, None), ("srflx", 0, None), ("stflux", 1, None), ("stflux", 2, None)]
    base = {k: (st[k[0]][:, :, k[1] - 1] if k[1] else st[k[0]]) for k in keys}
    return st, None, keys, base, dict(physics=True)


def _basin_case():
    st = cu.radnud(util.prepared_state("UPWELLING", overrides={"EWperiodic": False}))
    for sd in ("west", "east"):                              # clamped and Flather edges beside the RadNud ones
        for var, code in (("zeta", "Cla"), ("ubar", "Fla"), ("vbar", "Fla"), ("u", "Cla"), ("v", "Cla"), ("t", "Cla")):
            st.p.lbc[abi.LBS[sd]][abi.LBV[var]] = abi.LBC[code]
    keys, base = [], {}
    for side in su.SIDES:
        for n in BRY:
            for index in ((1, 2) if n == "t_bry" else (0,)):
                k = (n, index, side)
                (ii, jj), rec = su.edge_points(st.b, n, side)
                full = np.zeros(data.record_shape(st.b, n, side), order="F")
                src = st[n][:, :, :, index - 1] if index else st[n]
                full[rec] = src[ii, jj]
                keys.append(k)
                base[k] = full
    return st, None, keys, base, {}


def _clima_case():
    st = util.prepared_state("UPWELLING")
    b, p = st.b, st.p
    rng = np.random.default_rng(21)
    r = lambda *sh: rng.random(sh)
    ni, nj, N = st.ni, st.nj, b.N
    cl = clima.Clima(b, LnudgeM3CLM=True, M3nudgcof=(0.05 + r(ni, nj, N)) * 0.4 / p.dt, uclm=0.2 * (r(ni, nj, N) - 0.5),
                     vclm=0.2 * (r(ni, nj, N) - 0.5), LnudgeTCLM=np.ones(b.NT, dtype=np.int32),
                     Tnudgcof=(0.05 + r(ni, nj, N, b.NT)) * 0.4 / p.dt, tclm=5.0 + 20.0 * r(ni, nj, N, b.NT))
    keys = [("uclm", 0, None), ("vclm", 0, None)] + [("tclm", ic, None) for ic in range(1, b.NT + 1)]
    base = {k: (cl.arr[k[0]][..., k[1] - 1] if k[1] else cl.arr[k[0]]) for k in keys}
    return st, cl, keys, base, {}


@pytest.mark.parametrize("case", [_forcing_case, _basin_case, _clima_case], ids=["forcing", "open_basin", "climatology"])
def test_six_steps_equal_the_host_interpolating_and_uploading(case):
    st0, cl0, keys, base, mkw = case()
    b, dt = st0.b, st0.p.dt
    rng = np.random.default_rng(31)
    # three records per key: slots (1, 2) at 0 and 2.5 dt, then slot 1 again at 5.5 dt, loaded after step 3
    rec = {k: [base[k] * (1.0 + 0.005 * rng.standard_normal(base[k].shape)) + 1.0e-3 * rng.standard_normal(base[k].shape)
               for _ in range(3)] for k in keys}
    Trec = (0.0, 2.5 * dt, 5.5 * dt)

    def records(n):
        D = data.Data(b)
        for k in keys:
            for q in range(n):
                D.load(k[0], 1 + q % 2, Trec[q], rec[k][q], index=k[1], side=k[2])
        return D
    names = sorted({k[0] for k in keys if k[0] in abi.FIELD_ID})
    clnames = sorted({k[0] for k in keys if k[0] not in abi.FIELD_ID})
    prog = ("t", "u", "v", "ubar", "vbar", "zeta")

    # the device route
    sa = st0.copy()
    sa.clima = copy.deepcopy(cl0)
    be = hip.RomsHip(sa)
    try:
        Da = records(2)
        m = main3d.Main3D(be, data=Da, **mkw)
        m.initial()
        syn_a = []
        for n in range(6):
            if n == 3:
                for k in keys:
                    Da.load(k[0], 1, Trec[2], rec[k][2], index=k[1], side=k[2])
            m.step()
            syn_a.append(m.last_synchro)
        be.to_host()
        be.check_guards()
    finally:
        be.close()

    # the route a host takes without it: interpolate with numpy, upload the result every step
    sb = st0.copy()
    clb = copy.deepcopy(cl0)
    sb.clima = clb
    be = hip.RomsHip(sb)
    try:
        Db = records(2)
        m = main3d.Main3D(be, **mkw)
        m.initial()
        syn_b = []
        for n in range(6):
            if n == 3:
                for k in keys:
                    Db.load(k[0], 1, Trec[2], rec[k][2], index=k[1], side=k[2])
            syn_b.append(su.apply(sb, Db, n * dt, dt, clima=clb))
            if names:
                be.to_device(names)
            if clnames:
                be.set_clima(clb, only=clnames)
            m.step()
        be.to_host(prog)
    finally:
        be.close()
    assert syn_a == syn_b == [0, 0, 1, 0, 0, 1]
    for n in prog:
        assert same(sa[n], sb[n]), (n, float(np.nanmax(np.abs(sa[n] - sb[n]))))
        assert np.isfinite(sa.interior(n)).all(), n


# ------------------------------------------------------------------------------------------------ 11. reuse --
def test_set_bounds_drops_the_records():
    st = state("channel")
    b = st.b
    keys = [("srflx", 0, None), ("stflux", 2, None), ("vbar_bry", 0, "south")]
    D = su.random_data(b, keys, T=(TA, TB))
    names = ("srflx", "stflux", "vbar_bry")
    fresh = st.copy()
    be = hip.RomsHip(fresh)
    try:
        D.attach(be)
        be.set_data(TA + 500.0, 60.0)
        be.to_host(names)
    finally:
        be.close()
    be = hip.RomsHip(st)
    try:
        D.attach(be)
        be.set_data(TB, 60.0)
        be._chk(be.l.roms_hip_set_bounds(C.byref(st.b)), "set_bounds")
        be._chk(be.l.roms_hip_set_params(C.byref(st.p)), "set_params")
        assert be.set_data(TA + 500.0, 60.0) == 0                       # the records are gone: nothing to do
        for name, _, _ in abi.FIELDS:
            a = st.arr[name]
            be._chk(be.l.roms_hip_register_field(abi.FIELD_ID[name], a.ctypes.data, a.size), "register_field " + name)
        ref = state("channel")
        for n in names:
            st[n][:] = ref[n]
        be.to_device()
        assert be.set_data(TA + 500.0, 60.0) == 0
        be.to_host(names)
        assert all(same(st[n], ref[n]) for n in names)                  # ... and nothing was written
        D.attach(be)
        be.set_data(TA + 500.0, 60.0)
        be.to_host(names)
        be.check_guards()
    finally:
        be.close()
    for n in names:
        assert same(st[n], fresh[n]) and not same(st[n], ref[n]), n


# ----------------------------------------------------------------------------------------------- 10. tiling --
@pytest.mark.parametrize("variant", ["channel", "basin"])
@pytest.mark.parametrize("ntI,ntJ", [(2, 2), (4, 1)])
def test_tiled_set_data_equals_the_single_tile(tmp_path, ntI, ntJ, variant):
    """owned points, and for the rho-type and the boundary arrays every ghost point of the tile: the periodic images, the
    neighbours' points and the stretch of an edge row that a neighbour's corner reads"""
    import mp_gpu_set_data_worker as worker
    import tiling_util
    st = worker.tiled_state(variant)
    be = hip.RomsHip(st)
    try:
        want = worker.run(be, st)
    finally:
        be.close()
    ref = worker.tiled_state(variant)
    su.apply(ref, worker.records(ref), worker.TIME, 60.0)
    for n in worker.FIELDS:
        assert same(want[n], ref[n]) and not (want[n] == worker.SENTINEL).all(), n
    tiling_util.spawn_ranks("mp_gpu_set_data_worker.py", ntI * ntJ, [ntI, ntJ, tmp_path, variant], timeout=300)
    tiling_util.assert_tiles_equal(tmp_path, ntI * ntJ, want, st.b, worker.FIELDS, owned="IstrR:IendR",
                                   rho_ghosts=worker.RHO_GHOSTS)
