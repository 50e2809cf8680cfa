"""set_tides_tile (ROMS/Nonlinear/set_tides.F:116-643) and the SSH_TIDES-without-UV_TIDES boundary value of the Flather
and Shchepetkin conditions (u2dbc_im.F:219-255 ..., v2dbc_im.F:221-257 ...) restated in numpy, statement for statement
and in the reference's order: the yardstick of tests/test_tides.py (known answers, no GPU) and tests/test_gpu_tides.py.

The routine USEs mod_tides and the netCDF layer, so the reference cannot make a vector for it (as for set_avg and
step_floats).  Every statement is an elementwise operation on the index ranges the reference loops over, so the bits are
those of the scalar loops.  The edge vectors zeta_west(j) ... vbar_north(i) are written at the point the *_bry convention
of include/roms_fields.def gives them; the four corner rho-points of zeta_bry, where two vectors meet with different
values and which no condition reads, are left alone."""
import math

import numpy as np

from roms_trunk_mgh_amd import abi, ana, tides as tides_mod

PI = 3.14159265358979323846          # mod_scalars.F:788
DAY2SEC = 86400.0
SIDES = ("west", "east", "south", "north")


def acquire(p, side, var):
    """LBC(side, var)%acquire as inp_decode.F:1621-1655 sets it (no FSOBC_REDUCED)"""
    def code(v):
        c = p.lbc[abi.LBS[side]][abi.LBV[v]]
        if c:
            return c
        return {"west": p.lbc_west, "east": p.lbc_east, "south": p.lbc_south, "north": p.lbc_north}[side]
    own = lambda v: code(v) in (abi.LBC["Cla"], abi.LBC["Fla"], abi.LBC["Shc"], abi.LBC["RadNud"])
    fs = lambda v: code(v) in (abi.LBC["Fla"], abi.LBC["Shc"])
    if var == "zeta":
        return own("zeta") or fs("ubar") or fs("vbar")
    return own(var)


def ramp_of(td, time):
    return math.tanh((time / 86400.0 - td.dstart) / 1.0) if td.ramp else 1.0         # set_tides.F:249-253


def harmonics(st, td, time):
    """Etide, Utide, Vtide of set_tides_tile on the tile's extents (zero outside the reference's loop ranges; None for
    the group that is not defined)"""
    b, p = st.b, st.p
    I, J = st.I, st.J
    ramp = ramp_of(td, time)
    masked = bool(p.masking)
    cff = 2.0 * PI * (time - td.tide_start * DAY2SEC)
    Etide = Utide = Vtide = None
    if td.ssh:
        Etide = np.zeros((st.ni, st.nj))
        R = (I(b.IstrR, b.IendR), J(b.JstrR, b.JendR))
        for it in range(td.NTC):
            if td.Tperiod[it] > 0.0:
                omega = cff / td.Tperiod[it]
                Etide[R] = Etide[R] + ramp * td["SSH_Tamp"][R + (it,)] * np.cos(omega - td["SSH_Tphase"][R + (it,)])
                if masked:
                    Etide[R] = Etide[R] * st["rmask"][R]
    if td.uv:
        Utide = np.zeros((st.ni, st.nj))
        Vtide = np.zeros((st.ni, st.nj))
        Uwrk = np.zeros((st.ni, st.nj))
        Vwrk = np.zeros((st.ni, st.nj))
        angler = td.arr.get("angler", np.zeros((st.ni, st.nj)))
        i0, j0 = min(b.IstrR, b.Istr - 1), min(b.JstrR, b.Jstr - 1)
        W = (I(i0, b.IendR), J(j0, b.JendR))
        for it in range(td.NTC):
            if td.Tperiod[it] > 0.0:
                omega = cff / td.Tperiod[it]
                angle = td["UV_Tangle"][W + (it,)] - angler[W]
                Cangle, Sangle = np.cos(angle), np.sin(angle)
                phase = omega - td["UV_Tphase"][W + (it,)]
                Cphase, Sphase = np.cos(phase), np.sin(phase)
                major, minor = td["UV_Tmajor"][W + (it,)], td["UV_Tminor"][W + (it,)]
                Uwrk[W] = major * Cangle * Cphase - minor * Sangle * Sphase
                Vwrk[W] = major * Sangle * Cphase + minor * Cangle * Sphase
                U, Um = (I(b.Istr, b.IendR), J(b.JstrR, b.JendR)), (I(b.Istr - 1, b.IendR - 1), J(b.JstrR, b.JendR))
                Utide[U] = Utide[U] + ramp * 0.5 * (Uwrk[Um] + Uwrk[U])
                if masked:
                    Utide[U] = Utide[U] * st["umask"][U]
                V, Vm = (I(b.IstrR, b.IendR), J(b.Jstr, b.JendR)), (I(b.IstrR, b.IendR), J(b.Jstr - 1, b.JendR - 1))
                Vtide[V] = (Vtide[V] + ramp * 0.5 * (Vwrk[Vm] + Vwrk[V]))
                if masked:
                    Vtide[V] = Vtide[V] * st["vmask"][V]
    return Etide, Utide, Vtide


def edge_on(b, side):
    if side in ("west", "east"):
        return not b.EWperiodic and bool(b.west_edge if side == "west" else b.east_edge)
    return not b.NSperiodic and bool(b.south_edge if side == "south" else b.north_edge)


def set_tides(st, td, time):
    """set_tides_tile: the edge loads (:332-426, :512-638) into st's zeta_bry, ubar_bry, vbar_bry, in place"""
    b, p = st.b, st.p
    I, J = st.I, st.J
    Etide, Utide, Vtide = harmonics(st, td, time)

    def put(name, base, where, val):
        st[name][where] = (td[base][where] + val) if base else val

    zb = "zeta_base" if td.add_fsobc else None
    ub = "ubar_base" if td.add_m2obc else None
    vb = "vbar_base" if td.add_m2obc else None
    if td.ssh:
        # the corner rho-points are left alone: the W / E vectors run over the rows that are not a S / N boundary row
        ja = b.Jstr if (b.south_edge and b.JstrR == b.Jstr - 1) else b.JstrR
        jb = b.Jend if (b.north_edge and b.JendR == b.Jend + 1) else b.JendR
        ia = b.Istr if (b.west_edge and b.IstrR == b.Istr - 1) else b.IstrR
        ib = b.Iend if (b.east_edge and b.IendR == b.Iend + 1) else b.IendR
        for side in SIDES:
            if not (acquire(p, side, "zeta") or acquire(p, side, "ubar") or acquire(p, side, "vbar")) or not edge_on(b, side):
                continue
            if side == "west":
                put("zeta_bry", zb, (I(b.Istr - 1), J(ja, jb)), 0.5 * (Etide[I(b.Istr - 1), J(ja, jb)] + Etide[I(b.Istr), J(ja, jb)]))
            elif side == "east":
                put("zeta_bry", zb, (I(b.Iend + 1), J(ja, jb)), 0.5 * (Etide[I(b.Iend), J(ja, jb)] + Etide[I(b.Iend + 1), J(ja, jb)]))
            elif side == "south":
                put("zeta_bry", zb, (I(ia, ib), J(b.Jstr - 1)), 0.5 * (Etide[I(ia, ib), J(b.Jstr - 1)] + Etide[I(ia, ib), J(b.Jstr)]))
            else:
                put("zeta_bry", zb, (I(ia, ib), J(b.Jend + 1)), 0.5 * (Etide[I(ia, ib), J(b.Jend)] + Etide[I(ia, ib), J(b.Jend + 1)]))
    if td.uv:
        for side in SIDES:
            if not (acquire(p, side, "ubar") and acquire(p, side, "vbar")) or not edge_on(b, side):
                continue
            if side == "west":
                put("ubar_bry", ub, (I(b.Istr), J(b.JstrR, b.JendR)), Utide[I(b.Istr), J(b.JstrR, b.JendR)])
                put("vbar_bry", vb, (I(b.Istr - 1), J(b.Jstr, b.JendR)), Vtide[I(b.Istr - 1), J(b.Jstr, b.JendR)])
            elif side == "east":
                put("ubar_bry", ub, (I(b.Iend + 1), J(b.JstrR, b.JendR)), Utide[I(b.Iend + 1), J(b.JstrR, b.JendR)])
                put("vbar_bry", vb, (I(b.Iend + 1), J(b.Jstr, b.JendR)), Vtide[I(b.Iend + 1), J(b.Jstr, b.JendR)])
            elif side == "south":
                put("ubar_bry", ub, (I(b.Istr, b.IendR), J(b.Jstr - 1)), Utide[I(b.Istr, b.IendR), J(b.Jstr - 1)])
                put("vbar_bry", vb, (I(b.IstrR, b.IendR), J(b.Jstr)), Vtide[I(b.IstrR, b.IendR), J(b.Jstr)])
            else:
                put("ubar_bry", ub, (I(b.Istr, b.IendR), J(b.Jend + 1)), Utide[I(b.Istr, b.IendR), J(b.Jend + 1)])
                put("vbar_bry", vb, (I(b.IstrR, b.IendR), J(b.Jend + 1)), Vtide[I(b.IstrR, b.IendR), J(b.Jend + 1)])
    return st


def written_points(st, td):
    """{name: boolean array}: the points set_tides writes (for the sentinel checks)"""
    probe = st.copy()
    for name in ("zeta_bry", "ubar_bry", "vbar_bry"):
        probe[name][:] = np.nan
    set_tides(probe, td, td.tide_start * DAY2SEC)
    return {name: ~np.isnan(probe[name]) for name in ("zeta_bry", "ubar_bry", "vbar_bry")}


def ssh_only_bry_val(st, know):
    """bry_val of the SSH_TIDES-without-UV_TIDES blocks on the four edges from the state's time level know (1-based):
    (ubar_bry, vbar_bry) copies with the value at the normal velocity points of each edge (Jstr:Jend / Istr:Iend)"""
    b, p = st.b, st.p
    I, J = st.I, st.J
    g = p.g
    zeta, ubar, vbar = st["zeta"][:, :, know - 1], st["ubar"][:, :, know - 1], st["vbar"][:, :, know - 1]
    h, f, zb = st["h"], st["f"], st["zeta_bry"]
    ub, vb = st["ubar_bry"].copy(), st["vbar_bry"].copy()
    Jr, Jp = J(b.Jstr, b.Jend), J(b.Jstr + 1, b.Jend + 1)
    Ir, Ip = I(b.Istr, b.Iend), I(b.Istr + 1, b.Iend + 1)
    pm, pn = st["pm"], st["pn"]
    if edge_on(b, "west"):
        i0, i1, i2 = I(b.Istr - 1), I(b.Istr), I(b.Istr + 1)
        if acquire(p, "west", "zeta"):
            bry_pgr = -g * (zeta[i1, Jr] - zb[i0, Jr]) * 0.5 * pm[i1, Jr]
        else:
            bry_pgr = -g * (zeta[i1, Jr] - zeta[i0, Jr]) * 0.5 * (pm[i0, Jr] + pm[i1, Jr])
        bry_cor = 0.125 * (vbar[i0, Jr] + vbar[i0, Jp] + vbar[i1, Jr] + vbar[i1, Jp]) * (f[i0, Jr] + f[i1, Jr]) if p.uv_cor else 0.0
        cff1 = 1.0 / (0.5 * (h[i0, Jr] + zeta[i0, Jr] + h[i1, Jr] + zeta[i1, Jr]))
        bry_str = cff1 * (st["sustr"][i1, Jr] - st["bustr"][i1, Jr])
        Cx = 1.0 / np.sqrt(g * 0.5 * (h[i0, Jr] + zeta[i0, Jr] + h[i1, Jr] + zeta[i1, Jr]))
        cff2 = st["om_u"][i1, Jr] * Cx
        ub[i1, Jr] = ubar[i2, Jr] + cff2 * (bry_pgr + bry_cor + bry_str)
    if edge_on(b, "east"):
        i0, i1, im = I(b.Iend), I(b.Iend + 1), I(b.Iend)
        if acquire(p, "east", "zeta"):
            bry_pgr = -g * (zb[i1, Jr] - zeta[i0, Jr]) * 0.5 * pm[i0, Jr]
        else:
            bry_pgr = -g * (zeta[i1, Jr] - zeta[i0, Jr]) * 0.5 * (pm[i0, Jr] + pm[i1, Jr])
        bry_cor = 0.125 * (vbar[i0, Jr] + vbar[i0, Jp] + vbar[i1, Jr] + vbar[i1, Jp]) * (f[i0, Jr] + f[i1, Jr]) if p.uv_cor else 0.0
        cff1 = 1.0 / (0.5 * (h[i0, Jr] + zeta[i0, Jr] + h[i1, Jr] + zeta[i1, Jr]))
        bry_str = cff1 * (st["sustr"][i1, Jr] - st["bustr"][i1, Jr])
        Cx = 1.0 / np.sqrt(g * 0.5 * (h[i1, Jr] + zeta[i1, Jr] + h[i0, Jr] + zeta[i0, Jr]))
        cff2 = st["om_u"][i1, Jr] * Cx
        ub[i1, Jr] = ubar[im, Jr] + cff2 * (bry_pgr + bry_cor + bry_str)
    if edge_on(b, "south"):
        j0, j1, j2 = J(b.Jstr - 1), J(b.Jstr), J(b.Jstr + 1)
        if acquire(p, "south", "zeta"):
            bry_pgr = -g * (zeta[Ir, j1] - zb[Ir, j0]) * 0.5 * pn[Ir, j1]
        else:
            bry_pgr = -g * (zeta[Ir, j1] - zeta[Ir, j0]) * 0.5 * (pn[Ir, j0] + pn[Ir, j1])
        bry_cor = -0.125 * (ubar[Ir, j0] + ubar[Ip, j0] + ubar[Ir, j1] + ubar[Ip, j1]) * (f[Ir, j0] + f[Ir, j1]) if p.uv_cor else 0.0
        cff1 = 1.0 / (0.5 * (h[Ir, j0] + zeta[Ir, j0] + h[Ir, j1] + zeta[Ir, j1]))
        bry_str = cff1 * (st["svstr"][Ir, j1] - st["bvstr"][Ir, j1])
        Ce = 1.0 / np.sqrt(g * 0.5 * (h[Ir, j0] + zeta[Ir, j0] + h[Ir, j1] + zeta[Ir, j1]))
        cff2 = st["on_v"][Ir, j1] * Ce
        vb[Ir, j1] = vbar[Ir, j2] + cff2 * (bry_pgr + bry_cor + bry_str)
    if edge_on(b, "north"):
        j0, j1 = J(b.Jend), J(b.Jend + 1)
        if acquire(p, "north", "zeta"):
            bry_pgr = -g * (zb[Ir, j1] - zeta[Ir, j0]) * 0.5 * pn[Ir, j0]
        else:
            bry_pgr = -g * (zeta[Ir, j1] - zeta[Ir, j0]) * 0.5 * (pn[Ir, j0] + pn[Ir, j1])
        bry_cor = -0.125 * (ubar[Ir, j0] + ubar[Ip, j0] + ubar[Ir, j1] + ubar[Ip, j1]) * (f[Ir, j0] + f[Ir, j1]) if p.uv_cor else 0.0
        cff1 = 1.0 / (0.5 * (h[Ir, j0] + zeta[Ir, j0] + h[Ir, j1] + zeta[Ir, j1]))
        bry_str = cff1 * (st["svstr"][Ir, j1] - st["bvstr"][Ir, j1])
        Ce = 1.0 / np.sqrt(g * 0.5 * (h[Ir, j1] + zeta[Ir, j1] + h[Ir, j0] + zeta[Ir, j0]))
        cff2 = st["on_v"][Ir, j1] * Ce
        vb[Ir, j1] = vbar[Ir, j0] + cff2 * (bry_pgr + bry_cor + bry_str)
    return ub, vb


# ------------------------------------------------------------------------------------------- states and sets --
OPEN = {"zeta": "Cha", "ubar": "Fla", "vbar": "Fla", "u": "Rad", "v": "Rad", "t": "Rad"}


def open_all(st, table=OPEN, sides=SIDES):
    st.p = type(st.p).from_buffer_copy(st.p)
    for sd in sides:
        for var, code in table.items():
            st.p.lbc[abi.LBS[sd]][abi.LBV[var]] = abi.LBC[code]
    return st


def exact_set(st, ntc, mtc, uv=True, ssh=True, angler=None, seed=11, **kw):
    """Constituents for which no transcendental differs at time = tide_start: zero phases and UV_Tangle = angler, so every
    cos is 1 and every sin 0.  Amplitudes and semi-axes are seeded random numbers (no two alike), a function of the
    global indices; the second of three periods is zero (skipped)."""
    b = st.b
    rng = np.random.default_rng(seed)
    glob = rng.random((6, mtc, b.Lm + 12, b.Mm + 12))
    ii = (np.arange(b.LBi, b.UBi + 1) + 5) % (b.Lm + 12)
    jj = (np.arange(b.LBj, b.UBj + 1) + 5) % (b.Mm + 12)
    pick = lambda q: np.asfortranarray(np.moveaxis(glob[q][:, ii][:, :, jj], 0, 2))
    T = np.array([44714.0, 0.0, 43200.0, 86164.0, 92950.0][:mtc] + [50000.0] * max(0, mtc - 5))
    if ntc < 2:
        T[1] = 45000.0
    zeros = np.zeros((st.ni, st.nj, mtc), order="F")
    args = {}
    if ssh:
        args.update(SSH_Tamp=0.1 + pick(0), SSH_Tphase=zeros)
    if uv:
        ang = zeros.copy()
        if angler is not None:
            ang[:] = angler[:, :, None]
        args.update(UV_Tangle=ang, UV_Tphase=zeros, UV_Tmajor=0.05 + 0.1 * pick(1), UV_Tminor=0.02 * pick(2) - 0.01)
        if angler is not None:
            args["angler"] = angler
    return tides_mod.Tides(b, T, NTC=ntc, tide_start=kw.pop("tide_start", 3.25), **args, **kw)


def general_set(st, ntc=3, mtc=4, uv=True, ssh=True, angler=None, **kw):
    """ana.analytic_tides made to hold mtc planes"""
    return ana.analytic_tides(st, ntc=ntc, mtc=mtc, ssh=ssh, uv=uv, angler=angler, **kw)


def amp_bound(td):
    """(sum over the constituents of max|amp|, of max|major| + max|minor|)"""
    za = sum(float(np.abs(td["SSH_Tamp"][:, :, it]).max()) for it in range(td.NTC)) if td.ssh else 0.0
    ua = sum(float(np.abs(td["UV_Tmajor"][:, :, it]).max() + np.abs(td["UV_Tminor"][:, :, it]).max())
             for it in range(td.NTC)) if td.uv else 0.0
    return za, ua


class TidalOracle:
    """the CPU oracle as a Main3D backend that takes tides: the restatement writes the boundary arrays before each step"""

    def __init__(self, be):
        self._be = be
        self._td = None

    def __getattr__(self, name):
        return getattr(self._be, name)

    def set_tides(self, td):
        self._td = td

    def tides(self, time):
        set_tides(self._be.st, self._td, time)
