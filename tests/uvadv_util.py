"""numpy mirror of rhs3d_tile (ROMS/Nonlinear/rhs3d.F:465-1666) for the momentum advection schemes of
roms_params_t.uv_adv, written from the Fortran: Coriolis (:467-507), curvilinear terms (:509-564), horizontal advection
UV_C2ADVECTION (:605-656) / UV_C4ADVECTION / third-order upstream (:658-941) with the edge copies of the second
differences, vertical advection UV_SADVECTION / UV_C2ADVECTION / UV_C4ADVECTION / default (:1016-1505) and the vertical
integral rufrc, rvfrc (:1534-1666); and the C2 advection term of the 2-D step (step2d_LF_AM3.h:1026-1076).  Operation
for operation in the reference's order, so that a result is comparable bit for bit.  Every work array has the extents
of the state's arrays; a shifted array wraps around at the array's ends, which only reaches points no used range holds.
tests/test_uvadv.py pins the default pair against the oracle."""
import numpy as np

GADV = -0.25


def sh(A, di=0, dj=0):
    """B(i, j) = A(i + di, j + dj)"""
    return np.roll(A, (-di, -dj), axis=(0, 1))


def _edges(b):
    return (bool(b.west_edge and not b.EWperiodic), bool(b.east_edge and not b.EWperiodic),
            bool(b.south_edge and not b.NSperiodic), bool(b.north_edge and not b.NSperiodic))


def horizontal_fluxes(st, u, v, Huon, Hvom, hadv):
    """UFx, UFe, VFx, VFe of one level (2-D arrays), rhs3d.F:605-941"""
    b = st.b
    I, J = st.I, st.J
    if hadv == "C2":
        UFx = 0.25 * (u + sh(u, 1, 0)) * (Huon + sh(Huon, 1, 0))
        UFe = 0.25 * (sh(u, 0, -1) + u) * (sh(Hvom, -1, 0) + Hvom)
        VFx = 0.25 * (sh(v, -1, 0) + v) * (sh(Huon, 0, -1) + Huon)
        VFe = 0.25 * (v + sh(v, 0, 1)) * (Hvom + sh(Hvom, 0, 1))
        return UFx, UFe, VFx, VFe
    west, east, south, north = _edges(b)
    c4 = hadv == "C4"
    cff = 1.0 / 6.0
    uxx = sh(u, -1, 0) - 2.0 * u + sh(u, 1, 0)
    Huxx = sh(Huon, -1, 0) - 2.0 * Huon + sh(Huon, 1, 0)
    for A in (uxx, Huxx):
        if west:
            A[I(b.Istr)] = A[I(b.Istr + 1)]
        if east:
            A[I(b.Iend + 1)] = A[I(b.Iend)]
    if c4:
        UFx = 0.25 * (u + sh(u, 1, 0) - cff * (uxx + sh(uxx, 1, 0))) * \
              (Huon + sh(Huon, 1, 0) - cff * (Huxx + sh(Huxx, 1, 0)))
    else:
        cff1 = u + sh(u, 1, 0)
        c = np.where(cff1 > 0.0, uxx, sh(uxx, 1, 0))
        UFx = 0.25 * (cff1 + GADV * c) * (Huon + sh(Huon, 1, 0) + GADV * 0.5 * (Huxx + sh(Huxx, 1, 0)))
    uee = sh(u, 0, -1) - 2.0 * u + sh(u, 0, 1)
    if south:
        uee[:, J(b.Jstr - 1)] = uee[:, J(b.Jstr)]
    if north:
        uee[:, J(b.Jend + 1)] = uee[:, J(b.Jend)]
    Hvxx = sh(Hvom, -1, 0) - 2.0 * Hvom + sh(Hvom, 1, 0)
    if c4:
        UFe = 0.25 * (u + sh(u, 0, -1) - cff * (uee + sh(uee, 0, -1))) * \
              (Hvom + sh(Hvom, -1, 0) - cff * (Hvxx + sh(Hvxx, -1, 0)))
    else:
        cff1 = u + sh(u, 0, -1)
        cff2 = Hvom + sh(Hvom, -1, 0)
        c = np.where(cff2 > 0.0, sh(uee, 0, -1), uee)
        UFe = 0.25 * (cff1 + GADV * c) * (cff2 + GADV * 0.5 * (Hvxx + sh(Hvxx, -1, 0)))
    vxx = sh(v, -1, 0) - 2.0 * v + sh(v, 1, 0)
    if west:
        vxx[I(b.Istr - 1)] = vxx[I(b.Istr)]
    if east:
        vxx[I(b.Iend + 1)] = vxx[I(b.Iend)]
    Huee = sh(Huon, 0, -1) - 2.0 * Huon + sh(Huon, 0, 1)
    if c4:
        VFx = 0.25 * (v + sh(v, -1, 0) - cff * (vxx + sh(vxx, -1, 0))) * \
              (Huon + sh(Huon, 0, -1) - cff * (Huee + sh(Huee, 0, -1)))
    else:
        cff1 = v + sh(v, -1, 0)
        cff2 = Huon + sh(Huon, 0, -1)
        c = np.where(cff2 > 0.0, sh(vxx, -1, 0), vxx)
        VFx = 0.25 * (cff1 + GADV * c) * (cff2 + GADV * 0.5 * (Huee + sh(Huee, 0, -1)))
    vee = sh(v, 0, -1) - 2.0 * v + sh(v, 0, 1)
    Hvee = sh(Hvom, 0, -1) - 2.0 * Hvom + sh(Hvom, 0, 1)
    for A in (vee, Hvee):
        if south:
            A[:, J(b.Jstr)] = A[:, J(b.Jstr + 1)]
        if north:
            A[:, J(b.Jend + 1)] = A[:, J(b.Jend)]
    if c4:
        VFe = 0.25 * (v + sh(v, 0, 1) - cff * (vee + sh(vee, 0, 1))) * \
              (Hvom + sh(Hvom, 0, 1) - cff * (Hvee + sh(Hvee, 0, 1)))
    else:
        cff1 = v + sh(v, 0, 1)
        c = np.where(cff1 > 0.0, vee, sh(vee, 0, 1))
        VFe = 0.25 * (cff1 + GADV * c) * (Hvom + sh(Hvom, 0, 1) + GADV * 0.5 * (Hvee + sh(Hvee, 0, 1)))
    return UFx, UFe, VFx, VFe


def vertical_flux(q, W, Hz, di, dj, vadv):
    """FC(:, :, 0:N) of the column variable q(:, :, 1:N) staggered by (di, dj) = (1, 0) for u, (0, 1) for v:
    rhs3d.F:1016-1256 / :1267-1505"""
    N = q.shape[2]
    FC = np.zeros(q.shape[:2] + (N + 1,))
    Q = lambda k: q[:, :, k - 1]
    Ws = lambda k, d: sh(W[:, :, k], d * di, d * dj)
    if vadv == "SPLINES":
        cff1, cff2 = 9.0 / 16.0, 1.0 / 16.0
        Hs = lambda k, d: sh(Hz[:, :, k - 1], d * di, d * dj)
        DC = [None] + [cff1 * (Hs(k, 0) + Hs(k, -1)) - cff2 * (Hs(k, 1) + Hs(k, -2)) for k in range(1, N + 1)]
        CF = np.zeros_like(FC)
        with np.errstate(divide="ignore", invalid="ignore"):     # Hz = 0 on padding points no used range holds
            for k in range(1, N):
                cff = 1.0 / (2.0 * DC[k + 1] + DC[k] * (2.0 - FC[:, :, k - 1]))
                FC[:, :, k] = cff * DC[k + 1]
                CF[:, :, k] = cff * (6.0 * (Q(k + 1) - Q(k)) - DC[k] * CF[:, :, k - 1])
        CF[:, :, N] = 0.0
        for k in range(N - 1, 0, -1):
            CF[:, :, k] = CF[:, :, k] - FC[:, :, k] * CF[:, :, k + 1]
        cff3, cff4 = 1.0 / 3.0, 1.0 / 6.0
        for k in range(1, N):
            FC[:, :, k] = (cff1 * (Ws(k, 0) + Ws(k, -1)) - cff2 * (Ws(k, 1) + Ws(k, -2))) * \
                          (Q(k) + DC[k] * (cff3 * CF[:, :, k] + cff4 * CF[:, :, k - 1]))
        FC[:, :, N] = 0.0
        FC[:, :, 0] = 0.0
    elif vadv == "C2":
        for k in range(1, N):
            FC[:, :, k] = 0.25 * (Q(k) + Q(k + 1)) * (Ws(k, 0) + Ws(k, -1))
    else:
        if vadv == "C4":
            cff1, cff2 = 9.0 / 32.0, 1.0 / 32.0
            Wk = lambda k: Ws(k, 0) + Ws(k, -1)
        else:
            assert vadv == "C4W"
            cff1, cff2 = 9.0 / 16.0, 1.0 / 16.0
            Wk = lambda k: cff1 * (Ws(k, 0) + Ws(k, -1)) - cff2 * (Ws(k, 1) + Ws(k, -2))
        for k in range(2, N - 1):
            FC[:, :, k] = (cff1 * (Q(k) + Q(k + 1)) - cff2 * (Q(k - 1) + Q(k + 2))) * Wk(k)
        FC[:, :, N - 1] = (cff1 * (Q(N - 1) + Q(N)) - cff2 * (Q(N - 2) + Q(N))) * Wk(N - 1)
        FC[:, :, 1] = (cff1 * (Q(1) + Q(2)) - cff2 * (Q(1) + Q(3))) * Wk(1)
    return FC


def rhs3d_tile(st, s, hadv="U3", vadv="C4W", vertical=True):
    """ru, rv(nrhs) (0:N) and rufrc, rvfrc after rhs3d_tile, valid on the ranges the routine writes (IstrU:Iend,
    Jstr:Jend and Istr:Iend, JstrV:Jend); with FCu, FCv the vertical fluxes.  vertical = False leaves the vertical
    advection out (the k-sums then hold the other terms alone).  No climatology, no body force."""
    b, p = st.b, st.p
    N, n = b.N, s.nrhs - 1
    u, v = st["u"][:, :, :, n], st["v"][:, :, :, n]
    Huon, Hvom, Hz, W = st["Huon"], st["Hvom"], st["Hz"], st["W"]
    ru, rv = st["ru"][:, :, :, n].copy(), st["rv"][:, :, :, n].copy()
    for k in range(1, N + 1):
        uk, vk, Hzk = u[:, :, k - 1], v[:, :, k - 1], Hz[:, :, k - 1]
        if p.uv_cor:
            cff = 0.5 * Hzk * st["fomn"]
            UFx = cff * (vk + sh(vk, 0, 1))
            VFe = cff * (uk + sh(uk, 1, 0))
            ru[:, :, k] = ru[:, :, k] + 0.5 * (UFx + sh(UFx, -1, 0))
            rv[:, :, k] = rv[:, :, k] - 0.5 * (VFe + sh(VFe, 0, -1))
        if p.curvgrid and p.uv_adv:
            cff1 = 0.5 * (vk + sh(vk, 0, 1))
            cff2 = 0.5 * (uk + sh(uk, 1, 0))
            cff3 = cff1 * st["dndx"]
            cff4 = cff2 * st["dmde"]
            cff = Hzk * (cff3 - cff4)
            UFx = cff * cff1
            VFe = cff * cff2
            ru[:, :, k] = ru[:, :, k] + 0.5 * (UFx + sh(UFx, -1, 0))
            rv[:, :, k] = rv[:, :, k] - 0.5 * (VFe + sh(VFe, 0, -1))
        if p.uv_adv:
            UFx, UFe, VFx, VFe = horizontal_fluxes(st, uk, vk, Huon[:, :, k - 1], Hvom[:, :, k - 1], hadv)
            ru[:, :, k] = ru[:, :, k] - ((UFx - sh(UFx, -1, 0)) + (sh(UFe, 0, 1) - UFe))
            rv[:, :, k] = rv[:, :, k] - ((sh(VFx, 1, 0) - VFx) + (VFe - sh(VFe, 0, -1)))
    FCu = vertical_flux(u, W, Hz, 1, 0, vadv) if p.uv_adv else np.zeros_like(ru)
    FCv = vertical_flux(v, W, Hz, 0, 1, vadv) if p.uv_adv else np.zeros_like(rv)
    ru_h, rv_h = ru.copy(), rv.copy()
    if vertical and p.uv_adv:
        for k in range(1, N + 1):
            ru[:, :, k] = ru[:, :, k] - (FCu[:, :, k] - FCu[:, :, k - 1])
            rv[:, :, k] = rv[:, :, k] - (FCv[:, :, k] - FCv[:, :, k - 1])
    out = dict(ru=ru, rv=rv, ru_h=ru_h, rv_h=rv_h, FCu=FCu, FCv=FCv)
    for r, frc, om, on, ss, bs in ((ru, "rufrc", "om_u", "on_u", "sustr", "bustr"), (rv, "rvfrc", "om_v", "on_v", "svstr", "bvstr")):
        f = r[:, :, 1].copy()
        for k in range(2, N + 1):
            f = f + r[:, :, k]
        cff = st[om] * st[on]
        cff1 = st[ss] * cff
        cff2 = -st[bs] * cff
        out[frc] = f + cff1 + cff2
    return out


def ranges(st):
    """the index ranges rhs3d_tile writes: ((I, J) of ru / rufrc, (I, J) of rv / rvfrc)"""
    b = st.b
    return (st.I(b.IstrU, b.Iend), st.J(b.Jstr, b.Jend)), (st.I(b.Istr, b.Iend), st.J(b.JstrV, b.Jend))


def step2d_advection(st, krhs, DUon, DVom, c2):
    """the horizontal advection of the 2-D step, step2d_LF_AM3.h:1026-1283: (cff1 + cff2) of the ubar and of the vbar
    equation -- what the step subtracts from rhs_ubar, rhs_vbar -- in the C2 form (:1026-1076) or the default
    fourth-order form (:1077-1256)."""
    b = st.b
    I, J = st.I, st.J
    ub, vb = st["ubar"][:, :, krhs - 1], st["vbar"][:, :, krhs - 1]
    if c2:
        UFx = 0.25 * (DUon + sh(DUon, 1, 0)) * (ub + sh(ub, 1, 0))
        UFe = 0.25 * (DVom + sh(DVom, -1, 0)) * (ub + sh(ub, 0, -1))
        VFx = 0.25 * (DUon + sh(DUon, 0, -1)) * (vb + sh(vb, -1, 0))
        VFe = 0.25 * (DVom + sh(DVom, 0, 1)) * (vb + sh(vb, 0, 1))
    else:
        west, east, south, north = _edges(b)
        cff = 1.0 / 6.0
        d2i = lambda A: sh(A, -1, 0) - 2.0 * A + sh(A, 1, 0)
        d2j = lambda A: sh(A, 0, -1) - 2.0 * A + sh(A, 0, 1)
        grad, Dgrad = d2i(ub), d2i(DUon)
        for A in (grad, Dgrad):
            if west:
                A[I(b.Istr)] = A[I(b.Istr + 1)]
            if east:
                A[I(b.Iend + 1)] = A[I(b.Iend)]
        UFx = 0.25 * (ub + sh(ub, 1, 0) - cff * (grad + sh(grad, 1, 0))) * (DUon + sh(DUon, 1, 0) - cff * (Dgrad + sh(Dgrad, 1, 0)))
        grad = d2j(ub)
        if south:
            grad[:, J(b.Jstr - 1)] = grad[:, J(b.Jstr)]
        if north:
            grad[:, J(b.Jend + 1)] = grad[:, J(b.Jend)]
        Dgrad = d2i(DVom)
        UFe = 0.25 * (ub + sh(ub, 0, -1) - cff * (grad + sh(grad, 0, -1))) * (DVom + sh(DVom, -1, 0) - cff * (Dgrad + sh(Dgrad, -1, 0)))
        grad = d2i(vb)
        if west:
            grad[I(b.Istr - 1)] = grad[I(b.Istr)]
        if east:
            grad[I(b.Iend + 1)] = grad[I(b.Iend)]
        Dgrad = d2j(DUon)
        VFx = 0.25 * (vb + sh(vb, -1, 0) - cff * (grad + sh(grad, -1, 0))) * (DUon + sh(DUon, 0, -1) - cff * (Dgrad + sh(Dgrad, 0, -1)))
        grad, Dgrad = d2j(vb), d2j(DVom)
        for A in (grad, Dgrad):
            if south:
                A[:, J(b.Jstr)] = A[:, J(b.Jstr + 1)]
            if north:
                A[:, J(b.Jend + 1)] = A[:, J(b.Jend)]
        VFe = 0.25 * (vb + sh(vb, 0, 1) - cff * (grad + sh(grad, 0, 1))) * (DVom + sh(DVom, 0, 1) - cff * (Dgrad + sh(Dgrad, 0, 1)))
    adv_u = (UFx - sh(UFx, -1, 0)) + (sh(UFe, 0, 1) - UFe)
    adv_v = (sh(VFx, 1, 0) - VFx) + (VFe - sh(VFe, 0, -1))
    return adv_u, adv_v


def zero_pressure_gradient(st, seed=9):
    """The set-up in which a step2d call shows its advection term alone: g = 0 (the pressure gradient is an exact zero),
    no Coriolis, no viscosity, rufrc = rvfrc = 0, so that rhs_ubar = 0 - (cff1 + cff2) of step2d_LF_AM3.h:1257-1283 (plus,
    with CURVGRID, the curvilinear term of :1333-1382) for a
    call that is not the first predictor; random ubar, vbar, zeta, rubar, rvbar at every level.  On an E-W periodic
    grid the ghost columns hold the periodic images, as the exchange leaves them.  Changes st in place (a private copy
    of its parameters)."""
    st.p = type(st.p).from_buffer_copy(st.p)
    st.p.g, st.p.uv_cor, st.p.uv_vis2 = 0.0, 0, 0
    assert not st.p.masking and not st.p.uv_vis4
    rng = np.random.default_rng(seed)
    for name, amp in (("ubar", 0.2), ("vbar", 0.2), ("zeta", 0.3), ("rubar", 50.0), ("rvbar", 50.0), ("rzeta", 1.0)):
        st[name][:] = amp * rng.standard_normal(st[name].shape)
    st["rufrc"][:] = 0.0
    st["rvfrc"][:] = 0.0
    b = st.b
    if b.EWperiodic:
        for name in ("ubar", "vbar", "zeta", "rubar", "rvbar", "rzeta"):
            for i in range(b.LBi, b.UBi + 1):
                if i < 1 or i > b.Lm:
                    st[name][st.I(i)] = st[name][st.I((i - 1) % b.Lm + 1)]
    return st


def step2d_expected(st, s, zeta_knew, c2):
    """What a step2d call (iif > 1) leaves on a zero_pressure_gradient() state, from the mirror's advection term:
    rhs_ubar, rhs_vbar (the predictor stores them in rubar, rvbar(krhs)) and ubar, vbar(knew) of the leap-frog
    predictor (step2d_LF_AM3.h:2163-2205) or the Adams-Moulton corrector (:2206-2255).  zeta_knew: zeta(knew) of the
    call, which holds zeta_new (:770-868 are not mirrored here).  Valid on the ranges of ranges()."""
    assert s.iif > 1
    p = st.p
    D = st["zeta"][:, :, s.krhs - 1] + st["h"]                                   # Drhs, :509-544
    DUon = st["ubar"][:, :, s.krhs - 1] * ((0.5 * st["on_u"]) * (D + sh(D, -1, 0)))
    DVom = st["vbar"][:, :, s.krhs - 1] * ((0.5 * st["om_v"]) * (D + sh(D, 0, -1)))
    adv_u, adv_v = step2d_advection(st, s.krhs, DUon, DVom, c2)
    rhs = {"u": 0.0 - adv_u, "v": 0.0 - adv_v}
    if p.curvgrid and p.uv_adv:                                                  # curvilinear terms, :1333-1382
        ub, vb = st["ubar"][:, :, s.krhs - 1], st["vbar"][:, :, s.krhs - 1]
        cff1 = 0.5 * (vb + sh(vb, 0, 1))
        cff2 = 0.5 * (ub + sh(ub, 1, 0))
        cff = D * (cff1 * st["dndx"] - cff2 * st["dmde"])
        UFx, VFe = cff * cff1, cff * cff2
        rhs["u"] = rhs["u"] + 0.5 * (UFx + sh(UFx, -1, 0))
        rhs["v"] = rhs["v"] - 0.5 * (VFe + sh(VFe, 0, -1))
    Dnew = zeta_knew + st["h"]
    Dstp = st["zeta"][:, :, s.kstp - 1] + st["h"]
    ptsk = 3 - s.kstp
    pm, pn = st["pm"], st["pn"]
    out = {}
    for c, bar, rbar, di, dj in (("u", "ubar", "rubar", -1, 0), ("v", "vbar", "rvbar", 0, -1)):
        cff = (pm + sh(pm, di, dj)) * (pn + sh(pn, di, dj))
        fac = 1.0 / (Dnew + sh(Dnew, di, dj))
        old = st[bar][:, :, s.kstp - 1] * (Dstp + sh(Dstp, di, dj))
        if s.predictor_2d_step:
            cff1 = p.dtfast
            new = (old + cff * cff1 * rhs[c]) * fac
        else:
            cff1 = 0.5 * p.dtfast * 5.0 / 12.0
            cff2 = 0.5 * p.dtfast * 8.0 / 12.0
            cff3 = 0.5 * p.dtfast * 1.0 / 12.0
            new = (old + cff * (cff1 * rhs[c] + cff2 * st[rbar][:, :, s.kstp - 1] - cff3 * st[rbar][:, :, ptsk - 1])) * fac
        out["rhs_" + bar] = rhs[c]
        out[bar] = new
    return out
