"""The yardstick of the KPP double-diffusive mixing (LMD_DDMIX): a numpy restatement of exactly two things, written from
the Fortran in the operation order of the reference,

    alfaobeta_nonlin   Tcof / Scof of every rho-level, rho_eos.F:436-456 (with the polynomials of :250-420 it needs)
    alfaobeta_lin      the constant of rho_eos.F:782-797
    increment          (nu_ddt, nu_dds) of lmd_vmix.F:371-427 at the interior W-levels, with the regime of every point
                       and the margins of its branches

and the states the GPU tests run (ddmix_state) with the sequence they run (run_device): rho_eos, then lmd_vmix on the
density profiles of the state builder.

Parity status: pinned -- tests/test_ddmix.py compares both with the vectors of tests/golden/ref_ddmix.npz, which
tests/golden/make_golden_ddmix.py takes from the reference's own rho_eos.F / lmd_vmix.F built with LMD_DDMIX."""
import math
import os
import re

import numpy as np

import bkpp_util as bk

LMD_RRHO0, LMD_NUF, LMD_FDD, LMD_NU = 1.9, 10.0e-4, 0.7, 1.5e-6          # mod_scalars.F:1553-1577
LMD_TDD1, LMD_TDD2, LMD_TDD3 = 0.909, 4.6, 0.54
LMD_SDD1, LMD_SDD2, LMD_SDD3 = 0.15, 1.85, 0.85
REGIMES = ("finger", "finger_capped", "conv_lt_half", "conv_ge_half", "none")
FINGER, CAPPED, CONV_LO, CONV_HI, NONE = range(5)

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = {m.group(1): float(m.group(2)) for m in
       re.finditer(r"#define EOS_(\w+)\s+\(([-+0-9.e]+)\)", open(os.path.join(_ROOT, "include", "roms_eoscoef.h")).read())}

interior = bk.interior


def alfaobeta_nonlin(tt, ts, zr):
    """alfaobeta = Tcof / Scof at points of temperature tt, salinity ts and depth zr (negative), rho_eos.F:436-456, from
    den1, bulk and their derivatives (:250-420), every operation in the reference's order"""
    E = EOS
    Tt = np.maximum(-2.0, tt)
    Ts = np.maximum(0.0, ts)
    sqrtTs = np.sqrt(Ts)
    Tp = zr
    C0 = E["Q00"] + Tt * (E["Q01"] + Tt * (E["Q02"] + Tt * (E["Q03"] + Tt * (E["Q04"] + Tt * E["Q05"]))))
    C1 = E["U00"] + Tt * (E["U01"] + Tt * (E["U02"] + Tt * (E["U03"] + Tt * E["U04"])))
    C2 = E["V00"] + Tt * (E["V01"] + Tt * E["V02"])
    den1 = C0 + Ts * (C1 + sqrtTs * C2 + Ts * E["W00"])
    C3 = E["A00"] + Tt * (E["A01"] + Tt * (E["A02"] + Tt * (E["A03"] + Tt * E["A04"])))
    C4 = E["B00"] + Tt * (E["B01"] + Tt * (E["B02"] + Tt * E["B03"]))
    C5 = E["D00"] + Tt * (E["D01"] + Tt * E["D02"])
    C6 = E["E00"] + Tt * (E["E01"] + Tt * (E["E02"] + Tt * E["E03"]))
    C7 = E["F00"] + Tt * (E["F01"] + Tt * E["F02"])
    C8 = E["G01"] + Tt * (E["G02"] + Tt * E["G03"])
    C9 = E["H00"] + Tt * (E["H01"] + Tt * E["H02"])
    bulk0 = C3 + Ts * (C4 + sqrtTs * C5)
    bulk1 = C6 + Ts * (C7 + sqrtTs * E["G00"])
    bulk2 = C8 + Ts * C9
    bulk = bulk0 - Tp * (bulk1 - Tp * bulk2)
    d0 = E["Q01"] + Tt * (2.0 * E["Q02"] + Tt * (3.0 * E["Q03"] + Tt * (4.0 * E["Q04"] + Tt * 5.0 * E["Q05"])))
    d1 = E["U01"] + Tt * (2.0 * E["U02"] + Tt * (3.0 * E["U03"] + Tt * 4.0 * E["U04"]))
    d2 = E["V01"] + Tt * 2.0 * E["V02"]
    Dden1DS = C1 + 1.5 * C2 * sqrtTs + 2.0 * E["W00"] * Ts
    Dden1DT = d0 + Ts * (d1 + sqrtTs * d2)
    d3 = E["A01"] + Tt * (2.0 * E["A02"] + Tt * (3.0 * E["A03"] + Tt * 4.0 * E["A04"]))
    d4 = E["B01"] + Tt * (2.0 * E["B02"] + Tt * 3.0 * E["B03"])
    d5 = E["D01"] + Tt * 2.0 * E["D02"]
    d6 = E["E01"] + Tt * (2.0 * E["E02"] + Tt * 3.0 * E["E03"])
    d7 = E["F01"] + Tt * 2.0 * E["F02"]
    d8 = E["G02"] + Tt * 2.0 * E["G03"]
    d9 = E["H01"] + Tt * 2.0 * E["H02"]
    DbulkDS = C4 + sqrtTs * 1.5 * C5 - Tp * (C7 + sqrtTs * 1.5 * E["G00"] - Tp * C9)
    DbulkDT = d3 + Ts * (d4 + sqrtTs * d5) - Tp * (d6 + Ts * d7 - Tp * (d8 + Ts * d9))
    Tpr10 = 0.1 * zr                                                                                       # :436-452
    cff = bulk + Tpr10
    cff1 = Tpr10 * den1
    cff2 = bulk * cff
    Tcof = -(DbulkDT * cff1 + Dden1DT * cff2)
    Scof = DbulkDS * cff1 + Dden1DS * cff2
    return Tcof / Scof


def alfaobeta_lin(Tcoef, Scoef):
    """rho_eos.F:782-797: cff * Tcoef with cff = 1 / Scoef, or 1 where Scoef is zero"""
    cff = 1.0 if Scoef == 0.0 else 1.0 / Scoef
    return cff * Tcoef


def alfaobeta(st, nrhs=1):
    """alfaobeta (.., 0:N) on the tile's extents as rho_eos leaves it: the value of rho-level k at index k, level 0 not
    written (zero, as mod_mixing.F leaves it)"""
    out = np.zeros(st["z_w"].shape, order="F")
    if st.p.nonlin_eos:
        out[:, :, 1:] = alfaobeta_nonlin(st["t"][:, :, :, nrhs - 1, 0], st["t"][:, :, :, nrhs - 1, 1], st["z_r"])
    else:
        out[:, :, 1:] = alfaobeta_lin(st.p.Tcoef, st.p.Scoef)
    return out


def increment(tA, tB, sA, sB, aob):
    """lmd_vmix.F:371-427 at W-points between the rho-levels A (below, whose alfaobeta is aob) and B (above).  Returns
    (nu_ddt, nu_dds, regime, info): regime = index into REGIMES; info = dict(Rrho, ddDS: as the branches see them, raw_ddDS:
    before the floor, margin: the smallest of |Rrho - 1|, |Rrho - 0.5|, |Rrho - lmd_Rrho0|, |Rrho|)"""
    ddDT = tB - tA
    raw = sB - sA
    ddDS = np.copysign(1.0, raw) * np.maximum(np.abs(raw), 1.0e-14)
    Rrho = aob * ddDT / ddDS
    finger = (Rrho > 1.0) & (ddDS > 0.0)
    conv = ~finger & (0.0 < Rrho) & (Rrho < 1.0) & (ddDS < 0.0)
    Rf = np.minimum(Rrho, LMD_RRHO0)
    r = (Rf - 1.0) / (LMD_RRHO0 - 1.0)
    nf = 1.0 - r * r
    nf = LMD_NUF * nf * nf * nf
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        Rc = np.where(conv, Rrho, 0.5)
        ct = LMD_NU * LMD_TDD1 * np.exp(LMD_TDD2 * np.exp(-LMD_TDD3 * ((1.0 / Rc) - 1.0)))
        cs = np.where(Rc < 0.5, ct * LMD_SDD1 * Rc, ct * (LMD_SDD2 * Rc - LMD_SDD3))
    nu_dds = np.where(finger, nf, np.where(conv, cs, 0.0))
    nu_ddt = np.where(finger, LMD_FDD * nf, np.where(conv, ct, 0.0))
    regime = np.where(finger, np.where(Rrho < LMD_RRHO0, FINGER, CAPPED),
                      np.where(conv, np.where(Rrho < 0.5, CONV_LO, CONV_HI), NONE)).astype(np.int8)
    margin = np.minimum(np.minimum(np.abs(Rrho - 1.0), np.abs(Rrho - 0.5)), np.minimum(np.abs(Rrho - LMD_RRHO0), np.abs(Rrho)))
    return nu_ddt, nu_dds, regime, dict(Rrho=Rrho, ddDS=ddDS, raw_ddDS=raw, margin=margin)


def state_increment(st, aob=None, nstp=1):
    """increment at the W-levels 1 .. N-1 of the tile (arrays (ni, nj, N-1)) from t(nstp) and alfaobeta (default: the
    restatement's)"""
    aob = alfaobeta(st) if aob is None else aob
    T, S = st["t"][:, :, :, nstp - 1, 0], st["t"][:, :, :, nstp - 1, 1]
    return increment(T[:, :, :-1], T[:, :, 1:], S[:, :, :-1], S[:, :, 1:], aob[:, :, 1:-1])


# ------------------------------------------------------------------------------------------------ the states --
GRIDS = {g: bk.GRIDS[g] for g in ("TINY", "PARTIAL", "N32", "N33")}
CASES = [(g, m) for g in GRIDS for m in (None, "island")]
ZERO_DS = ((5, 2, 1), (9, 3, 2), (14, 4, 1), (20, 2, 2))      # (i, j, W-level k) with ddDS == 0 exactly: the SIGN / 1e-14 floor
DS = 0.1                                                       # |ddDS| of every other point


def case_id(case):
    return f"{case[0]}-{'mask' if case[1] else 'nomask'}"


def ddmix_state(grid="TINY", mask=None):
    """bkpp_util.bkpp_state (channel, stable) with temperature and salinity of t(nstp = nrhs = 1) shaped so that every
    regime of lmd_vmix.F:371-419 occurs at a fifth of the W-points, in every column and at every depth: built upwards
    from level 1 (5 degrees, 34 psu), the salinity step of W-level k is +-DS and the temperature step follows from the
    density ratio wanted there and alfaobeta of the level below.  regime = (i + 2 j + k) mod 5; within a regime the
    ratio varies with the point (u in [0, 1), a fixed irrational rotation):
        fingering        Rrho = 1.05 + 0.8 u    ddDS > 0         capped     Rrho = 2.0 + u    ddDS > 0
        convection < .5  Rrho = 0.05 + 0.4 u    ddDS < 0         >= .5      Rrho = 0.55 + 0.4 u    ddDS < 0
        none             Rrho = -(0.2 + 2 u) with either sign of ddDS, or a ratio of the other regimes' ranges with the
                         sign of ddDS that rules them out
    and at the points of ZERO_DS ddDS = 0 exactly.  The density profiles lmd_vmix reads stay the builder's (run_device
    says how).  Returns (state, hbbl of the previous step)."""
    st, hprev = bk.bkpp_state(grid, mask, False, False)
    shape_ts(st)
    return st, hprev


def shape_ts(st):
    """the temperature and salinity of ddmix_state, written into t(:,:,:,1,:) of any tile: functions of the global
    indices and of the column's own z_r, the same on every tiling"""
    b, N = st.b, st.b.N
    ii = np.arange(b.LBi, b.UBi + 1)[:, None] * np.ones((1, st.nj), dtype=int)
    jj = np.arange(b.LBj, b.UBj + 1)[None, :] * np.ones((st.ni, 1), dtype=int)
    ii = np.mod(ii - 1, b.Lm) + 1                      # periodic in i: the ghost columns are images
    T, S = st["t"][:, :, :, 0, 0], st["t"][:, :, :, 0, 1]
    T[:, :, 0] = 5.0 + 0.01 * np.mod(ii + jj, 7)
    S[:, :, 0] = 34.0 + 0.01 * np.mod(ii, 5)
    for k in range(1, N):
        reg = np.mod(ii + 2 * jj + k, 5)
        u = np.mod(0.6180339887 * ii + 0.7548776662 * jj + 0.5698402910 * k, 1.0)
        var = np.mod(ii + jj + k, 4)
        R = np.select([reg == FINGER, reg == CAPPED, reg == CONV_LO, reg == CONV_HI],
                      [1.05 + 0.8 * u, 2.0 + u, 0.05 + 0.4 * u, 0.55 + 0.4 * u],
                      np.select([var == 0, var == 1, var == 2], [-(0.2 + 2.0 * u), -(0.2 + 2.0 * u), 1.2 + u], 0.2 + 0.7 * u))
        sgn = np.select([reg <= CAPPED, reg <= CONV_HI], [1.0, -1.0],
                        np.select([var == 0, var == 1, var == 2], [1.0, -1.0, -1.0], 1.0))
        dS = sgn * DS
        aob = alfaobeta_nonlin(T[:, :, k - 1], S[:, :, k - 1], st["z_r"][:, :, k - 1])
        dT = R * dS / aob
        for (i0, j0, k0) in ZERO_DS:
            if k0 == k and i0 <= b.Lm and j0 <= b.Mm:
                m = (ii == i0) & (jj == j0)
                dS = np.where(m, 0.0, dS)
                dT = np.where(m, np.where(np.mod(i0, 2) == 0, 0.3, -0.3), dT)
        T[:, :, k] = T[:, :, k - 1] + dT
        S[:, :, k] = S[:, :, k - 1] + dS
    assert T.min() > -2.0 and T.max() < 40.0 and S.min() > 0.0 and S.max() < 42.0, (T.min(), T.max(), S.min(), S.max())


RHO_EOS_OUT = ("rho", "pden", "bvf", "alpha", "beta", "rhoA", "rhoS")
OUT = ("Akv", "Akt", "ghats", "hsbl")


def run_device(be, sh, st0, S, ddmix, bkpp=False, hprev=None):
    """The sequence every GPU case runs in the context `be` of the state sh (a copy of st0): the switches, rho_eos, then
    the builder's own density profiles, expansion coefficients and KPP inputs back on the device (rho_eos has just
    overwritten the former with those of the shaped t, and an earlier run the latter), then lmd_vmix.  Returns
    dict(Akv, Akt, ghats, hsbl[, alfaobeta][, hbbl, kbbl, ksbl], eos: the outputs of rho_eos)."""
    be.set_ddmix(bool(ddmix))
    be.set_kpp(bool(bkpp), hprev if bkpp else None)
    for name in OUT:
        sh[name][...] = st0[name]
    be.to_device(list(OUT))
    be.call("rho_eos", S)
    be.to_host(list(RHO_EOS_OUT))
    out = {"eos": {n: sh[n].copy() for n in RHO_EOS_OUT}}
    for name in RHO_EOS_OUT:
        sh[name][...] = st0[name]
    be.to_device(list(RHO_EOS_OUT))
    be.call("lmd_vmix", S)
    be.to_host(list(OUT))
    out.update({n: sh[n].copy() for n in OUT})
    if ddmix:
        out["alfaobeta"] = be.get_kpp("alfaobeta")
    if bkpp:
        out.update({n: be.get_kpp(n) for n in ("hbbl", "kbbl", "ksbl")})
    return out
