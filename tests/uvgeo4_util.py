"""The horizontal viscosity rotated to geopotential surfaces (MIX_GEO_UV) restated in numpy, statement for statement
and in the reference's order: uv3dmix2_geo_tile (ROMS/Nonlinear/uv3dmix2_geo.h:116-756) and uv3dmix4_geo_tile
(uv3dmix4_geo.h:262-1478; default branch: no VISC_3DCOEF, UV_U3ADV_SPLIT, DIAGNOSTICS_UV; MASKING and WET_DRY by the
parameters).  A yardstick of tests/test_uvgeo4.py (no GPU) and tests/test_gpu_uvgeo4.py, kept as a second statement
independent of the C oracle's (oracle/oracle_uvmix_geo.c): both are pinned bit for bit to the reference built with
MIX_GEO_UV and UV_VIS4 (oracle/_ref/*_GEOUV4, tests/test_ref_pinning.py; tests/golden/ref_geouv4.npz).

One level body -- the slopes, the six gradients, the four horizontal and the four vertical fluxes, on the ranges it is
given -- serves the harmonic operator and both passes of the biharmonic one.  Its parameters are the velocity arrays,
the coefficient pair, whether Hz is inside the horizontal fluxes, and what is done with the fluxes of a level (`finish`).
Every statement is an elementwise operation on the index ranges the reference loops over, so the bits are those of the
scalar loops; the harmonic form is pinned to the oracle's uv3dmix2_geo (itself pinned to four reference builds) and the
biharmonic one to the oracle's uv3dmix4_geo in tests/test_uvgeo4.py."""
import numpy as np

from roms_trunk_mgh_amd import abi


def _sh(r, di=0, dj=0):
    return (slice(r[0].start + di, r[0].stop + di), slice(r[1].start + dj, r[1].stop + dj))


def _min0(a):
    return np.where(a < 0.0, a, 0.0)          # MIN(a, 0.0_r8)


def _max0(a):
    return np.where(a > 0.0, a, 0.0)          # MAX(a, 0.0_r8)


def tile_ranges(b):
    """the loop ranges of uv3dmix2_geo.h and of K_LOOP2 of uv3dmix4_geo.h: (i from, i to, j from, j to)"""
    return {"U": (b.IstrU - 1, b.Iend + 1, b.Jstr - 1, b.Jend + 1),       # slopes at u-faces, dUdz
            "V": (b.Istr - 1, b.Iend + 1, b.JstrV - 1, b.Jend + 1),       # slopes at v-faces, dVdz
            "P": (b.Istr, b.Iend + 1, b.Jstr, b.Jend + 1),                # psi-points
            "R": (b.IstrU - 1, b.Iend, b.JstrV - 1, b.Jend),              # rho-points
            "OU": (b.IstrU, b.Iend, b.Jstr, b.Jend),                      # the u-points of the result
            "OV": (b.Istr, b.Iend, b.JstrV, b.Jend)}


def first_ranges(b):
    """the loop ranges of K_LOOP1 of uv3dmix4_geo.h (:330-799)"""
    return {"U": (b.IstrUm2, b.Iendp2, b.Jstrm2, b.Jendp2),
            "V": (b.Istrm2, b.Iendp2, b.JstrVm2, b.Jendp2),
            "P": (b.Istrm1, b.Iendp2, b.Jstrm1, b.Jendp2),
            "R": (b.IstrUm2, b.Iendp1, b.JstrVm2, b.Jendp1),
            "OU": (b.IstrUm1, b.Iendp1, b.Jstrm1, b.Jendp1),
            "OV": (b.Istrm1, b.Iendp1, b.JstrVm1, b.Jendp1)}


def level_body(st, U, V, visc_r, visc_p, ranges, hz_in_flux, finish):
    """K_LOOP of the rotated operator on U, V (ni, nj, N).  finish(k, W): the last statement group of level k = 1..N,
    with W the work arrays (UFx, UFe, VFx, VFe of the level; UFsx, UFse, VFsx, VFse slabs with W.k1, W.k2; W.X(range)
    the index tuple of a named range)."""
    b, p = st.b, st.p
    N = b.N
    masking, wet = bool(p.masking), bool(p.wet_dry)
    pm, pn, z_r, Hz = st["pm"], st["pn"], st["z_r"], st["Hz"]
    on_r, om_r, on_p, om_p = st["on_r"], st["om_r"], st["on_p"], st["om_p"]
    on_u, om_u, on_v, om_v = st["on_u"], st["om_u"], st["on_v"], st["om_v"]

    def X(name):
        ia, ib, ja, jb = ranges[name]
        return (st.I(ia, ib), st.J(ja, jb))

    def masked(cff, r, kind):
        if masking:
            cff = cff * st[kind + "mask"][r]
        if wet:
            cff = cff * st[kind + "mask_wet"][r]
        return cff

    class W:
        pass
    W.X = staticmethod(X)
    W.masked = staticmethod(masked)
    z2 = lambda: np.zeros((st.ni, st.nj))
    z3 = lambda: np.zeros((st.ni, st.nj, 2))
    UFx, VFe, UFe, VFx = z2(), z2(), z2(), z2()
    UFse, UFsx, VFse, VFsx = z3(), z3(), z3(), z3()
    dmUde, dmVde, dnUdx, dnVdx, dUdz, dVdz = z3(), z3(), z3(), z3(), z3(), z3()
    dZde_p, dZde_r, dZdx_p, dZdx_r = z3(), z3(), z3(), z3()
    W.UFx, W.VFe, W.UFe, W.VFx, W.UFse, W.UFsx, W.VFse, W.VFsx = UFx, VFe, UFe, VFx, UFse, UFsx, VFse, VFsx
    rU, rV, rP, rR, oU, oV = X("U"), X("V"), X("P"), X("R"), X("OU"), X("OV")
    k2 = 0
    for k in range(0, N + 1):
        k1 = k2
        k2 = 1 - k1
        W.k1, W.k2 = k1, k2
        if k < N:
            n = k                                  # array index of level k+1
            # slopes at RHO- and PSI-points
            cff = masked(0.5 * (pm[_sh(rU, -1)] + pm[rU]), rU, "u")
            UFx[rU] = cff * (z_r[rU + (n,)] - z_r[_sh(rU, -1) + (n,)])
            cff = masked(0.5 * (pn[_sh(rV, 0, -1)] + pn[rV]), rV, "v")
            VFe[rV] = cff * (z_r[rV + (n,)] - z_r[_sh(rV, 0, -1) + (n,)])
            dZdx_p[rP + (k2,)] = 0.5 * (UFx[_sh(rP, 0, -1)] + UFx[rP])
            dZde_p[rP + (k2,)] = 0.5 * (VFe[_sh(rP, -1)] + VFe[rP])
            dZdx_r[rR + (k2,)] = 0.5 * (UFx[rR] + UFx[_sh(rR, 1)])
            dZde_r[rR + (k2,)] = 0.5 * (VFe[rR] + VFe[_sh(rR, 0, 1)])
            # horizontal gradients
            cff = masked(0.5 * pm[rR], rR, "r")
            dnUdx[rR + (k2,)] = cff * ((pn[rR] + pn[_sh(rR, 1)]) * U[_sh(rR, 1) + (n,)] -
                                       (pn[_sh(rR, -1)] + pn[rR]) * U[rR + (n,)])
            cff = masked(0.125 * (pn[_sh(rP, -1)] + pn[rP] + pn[_sh(rP, -1, -1)] + pn[_sh(rP, 0, -1)]), rP, "p")
            dmUde[rP + (k2,)] = cff * ((pm[_sh(rP, -1)] + pm[rP]) * U[rP + (n,)] -
                                       (pm[_sh(rP, -1, -1)] + pm[_sh(rP, 0, -1)]) * U[_sh(rP, 0, -1) + (n,)])
            cff = masked(0.125 * (pm[_sh(rP, -1)] + pm[rP] + pm[_sh(rP, -1, -1)] + pm[_sh(rP, 0, -1)]), rP, "p")
            dnVdx[rP + (k2,)] = cff * ((pn[_sh(rP, 0, -1)] + pn[rP]) * V[rP + (n,)] -
                                       (pn[_sh(rP, -1, -1)] + pn[_sh(rP, -1)]) * V[_sh(rP, -1) + (n,)])
            cff = masked(0.5 * pn[rR], rR, "r")
            dmVde[rR + (k2,)] = cff * ((pm[rR] + pm[_sh(rR, 0, 1)]) * V[_sh(rR, 0, 1) + (n,)] -
                                       (pm[_sh(rR, 0, -1)] + pm[rR]) * V[rR + (n,)])
        if k == 0 or k == N:
            dUdz[rU + (k2,)] = 0.0
            dVdz[rV + (k2,)] = 0.0
            UFsx[oU + (k2,)] = 0.0
            UFse[oU + (k2,)] = 0.0
            VFsx[oV + (k2,)] = 0.0
            VFse[oV + (k2,)] = 0.0
        else:
            n, m = k, k - 1                        # levels k+1, k
            cff = 1.0 / (0.5 * (z_r[_sh(rU, -1) + (n,)] - z_r[_sh(rU, -1) + (m,)] + z_r[rU + (n,)] - z_r[rU + (m,)]))
            dUdz[rU + (k2,)] = cff * (U[rU + (n,)] - U[rU + (m,)])
            cff = 1.0 / (0.5 * (z_r[_sh(rV, 0, -1) + (n,)] - z_r[_sh(rV, 0, -1) + (m,)] + z_r[rV + (n,)] - z_r[rV + (m,)]))
            dVdz[rV + (k2,)] = cff * (V[rV + (n,)] - V[rV + (m,)])
        if k > 0:
            m = k - 1                              # array index of level k
            # rotated horizontal fluxes
            r = rR
            cff1, cff2 = _min0(dZdx_r[r + (k1,)]), _max0(dZdx_r[r + (k1,)])
            cff3, cff4 = _min0(dZde_r[r + (k1,)]), _max0(dZde_r[r + (k1,)])
            inner = (on_r[r] * (dnUdx[r + (k1,)] - 0.5 * pn[r] *
                                (cff1 * (dUdz[r + (k1,)] + dUdz[_sh(r, 1) + (k2,)]) +
                                 cff2 * (dUdz[r + (k2,)] + dUdz[_sh(r, 1) + (k1,)]))) -
                     om_r[r] * (dmVde[r + (k1,)] - 0.5 * pm[r] *
                                (cff3 * (dVdz[r + (k1,)] + dVdz[_sh(r, 0, 1) + (k2,)]) +
                                 cff4 * (dVdz[r + (k2,)] + dVdz[_sh(r, 0, 1) + (k1,)]))))
            cff = Hz[r + (m,)] * inner if hz_in_flux else inner
            cff = masked(cff, r, "r")
            UFx[r] = on_r[r] * on_r[r] * visc_r[r] * cff
            VFe[r] = om_r[r] * om_r[r] * visc_r[r] * cff
            r = rP
            pm_p = 0.25 * (pm[_sh(r, -1, -1)] + pm[_sh(r, -1)] + pm[_sh(r, 0, -1)] + pm[r])
            pn_p = 0.25 * (pn[_sh(r, -1, -1)] + pn[_sh(r, -1)] + pn[_sh(r, 0, -1)] + pn[r])
            cff1, cff2 = _min0(dZdx_p[r + (k1,)]), _max0(dZdx_p[r + (k1,)])
            cff3, cff4 = _min0(dZde_p[r + (k1,)]), _max0(dZde_p[r + (k1,)])
            inner = (on_p[r] * (dnVdx[r + (k1,)] - 0.5 * pn_p *
                                (cff1 * (dVdz[_sh(r, -1) + (k1,)] + dVdz[r + (k2,)]) +
                                 cff2 * (dVdz[_sh(r, -1) + (k2,)] + dVdz[r + (k1,)]))) +
                     om_p[r] * (dmUde[r + (k1,)] - 0.5 * pm_p *
                                (cff3 * (dUdz[_sh(r, 0, -1) + (k1,)] + dUdz[r + (k2,)]) +
                                 cff4 * (dUdz[_sh(r, 0, -1) + (k2,)] + dUdz[r + (k1,)]))))
            if hz_in_flux:
                cff = 0.25 * (Hz[_sh(r, -1) + (m,)] + Hz[r + (m,)] + Hz[_sh(r, -1, -1) + (m,)] + Hz[_sh(r, 0, -1) + (m,)]) * inner
            else:
                cff = inner
            cff = masked(cff, r, "p")
            UFe[r] = om_p[r] * om_p[r] * visc_p[r] * cff
            VFx[r] = on_p[r] * on_p[r] * visc_p[r] * cff
            # vertical fluxes due to the sloping surfaces
            if k < N:
                r = oU
                w, nn, ne = _sh(r, -1), _sh(r, 0, 1), _sh(r, -1, 1)
                cff = 0.25 * (visc_r[w] + visc_r[r])
                fac1 = cff * on_u[r]
                fac2 = cff * om_u[r]
                cff = 0.5 * (pn[w] + pn[r])
                dnUdz = cff * dUdz[r + (k2,)]
                dnVdz = cff * 0.25 * (dVdz[ne + (k2,)] + dVdz[nn + (k2,)] + dVdz[w + (k2,)] + dVdz[r + (k2,)])
                cff = 0.5 * (pm[w] + pm[r])
                dmUdz = cff * dUdz[r + (k2,)]
                dmVdz = cff * 0.25 * (dVdz[ne + (k2,)] + dVdz[nn + (k2,)] + dVdz[w + (k2,)] + dVdz[r + (k2,)])
                cff1, cff2 = _min0(dZdx_r[w + (k1,)]), _min0(dZdx_r[r + (k2,)])
                cff3, cff4 = _max0(dZdx_r[w + (k2,)]), _max0(dZdx_r[r + (k1,)])
                UFsx[r + (k2,)] = fac1 * (cff1 * (cff1 * dnUdz - dnUdx[w + (k1,)]) + cff2 * (cff2 * dnUdz - dnUdx[r + (k2,)]) +
                                          cff3 * (cff3 * dnUdz - dnUdx[w + (k2,)]) + cff4 * (cff4 * dnUdz - dnUdx[r + (k1,)]))
                cff1, cff2 = _min0(dZde_p[r + (k1,)]), _min0(dZde_p[nn + (k2,)])
                cff3, cff4 = _max0(dZde_p[r + (k2,)]), _max0(dZde_p[nn + (k1,)])
                UFse[r + (k2,)] = fac2 * (cff1 * (cff1 * dmUdz - dmUde[r + (k1,)]) + cff2 * (cff2 * dmUdz - dmUde[nn + (k2,)]) +
                                          cff3 * (cff3 * dmUdz - dmUde[r + (k2,)]) + cff4 * (cff4 * dmUdz - dmUde[nn + (k1,)]))
                cff5, cff6 = _min0(dZdx_p[r + (k1,)]), _min0(dZdx_p[nn + (k2,)])
                cff7, cff8 = _max0(dZdx_p[r + (k2,)]), _max0(dZdx_p[nn + (k1,)])
                UFsx[r + (k2,)] = UFsx[r + (k2,)] + \
                    fac1 * (cff1 * (cff5 * dnVdz - dnVdx[r + (k1,)]) + cff2 * (cff6 * dnVdz - dnVdx[nn + (k2,)]) +
                            cff3 * (cff7 * dnVdz - dnVdx[r + (k2,)]) + cff4 * (cff8 * dnVdz - dnVdx[nn + (k1,)]))
                cff1, cff2 = _min0(dZdx_r[w + (k1,)]), _min0(dZdx_r[r + (k2,)])
                cff3, cff4 = _max0(dZdx_r[w + (k2,)]), _max0(dZdx_r[r + (k1,)])
                cff5, cff6 = _min0(dZde_r[w + (k1,)]), _min0(dZde_r[r + (k2,)])
                cff7, cff8 = _max0(dZde_r[w + (k2,)]), _max0(dZde_r[r + (k1,)])
                UFse[r + (k2,)] = UFse[r + (k2,)] - \
                    fac2 * (cff1 * (cff5 * dmVdz - dmVde[w + (k1,)]) + cff2 * (cff6 * dmVdz - dmVde[r + (k2,)]) +
                            cff3 * (cff7 * dmVdz - dmVde[w + (k2,)]) + cff4 * (cff8 * dmVdz - dmVde[r + (k1,)]))
                r = oV
                s_, e, se = _sh(r, 0, -1), _sh(r, 1), _sh(r, 1, -1)
                cff = 0.25 * (visc_r[s_] + visc_r[r])
                fac1 = cff * on_v[r]
                fac2 = cff * om_v[r]
                cff = 0.5 * (pn[s_] + pn[r])
                dnUdz = cff * 0.25 * (dUdz[r + (k2,)] + dUdz[e + (k2,)] + dUdz[s_ + (k2,)] + dUdz[se + (k2,)])
                dnVdz = cff * dVdz[r + (k2,)]
                cff = 0.5 * (pm[s_] + pm[r])
                dmUdz = cff * 0.25 * (dUdz[r + (k2,)] + dUdz[e + (k2,)] + dUdz[s_ + (k2,)] + dUdz[se + (k2,)])
                dmVdz = cff * dVdz[r + (k2,)]
                cff1, cff2 = _min0(dZdx_p[r + (k1,)]), _min0(dZdx_p[e + (k2,)])
                cff3, cff4 = _max0(dZdx_p[r + (k2,)]), _max0(dZdx_p[e + (k1,)])
                VFsx[r + (k2,)] = fac1 * (cff1 * (cff1 * dnVdz - dnVdx[r + (k1,)]) + cff2 * (cff2 * dnVdz - dnVdx[e + (k2,)]) +
                                          cff3 * (cff3 * dnVdz - dnVdx[r + (k2,)]) + cff4 * (cff4 * dnVdz - dnVdx[e + (k1,)]))
                cff1, cff2 = _min0(dZde_r[s_ + (k1,)]), _min0(dZde_r[r + (k2,)])
                cff3, cff4 = _max0(dZde_r[s_ + (k2,)]), _max0(dZde_r[r + (k1,)])
                VFse[r + (k2,)] = fac2 * (cff1 * (cff1 * dmVdz - dmVde[s_ + (k1,)]) + cff2 * (cff2 * dmVdz - dmVde[r + (k2,)]) +
                                          cff3 * (cff3 * dmVdz - dmVde[s_ + (k2,)]) + cff4 * (cff4 * dmVdz - dmVde[r + (k1,)]))
                cff5, cff6 = _min0(dZdx_r[s_ + (k1,)]), _min0(dZdx_r[r + (k2,)])
                cff7, cff8 = _max0(dZdx_r[s_ + (k2,)]), _max0(dZdx_r[r + (k1,)])
                VFsx[r + (k2,)] = VFsx[r + (k2,)] - \
                    fac1 * (cff1 * (cff5 * dnUdz - dnUdx[s_ + (k1,)]) + cff2 * (cff6 * dnUdz - dnUdx[r + (k2,)]) +
                            cff3 * (cff7 * dnUdz - dnUdx[s_ + (k2,)]) + cff4 * (cff8 * dnUdz - dnUdx[r + (k1,)]))
                cff1, cff2 = _min0(dZdx_p[r + (k1,)]), _min0(dZdx_p[e + (k2,)])
                cff3, cff4 = _max0(dZdx_p[r + (k2,)]), _max0(dZdx_p[e + (k1,)])
                cff5, cff6 = _min0(dZde_p[r + (k1,)]), _min0(dZde_p[e + (k2,)])
                cff7, cff8 = _max0(dZde_p[r + (k2,)]), _max0(dZde_p[e + (k1,)])
                VFse[r + (k2,)] = VFse[r + (k2,)] + \
                    fac2 * (cff1 * (cff5 * dmUdz - dmUde[r + (k1,)]) + cff2 * (cff6 * dmUdz - dmUde[e + (k2,)]) +
                            cff3 * (cff7 * dmUdz - dmUde[r + (k2,)]) + cff4 * (cff8 * dmUdz - dmUde[e + (k1,)]))
            finish(k, W)


def _time_step(st, nnew, sign, mag=None):
    """the last statement group of uv3dmix2_geo.h (:710-752, sign = +1) and of K_LOOP2 of uv3dmix4_geo.h (:1430-1474,
    sign = -1): momentum is Hz*u, Hz*v here.  mag: a dict whose arrays "rufrc", "rvfrc" receive the sum over the levels
    of the magnitudes of the fluxes whose differences cff1 .. cff4 are (at least |cff1| + |cff2| + |cff3| + |cff4|; for
    rounding bounds: the roundings the four terms inherit are relative to the fluxes, not to their differences)"""
    pm, pn, dt = st["pm"], st["pn"], st.p.dt
    u, v, rufrc, rvfrc = st["u"], st["v"], st["rufrc"], st["rvfrc"]

    def finish(k, W):
        k1, k2, m = W.k1, W.k2, k - 1
        r = W.X("OU")
        w, nn = _sh(r, -1), _sh(r, 0, 1)
        cff = dt * 0.25 * (pm[w] + pm[r]) * (pn[w] + pn[r])
        cff1 = 0.5 * (pn[w] + pn[r]) * (W.UFx[r] - W.UFx[w])
        cff2 = 0.5 * (pm[w] + pm[r]) * (W.UFe[nn] - W.UFe[r])
        cff3 = W.UFsx[r + (k2,)] - W.UFsx[r + (k1,)]
        cff4 = W.UFse[r + (k2,)] - W.UFse[r + (k1,)]
        cff5 = cff * (cff1 + cff2)
        cff6 = dt * (cff3 + cff4)
        if mag is not None:
            mag["rufrc"][r] += (0.5 * (pn[w] + pn[r]) * (np.abs(W.UFx[r]) + np.abs(W.UFx[w])) +
                                0.5 * (pm[w] + pm[r]) * (np.abs(W.UFe[nn]) + np.abs(W.UFe[r])) +
                                np.abs(W.UFsx[r + (k2,)]) + np.abs(W.UFsx[r + (k1,)]) +
                                np.abs(W.UFse[r + (k2,)]) + np.abs(W.UFse[r + (k1,)]))
        if sign > 0:
            rufrc[r] = rufrc[r] + cff1 + cff2 + cff3 + cff4
            u[r + (m, nnew - 1)] = u[r + (m, nnew - 1)] + cff5 + cff6
        else:
            rufrc[r] = rufrc[r] - cff1 - cff2 - cff3 - cff4
            u[r + (m, nnew - 1)] = u[r + (m, nnew - 1)] - cff5 - cff6
        r = W.X("OV")
        s_, e = _sh(r, 0, -1), _sh(r, 1)
        cff = dt * 0.25 * (pm[r] + pm[s_]) * (pn[r] + pn[s_])
        cff1 = 0.5 * (pn[s_] + pn[r]) * (W.VFx[e] - W.VFx[r])
        cff2 = 0.5 * (pm[s_] + pm[r]) * (W.VFe[r] - W.VFe[s_])
        cff3 = W.VFsx[r + (k2,)] - W.VFsx[r + (k1,)]
        cff4 = W.VFse[r + (k2,)] - W.VFse[r + (k1,)]
        cff5 = cff * (cff1 - cff2)
        cff6 = dt * (cff3 + cff4)
        if mag is not None:
            mag["rvfrc"][r] += (0.5 * (pn[s_] + pn[r]) * (np.abs(W.VFx[e]) + np.abs(W.VFx[r])) +
                                0.5 * (pm[s_] + pm[r]) * (np.abs(W.VFe[r]) + np.abs(W.VFe[s_])) +
                                np.abs(W.VFsx[r + (k2,)]) + np.abs(W.VFsx[r + (k1,)]) +
                                np.abs(W.VFse[r + (k2,)]) + np.abs(W.VFse[r + (k1,)]))
        if sign > 0:
            rvfrc[r] = rvfrc[r] + cff1 - cff2 + cff3 + cff4
            v[r + (m, nnew - 1)] = v[r + (m, nnew - 1)] + cff5 + cff6
        else:
            rvfrc[r] = rvfrc[r] - cff1 + cff2 - cff3 - cff4
            v[r + (m, nnew - 1)] = v[r + (m, nnew - 1)] - cff5 - cff6
    return finish


def _first_operator(st, LapU, LapV):
    """the first harmonic operator, uv3dmix4_geo.h:761-799"""
    pm, pn, Hz = st["pm"], st["pn"], st["Hz"]

    def finish(k, W):
        k1, k2, m = W.k1, W.k2, k - 1
        r = W.X("OU")
        w, nn = _sh(r, -1), _sh(r, 0, 1)
        cff = 0.125 * (pm[w] + pm[r]) * (pn[w] + pn[r])
        cff1 = 1.0 / (0.5 * (Hz[w + (m,)] + Hz[r + (m,)]))
        lap = cff * ((pn[w] + pn[r]) * (W.UFx[r] - W.UFx[w]) + (pm[w] + pm[r]) * (W.UFe[nn] - W.UFe[r])) + \
            cff1 * ((W.UFsx[r + (k2,)] + W.UFse[r + (k2,)]) - (W.UFsx[r + (k1,)] + W.UFse[r + (k1,)]))
        LapU[r + (m,)] = W.masked(lap, r, "u")
        r = W.X("OV")
        s_, e = _sh(r, 0, -1), _sh(r, 1)
        cff = 0.125 * (pm[r] + pm[s_]) * (pn[r] + pn[s_])
        cff1 = 1.0 / (0.5 * (Hz[s_ + (m,)] + Hz[r + (m,)]))
        lap = cff * ((pn[s_] + pn[r]) * (W.VFx[e] - W.VFx[r]) - (pm[s_] + pm[r]) * (W.VFe[r] - W.VFe[s_])) + \
            cff1 * ((W.VFsx[r + (k2,)] + W.VFse[r + (k2,)]) - (W.VFsx[r + (k1,)] + W.VFse[r + (k1,)]))
        LapV[r + (m,)] = W.masked(lap, r, "v")
    return finish


def _closed(p, side, var):
    c = p.lbc[abi.LBS[side]][abi.LBV[var]]
    if not c:
        c = {"west": p.lbc_west, "east": p.lbc_east, "south": p.lbc_south, "north": p.lbc_north}[side]
    return c == abi.LBC["Clo"]


def lap_rules(st, LapU, LapV):
    """the rule for LapU, LapV outside closed or open edges and at the corners, uv3dmix4_geo.h:806-976"""
    b, p = st.b, st.p
    I, J = st.I, st.J
    g2 = p.gamma2
    ju, jv = J(b.Jstrm1, b.Jendp1), J(b.JstrVm1, b.Jendp1)
    iu, iv = I(b.IstrUm1, b.Iendp1), I(b.Istrm1, b.Iendp1)
    if not b.EWperiodic:
        if b.west_edge:
            LapU[I(b.IstrU - 1), ju] = 0.0 if _closed(p, "west", "u") else LapU[I(b.IstrU), ju]
            LapV[I(b.Istr - 1), jv] = g2 * LapV[I(b.Istr), jv] if _closed(p, "west", "v") else 0.0
        if b.east_edge:
            LapU[I(b.Iend + 1), ju] = 0.0 if _closed(p, "east", "u") else LapU[I(b.Iend), ju]
            LapV[I(b.Iend + 1), jv] = g2 * LapV[I(b.Iend), jv] if _closed(p, "east", "v") else 0.0
    if not b.NSperiodic:
        if b.south_edge:
            LapU[iu, J(b.Jstr - 1)] = g2 * LapU[iu, J(b.Jstr)] if _closed(p, "south", "u") else 0.0
            LapV[iv, J(b.JstrV - 1)] = 0.0 if _closed(p, "south", "v") else LapV[iv, J(b.JstrV)]
        if b.north_edge:
            LapU[iu, J(b.Jend + 1)] = g2 * LapU[iu, J(b.Jend)] if _closed(p, "north", "u") else 0.0
            LapV[iv, J(b.Jend + 1)] = 0.0 if _closed(p, "north", "v") else LapV[iv, J(b.Jend)]
    if not b.EWperiodic and not b.NSperiodic:
        Is, Ie, Js, Je = b.Istr, b.Iend, b.Jstr, b.Jend
        if b.south_edge and b.west_edge:
            LapU[I(Is), J(Js - 1)] = 0.5 * (LapU[I(Is + 1), J(Js - 1)] + LapU[I(Is), J(Js)])
            LapV[I(Is - 1), J(Js)] = 0.5 * (LapV[I(Is - 1), J(Js + 1)] + LapV[I(Is), J(Js)])
        if b.south_edge and b.east_edge:
            LapU[I(Ie + 1), J(Js - 1)] = 0.5 * (LapU[I(Ie), J(Js - 1)] + LapU[I(Ie + 1), J(Js)])
            LapV[I(Ie + 1), J(Js)] = 0.5 * (LapV[I(Ie), J(Js)] + LapV[I(Ie + 1), J(Js + 1)])
        if b.north_edge and b.west_edge:
            LapU[I(Is), J(Je + 1)] = 0.5 * (LapU[I(Is + 1), J(Je + 1)] + LapU[I(Is), J(Je)])
            LapV[I(Is - 1), J(Je + 1)] = 0.5 * (LapV[I(Is), J(Je + 1)] + LapV[I(Is - 1), J(Je)])
        if b.north_edge and b.east_edge:
            LapU[I(Ie + 1), J(Je + 1)] = 0.5 * (LapU[I(Ie), J(Je + 1)] + LapU[I(Ie + 1), J(Je)])
            LapV[I(Ie + 1), J(Je + 1)] = 0.5 * (LapV[I(Ie), J(Je + 1)] + LapV[I(Ie + 1), J(Je)])


def uv3dmix2_geo(st, s):
    """uv3dmix2_geo_tile on the state, in place"""
    U, V = st["u"][:, :, :, s.nrhs - 1], st["v"][:, :, :, s.nrhs - 1]
    if s.nrhs == s.nnew:
        U, V = U.copy(), V.copy()
    level_body(st, U, V, st["visc2_r"], st["visc2_p"], tile_ranges(st.b), True, _time_step(st, s.nnew, +1))
    return st


def uv3dmix4_geo(st, s, keep=None, mag=None):
    """uv3dmix4_geo_tile on the state, in place.  keep: a dict that receives LapU, LapV (after the rules); mag: see
    _time_step"""
    assert st.b.NghostPoints == 3
    assert s.nrhs != s.nnew
    U, V = st["u"][:, :, :, s.nrhs - 1], st["v"][:, :, :, s.nrhs - 1]
    LapU = np.zeros((st.ni, st.nj, st.b.N), order="F")
    LapV = np.zeros((st.ni, st.nj, st.b.N), order="F")
    level_body(st, U, V, st["visc4_r"], st["visc4_p"], first_ranges(st.b), False, _first_operator(st, LapU, LapV))
    lap_rules(st, LapU, LapV)
    level_body(st, LapU, LapV, st["visc4_r"], st["visc4_p"], tile_ranges(st.b), True, _time_step(st, s.nnew, -1, mag))
    if keep is not None:
        keep["LapU"], keep["LapV"] = LapU, LapV
    return st


def forcing_magnitude(st0, s):
    """{"rufrc", "rvfrc"}: the sum over the levels of the magnitudes of the fluxes behind the four terms uv3dmix4_geo
    adds to them (see _time_step)"""
    mag = {"rufrc": np.zeros((st0.ni, st0.nj)), "rvfrc": np.zeros((st0.ni, st0.nj))}
    uv3dmix4_geo(st0.copy(), s, mag=mag)
    return mag
