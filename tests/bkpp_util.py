"""The yardstick of the KPP bottom boundary layer (LMD_BKPP): a numpy restatement of lmd_bkpp_tile written from the
Fortran (ROMS/Nonlinear/lmd_bkpp.F:233-804; the file's own SASHA, RI_SPLINES, SALINITY, MASKING by the state's switch, no
LMD_SHAPIRO) -- loops over k, vectorised over i, j, the operation order of the reference -- with

    ksbl_from_hsbl     ksbl as lmd_skpp.F:653-658 and :787 leave it
    finish_increment   the lmd_finish increment (lmd_vmix.F:524-540)
    bc_hbbl            the gradient / periodic rule of bc_r2d_tile for hbbl on one tile (lmd_bkpp.F:577-586)
    expected           what roms_hip_lmd_vmix with the switch on must give, from its result with the switch off
    bkpp_state         the states the GPU tests run, and PARITY_CASES, their table

Parity status: pinned -- tests/test_ref_pinning.py compares `expected` with the reference's own lmd_vmix(ng, tile) built
with LMD_BKPP (oracle/_ref/BENCHMARK_BKPP, BENCHMARK_MASK_BKPP) on every state of PARITY_CASES (kbbl, ksbl identical; hbbl,
Akv, Akt within 1e-13 of each field's maximum), tests/test_golden.py with the vectors of tests/golden/ref_bkpp.npz.

lmd_bkpp_tile also returns a branch census and the decision margins per column (tests/test_bkpp.py asserts both over
PARITY_CASES, tests/test_gpu_bkpp.py compares the device with the restatement on the same cases)."""
import math

import numpy as np

VONKAR, EPS, SMALL = 0.41, 1.0e-10, 1.0e-20
LMD_RIC, LMD_CEKMAN, LMD_EPSILON, LMD_CV, LMD_BETAT = 0.3, 0.7, 0.1, 1.25, -0.2
LMD_AM, LMD_AS, LMD_CM, LMD_CS, LMD_ZETAM, LMD_ZETAS = 1.257, -28.86, 8.36, 98.96, -0.2, -1.0
LMD_BVFCON, LMD_NU0C = -2.0e-5, 0.01
R3 = 1.0 / 3.0
BRANCHES = ("stable", "zetam_gt", "zetam_le", "zetas_gt", "zetas_le")


def interior(b):
    return slice(b.Istr - b.LBi, b.Iend - b.LBi + 1), slice(b.Jstr - b.LBj, b.Jend - b.LBj + 1)


def _shift(b, di, dj):
    return (slice(b.Istr - b.LBi + di, b.Iend - b.LBi + 1 + di), slice(b.Jstr - b.LBj + dj, b.Jend - b.LBj + 1 + dj))


def swfrac(p, Z):
    """lmd_swfrac_tile with Zscale = -1 (lmd_swfrac.F:60-75)"""
    fac1, fac2, fac3 = -1.0 / p.swfrac_mu1, -1.0 / p.swfrac_mu2, p.swfrac_r1
    return np.exp(Z * fac1) * fac3 + np.exp(Z * fac2) * (1.0 - fac3)


def wscale(Ustar, sigma, Bf, seen=None):
    """wm, ws of lmd_bkpp.F:428-447 (= :642-661, :740-759); seen: {branch: boolean column array}, or-ed in"""
    Ustar3 = Ustar * Ustar * Ustar
    zetahat = VONKAR * sigma * Bf
    zetapar = zetahat / (Ustar3 + SMALL)
    stable = zetahat >= 0.0
    zp = np.where(stable, 0.0, zetapar)                 # the unstable formulas, evaluated where they apply only
    zh = np.where(stable, 0.0, zetahat)
    wm_u = np.where(zp > LMD_ZETAM, VONKAR * Ustar * (1.0 - 16.0 * zp) ** 0.25, VONKAR * np.abs(LMD_AM * Ustar3 - LMD_CM * zh) ** R3)
    ws_u = np.where(zp > LMD_ZETAS, VONKAR * Ustar * (1.0 - 16.0 * zp) ** 0.5, VONKAR * np.abs(LMD_AS * Ustar3 - LMD_CS * zh) ** R3)
    wm_s = VONKAR * Ustar / (1.0 + 5.0 * np.where(stable, zetapar, 0.0))
    if seen is not None:
        for name, m in (("stable", stable), ("zetam_gt", ~stable & (zetapar > LMD_ZETAM)), ("zetam_le", ~stable & ~(zetapar > LMD_ZETAM)),
                        ("zetas_gt", ~stable & (zetapar > LMD_ZETAS)), ("zetas_le", ~stable & ~(zetapar > LMD_ZETAS))):
            seen[name] = seen.get(name, False) | m
    return np.where(stable, wm_s, wm_u), np.where(stable, wm_s, ws_u)


def ksbl_from_hsbl(st, hsbl):
    """ksbl on the interior points (zero elsewhere): lmd_skpp.F:653-658, then 0 where the surface layer reaches the
    bottom layer (:742, :787)"""
    b, N = st.b, st.b.N
    I = interior(b)
    zw, hs = st["z_w"][I], hsbl[I]
    k_ = np.ones(hs.shape, dtype=np.int32)
    for k in range(N, 1, -1):
        k_ = np.where((k_ == 1) & (zw[:, :, k - 1] < hs), k, k_)
    k_ = np.where(hs > zw[:, :, 1], k_, 0).astype(np.int32)
    out = np.zeros((st.ni, st.nj), dtype=np.int32)
    out[I] = k_
    return out


def finish_increment(st):
    """lmd_nu0c * nu_sxc of lmd_finish_tile (LMD_CONVEC, lmd_vmix.F:524-540) on W-levels 1 .. N-1 of the interior
    points, zero elsewhere; exactly zero where bvf >= 0"""
    b, N = st.b, st.b.N
    I = interior(b)
    out = np.zeros_like(st["bvf"])
    cff = np.maximum(st["bvf"][I][:, :, 1:N], LMD_BVFCON)
    cff = np.minimum(1.0, (LMD_BVFCON - cff) / LMD_BVFCON)
    nu = 1.0 - cff * cff
    out[I[0], I[1], 1:N] = LMD_NU0C * (nu * nu * nu)
    return out


def bc_hbbl(b, A):
    """bc_r2d_tile (bc_2d.F:74-157) on one tile, in place: gradient edges and corner means, or the periodic images"""
    i0, i1, j0, j1 = b.Istr - b.LBi, b.Iend - b.LBi, b.Jstr - b.LBj, b.Jend - b.LBj
    if not b.EWperiodic:
        A[i1 + 1, j0:j1 + 1] = A[i1, j0:j1 + 1]
        A[i0 - 1, j0:j1 + 1] = A[i0, j0:j1 + 1]
    A[i0:i1 + 1, j1 + 1] = A[i0:i1 + 1, j1]
    A[i0:i1 + 1, j0 - 1] = A[i0:i1 + 1, j0]
    if not b.EWperiodic:
        A[i0 - 1, j0 - 1] = 0.5 * (A[i0, j0 - 1] + A[i0 - 1, j0])
        A[i1 + 1, j0 - 1] = 0.5 * (A[i1, j0 - 1] + A[i1 + 1, j0])
        A[i0 - 1, j1 + 1] = 0.5 * (A[i0 - 1, j1] + A[i0, j1 + 1])
        A[i1 + 1, j1 + 1] = 0.5 * (A[i1 + 1, j1] + A[i1, j1 + 1])
    else:
        for i in range(max(b.LBi, -2), min(b.UBi, b.Lm + b.NghostPoints) + 1):
            if i < 1 or i > b.Lm:
                A[i - b.LBi, :] = A[(i - 1) % b.Lm + 1 - b.LBi, :]
    return A


def defined_points(b):
    """the points of (LBi:UBi, LBj:UBj) where hbbl is defined after bc_r2d_tile on one tile"""
    if b.EWperiodic:
        ii = slice(max(b.LBi, -2) - b.LBi, min(b.UBi, b.Lm + b.NghostPoints) - b.LBi + 1)
    else:
        ii = slice(b.Istr - 1 - b.LBi, b.Iend + 1 - b.LBi + 1)
    return ii, slice(b.Jstr - 1 - b.LBj, b.Jend + 1 - b.LBj + 1)


def lmd_bkpp_tile(st, Akv, Akt, ksbl, hbbl_prev, nstp=1):
    """lmd_bkpp_tile on the interior points of one tile.  Akv (.., 0:N), Akt (.., 0:N, NAT), ksbl, hbbl_prev: arrays of
    the tile's extents (inputs, not changed).  Returns dict(hbbl, kbbl, Akv, Akt: arrays of the tile's extents, hbbl before
    bc_r2d_tile; census: {name: bool array on the interior}; margins: {name: float array on the interior, the smallest
    relative distance of a discrete decision of the column from its threshold; inf where there is none})."""
    b, p, N = st.b, st.p, st.b.N
    I, Ip, Jp = interior(b), _shift(b, 1, 0), _shift(b, 0, 1)
    masking = bool(p.masking)
    rmask = st["rmask"][I] if masking else None
    mul = (lambda x: x * rmask) if masking else (lambda x: x)
    g = p.g
    gorho0 = g / p.rho0
    Hz, z_w, pden, bvf = st["Hz"][I], st["z_w"][I], st["pden"][I], st["bvf"][I]
    u, v = st["u"][:, :, :, nstp - 1], st["v"][:, :, :, nstp - 1]
    ua, ub, va, vb = u[I], u[Ip], v[I], v[Jp]
    Akv, Akt = Akv[I].copy(), Akt[I].copy()
    ksbl = ksbl[I]
    shape = ksbl.shape
    seen = {}
    Vtc = LMD_CV * math.sqrt(-LMD_BETAT) / (math.sqrt(LMD_CS * LMD_EPSILON) * LMD_RIC * VONKAR * VONKAR)      # :233
    bl_dpth = LMD_EPSILON * (hbbl_prev[I] - z_w[:, :, 0])                                                     # :243
    bu, bv = 0.5 * (st["bustr"][I] + st["bustr"][Ip]), 0.5 * (st["bvstr"][I] + st["bvstr"][Jp])
    Ustar = mul(np.sqrt(np.sqrt(bu * bu + bv * bv)))                                                          # :254-257
    alpha, beta = st["alpha"][I], st["beta"][I]
    Bo = g * (alpha * st["btflx"][I][:, :, 0] - beta * st["btflx"][I][:, :, 1])                                # :272
    Bosol = g * alpha * st["srflx"][I]                                                                        # :277
    Bflux = np.zeros(shape + (N + 1,))
    for k in range(N + 1):                                                                                    # :285-303
        Bflux[:, :, k] = mul(Bo + Bosol * (1.0 - swfrac(p, z_w[:, :, N] - z_w[:, :, k])))
    # the three parabolic splines, :316-348
    FC, dR, dU, dV = (np.zeros(shape + (N + 1,)) for _ in range(4))
    for k in range(1, N):
        cff = 1.0 / (2.0 * Hz[:, :, k] + Hz[:, :, k - 1] * (2.0 - FC[:, :, k - 1]))
        FC[:, :, k] = cff * Hz[:, :, k]
        dR[:, :, k] = cff * (6.0 * (pden[:, :, k] - pden[:, :, k - 1]) - Hz[:, :, k - 1] * dR[:, :, k - 1])
        dU[:, :, k] = cff * (3.0 * (ua[:, :, k] - ua[:, :, k - 1] + ub[:, :, k] - ub[:, :, k - 1]) - Hz[:, :, k - 1] * dU[:, :, k - 1])
        dV[:, :, k] = cff * (3.0 * (va[:, :, k] - va[:, :, k - 1] + vb[:, :, k] - vb[:, :, k - 1]) - Hz[:, :, k - 1] * dV[:, :, k - 1])
    for k in range(N - 1, 0, -1):
        dR[:, :, k] = dR[:, :, k] - FC[:, :, k] * dR[:, :, k + 1]
        dU[:, :, k] = dU[:, :, k] - FC[:, :, k] * dU[:, :, k + 1]
        dV[:, :, k] = dV[:, :, k] - FC[:, :, k] * dV[:, :, k + 1]
    cff1, cff2 = 1.0 / 3.0, 1.0 / 6.0
    Rref = pden[:, :, 0] - Hz[:, :, 0] * (cff1 * dR[:, :, 0] + cff2 * dR[:, :, 1])                             # :408-413
    Uref = 0.5 * (ua[:, :, 0] + ub[:, :, 0]) - Hz[:, :, 0] * (cff1 * dU[:, :, 0] + cff2 * dU[:, :, 1])
    Vref = 0.5 * (va[:, :, 0] + vb[:, :, 0]) - Hz[:, :, 0] * (cff1 * dV[:, :, 0] + cff2 * dV[:, :, 1])
    FC[:, :, 0] = 0.0                                                                                         # :419-465
    searched = {}
    for k in range(1, N + 1):
        depth = z_w[:, :, k] - z_w[:, :, 0]
        sigma = np.where(Bflux[:, :, k] < 0.0, np.minimum(bl_dpth, depth), depth)
        s_k = {}
        wm, ws = wscale(Ustar, sigma, Bflux[:, :, k], s_k)
        searched[k] = s_k
        dRk, dUk, dVk = ((d[:, :, k] if k < N else 0.0 * d[:, :, 0]) for d in (dR, dU, dV))
        Rk = pden[:, :, k - 1] + Hz[:, :, k - 1] * (cff1 * dRk + cff2 * dR[:, :, k - 1])
        Uk = 0.5 * (ua[:, :, k - 1] + ub[:, :, k - 1]) + Hz[:, :, k - 1] * (cff1 * dUk + cff2 * dU[:, :, k - 1])
        Vk = 0.5 * (va[:, :, k - 1] + vb[:, :, k - 1]) + Hz[:, :, k - 1] * (cff1 * dVk + cff2 * dV[:, :, k - 1])
        Ritop = -gorho0 * (Rk - Rref) * depth
        Ribot = (Uk - Uref) ** 2 + (Vk - Vref) ** 2 + Vtc * depth * ws * np.sqrt(np.abs(bvf[:, :, k]))
        FC[:, :, k] = Ritop - LMD_RIC * Ribot
    kbbl = np.full(shape, N, dtype=np.int32)                                                                  # :469-482
    hbbl = z_w[:, :, N].copy()
    for k in range(1, N):
        hit = (kbbl == N) & (FC[:, :, k] > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            val = (z_w[:, :, k] * FC[:, :, k - 1] - z_w[:, :, k - 1] * FC[:, :, k]) / (FC[:, :, k - 1] - FC[:, :, k])
        # the branches of wscale a thread that stops at the crossing has taken: the levels up to it
        for name, m in searched[k].items():
            seen[name] = seen.get(name, False) | (m & (kbbl == N))
        hbbl = np.where(hit, val, hbbl)
        kbbl = np.where(hit, k, kbbl).astype(np.int32)
    kcross, h_search = kbbl.copy(), hbbl.copy()
    hekman = LMD_CEKMAN * Ustar / np.maximum(np.abs(st["f"][I]), EPS) - st["h"][I]                             # :528-536
    hbbl = np.where(Ustar >= 0.0, np.minimum(hekman, hbbl), hbbl)
    hbbl = np.minimum(hbbl, z_w[:, :, N])
    h_premax = hbbl.copy()
    hbbl = mul(np.maximum(hbbl, z_w[:, :, 0]))
    kbbl = np.full(shape, N, dtype=np.int32)                                                                  # :592-597
    for k in range(1, N + 1):
        kbbl = np.where((kbbl == N) & (z_w[:, :, k] > hbbl), k, kbbl).astype(np.int32)
    Bfbot = mul(Bo + Bosol * (1.0 - swfrac(p, mul(z_w[:, :, N] - hbbl))))                                      # :607-621
    bl_dpth = LMD_EPSILON * (hbbl - z_w[:, :, 0])                                                             # :635-661
    sigma = np.where(Bfbot > 0.0, 1.0, LMD_EPSILON) * (hbbl - z_w[:, :, 0])
    wm, ws = wscale(Ustar, sigma, Bfbot, seen)
    f1 = 5.0 * np.maximum(0.0, Bfbot) * VONKAR / (Ustar * Ustar * Ustar * Ustar + EPS)                         # :673
    zbl = hbbl - z_w[:, :, 0]                                                                                 # :680-719
    at = lambda A, k: np.take_along_axis(A, k[:, :, None].astype(np.intp), axis=2)[:, :, 0]
    zk, zm = at(z_w, kbbl), at(z_w, kbbl - 1)
    cff = 1.0 / (zk - zm)
    cff_dn, cff_up = cff * (hbbl - zm), cff * (zk - hbbl)

    def shape_fn(A, w):
        K_bl = cff_dn * at(A, kbbl) + cff_up * at(A, kbbl - 1)
        dK_bl = -cff * (at(A, kbbl) - at(A, kbbl - 1))
        return mul(K_bl / (zbl * w + EPS)), np.minimum(0.0, K_bl * f1 - dK_bl / (w + EPS))
    Gm1, dGm1dS = shape_fn(Akv, wm)
    Gt1, dGt1dS = shape_fn(Akt[:, :, :, 0], ws)
    Gs1, dGs1dS = shape_fn(Akt[:, :, :, 1], ws)
    overlap = np.zeros(shape, dtype=bool)
    m_max = np.full(shape, np.inf)
    for k in range(1, N):                                                                                     # :727-804
        inside = z_w[:, :, k] < hbbl
        depth = z_w[:, :, k] - z_w[:, :, 0]
        sigma = np.where(Bflux[:, :, k] < 0.0, np.minimum(bl_dpth, depth), depth)
        s_k = {}
        wm, ws = wscale(Ustar, sigma, Bflux[:, :, k], s_k)
        for name, m in s_k.items():
            seen[name] = seen.get(name, False) | (m & inside)
        sigma = mul(depth / (hbbl - z_w[:, :, 0] + EPS))
        a1, a2, a3 = sigma - 2.0, 3.0 - 2.0 * sigma, sigma - 1.0
        Gm = a1 + a2 * Gm1 + a3 * dGm1dS
        Gt = a1 + a2 * Gt1 + a3 * dGt1dS
        Gs = a1 + a2 * Gs1 + a3 * dGs1dS
        both = k > ksbl
        overlap |= inside & both
        for A, val in ((Akv[:, :, k], depth * wm * (1.0 + sigma * Gm)), (Akt[:, :, k, 0], depth * ws * (1.0 + sigma * Gt)),
                       (Akt[:, :, k, 1], depth * ws * (1.0 + sigma * Gs))):
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.abs(A - val) / np.maximum(np.abs(A), np.abs(val))
            m_max = np.where(inside & both, np.minimum(m_max, rel), m_max)
            A[...] = np.where(inside, np.where(both, np.maximum(A, val), val), A)
    # ---- census and margins ----
    water = rmask > 0.0 if masking else np.ones(shape, dtype=bool)
    found = kcross < N
    # clipped to the bottom: a crossing at k = 1 interpolates between FC(0) = 0 and FC(1) to z_w(0) itself (to an ulp)
    at_bottom = (hbbl == mul(z_w[:, :, 0])) | (found & (kcross == 1) & (h_search <= hekman))
    census = {"crossing": found & (kbbl > 1) & water,
              "no_crossing_ekman": ~found & (hekman < z_w[:, :, N]) & (hekman > z_w[:, :, 0]) & water,
              "clipped_to_bottom": at_bottom & water,
              "overlap": overlap & water,
              "ksbl_zero": (ksbl == 0) & water,
              "land": ~water}
    for name in BRANCHES:
        census[name] = np.broadcast_to(seen.get(name, False), shape) & water
    absFC = np.abs(FC[:, :, 1:N])
    fcmax = absFC.max(axis=2) if N > 1 else np.ones(shape)
    # FC on both sides of the crossing: k and k - 1 (FC(0) = 0 is the definition of :420, not a computed value)
    kk = np.arange(1, N)[None, None, :]
    looked = found[:, :, None] & ((kk == kcross[:, :, None]) | (kk == kcross[:, :, None] - 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        m_fc = np.where(looked, absFC / fcmax[:, :, None], np.inf).min(axis=2, initial=np.inf)
        # the levels lmd_bkpp compares with hbbl: z_w(k) > hbbl (:594) and z_w(k) < hbbl (:730), k = 1 .. N
        m_zw = (np.abs(z_w[:, :, 1:] - hbbl[:, :, None]) / Hz).min(axis=2)
        m_ek = np.abs(hekman - h_search) / st["h"][I]
        # MAX(hbbl, z_w(0)), :533: its arguments are equal by construction in a column clipped to the bottom (a crossing
        # at k = 1 interpolates to z_w(0) itself; Ustar = 0 gives hekman - h = z_w(0)); there the MAX is continuous and
        # decides nothing else, so those columns carry no margin of this kind
        m_clamp = np.where(at_bottom, np.inf, np.abs(h_premax - z_w[:, :, 0]) / np.maximum(np.abs(h_premax), np.abs(z_w[:, :, 0])))
    margins = {"FC": m_fc, "z_w": m_zw, "ekman": m_ek, "max_profile": m_max, "max_clamp": m_clamp}
    for name in margins:                     # land: every product is zero, no decision reaches a result
        margins[name] = np.where(water, margins[name], np.inf)
    out = {"census": census, "margins": margins}
    for name, A, dt in (("hbbl", hbbl, np.float64), ("kbbl", kbbl, np.int32)):
        full = np.zeros((st.ni, st.nj), dtype=dt, order="F")
        full[I] = A
        out[name] = full
    return dict(out, Akv=Akv, Akt=Akt, FC=FC, hekman=hekman, Ustar=Ustar, kcross=kcross)


def expected(st, A_Akv, A_Akt, A_hsbl, hbbl_prev, nstp=1):
    """What the device must give with the switch on, from its result with the switch off on the same inputs (A):
    lmd_bkpp_tile of A without the lmd_finish increment (exactly zero where bvf >= 0) with ksbl from A's hsbl, then the
    increment, then bc_r2d_tile(hbbl).  Akv / Akt: interior columns, W-levels 1 .. N-1 (lmd_finish's edges copy them)."""
    I = interior(st.b)
    inc = finish_increment(st)
    ksbl = ksbl_from_hsbl(st, A_hsbl)
    r = lmd_bkpp_tile(st, A_Akv - inc, A_Akt - inc[:, :, :, None], ksbl, hbbl_prev, nstp)
    r["Akv"] = r["Akv"] + inc[I]
    r["Akt"] = r["Akt"] + inc[I][:, :, :, None]
    if st.b.east_edge:
        # lmd_finish_tile's boundary values as written (lmd_vmix.F:560-575: "Iend-1" on the eastern edge, no periodicity
        # guard): the interior column Iend-1 receives column Iend -- in A, whose column Iend-1 therefore is no input of
        # that column's own profile, and in the result
        r["Akv"][-2] = r["Akv"][-1]
        r["Akt"][-2] = r["Akt"][-1]
    r["ksbl"] = ksbl
    r["hbbl"] = bc_hbbl(st.b, r["hbbl"])
    return r


# ------------------------------------------------------------------------------------------------ the states --
GRIDS = {"TINY": {}, "PARTIAL": dict(Lm=67, Mm=6, N=4), "N32": dict(Lm=66, Mm=9, N=32), "N33": dict(Lm=66, Mm=9, N=33),
         "N64": dict(Lm=66, Mm=9, N=64)}
# (grid, mask, basin, unstable): every grid as a channel and as a basin, with and without the island; the variant with
# unstable patches in bvf on BENCHMARK_TINY
PARITY_CASES = [(g, m, bs, False) for g in GRIDS for m in (None, "island") for bs in (False, True)] + \
               [("TINY", None, False, True), ("TINY", "island", True, True)]


def case_id(case):
    g, m, bs, un = case
    return "-".join([g, "mask" if m else "nomask", "basin" if bs else "channel"] + (["unstable"] if un else []))


def bkpp_state(grid="TINY", mask=None, basin=False, unstable=False, stress=True):
    """util.kpp_state with what the bottom layer needs: bottom stress in two strengths (weak in the southern half, strong
    in the northern one; stress=False: none at all), a bottom heat flux of both signs (by quarters of the domain in i), f
    of both magnitudes (1e-4 and 1e-5 1/s, alternating every eighth of the domain in i, so that every combination with the
    other two occurs), and with `unstable` patches of negative bvf.  Returns (state, hbbl of the previous step)."""
    import util
    ov = dict(GRIDS[grid])
    if basin:
        ov["EWperiodic"] = False
    st = util.kpp_state("BENCHMARK_TINY", mask=mask, overrides=ov or None)
    b = st.b
    ii = np.arange(b.LBi, b.UBi + 1, dtype=np.float64)[:, None]
    jj = np.arange(b.LBj, b.UBj + 1, dtype=np.float64)[None, :]
    x = (np.mod(ii - 1.0, b.Lm) + 0.5) / b.Lm          # periodic in i: the ghost columns are images
    y = (jj - 0.5) / b.Mm
    wob = 1.0 + 0.3 * np.sin(2.0 * math.pi * 2.0 * x) * np.cos(math.pi * y)
    strong = y > 0.5
    if stress:
        st["bustr"][:] = np.where(strong, 2.0e-3, 1.0e-5) * wob
        st["bvstr"][:] = np.where(strong, 1.0e-3, 0.6e-5) * (2.0 - wob)
    else:
        st["bustr"][:] = 0.0
        st["bvstr"][:] = 0.0
    st["btflx"][:, :, 0] = np.where(np.mod(np.floor(4.0 * x), 2.0) == 0.0, 3.0e-4, -3.0e-4) * wob
    st["f"][:] = np.where(np.mod(np.floor(8.0 * x), 2.0) == 0.0, 1.0e-4, 1.0e-5) * (1.0 + 0.1 * (wob - 1.0))
    # weakly stratified columns (every other sixteenth of the domain in i): the density and bvf profiles shrink towards
    # the bottom value, so that the bulk Richardson function finds no crossing there and the Ekman limit decides; under
    # the strong wind the surface layer then reaches the bottom (ksbl = 0), and the two layers overlap
    weak = (np.mod(np.floor(16.0 * x), 2.0) == 1.0)[:, :, None]
    shrink = np.where(weak, 1.0e-3, 1.0)
    st["pden"][:] = st["pden"][:, :, :1] + shrink * (st["pden"] - st["pden"][:, :, :1])
    st["bvf"][:] = shrink * st["bvf"]
    if unstable:
        kk = np.arange(b.N + 1)[None, None, :]
        patch = (np.sin(2.0 * math.pi * 3.0 * x) > 0.6)[:, :, None] & (kk >= 1) & (kk <= max(1, b.N // 3))
        st["bvf"][:] = np.where(patch, -0.3 * np.abs(st["bvf"]) - 1.0e-7, st["bvf"])
    else:
        st["bvf"][:] = np.abs(st["bvf"])
    if mask is not None:
        st["bustr"] *= st["umask"]
        st["bvstr"] *= st["vmask"]
        st["btflx"] *= st["rmask"][:, :, None]
    # the depth of the previous step: a tenth of the way up the column, not the zero of a first step
    hprev = np.asfortranarray(st["z_w"][:, :, 0] + 0.1 * (st["z_w"][:, :, -1] - st["z_w"][:, :, 0]))
    if mask is not None:
        hprev *= st["rmask"]
    # No column may sit within rounding of a discrete decision (tests/test_bkpp.py, test_margins).  The crossing of the
    # critical function, the levels around hbbl and the Ekman limit depend on the column's own inputs only, so a column
    # that fails has its stratification (pden about its bottom value, and bvf) weakened by a fifth and its bottom heat
    # flux raised by a quarter, at most four times: a rule of the state, the same on every tiling.  (The interior Akv / Akt enter the MAX of the merged profile only; test_margins checks that one.)
    if stress:
        I = interior(b)
        zero = np.zeros((st.ni, st.nj), dtype=np.int32)
        for _ in range(4):
            m = lmd_bkpp_tile(st, st["Akv"], st["Akt"], zero, hprev)["margins"]
            bad = (m["FC"] <= 1.0e-5) | (m["z_w"] <= 1.0e-5) | (m["ekman"] <= 1.0e-5)
            if not bad.any():
                break
            st["btflx"][I[0], I[1], 0] = np.where(bad, 1.25 * st["btflx"][I][:, :, 0], st["btflx"][I][:, :, 0])
            fac = np.where(bad, 0.8, 1.0)[:, :, None]
            st["pden"][I] = st["pden"][I][:, :, :1] + fac * (st["pden"][I] - st["pden"][I][:, :, :1])
            st["bvf"][I] = fac * st["bvf"][I]
    return st, hprev
