"""The yardstick of the NPZD_POWELL biology (roms_hip_biology): a vectorised numpy restatement of npzd_powell_tile,
ROMS/Nonlinear/Biology/npzd_Powell.h:199-656, written from the Fortran text and not from the kernel, with the same
operation order (one numpy operation per Fortran operation, on all columns at once; the loops over k that carry a
dependence stay loops).  Parity status: pinned -- tests/test_ref_pinning.py compares it with
the reference's own biology(ng, tile) (oracle/_ref/UPWELLING_BIO, UPWELLING_BIO_CPAR) on the states of bio_state within 1e-13
of each pool's maximum (measured: 1e-16 and below), tests/test_golden.py with the vectors of tests/golden/ref_bio.npz;
tests/test_bio.py pins it to closed forms as well.

    positive           :237-251, one time level
    light              :337-363
    reactions          :371-450
    sink_column        :460-628 (the default end conditions)
    npzd_powell        the tile routine on arrays of columns
    expected           ... on a TileState: t with t(nnew) of the biological tracers updated on Istr:Iend, Jstr:Jend
    bio_state          the states tests/test_gpu_bio.py runs; GRIDS, PARAMS, PARITY_CASES: their tables
"""
import numpy as np

import util
from roms_trunk_mgh_amd import bio

MINVAL = 1.0e-6
iNO3, iPhyt, iZoop, iSDet = range(4)          # positions in idbio


def interior(b):
    return slice(b.Istr - b.LBi, b.Iend - b.LBi + 1), slice(b.Jstr - b.LBj, b.Jend - b.LBj + 1)


def positive(v):
    """:237-251 for one time level: v[..., 4] in the order of idbio; returns the positive-definite pools"""
    v = np.array(v, dtype=np.float64)
    cff1 = np.zeros(v.shape[:-1])
    imax = np.zeros(v.shape[:-1] + (1,), dtype=np.int64)
    for q in range(4):
        cff1 = cff1 + np.maximum(0.0, MINVAL - v[..., q])
        now = np.take_along_axis(v, imax, -1)[..., 0]            # BioTrc(iTrcMax): already lifted
        imax = np.where((v[..., q] > now)[..., None], q, imax)
        v[..., q] = np.maximum(MINVAL, v[..., q])
    top = np.take_along_axis(v, imax, -1)[..., 0]
    np.put_along_axis(v, imax, np.where(top > cff1, top - cff1, top)[..., None], -1)
    return v


def light(par, PARsur, phyt, z_w):
    """:337-363: Light[..., N] from the surface PAR, the phytoplankton column and z_w[..., 0:N+1]"""
    N = phyt.shape[-1]
    out = np.zeros(phyt.shape)
    PAR = PARsur.copy()
    day = PARsur > 0.0
    for k in range(N, 0, -1):
        Att = (par.AttSW + par.AttPhy * phyt[..., k - 1]) * (z_w[..., k] - z_w[..., k - 1])
        ExpAtt = np.exp(-Att)
        Itop = PAR
        PAR = Itop * (1.0 - ExpAtt) / Att
        out[..., k - 1] = np.where(day, PAR, 0.0)
        PAR = Itop * ExpAtt
    return out


def reactions(par, dtdays, Bio, Light):
    """:371-450 in place on Bio[..., N, 4]"""
    N_, P_, Z_, D_ = (Bio[..., q] for q in range(4))             # views
    cff1 = dtdays * par.Vm_NO3 * par.PhyIS
    cff2 = par.Vm_NO3 * par.Vm_NO3
    cff3 = par.PhyIS * par.PhyIS
    cff4 = 1.0 / np.sqrt(cff2 + cff3 * Light * Light)
    cff = P_ * cff1 * cff4 * Light / (par.K_NO3 + N_)
    N_[...] = N_ / (1.0 + cff)
    P_[...] = P_ + N_ * cff
    cff1 = dtdays * par.ZooGR
    cff2 = 1.0 - par.ZooEEN - par.ZooEED
    cff = Z_ * cff1 * (1.0 - np.exp(-par.Ivlev * P_)) / P_
    P_[...] = P_ / (1.0 + cff)
    Z_[...] = Z_ + P_ * cff2 * cff
    N_[...] = N_ + P_ * par.ZooEEN * cff
    D_[...] = D_ + P_ * par.ZooEED * cff
    cff3 = dtdays * par.PhyMRD
    cff2 = dtdays * par.PhyMRN
    cff1 = 1.0 / (1.0 + cff2 + cff3)
    P_[...] = P_ * cff1
    N_[...] = N_ + P_ * cff2
    D_[...] = D_ + P_ * cff3
    cff3 = dtdays * par.ZooMRD
    cff2 = dtdays * par.ZooMRN
    cff1 = 1.0 / (1.0 + cff2 + cff3)
    Z_[...] = Z_ * cff1
    N_[...] = N_ + Z_ * cff2
    D_[...] = D_ + Z_ * cff3
    cff2 = dtdays * par.DetRR
    cff1 = 1.0 / (1.0 + cff2)
    D_[...] = D_ * cff1
    N_[...] = N_ + D_ * cff2


def _ppm_limit(dltR, dltL, cffR, cffL, strict):
    """the IF / ELSE IF chains of :490-497 (strict = False: .le.) and :562-569 (strict = True: .lt.)"""
    flat = (dltR * dltL < 0.0) if strict else (dltR * dltL <= 0.0)
    capR = ~flat & (np.abs(dltR) > np.abs(cffL))
    capL = ~flat & ~capR & (np.abs(dltL) > np.abs(cffR))
    return np.where(flat, 0.0, np.where(capR, cffL, dltR)), np.where(flat, 0.0, np.where(capL, cffR, dltL))


def sink_column(Hz, z_w, qc, cff):
    """:468-628 for one constituent: Hz[..., N], z_w[..., 0:N+1], qc[..., N], cff = dtdays * |w|.
    Returns (the new column, FC(0), ksource[..., N])."""
    N = Hz.shape[-1]
    lead = Hz.shape[:-1]
    Hz_inv = 1.0 / Hz
    Hz_inv2 = 1.0 / (Hz[..., :-1] + Hz[..., 1:])                 # k = 1 .. N-1
    Hz_inv3 = 1.0 / (Hz[..., :-2] + Hz[..., 1:-1] + Hz[..., 2:])  # k = 2 .. N-1
    FC = np.zeros(lead + (N + 1,))
    FC[..., 1:N] = (qc[..., 1:] - qc[..., :-1]) * Hz_inv2
    bR, bL, WR, WL = (np.zeros(lead + (N,)) for _ in range(4))
    c, m, p = slice(1, N - 1), slice(0, N - 2), slice(2, N)      # cells k = 2 .. N-1, k-1, k+1
    FCk, FCm = FC[..., 2:N], FC[..., 1:N - 1]
    dltR = Hz[..., c] * FCk
    dltL = Hz[..., c] * FCm
    cf = Hz[..., m] + 2.0 * Hz[..., c] + Hz[..., p]
    cffR = cf * FCk
    cffL = cf * FCm
    dltR, dltL = _ppm_limit(dltR, dltL, cffR, cffL, strict=False)
    cf = (dltR - dltL) * Hz_inv3
    dltR = dltR - cf * Hz[..., p]
    dltL = dltL + cf * Hz[..., m]
    bR[..., c] = qc[..., c] + dltR
    bL[..., c] = qc[..., c] - dltL
    WR[..., c] = (2.0 * dltR - dltL) ** 2
    WL[..., c] = (dltR - 2.0 * dltL) ** 2
    # WENO reconciliation, k = 2 .. N-2 (step k reads nothing step k-1 wrote)
    kk, kp = slice(1, N - 2), slice(2, N - 1)
    dL = np.maximum(1.0E-14, WL[..., kk])
    dR = np.maximum(1.0E-14, WR[..., kp])
    rec = (dR * bR[..., kk] + dL * bL[..., kp]) / (dR + dL)
    bR[..., kk] = rec
    bL[..., kp] = rec
    FC[..., N] = 0.0
    bR[..., N - 1] = qc[..., N - 1]                               # :535-537
    bL[..., N - 1] = qc[..., N - 1]
    bR[..., N - 2] = qc[..., N - 1]
    bL[..., 1] = qc[..., 0]                                       # :546-548
    bR[..., 0] = qc[..., 0]
    bL[..., 0] = qc[..., 0]
    dltR = bR - qc
    dltL = qc - bL
    dltR, dltL = _ppm_limit(dltR, dltL, 2.0 * dltR, 2.0 * dltL, strict=True)
    bR = qc + dltR
    bL = qc - dltL
    # the flux, :589-623
    FC[..., 0:N] = 0.0
    WLd = z_w[..., 0:N] + cff
    WRw = Hz * qc
    ksource = np.broadcast_to(np.arange(1, N + 1), lead + (N,)).copy()
    for k in range(1, N + 1):
        for ks in range(k, N):
            hit = WLd[..., k - 1] > z_w[..., ks]
            ksource[..., k - 1] = np.where(hit, ks + 1, ksource[..., k - 1])
            FC[..., k - 1] = np.where(hit, FC[..., k - 1] + WRw[..., ks - 1], FC[..., k - 1])
    ix = ksource - 1
    g = lambda A: np.take_along_axis(A, ix, -1)
    cu = np.minimum(1.0, (WLd - g(z_w[..., 0:N])) * g(Hz_inv))
    FC[..., 0:N] = FC[..., 0:N] + g(Hz) * cu * (g(bL) + cu * (0.5 * (g(bR) - g(bL)) - (1.5 - cu) * (g(bR) + g(bL) - 2.0 * g(qc))))
    new = qc + (FC[..., 1:] - FC[..., :-1]) * Hz_inv
    return new, FC[..., 0].copy(), ksource


def npzd_powell(par, dt, rho0, Hz, z_w, srflx, tS, tN, info=None):
    """npzd_powell_tile on columns: Hz[..., N], z_w[..., N+1], srflx[...], tS = t(nstp) and tN = t(nnew) (transport
    units) as [..., N, 4] in the order of idbio.  Returns the new t(nnew).  info (a dict) receives ksource of the last
    iteration per sinking constituent, the day flag and FC(0)."""
    if par.BioIter <= 0:                                          # :180
        return tN.copy()
    dtdays = dt * (1.0 / 86400.0) / float(par.BioIter)            # :184
    Hz_inv = 1.0 / Hz
    Bio_old = positive(tS)
    positive(tN * Hz_inv[..., None])                              # itime = nnew: evaluated, and nothing reads it (:256-260)
    Bio = Bio_old.copy()
    if par.const_par:
        PARsur = np.full(srflx.shape, 158.075)
    else:
        PARsur = par.PARfrac * srflx * rho0 * par.Cp
    with np.errstate(all="ignore"):
        for _ in range(par.BioIter):
            L = light(par, PARsur, Bio[..., iPhyt], z_w)
            reactions(par, dtdays, Bio, L)
            for name, q, w in (("Phyt", iPhyt, par.wPhy), ("SDet", iSDet, par.wDet)):
                new, FC0, ksource = sink_column(Hz, z_w, Bio[..., q].copy(), dtdays * abs(w))
                Bio[..., q] = new
                if info is not None:
                    info["ksource_" + name], info["FC0_" + name] = ksource, FC0
    if info is not None:
        info["day"] = PARsur > 0.0
    return tN + (Bio - Bio_old) * Hz[..., None]


def columns(st, par, nstp=1, nnew=2):
    """the arguments of npzd_powell for the interior columns of a TileState"""
    I = interior(st.b)
    it = [q - 1 for q in par.tracers(st.b)]
    t = st["t"]
    tS = np.stack([t[I][:, :, :, nstp - 1, q] for q in it], axis=-1)
    tN = np.stack([t[I][:, :, :, nnew - 1, q] for q in it], axis=-1)
    return dict(Hz=st["Hz"][I].copy(), z_w=st["z_w"][I].copy(), srflx=st["srflx"][I].copy(), tS=tS, tN=tN)


def expected(st, par, nstp=1, nnew=2, info=None, perturb=None):
    """t of the state after biology(ng, tile): a copy with t(nnew) of the biological tracers replaced on Istr:Iend,
    Jstr:Jend.  perturb: a relative factor array maker f(shape) applied to every input (tests/test_bio.py)."""
    a = columns(st, par, nstp, nnew)
    if perturb is not None:
        a = {k: v * perturb(v.shape) for k, v in a.items()}
    new = npzd_powell(par, st.p.dt, st.p.rho0, info=info, **a)
    out = st["t"].copy()
    I = interior(st.b)
    for q, itrc in enumerate(par.tracers(st.b)):
        out[I[0], I[1], :, nnew - 1, itrc - 1] = new[..., q]
    return out


# ------------------------------------------------------------------------------------------ the parity cases --
GRIDS = {"TINY": {}, "PARTIAL": dict(Lm=67, Mm=6, N=4), "N17": dict(Lm=66, Mm=9, N=17), "N32": dict(Lm=66, Mm=9, N=32),
         "N33": dict(Lm=66, Mm=9, N=33), "N48": dict(Lm=66, Mm=9, N=48), "N49": dict(Lm=66, Mm=9, N=49),
         "N64": dict(Lm=66, Mm=9, N=64)}
SINK_DEPTH = 60.0      # m: dtdays * wDet of the "sink" set -- several thin cells, and more than the shallowest columns hold
PHY_DEPTH = 1.5        # m: dtdays * wPhy of the "sink" set


def params(name, dt):
    """the parameter sets of the parity cases: the .in defaults, BioIter = 3, sinking of both constituents, CONST_PAR"""
    base = bio.PowellPar()
    if name == "default":
        return base
    if name == "iter3":
        return base.replace(BioIter=3)
    if name == "sink":
        dtdays = dt / 86400.0
        return base.replace(wPhy=PHY_DEPTH / dtdays, wDet=SINK_DEPTH / dtdays)
    if name == "constpar":
        return base.replace(const_par=1)
    raise KeyError(name)


PARAMS = ("default", "iter3", "sink", "constpar")
# every grid with and without the island under the sinking set (the search, the end conditions and the level-count
# boundaries of the instantiations); the other sets on the smallest grid and across the 32 / 33 and the 64 boundary
PARITY_CASES = [(g, m, "sink") for g in GRIDS for m in (None, "island")] + \
               [(g, m, ps) for g in ("TINY", "N33", "N64") for m in (None, "island") for ps in ("default", "iter3", "constpar")]


def case_id(case):
    g, m, ps = case
    return "-".join([g, "mask" if m else "nomask", ps])


def bio_state(grid="TINY", mask=None):
    """util.prepared_state(BENCHMARK_TINY, NT = 6) with what the biology reads made non-trivial:
      * columns between 25 m and 400 m deep with thin cells at the surface (Hz, z_w set here: the routine reads nothing
        else of the grid), so that one sinking distance stays inside a cell, crosses several, or passes the surface;
      * non-uniform pools at both time levels, t(nnew) in transport units;
      * srflx positive in runs of five columns and zero in the next five (day and night inside one wavefront);
      * scattered cells with negative pools at t(nstp) and t(nnew): a deficit the largest pool covers, and cells whose
        every pool lies below the deficit, so that nothing is deducted.
    Land columns carry values like any other: the reference never looks at rmask."""
    st = util.prepared_state("BENCHMARK_TINY", NT=6, overrides=dict(GRIDS[grid]) or None, mask=mask)
    b, N = st.b, st.b.N
    ii = np.arange(b.LBi, b.UBi + 1, dtype=np.float64)[:, None]
    jj = np.arange(b.LBj, b.UBj + 1, dtype=np.float64)[None, :]
    x = 2.0 * np.pi * ii / b.Lm
    y = np.pi * jj / (b.Mm + 1.0)
    depth = 25.0 + 375.0 * (0.5 + 0.5 * np.sin(x + 0.4) * np.cos(y)) ** 2
    s = np.arange(0, N + 1, dtype=np.float64) / N                                   # 0 at the bed, 1 at the surface
    zeta = 0.2 * np.cos(2.0 * x) * np.sin(y)
    z_w = zeta[:, :, None] - (depth + zeta)[:, :, None] * (1.0 - s[None, None, :]) ** 2.0   # thin cells at the surface
    st["z_w"][:] = z_w
    st["Hz"][:] = z_w[:, :, 1:] - z_w[:, :, :-1]
    kk = (np.arange(1, N + 1, dtype=np.float64) / N)[None, None, :]
    amp = (17.0, 1.3, 0.8, 0.6)
    for q, it in enumerate(range(b.NAT, b.NAT + 4)):
        for lev in range(3):
            f = 0.55 + 0.4 * np.sin((q + 1) * x + 0.3 * lev + q)[:, :, None] * np.cos(y[:, :, None] * (1 + q % 2) + 2.0 * kk) \
                + 0.05 * np.sin(7.0 * x + 3.0 * y + q)[:, :, None] * kk
            st["t"][:, :, :, lev, it] = amp[q] * f
    # negative cells: every 7th / 11th point in a pattern of the global indices, at alternating levels
    neg = ((ii.astype(int) * 3 + jj.astype(int) * 5) % 7 == 0)[:, :, None] & ((np.arange(N) % 3) == 1)[None, None, :]
    low = ((ii.astype(int) * 5 + jj.astype(int) * 3) % 11 == 0)[:, :, None] & ((np.arange(N) % 4) == 2)[None, None, :]
    for lev in range(2):
        st["t"][:, :, :, lev, b.NAT + 1][neg] = -0.05 - 0.01 * lev       # phytoplankton below zero: nitrate pays
        st["t"][:, :, :, lev, b.NAT + 3][neg] = -0.002
        for q in range(4):                                                # all four pools tiny or negative: nobody can pay
            st["t"][:, :, :, lev, b.NAT + q][low] = (-3.0e-7, 2.0e-7, -1.0e-7, 4.0e-7)[q] * (1.0 + lev)
    st["t"][:, :, :, 1, b.NAT:b.NAT + 4] *= st["Hz"][:, :, :, None]        # t(nnew = 2): transport units
    run = (np.floor((ii - 1.0) / 5.0) % 2 == 0)
    st["srflx"][:] = np.where(run, 6.0e-5 * (1.0 + 0.5 * np.sin(3.0 * x) * np.sin(y)), 0.0) + 0.0 * jj
    return st
