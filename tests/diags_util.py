"""Expected values of the tracer budget terms (DIAGNOSTICS_TS), recovered from the per-routine entry points of the
oracle, which has no diagnostic lines (tests/test_diags.py, tests/test_gpu_diags.py).

Stage differences: pre_step3d leaves t(nnew) = Hz*t(nstp) + (FC(k)-FC(k-1)), so iTvdif of the predictor is
t_after_pre - Hz*t(nstp); t3dmix2 adds iThdif; step3d_t with Akt = 0 leaves t_new = (t_in + advection) * oHz, so the
advection is t_new*Hz - t_in; with the full Akt the implicit increment is t_new - t_new(Akt = 0).  Zeroing one
transport isolates a direction: Hvom = W = 0 leaves iTxadv, Huon = W = 0 iTyadv, Huon = Hvom = 0 iTvadv, W = 0 iThadv.
The diffusion is split the same way through the face metrics: pnom_v = 0 leaves iTxdif, pmon_u = 0 iTydif.

Tolerance.  A value recovered as a - b (m Tunits) and scaled by oHz is compared within 8 * eps * max(|a|, |b|) * oHz
per point: the roundings in forming a and b and in the scaling, with a factor of two of room.  A sum of recovered values
takes the sum of their bounds.  Differences of values already in Tunits take the same bound without the oHz."""
import numpy as np

EPS = np.finfo(np.float64).eps


class Rec:
    """a recovered value with its per-point bound"""

    def __init__(self, val, bound):
        self.val, self.bound = val, bound

    def __add__(self, other):
        return Rec(self.val + other.val, self.bound + other.bound)


def diff(a, b, scale=1.0):
    """(a - b) * scale with the bound 8 eps max(|a|, |b|) scale"""
    return Rec((a - b) * scale, 8.0 * EPS * np.maximum(np.abs(a), np.abs(b)) * np.abs(scale))


def within(got, rec, where=None):
    """the largest excess of |got - rec.val| over rec.bound at the points `where` (<= 0: inside the bound everywhere)"""
    ex = np.abs(got - rec.val) - rec.bound
    if where is not None:
        ex = ex[where]
    return float(ex.max())


def interior(st):
    b = st.b
    return st.I(b.Istr, b.Iend), st.J(b.Jstr, b.Jend)


def _tnew(st, s):
    return st["t"][:, :, :, s.nnew - 1, :].copy()


def recover(st0, s):
    """{term: Rec} on the whole arrays (N, NT trailing; valid at interior water points) of one pre_step3d, t3dmix2 (with
    ts_dif2), step3d_t sequence from state st0, computed by the oracle alone; also "t_new" and "rate0s" = Hz*t(nstp)*oHz."""
    import oracle
    st = st0.copy()
    o = oracle.Oracle(st)
    Hz = st["Hz"][:, :, :, None].copy()
    oHz = 1.0 / np.where(Hz > 0.0, Hz, 1.0)                          # (Hz is not set outside the tile's ghost points)
    rate0 = Hz * st["t"][:, :, :, s.nstp - 1, :]                     # exact restatement of cff1 = Hz*t(nstp)
    o.call("pre_step3d", s)
    t_pre = _tnew(st, s)
    t_dir = {}
    if st.p.ts_dif2:
        # the xi-flux of t3dmix2_s.h carries the factor pmon_u and never reads pnom_v, the eta-flux the converse: with
        # one of the two metrics zeroed the whole of the routine is the other direction's term
        for name, metric in (("iTxdif", "pnom_v"), ("iTydif", "pmon_u")):
            v = st.copy()
            v[metric][:] = 0.0
            oracle.Oracle(v).call("t3dmix2", s)
            t_dir[name] = _tnew(v, s)
        o.call("t3dmix2", s)
    t_mix = _tnew(st, s)
    st_in = st.copy()
    o.call("step3d_t", s)
    t_new = _tnew(st, s)

    def variant(zero):
        v = st_in.copy()
        for name in zero:
            v[name][:] = 0.0
        oracle.Oracle(v).call("step3d_t", s)
        return _tnew(v, s)

    t_adv = variant(["Akt"])
    out = {"iTvdif_pre": diff(t_pre, rate0, oHz)}
    if st.p.ts_dif2:
        out["iThdif"] = diff(t_mix, t_pre, oHz)
        for name, t_one in t_dir.items():
            out[name] = diff(t_one, t_pre, oHz)
    for name, zero in (("iThadv", ["W"]), ("iTxadv", ["W", "Hvom"]), ("iTyadv", ["W", "Huon"]), ("iTvadv", ["Huon", "Hvom"]),
                       ("adv", [])):
        out[name] = diff(variant(["Akt"] + zero) * Hz, t_mix, oHz)
    out["iTvdif"] = out["iTvdif_pre"] + diff(t_new, t_adv)
    out["iTrate"] = diff(t_new, rate0 * oHz)
    out["t_new"], out["rate0s"] = t_new, rate0 * oHz
    return out


def uniform_along(st, axis):
    """a copy of the state whose tracers (every time level) do not vary along "x" or "y": the row j = 3 or the column
    in the middle of the tile, repeated"""
    v = st.copy()
    ref = v["t"][:, 3:4] if axis == "y" else v["t"][st.ni // 2:st.ni // 2 + 1]
    v["t"][:] = np.broadcast_to(ref, v["t"].shape).copy()
    return v


def water(st):
    """interior water points as a boolean array over (ni, nj, 1, 1)"""
    I, J = interior(st)
    w = np.zeros((st.ni, st.nj), dtype=bool)
    w[I, J] = True
    if st.p.masking:
        w &= st["rmask"] == 1.0
    return w[:, :, None, None]


def schedule(iic, nDIA, ntsDIA, ntstart, nrrec):
    """(initialise, accumulate): the IF conditions of set_diags.F:121-124 and :244, term for term"""
    if nDIA == 0:                                                    # set_diags.F:113
        return False, False
    ini = (((iic > ntsDIA) and ((iic - 1) % nDIA == 1)) or
           ((iic >= ntsDIA) and (nDIA == 1)) or
           ((nrrec > 0) and (iic == ntstart)))
    acc = (not ini) and (iic > ntsDIA)                               # ELSE IF
    return ini, acc


class DiaRef:
    """DiaTrc, avgzeta and rmask_dia of one tile: the numpy restatement of set_diags.F:126-190 and :246-317"""

    def __init__(self, b, wet, nDIA, ntsDIA, ntstart=1, nrrec=0):
        self.b, self.wet = b, bool(wet)
        self.sched = (nDIA, ntsDIA, ntstart, nrrec)
        ni, nj = b.UBi - b.LBi + 1, b.UBj - b.LBj + 1
        self.trc = {}
        self.avgzeta = np.zeros((ni, nj), order="F")
        self.cnt = np.zeros((ni, nj), order="F")
        self.I = slice(b.IstrR - b.LBi, b.IendR - b.LBi + 1)
        self.J = slice(b.JstrR - b.LBj, b.JendR - b.LBj + 1)

    def set_diags(self, iic, wrk, zeta_kout, rmask_full=None):
        """wrk: {(term, itrc): plane of DiaTwrk}; returns (initialise, accumulate)"""
        ini, acc = schedule(iic, *self.sched)
        I, J = self.I, self.J
        if not (ini or acc):
            return ini, acc
        m = rmask_full[I, J] if self.wet else None
        if self.wet:
            w = np.maximum(0.0, np.minimum(m, 1.0))
            self.cnt[I, J] = w if ini else self.cnt[I, J] + w
        z = zeta_kout[I, J]
        if ini:
            self.avgzeta[I, J] = z * m if self.wet else z
        else:
            self.avgzeta[I, J] = self.avgzeta[I, J] + (m * z if self.wet else z)
        for key, plane in wrk.items():
            a = self.trc.setdefault(key, np.zeros(plane.shape, order="F"))
            x = plane[I, J]
            if self.wet:
                x = m[:, :, None] * x
            a[I, J] = x if ini else a[I, J] + x
        return ini, acc
