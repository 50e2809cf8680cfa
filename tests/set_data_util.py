"""Helpers of the set_data tests (tests/test_set_data.py, tests/test_gpu_set_data.py, tests/mp_gpu_set_data_worker.py): a numpy
statement of the time interpolation of set_2dfld_tile (ROMS/Utility/set_2dfld.F:90-134; set_3dfld.F:94-146 and
set_ngfld.F:79-104 repeat it) with the lines cited, stated separately from roms_hip_set_data_factors, and of where
set_data_tile (ROMS/Nonlinear/set_data.F) puts each result in this repository's arrays."""
import numpy as np

from roms_trunk_mgh_amd import data as data_mod

SIDES = data_mod.SIDES


def anint(x):
    """Fortran ANINT: to the nearest whole number, halves away from zero"""
    x = np.float64(x)
    return np.copysign(np.floor(np.abs(x) + np.float64(0.5)), x)


def factors(time, dt, T1, T2, Tindex, onerec=False):
    """(fac1, fac2, synchro) of set_2dfld.F:90-141 for Tintrp(1:2) = T1, T2; None where the routine takes its error branch
    (:145).  Lonerec (:98): Fout = Finp(Tindex), written here as the weights 0 and 1."""
    time, dt = np.float64(time), np.float64(dt)
    Tintrp = {1: np.float64(T1), 2: np.float64(T2)}
    SecScale = np.float64(1000.0)                                        # :90
    it1 = 3 - Tindex                                                     # :91
    it2 = Tindex                                                         # :92
    fac1 = anint((Tintrp[it2] - time) * SecScale)                        # :93
    fac2 = anint((time - Tintrp[it1]) * SecScale)                        # :94
    if onerec:                                                           # :98
        return 0.0, 1.0, 0
    if fac1 * fac2 >= 0.0 and fac1 + fac2 > 0.0:                         # :116-117
        fac = np.float64(1.0) / (fac1 + fac2)                            # :118
        fac1 = fac * fac1                                                # :119
        fac2 = fac * fac2                                                # :120
        return float(fac1), float(fac2), int(time + dt > Tintrp[it2])    # :139
    return None


def interpolate(r, time, dt):
    """Fout of one key of a data.Data (whole record extents) and its synchro flag; ValueError = the error branch"""
    f = factors(time, dt, r["Tintrp"].get(1, 0.0), r["Tintrp"].get(2, 0.0), r["Tindex"], r["onerec"])
    if f is None:
        raise ValueError("exceeds ending value")
    fac1, fac2, syn = f
    it2 = r["Tindex"]
    it1 = 3 - it2
    if r["onerec"]:
        return r["slot"][it2], syn                                       # :102, :106
    return fac1 * r["slot"][it1] + fac2 * r["slot"][it2], syn            # :124, :128


def periodic_images(b, A, grid):
    """exchange_r2d / u2d / v2d _tile on one tile with E-W periodicity (exchange_2d.F:229-414), any trailing extents"""
    if not b.EWperiodic:
        return
    assert b.ntileI == 1
    j0 = (b.Jstr if grid == "v" else b.JstrR) - b.LBj
    j1 = b.JendR - b.LBj + 1
    I = lambda i: i - b.LBi
    for m in range(1, b.NghostPoints + 1):
        A[I(b.Lm + m), j0:j1] = A[I(m), j0:j1]
    for m in range(3):
        A[I(-m), j0:j1] = A[I(b.Lm - m), j0:j1]


def edge_points(b, name, side):
    """(index arrays of the points of the tile's array, slice of the record) an edge vector of target `name` is written
    to on `side`: the row or column of roms_fields.def's convention, over the reference's range (set_data.F:891-1215: from
    0, or from 1 for a v-type vector on a western / eastern and a u-type vector on a southern / northern edge, to Mm+1 /
    Lm+1) within the allocated extent; a western / eastern vector leaves the point it shares with a southern / northern
    one to that vector.  None where `side` is not a physical edge of the tile."""
    grid = data_mod.LINES[data_mod.DATA_ID[name]]["grid"]
    sd = SIDES.index(side)
    we, hi = sd <= 1, sd in (1, 3)
    if not (b.west_edge, b.east_edge, b.south_edge, b.north_edge)[sd] or (b.EWperiodic if we else b.NSperiodic):
        return None
    lb, ub = (b.LBj, b.UBj) if we else (b.LBi, b.UBi)
    first = (1 if grid == "v" else 0) if we else (1 if grid == "u" else 0)
    a0, a1 = max(lb, first), min(ub, (b.Mm if we else b.Lm) + 1)
    if we:
        fixed = b.Iend + 1 if hi else (b.Istr if grid == "u" else b.Istr - 1)
        # the points a southern / northern vector of this tile also maps to are that vector's (no condition reads them)
        if b.south_edge:
            a0 = max(a0, (b.Jstr if grid == "v" else b.Jstr - 1) + 1)
        if b.north_edge:
            a1 = min(a1, b.Jend)
    else:
        fixed = b.Jend + 1 if hi else (b.Jstr if grid == "v" else b.Jstr - 1)
    along = np.arange(a0, a1 + 1)
    rec = slice(a0 - lb, a1 - lb + 1)
    if we:
        return (np.full(along.shape, fixed - b.LBi), along - b.LBj), rec
    return (along - b.LBi, np.full(along.shape, fixed - b.LBj)), rec


def apply(st, D, time, dt, clima=None, bases=None):
    """set_data_tile on host arrays: every key of the data.Data `D` into st (a TileState), the climatology arrays of
    `clima` (a clima.Clima) and, where `bases` (dict name -> array: the sub-tidal bases of the ADD options) holds the
    boundary array's name, into that base.  All or nothing (ValueError).  Returns the synchro flag."""
    b, p = st.b, st.p
    out, synchro = [], 0
    for k, r in D.rec.items():
        if r["point"]:
            rr = dict(r, slot={s: np.float64(v) for s, v in r["slot"].items()})
            F, syn = interpolate(rr, time, dt)
        else:
            F, syn = interpolate(r, time, dt)
        synchro |= syn
        out.append((k, F))
    ir = slice(b.IstrR - b.LBi, b.IendR - b.LBi + 1)
    jr = slice(b.JstrR - b.LBj, b.JendR - b.LBj + 1)
    for (name, index, side), F in out:
        line = data_mod.LINES[data_mod.DATA_ID[name]]
        if line["dest"] != "DD_BRY":
            if line["dest"] == "DD_CLIMA":
                A = clima.arr[name][..., index - 1] if name == "tclm" else clima.arr[name]
            else:
                A = st[name][:, :, index - 1] if line["shape"] == "DS_2DT" else st[name]
            A[ir, jr] = F[ir, jr] if np.ndim(F) else F                   # set_2dfld.F:122-133: IstrR:IendR, JstrR:JendR
            periodic_images(b, A, line["grid"])                          # :170-185
            continue
        pts = edge_points(b, name, side)
        if pts is None:
            continue
        (ii, jj), rec = pts
        A = bases[name] if bases and name in bases else st[name]
        if name == "t_bry":
            A = A[:, :, :, index - 1]
        val = F[rec]
        if name == "zeta_bry" and p.wet_dry:                             # set_data.F:928-1003
            along, lo, hi_ = (jj + b.LBj, b.JstrR, b.JendR) if SIDES.index(side) <= 1 else (ii + b.LBi, b.IstrR, b.IendR)
            cff = p.Dcrit - st["h"][ii, jj]
            val = np.where((along >= lo) & (along <= hi_) & (val <= cff), cff, val)
        A[ii, jj] = val
    return synchro


def random_data(b, keys, T=(100.0, 400.0), Tindex=2, seed=3, onerec=False, scale=1.0):
    """A data.Data with two seeded random records per key (name, index, side); slot Tindex holds the later time."""
    rng = np.random.default_rng(seed)
    D = data_mod.Data(b)
    for name, index, side in keys:
        sh = data_mod.record_shape(b, name, side)
        for slot in (3 - Tindex, Tindex):
            D.load(name, slot, T[0] if slot != Tindex else T[1], scale * rng.standard_normal(sh), index=index, side=side, onerec=onerec)
    return D
