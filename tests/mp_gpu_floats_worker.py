"""Worker of the tiling-invariance test of the Lagrangian floats (tests/test_gpu_floats.py): one rank = one tile through
the HIP library with floats set, halos and the floats' collection over the gloo relay or (variant "...+rccl", one rank)
through RCCL in loopback -- the rank harness and transports of tests/tiling_util.py."""
import sys

import numpy as np

import tiling_util

SHAPE = dict(Lm=128, Mm=10, N=5)
NFLOATS, NSTEPS = 197, 4


def tiled_state(variant, ntI=1, ntJ=1, tile=0):
    from roms_trunk_mgh_amd import ana
    ov = dict(SHAPE)
    if "basin" in variant:
        ov["EWperiodic"] = False
    return ana.make_tile("UPWELLING", ntI, ntJ, tile, perturb=1.0, overrides=ov)


def drifter(st):
    """197 floats released from a fresh (zero) track: next to every tile edge of the 2x2 and 4x1 splits and to the
    periodic seam, all three types, release before the start (never), on the first step, and after the end (never),
    out-of-grid releases at x < 0.5 and x >= Lm + 0.5"""
    from roms_trunk_mgh_amd import floats
    b = st.b
    n, Lm, Mm, N = NFLOATS, b.Lm, b.Mm, b.N
    rng = np.random.default_rng(11)
    x = 0.5 + Lm * rng.random(n)
    y = 1.0 + (Mm - 1.0) * rng.random(n)
    z = 0.2 + (N - 0.4) * rng.random(n)
    seams = [32.5, 64.5, 96.5, 0.5, Lm + 0.5]
    q = 0
    for sx in seams:
        for off in (-0.45, -0.01, 0.0, 0.01, 0.45):
            x[q] = min(max(sx + off, 0.5), Lm + 0.499)
            y[q] = (5.5 + off) if q % 2 else y[q]
            q += 1
    x[q], x[q + 1], y[q + 2] = 0.25, Lm + 0.5 + 1e-9, 0.25      # releases outside the grid
    q += 3
    z[q], z[q + 1] = N - 0.01, 0.01                             # within one step of the surface and of the bottom
    dt = st.p.dt
    tstr = np.zeros(n)
    tstr[5::7] = -10.0 * dt
    tstr[6::7] = 1000.0 * dt
    T = np.zeros((10, n), order="F")
    T[floats.itstr], T[floats.ixgrd], T[floats.iygrd], T[floats.izgrd] = tstr, x, y, z
    Ftype = 1 + np.arange(n) % 3
    ni, nj = b.UBi - b.LBi + 1, b.UBj - b.LBj + 1
    ii = np.arange(b.LBi, b.UBi + 1, dtype=float)[:, None] + np.zeros((1, nj))
    jj = np.arange(b.LBj, b.UBj + 1, dtype=float)[None, :] + np.zeros((ni, 1))
    return floats.Floats(b, Ftype, T, -1.0 - 20.0 * rng.random(n), 1000.0 * ii, 500.0 * jj)


def run(be, st):
    """NSTEPS steps with the floats on; (track, bounded)"""
    from roms_trunk_mgh_amd import main3d
    m = main3d.Main3D(be, floats=drifter(st))
    m.initial()
    m.run(NSTEPS)
    out = be.floats_get()
    be.check_guards()
    return out


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        variant = rk.args[0]
        st = tiled_state(variant, rk.ntI, rk.ntJ, rk.rank)
        track, bounded = run(rk.hip(st, rccl="rccl" in variant.split("+")), st)
        rk.save(st.b, dict(track=track, bounded=bounded))
