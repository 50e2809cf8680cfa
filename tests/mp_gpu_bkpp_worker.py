"""Worker of the tiling-invariance test of the KPP bottom boundary layer (tests/test_gpu_bkpp.py): one rank = one tile
through the HIP library with LMD_BKPP on, halos over the gloo relay -- the rank harness and transport of
tests/tiling_util.py."""
import sys

import tiling_util

SHAPE = dict(Lm=130, Mm=10, N=5)
NSTEPS = 3


def tiled_state(variant, ntI=1, ntJ=1, tile=0):
    import numpy as np
    from roms_trunk_mgh_amd import ana
    ov = dict(SHAPE)
    if "basin" in variant:
        ov["EWperiodic"] = False
    st = ana.make_tile("BENCHMARK_TINY", ntI, ntJ, tile, perturb=1.0, overrides=ov)
    b = st.b
    # a slow rotation, a bottom current and a weak stratification (the temperature shrunk towards its bottom value), so
    # that the Ekman limit decides and the bottom layer spans levels and differs from column to column (functions of the
    # global indices: the same on every tiling)
    ii = np.arange(b.LBi, b.UBi + 1, dtype=np.float64)[:, None]
    jj = np.arange(b.LBj, b.UBj + 1, dtype=np.float64)[None, :]
    x = (np.mod(ii - 1.0, b.Lm) + 0.5) / b.Lm
    st["t"][:, :, :, :, 0] = st["t"][:, :, :1, :, 0] + 1.0e-3 * (st["t"][:, :, :, :, 0] - st["t"][:, :, :1, :, 0])
    st["f"][:] = 5.0e-6 * (1.0 + 0.5 * np.sin(2.0 * np.pi * x) * np.cos(np.pi * (jj - 0.5) / b.Mm))
    cur = 0.3 * (1.0 + 0.5 * np.cos(2.0 * np.pi * 2.0 * x)) * np.sin(np.pi * jj / (b.Mm + 1.0))
    if "basin" in variant:                # no flow through the western and eastern walls (u-points 1 and Lm + 1)
        cur = cur * np.sin(np.pi * (ii - 1.0) / b.Lm)
    st["u"][:] += cur[:, :, None, None]
    return st


def run(be, st):
    """NSTEPS whole steps with the physics and the bottom layer on; {name: array}"""
    from roms_trunk_mgh_amd import main3d
    m = main3d.Main3D(be, physics=True, bkpp=True)
    m.initial()
    m.run(NSTEPS)
    be.to_host(["Akv", "Akt", "hsbl"])
    out = {"hbbl": be.get_kpp("hbbl"), "kbbl": be.get_kpp("kbbl"), "ksbl": be.get_kpp("ksbl"),
           "Akv": st["Akv"].copy(), "Akt": st["Akt"].copy(), "hsbl": st["hsbl"].copy()}
    be.check_guards()
    return out


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        st = tiled_state(rk.args[0], rk.ntI, rk.ntJ, rk.rank)
        rk.save(st.b, run(rk.hip(st), st))
