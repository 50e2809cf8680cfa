"""Worker of the tiling-invariance test of the biology (tests/test_gpu_bio.py): one rank = one tile through the HIP
library with NPZD_POWELL on, halos over the gloo relay -- the rank harness and transport of tests/tiling_util.py."""
import sys

import tiling_util

SHAPE = dict(Lm=130, Mm=10, N=5)
NSTEPS = 5


def tiled_state(ntI=1, ntJ=1, tile=0):
    import numpy as np
    from roms_trunk_mgh_amd import ana, bio
    st = ana.make_tile("BENCHMARK_TINY", ntI, ntJ, tile, perturb=1.0, NT=6, overrides=dict(SHAPE))
    b = st.b
    bio.analytic_biology(st)
    # pools that differ from column to column and day beside night (functions of the global indices: the same on every tiling)
    ii = np.arange(b.LBi, b.UBi + 1, dtype=np.float64)[:, None]
    jj = np.arange(b.LBj, b.UBj + 1, dtype=np.float64)[None, :]
    x = 2.0 * np.pi * (np.mod(ii - 1.0, b.Lm) + 0.5) / b.Lm
    for q in range(4):
        st["t"][:, :, :, 0, b.NAT + q] *= (1.0 + 0.3 * np.sin((q + 1) * x) * np.cos(np.pi * (jj - 0.5) / b.Mm))[:, :, None]
    st["srflx"][:] = 5.0e-5 * (np.mod(ii - 1.0, b.Lm) % 9 < 6) + 0.0 * jj
    return st


def run(be, st):
    """NSTEPS whole steps with the biology on; {name: array}"""
    from roms_trunk_mgh_amd import bio, main3d
    m = main3d.Main3D(be, biology=bio.PowellPar(BioIter=2, wPhy=0.5))
    m.initial()
    m.run(NSTEPS)
    be.to_host(["t"])
    out = {"t": st["t"].copy()}
    be.check_guards()
    return out


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        st = tiled_state(rk.ntI, rk.ntJ, rk.rank)
        rk.save(st.b, run(rk.hip(st), st))
