"""Worker of the tiling-invariance test of the time-averaged fields (tests/test_gpu_avg.py): one rank = one tile through
the HIP library with averages selected, halos over the gloo relay or (variant "...+rccl", one rank) through RCCL in
loopback -- the rank harness and transports of tests/tiling_util.py."""
import sys

import tiling_util

SHAPE = dict(Lm=130, Mm=10, N=5)
NAVG, NSTEPS = 3, 4                       # the window closes at iic = 4
SELECT = [("avgzeta", 0), ("avgu2d", 0), ("avgv3d", 0), ("avgw3d", 0), ("avgAKv", 0), ("avgUV", 0), ("avgHuon", 0),
          ("avgt", 1), ("avgUT", 2), ("avgVT", 1), ("avgHvomT", 2)]


def tiled_state(variant, ntI=1, ntJ=1, tile=0):
    from roms_trunk_mgh_amd import ana
    ov = dict(SHAPE)
    if "basin" in variant:
        ov["EWperiodic"] = False
    return ana.make_tile("UPWELLING", ntI, ntJ, tile, perturb=1.0, overrides=ov)


def run(be, st):
    """NSTEPS steps with the averages on; {(name, itrc): array}"""
    import avg_util
    from roms_trunk_mgh_amd import main3d
    av = avg_util.averages_of(st.b, SELECT, nAVG=NAVG)
    m = main3d.Main3D(be, averages=av)
    m.initial()
    m.run(NSTEPS)
    out = {f"{n}:{it}": be.get_average(n, it) for n, it in SELECT}
    be.check_guards()
    return out


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        variant = rk.args[0]
        st = tiled_state(variant, rk.ntI, rk.ntJ, rk.rank)
        rk.save(st.b, run(rk.hip(st, rccl="rccl" in variant.split("+")), st))
