"""Worker of the tiling-invariance test of the momentum advection schemes (tests/test_gpu_uvadv.py): one rank = one tile
of ana.make_tile under the scheme pair through the HIP library, halos over the gloo relay (the rank harness of
tests/tiling_util.py)."""
import sys

import tiling_util

FIELDS = ("zeta", "ubar", "vbar", "u", "v", "t", "Huon", "W", "Hz")


def tiled_state(config, hadv, vadv, ntI=1, ntJ=1, tile=0):
    from roms_trunk_mgh_amd import ana
    return ana.make_tile(config, ntI, ntJ, tile, perturb=1.0, overrides={"uv_hadv": hadv, "uv_vadv": vadv})


def run(be, st, nsteps):
    from roms_trunk_mgh_amd import main3d
    m = main3d.Main3D(be)
    m.initial()
    m.run(nsteps)
    be.to_host()
    be.check_guards()
    return {k: st[k] for k in FIELDS}


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        config, nsteps, hadv, vadv = rk.args[0], int(rk.args[1]), rk.args[2], rk.args[3]
        st = tiled_state(config, hadv, vadv, rk.ntI, rk.ntJ, rk.rank)
        rk.save(st.b, run(rk.hip(st), st, nsteps))
