"""Worker of the tiling-invariance test of the climatology nudging (tests/test_gpu_clima.py): one rank = one tile of
clima_util.tiled_state through the HIP library, halos over the gloo relay or (variant "...+rccl", one rank) through
RCCL in loopback -- the rank harness and transports of tests/tiling_util.py."""
import sys

import tiling_util

FIELDS = ("zeta", "ubar", "vbar", "u", "v", "t", "Huon", "W", "Hz")


def tiled_state(config, variant, ntI=1, ntJ=1, tile=0):
    import clima_util
    return clima_util.tiled_state(config, "basin" if "basin" in variant.split("+") else "", ntI, ntJ, tile)


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
        config, nsteps, variant = rk.args[0], int(rk.args[1]), rk.args[2]
        st = tiled_state(config, variant, rk.ntI, rk.ntJ, rk.rank)
        rk.save(st.b, run(rk.hip(st, rccl="rccl" in variant.split("+")), st, nsteps))
