"""Scenario of the multi-process CPU tests (tests/test_multitile_gloo.py, tests/test_masking.py): whole steps of the CPU
oracle on one tile of the variant table; as a worker, one rank of tests/tiling_util.py with the oracle's exchange hook."""
import sys

import tiling_util
from tiling_util import FIELDS


def tiled_state(config, variant, ntI=1, ntJ=1, tile=0):
    return tiling_util.make_variant_tile(config, variant, ntI, ntJ, tile)


def run(be, st, nsteps):
    from roms_trunk_mgh_amd import main3d
    m = main3d.Main3D(be)
    m.initial()
    m.run(nsteps)
    return {k: st[k] for k in FIELDS}


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        config, nsteps, variant = rk.args[0], int(rk.args[1]), rk.args[2]
        st = tiled_state(config, variant, rk.ntI, rk.ntJ, rk.rank)
        rk.save(st.b, run(rk.oracle(st), st, nsteps))
