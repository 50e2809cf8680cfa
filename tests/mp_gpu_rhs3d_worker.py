"""Worker for tests/test_gpu_rhs3d_fused.py::test_tiling_invariance: one rank per tile (all on one GPU), halos through
the library's host-relay transport over gloo (the rank harness of tests/tiling_util.py).  One full step brings the fields
away from the initial state; then rhs3d ALONE runs on the rotated time indices and its outputs are saved."""
import sys

import tiling_util

OVERRIDES = {"tnu2": 300.0}
FIELDS = ("t", "u", "v", "ru", "rv", "rufrc", "rvfrc")


def rotated_geo(st):
    """UPWELLING mixes along s-surfaces; the fused path needs the rotated operator"""
    st.p = type(st.p).from_buffer_copy(st.p)
    st.p.mix_geo_ts, st.p.mix_s_ts = 1, 0
    return st


def tiled_state(config, ntI=1, ntJ=1, tile=0):
    from roms_trunk_mgh_amd import ana
    return rotated_geo(ana.make_tile(config, ntileI=ntI, ntileJ=ntJ, tile=tile, perturb=1.0, overrides=OVERRIDES))


def run(be, st):
    """one step, then rhs3d alone; {field: array} and nnew of the rotated indices"""
    import numpy as np
    from roms_trunk_mgh_amd import main3d
    m = main3d.Main3D(be)
    m.initial()
    m.run(1)
    m._rotate()
    be.call("rhs3d", m.s)
    be.to_host()
    return dict({k: st[k] for k in FIELDS}, nnew=np.array(m.s.nnew))


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        st = tiled_state(rk.args[0], rk.ntI, rk.ntJ, rk.rank)
        rk.save(st.b, run(rk.hip(st), st))
