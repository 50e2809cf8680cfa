"""Scenario of the multi-tile GPU tests (tests/test_gpu_multitile.py, tests/test_gpu_rccl.py): whole steps of the HIP
library on one tile of the variant table; as a worker, one rank of tests/tiling_util.py over the gloo relay or (option
rccl) over RCCL."""
import sys

import numpy as np

import tiling_util
from tiling_util import FIELDS

RUN_OPTIONS = ("rccl", "physics", "slim")         # of the run, not of the state


def tiled_state(config, variant, ntI=1, ntJ=1, tile=0):
    return tiling_util.make_variant_tile(config, variant, ntI, ntJ, tile, run_options=RUN_OPTIONS)


def run(be, st, nsteps, variant):
    """nsteps steps; {field: array} and rowm = row_metrics_state()"""
    from roms_trunk_mgh_amd import main3d
    opts = tiling_util.options(variant, RUN_OPTIONS)
    m = main3d.Main3D(be, physics=("physics" in opts), diagnostics=("physics" in opts))
    m.initial()
    m.run(nsteps)
    rowm = be.row_metrics_state()
    be.to_host()
    out = {k: st[k] for k in FIELDS}
    if "slim" in opts:      # full-size grids: only the newest time level of the 3-D prognostic fields
        lev = m.s.nnew - 1
        out["u"], out["v"], out["t"] = st["u"][:, :, :, lev], st["v"][:, :, :, lev], st["t"][:, :, :, lev, :]
    return dict(out, rowm=np.array(rowm))


def single_tile(config, nsteps, variant):
    """the one-tile reference on a plain context, closed on return: (state, run()'s arrays)"""
    from roms_trunk_mgh_amd import hip
    st = tiled_state(config, variant)
    be = hip.RomsHip(st)
    try:
        return st, run(be, st, nsteps, variant)
    finally:
        be.close()


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        config, nsteps, variant = rk.args[0], int(rk.args[1]), rk.args[2]
        st = tiled_state(config, variant, rk.ntI, rk.ntJ, rk.rank)
        be = rk.hip(st, rccl="rccl" in tiling_util.options(variant, RUN_OPTIONS))
        rk.save(st.b, run(be, st, nsteps, variant))
