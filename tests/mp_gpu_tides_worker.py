"""Worker of the tiling-invariance test of the tidal boundary forcing (tests/test_gpu_tides.py): one rank = one tile
through the HIP library under Main3D(tides=...), halos over the gloo relay or (variant "...+rccl", one rank) through RCCL
in loopback -- the rank harness and transports of tests/tiling_util.py."""
import sys

import tiling_util

SHAPE = dict(Lm=16, Mm=10, N=4, EWperiodic=False)
NSTEPS = 7
FIELDS = ("zeta_bry", "ubar_bry", "vbar_bry", "zeta", "ubar", "vbar", "u", "v", "t")


def tiled_state(variant, ntI=1, ntJ=1, tile=0):
    """(state, tides): the open basin; variant "ssh" = SSH_TIDES alone (the reduced-physics boundary value), otherwise
    SSH_TIDES + UV_TIDES"""
    import tides_util as tu
    from roms_trunk_mgh_amd import ana
    st = ana.make_tile("UPWELLING", ntI, ntJ, tile, perturb=1.0, overrides=dict(SHAPE))
    tu.open_all(st)
    td = ana.analytic_tides(st, ntc=3, mtc=4, uv="ssh" not in variant, tide_start=-0.2, ramp=True, dstart=-1.0)
    return st, td


def run(be, st, td):
    """NSTEPS steps with the tides on; {field: array}, the boundary arrays as the last step's call left them"""
    from roms_trunk_mgh_amd import main3d
    m = main3d.Main3D(be, tides=td)
    m.initial()
    m.run(NSTEPS)
    be.to_host()
    be.check_guards()
    return {name: st[name].copy() for name in FIELDS}


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        variant = rk.args[0]
        st, td = tiled_state(variant, rk.ntI, rk.ntJ, rk.rank)
        rk.save(st.b, run(rk.hip(st, rccl="rccl" in variant.split("+")), st, td))
