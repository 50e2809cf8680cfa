"""Worker of the tiling-invariance test of the tracer budget diagnostics (tests/test_gpu_diags.py): one rank = one tile
through the HIP library with the diagnostics on, halos over the gloo relay -- the rank harness and transport of
tests/tiling_util.py."""
import sys

import tiling_util

SHAPE = dict(Lm=130, Mm=10, N=5)
NDIA, NSTEPS = 3, 5                       # set_diags at iic = 1 .. 5: accumulate, initialise, accumulate, accumulate, initialise


def tiled_state(variant, ntI=1, ntJ=1, tile=0):
    from roms_trunk_mgh_amd import ana
    ov = dict(SHAPE)
    if "basin" in variant:
        ov["EWperiodic"] = False
    st = ana.make_tile("UPWELLING", ntI, ntJ, tile, perturb=1.0, overrides=ov)
    st["diff2"][:] = 40.0                 # UPWELLING ships tnu2 = 0: the iT?dif terms would all be zero
    return st


def run(be, st):
    """NSTEPS steps with the diagnostics on; {"wrk:term:itrc" | "trc:term:itrc" | "avgzeta": array}"""
    from roms_trunk_mgh_amd import diags, main3d
    m = main3d.Main3D(be, diags=diags.Diags(st.b, NDIA, 0))
    m.initial()
    m.run(NSTEPS)
    m.s.iic = m.iic                       # one more set_diags (accumulate): DiaTrc then holds the terms of the last two steps
    be.call("set_diags", m.s)
    out = {"avgzeta": be.get_diagnostic("avgzeta")}
    for name, idiag in diags.indices(st.p.ts_dif2).items():
        if name == "NDT":
            continue
        for it in range(1, st.b.NT + 1):
            out[f"wrk:{name}:{it}"] = be.get_diagnostic(name, it, False)
            out[f"trc:{name}:{it}"] = be.get_diagnostic(name, it, True)
    be.check_guards()
    return out


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        st = tiled_state(rk.args[0], rk.ntI, rk.ntJ, rk.rank)
        rk.save(st.b, run(rk.hip(st), st))
