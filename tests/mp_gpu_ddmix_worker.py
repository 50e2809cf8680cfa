"""Worker of the tiling-invariance tests of the KPP double-diffusive mixing (tests/test_gpu_ddmix.py): one rank = one
tile through the HIP library with LMD_DDMIX on, halos over the gloo relay -- the rank harness and transport of
tests/tiling_util.py.  Variant "kernels": rho_eos, then lmd_vmix, on temperature and salinity shaped by
ddmix_util.shape_ts; variant "steps": NSTEPS whole steps of Main3D(physics, bkpp, ddmix) on BENCHMARK_TINY."""
import sys

import tiling_util

SHAPE = dict(Lm=130, Mm=10, N=5)
NSTEPS = 10
NAMES = ["alfaobeta", "Akv", "Akt", "hsbl", "ghats"]


def tiled_state(variant, ntI=1, ntJ=1, tile=0):
    import ddmix_util as dd
    from roms_trunk_mgh_amd import ana
    if variant == "steps":
        return ana.make_tile("BENCHMARK_TINY", ntI, ntJ, tile, perturb=1.0)
    st = ana.make_tile("BENCHMARK_TINY", ntI, ntJ, tile, perturb=1.0, overrides=dict(SHAPE))
    dd.shape_ts(st)
    return st


def run(be, st, variant):
    """{name: array} of NAMES (and t after the whole steps)"""
    import util
    from roms_trunk_mgh_amd import main3d
    if variant == "steps":
        m = main3d.Main3D(be, physics=True, bkpp=True, ddmix=True)
        m.initial()
        m.run(NSTEPS)
    else:
        be.set_ddmix(True)
        s = util.step_idx()
        be.call("rho_eos", s)
        be.call("lmd_vmix", s)
    be.to_host(["Akv", "Akt", "hsbl", "ghats", "t"])
    out = {n: st[n].copy() for n in ("Akv", "Akt", "hsbl", "ghats", "t")}
    out["alfaobeta"] = be.get_kpp("alfaobeta")
    be.check_guards()
    return out


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        st = tiled_state(rk.args[0], rk.ntI, rk.ntJ, rk.rank)
        rk.save(st.b, run(rk.hip(st), st, rk.args[0]))
