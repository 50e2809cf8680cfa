"""Worker of the tiling-invariance test of set_data on the device (tests/test_gpu_set_data.py): one rank = one tile through
the HIP library, one roms_hip_set_data with gridded and open-boundary targets whose records are a function of the global
indices, halos over the gloo relay -- the rank harness of tests/tiling_util.py."""
import sys

import numpy as np

import tiling_util

SHAPE = dict(Lm=16, Mm=10, N=4)
GRIDDED = (("sustr", 0), ("svstr", 0), ("srflx", 0), ("stflux", 2), ("Tair", 0))
BRY = ("zeta_bry", "ubar_bry", "vbar_bry", "u_bry", "v_bry", "t_bry")
FIELDS = tuple(n for n, _ in GRIDDED) + BRY
RHO_GHOSTS = ("srflx", "stflux", "Tair") + BRY
SENTINEL = 777.25
TA, TB, TIME = 1000.0, 4000.0, 2234.5625


def tiled_state(variant, ntI=1, ntJ=1, tile=0):
    from roms_trunk_mgh_amd import ana
    ov = dict(SHAPE, EWperiodic=False) if variant == "basin" else dict(SHAPE)
    st = ana.make_tile("UPWELLING", ntI, ntJ, tile, perturb=1.0, overrides=ov)
    for name in FIELDS:
        st[name][:] = SENTINEL
    return st


def records(st):
    """data.Data whose records depend on the global indices only -- and, in the ghost points of a periodic direction, NOT
    on the wrapped index: the images must come from the exchange, not from the record"""
    from roms_trunk_mgh_amd import data
    b = st.b
    ii = np.arange(b.LBi, b.UBi + 1, dtype=np.float64)
    jj = np.arange(b.LBj, b.UBj + 1, dtype=np.float64)
    kk = np.arange(b.N, dtype=np.float64)
    D = data.Data(b)
    for q, (name, index) in enumerate(GRIDDED):
        for slot, T in ((1, TA), (2, TB)):
            D.load(name, slot, T, np.sin(0.37 * ii[:, None] + slot + q) * np.cos(0.23 * jj[None, :]) + 0.1 * q, index=index)
    for sd, side in enumerate(data.SIDES):
        along = jj if sd <= 1 else ii
        for q, name in enumerate(BRY):
            sh = data.record_shape(b, name, side)
            for slot, T in ((1, TA), (2, TB)):
                v = np.sin(0.41 * along + slot + q + 2 * sd)
                D.load(name, slot, T, v if len(sh) == 1 else v[:, None] + 0.01 * kk[None, :], index=2 if name == "t_bry" else 0, side=side)
    return D


def run(be, st):
    D = records(st)
    D.attach(be)
    be.set_data(TIME, 60.0)
    be.to_host(FIELDS)
    be.check_guards()
    return {name: st[name].copy() for name in FIELDS}


if __name__ == "__main__":
    with tiling_util.Rank(sys.argv) as rk:
        st = tiled_state(rk.args[0], rk.ntI, rk.ntJ, rk.rank)
        rk.save(st.b, run(rk.hip(st), st))
