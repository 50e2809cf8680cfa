"""Helpers of the climatology-nudging tests (tests/test_gpu_clima.py, tests/mp_gpu_clima_worker.py): states, runs through
the HIP library with and without a climatology, and the set-up both the one-tile run and the tile workers build."""
import numpy as np

import util
from roms_trunk_mgh_amd import abi, ana, clima, hip, main3d

NUDGED = ("ubar", "vbar", "u", "v", "t")


def same(a, b):
    """bit for bit (NaN == NaN: a field no kernel wrote may hold one in both runs)"""
    return np.array_equal(a, b, equal_nan=True)


def differing(st_a, st_b):
    return [name for name, _, _ in abi.FIELDS if not same(st_a[name], st_b[name])]


def run_hip(st0, calls=(), clima_=None, steps=0):
    """A copy of st0 through the HIP library: `steps` whole steps (main3d), then the listed (entry, indices) once each;
    ends with check_guards()."""
    st = st0.copy()
    st.clima = clima_
    be = hip.RomsHip(st)
    try:
        if steps:
            m = main3d.Main3D(be)
            m.initial()
            m.run(steps)
        for name, s in calls:
            be.call(name, s)
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    return st


def radnud(st, out=2.0e-4, fac=7.5, others=None):
    """Radiation + nudging for every variable on all four sides of a basin; boundary data around the initial state.
    obc_out = `out`, obc_in = fac * out (computed as the library computes it from obcfac); others = (out, in) for the
    five variables the climatology switches cover, where they are to differ from the free surface's."""
    st.p = type(st.p).from_buffer_copy(st.p)
    for sd in range(4):
        for var in ("zeta",) + NUDGED:
            st.p.lbc[sd][abi.LBV[var]] = abi.LBC["RadNud"]
            o, i = (out, fac * out) if (others is None or var == "zeta") else others
            st.p.obc_out[sd][abi.LBV[var]] = o
            st.p.obc_in[sd][abi.LBV[var]] = i
    rng = np.random.default_rng(5)
    for name in ("zeta_bry", "ubar_bry", "vbar_bry", "u_bry", "v_bry"):
        st[name][:] = 1.0e-2 * rng.standard_normal(st[name].shape)
    st["t_bry"][:] = st["t"][:, :, :, 0, :] * (1.0 + 1.0e-3 * rng.standard_normal(st["t_bry"].shape))
    return st


def random_clima(st, seed=11, coef=1.0, tracers=None, obcfac=7.5):
    """All three switches on: coefficients `coef` times a random positive field (dt * c < 0.5), climatology random."""
    b, p = st.b, st.p
    rng = np.random.default_rng(seed)
    ni, nj, N = st.ni, st.nj, b.N
    flags = np.ones(b.NT, dtype=np.int32) if tracers is None else np.asarray(tracers, dtype=np.int32)
    nc = int(flags.sum())
    r = lambda *sh: rng.random(sh)
    kw = dict(LnudgeM2CLM=True, M2nudgcof=coef * (0.05 + r(ni, nj)) * 0.4 / p.dt, ubarclm=0.1 * (r(ni, nj) - 0.5),
              vbarclm=0.1 * (r(ni, nj) - 0.5),
              LnudgeM3CLM=True, M3nudgcof=coef * (0.05 + r(ni, nj, N)) * 0.4 / p.dt, uclm=0.2 * (r(ni, nj, N) - 0.5),
              vclm=0.2 * (r(ni, nj, N) - 0.5), obcfac=obcfac)
    if nc:
        kw.update(LnudgeTCLM=flags, Tnudgcof=coef * (0.05 + r(ni, nj, N, nc)) * 0.4 / p.dt, tclm=5.0 + 20.0 * r(ni, nj, N, nc))
    return clima.Clima(b, **kw)


def tiled_state(config, variant, ntI=1, ntJ=1, tile=0):
    """The state of the tiling-invariance runs: all three switches on, the analytic sponge of ana.py towards every
    physical side, non-zero everywhere and varying in i, j and k.  variant: "" (the application's channel) or
    "basin" (no periodic direction, RadNud on all sides, island mask)."""
    if variant == "basin":
        st = ana.make_tile(config, ntI, ntJ, tile, perturb=1.0, overrides={"EWperiodic": False}, mask="island")
        radnud(st)
        # boundary data that are a function of the global indices (the random ones of radnud() are not)
        for name in ("zeta_bry", "ubar_bry", "vbar_bry", "u_bry", "v_bry"):
            st[name][:] = 0.0
        st["t_bry"][:] = st["t"][:, :, :, 0, :]
        ana.analytic_clima(st, sides=("west", "east", "south", "north"), width=5.0)
    else:
        st = ana.make_tile(config, ntI, ntJ, tile, perturb=1.0)
        ana.analytic_clima(st, sides=("south", "north"), width=5.0)
    return st
