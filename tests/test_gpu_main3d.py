"""-m gpu: whole hot-path parity.  100 baroclinic steps (each with the full
59-call barotropic loop) through the C ABI against the CPU oracle; the
north_star bound is 1e-10 relative RMS on zeta, ubar, vbar, u, v, T, S."""
import os

import numpy as np
import pytest

from roms_trunk_mgh_amd import abi, ana, hip, main3d
from roms_trunk_mgh_amd.state import rel_rms

pytestmark = pytest.mark.gpu
TOL = 1e-10
GEO4 = {"uv_vis2": 2, "uv_vis4": 2, "visc2": 50.0, "visc4": 1.0e8}      # tests/test_gpu_uvgeo4.py
# stated magnitudes for fields whose reference RMS is ~0 (SEAMOUNT is at rest
# up to the pressure-gradient error)
FLOOR = {"zeta": 1e-3, "ubar": 1e-4, "vbar": 1e-4, "u": 1e-4, "v": 1e-4, "t": 1e-3}


def _run(config, nsteps, perturb, physics=False, overrides=None):
    import oracle
    st_o = ana.make_tile(config, perturb=perturb, overrides=overrides)
    st_h = st_o.copy()
    mo = main3d.Main3D(oracle.Oracle(st_o), physics=physics, diagnostics=physics)
    mo.initial()
    mo.run(nsteps)
    be = hip.RomsHip(st_h)
    try:
        mh = main3d.Main3D(be, physics=physics, diagnostics=physics)
        mh.initial()
        mh.run(nsteps)
        be.to_host()
    finally:
        be.close()
    mo.hip_last_diag = mh.last_diag
    return st_h, st_o, mo


@pytest.mark.parametrize("config,perturb,physics", [("UPWELLING", 1.0, False), ("SEAMOUNT", 0.0, False),
                                                    ("BENCHMARK_TINY", 1.0, False),
                                                    # with bulk_flux + set_vbc recomputed every step on the device
                                                    ("BENCHMARK_TINY", 1.0, True), ("UPWELLING", 1.0, True),
                                                    # the reference's default pressure gradient (prsgrd31.h)
                                                    ("SEAMOUNT", 0.0, "STANDARD"), ("UPWELLING", 1.0, "WJ_GRADP"),
                                                    # the finite-volume pressure Jacobian (prsgrd40.h)
                                                    ("SEAMOUNT", 0.0, "PJ_GRADP"),
                                                    # both viscosities rotated to geopotentials (uv3dmix2_geo.h,
                                                    # uv3dmix4_geo.h) over the seamount's sloping levels
                                                    ("SEAMOUNT", 0.0, "GEO4")])
def test_100_steps(config, perturb, physics):
    ov = None
    if physics == "GEO4":
        ov, physics = GEO4, False
    elif isinstance(physics, str):
        ov, physics = {"pgf": physics}, False
    st_h, st_o, mo = _run(config, 100, perturb, physics, overrides=ov)
    if ov is GEO4:         # the rotated pair runs inside rhs3d with the momentum start fused into prsgrd32 (lambda = 1)
        assert (st_h.p.uv_vis2, st_h.p.uv_vis4) == (2, 2) and st_h.p.pgf == abi.PGF["DJ_GRADPS"] and st_h.p.lambda_ == 1.0
    s = mo.s
    out = {}
    out["zeta"] = rel_rms(st_h.interior("zeta")[..., mo.indx1 - 1], st_o.interior("zeta")[..., mo.indx1 - 1], FLOOR["zeta"])
    for name in ("ubar", "vbar"):
        out[name] = rel_rms(st_h.interior(name)[..., 0], st_o.interior(name)[..., 0], FLOOR[name])
    for name in ("u", "v"):
        out[name] = rel_rms(st_h.interior(name)[..., s.nnew - 1], st_o.interior(name)[..., s.nnew - 1], FLOOR[name])
    for it in range(st_o.b.NT):
        out[f"t{it+1}"] = rel_rms(st_h.interior("t")[..., s.nnew - 1, it], st_o.interior("t")[..., s.nnew - 1, it], FLOOR["t"])
    assert np.isfinite(st_o["t"]).all() and np.isfinite(st_h["t"]).all()
    print(config, perturb, physics, "relative RMS differences:", out)
    assert all(v <= TOL for v in out.values()), out
    # the run must have done something
    assert float(np.abs(st_o["u"]).max()) > 1e-6
    if physics:
        # diag of step 100 (wvelocity + diag ran every step, as main3d.F:314/475 do): energies and volume to the
        # tolerance of the fields; the Courant maximum is a max over nearly equal candidates, so only its value
        d_h, d_o = mo.hip_last_diag, mo.last_diag
        assert d_o is not None and d_o[1] > 0.0
        assert all(abs(d_h[q] - d_o[q]) <= 1e-9 * abs(d_o[q]) for q in (0, 1, 2, 3, 4, 5)), (d_h, d_o)


def test_20_steps_48_levels():
    """the whole step with N = 48 (register arrays of the column kernels in AGPRs)."""
    import oracle
    st_o = ana.make_tile("UPWELLING", perturb=1.0, overrides={"N": 48})
    st_h = st_o.copy()
    mo = main3d.Main3D(oracle.Oracle(st_o), physics=True)
    mo.initial()
    mo.run(20)
    be = hip.RomsHip(st_h)
    try:
        mh = main3d.Main3D(be, physics=True)
        mh.initial()
        mh.run(20)
        be.to_host()
    finally:
        be.close()
    s = mo.s
    for name in ("u", "v"):
        assert rel_rms(st_h.interior(name)[..., s.nnew - 1], st_o.interior(name)[..., s.nnew - 1], FLOOR[name]) <= TOL
    for it in range(st_o.b.NT):
        assert rel_rms(st_h.interior("t")[..., s.nnew - 1, it], st_o.interior("t")[..., s.nnew - 1, it], FLOOR["t"]) <= TOL


def test_async_snapshot():
    """a snapshot started after step 5 and collected after step 8 holds the state of step 5,
    whatever the steps in between did to the device fields."""
    names = ["zeta", "ubar", "vbar", "u", "v", "t"]
    st_a = ana.make_tile("BENCHMARK_TINY", perturb=1.0)
    st_b = st_a.copy()
    be = hip.RomsHip(st_a)
    try:
        m = main3d.Main3D(be, physics=True)
        m.initial()
        m.run(5)
        be.to_host(names)                      # synchronous reference copy of step 5
        want = {n: st_a[n].copy() for n in names}
    finally:
        be.close()
    be = hip.RomsHip(st_b)
    try:
        m = main3d.Main3D(be, physics=True)
        m.initial()
        m.run(5)
        be.snapshot_begin(names)
        m.run(3)                               # overwrites every snapshotted field on the device
        be.snapshot_end()
        got = {n: st_b[n].copy() for n in names}
        be.snapshot_begin(["zeta"])            # a second one reuses the staging buffers
        be.snapshot_end()
        be.to_host(["t"])
        assert not np.array_equal(st_b["t"], got["t"])         # the device had really moved on
    finally:
        be.close()
    for n in names:
        assert np.array_equal(got[n], want[n]), n
