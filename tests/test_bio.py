"""CPU: the numpy restatement of npzd_Powell.h (tests/bio_util.py), the yardstick of tests/test_gpu_bio.py, pinned to closed
forms -- conservation and the one-line formulas of the reaction sweeps, the analytic cell average of the light, sinking
of a uniform profile, sinking over many cells and past the surface, the four outcomes of the positivity step -- and
shown to be continuous at every parity case; the table roms_bio.def through abi.py, the header and the Fortran module.
The restatement itself is pinned to the reference builds UPWELLING_BIO / UPWELLING_BIO_CPAR by tests/test_ref_pinning.py
and to their vectors (tests/golden/ref_bio.npz) by tests/test_golden.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bio_util as bu
from roms_trunk_mgh_amd import abi, bio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, RHO0 = 150.0, 1025.0


def _columns(seed=3, shape=(5, 4), N=12, low=0.05):
    rng = np.random.default_rng(seed)
    Hz = 0.5 + 4.0 * rng.random(shape + (N,))
    z_w = np.concatenate([np.zeros(shape + (1,)), np.cumsum(Hz, axis=-1)], axis=-1) - Hz.sum(axis=-1, keepdims=True)
    Hz = z_w[..., 1:] - z_w[..., :-1]
    pools = low + rng.random(shape + (N, 4)) * np.array([15.0, 2.0, 1.5, 1.0])
    return Hz, z_w, pools


# ------------------------------------------------------------------------------------------------ 1. reactions --
@pytest.mark.parametrize("iters", [1, 3])
def test_reactions_conserve_nitrogen(iters):
    Hz, z_w, pools = _columns()
    par = bio.PowellPar(BioIter=iters, wPhy=0.0, wDet=0.0, PhyMRN=0.05, ZooMRN=0.02, ZooEED=0.1)
    srflx = np.full(Hz.shape[:-1], 6.0e-5)
    tN = pools * Hz[..., None] * 1.01
    new = bu.npzd_powell(par, DT, RHO0, Hz, z_w, srflx, pools, tN)
    inc = (new - tN) / Hz[..., None]
    assert np.abs(inc).min() > 1e-9                                   # every pool of every cell moved
    # per cell the four increments cancel: each is a difference of numbers of the size of the pools (2^-53 relative
    # each), through about ten operations per sweep
    assert np.all(np.abs(inc.sum(axis=-1)) <= 64 * iters * 2.0 ** -53 * pools.sum(axis=-1))


def test_night_sweeps_match_their_formulas():
    Hz, z_w, pools = _columns(seed=4)
    par = bio.PowellPar(wPhy=0.0, wDet=0.0, PhyMRN=0.05, ZooMRN=0.02, ZooEED=0.1)
    new = bu.npzd_powell(par, DT, RHO0, Hz, z_w, np.zeros(Hz.shape[:-1]), pools, pools * Hz[..., None])
    got = new / Hz[..., None]
    d = DT / 86400.0
    N0, P0, Z0, D0 = (pools[..., q] for q in range(4))
    # no light: the uptake coefficient is exactly zero, nitrate and phytoplankton pass the first sweep unchanged
    g = Z0 * d * par.ZooGR * (1.0 - np.exp(-par.Ivlev * P0)) / P0
    P1 = P0 / (1.0 + g)
    Z1 = Z0 + P1 * (1.0 - par.ZooEEN - par.ZooEED) * g
    N1 = N0 + P1 * par.ZooEEN * g
    D1 = D0 + P1 * par.ZooEED * g
    P2 = P1 / (1.0 + d * par.PhyMRN + d * par.PhyMRD)
    N2, D2 = N1 + P2 * d * par.PhyMRN, D1 + P2 * d * par.PhyMRD
    Z2 = Z1 / (1.0 + d * par.ZooMRN + d * par.ZooMRD)
    N3, D3 = N2 + Z2 * d * par.ZooMRN, D2 + Z2 * d * par.ZooMRD
    D4 = D3 / (1.0 + d * par.DetRR)
    N4 = N3 + D4 * d * par.DetRR
    for q, want in enumerate((N4, P2, Z2, D4)):
        assert np.allclose(got[..., q], want, rtol=1e-13, atol=0.0), q
    L = bu.light(par, np.zeros(Hz.shape[:-1]), P0, z_w)
    assert np.all(L == 0.0)
    B = pools.copy()
    bu.reactions(par, d, B, L)
    uptake_only = bio.PowellPar(ZooGR=0.0, PhyMRD=0.0, ZooMRD=0.0, DetRR=0.0)
    B = pools.copy()
    bu.reactions(uptake_only, d, B, L)
    assert np.array_equal(B, pools)                                   # nitrate uptake exactly zero at night


# ---------------------------------------------------------------------------------------------------- 2. light --
def test_light_is_the_cell_average_of_the_exponential():
    Hz, z_w, _ = _columns(seed=5, N=20)
    par = bio.PowellPar()
    P = 0.8
    a = par.AttSW + par.AttPhy * P
    PARsur = np.full(Hz.shape[:-1], 120.0)
    L = bu.light(par, PARsur, np.full(Hz.shape, P), z_w)
    top = z_w[..., -1:]
    d1, d0 = top - z_w[..., 1:], top - z_w[..., :-1]                  # depth of the top and the bottom of each cell
    want = 120.0 * (np.exp(-a * d1) - np.exp(-a * d0)) / (a * (d0 - d1))
    assert np.allclose(L, want, rtol=1e-12, atol=0.0)


# -------------------------------------------------------------------------------------------------- 3. sinking --
def test_sinking_of_a_uniform_profile_inside_the_cell_below():
    Hz, z_w, _ = _columns(seed=6, N=15)
    q, cff = 0.7, 0.4                                                 # cff < the thinnest Hz (0.5)
    assert cff < Hz.min()
    new, FC0, ks = bu.sink_column(Hz, z_w, np.full(Hz.shape, q), cff)
    assert np.array_equal(ks, np.broadcast_to(np.arange(1, 16), ks.shape))
    # rounding: (z_w + cff) - z_w is off by up to two roundings at the size of z_w, the products of the flux by four at
    # the size of the flux; a cell takes the difference of two fluxes times 1 / Hz and one more rounding at the size of q
    eps = 2.0 ** -53
    dFC = q * (2.0 * eps * np.abs(z_w).max() + 4.0 * eps * cff)
    dq = 2.0 * dFC / Hz.min() + 2.0 * eps * q
    assert np.abs(new[..., :-1] - q).max() <= dq                      # every cell below the top: what enters leaves
    assert np.abs(new[..., -1] - (q - q * cff / Hz[..., -1])).max() <= dq
    assert np.abs(FC0 - q * cff).max() <= dFC


@pytest.mark.parametrize("cff", [11.0, 1000.0], ids=["several-cells", "taller-than-the-column"])
def test_sinking_far_past_one_cell(cff):
    Hz, z_w, _ = _columns(seed=7, N=18)
    assert cff > 3 * Hz.max() - 3.0 and (cff < Hz.sum(axis=-1).min() or cff > Hz.sum(axis=-1).max())
    k = np.arange(18, dtype=np.float64)
    # decreasing towards the surface, which supplies nothing (FC(N) = 0): the profile that can stay monotone
    qc = np.broadcast_to(3.2 - 0.1 * k - 0.004 * k * k, Hz.shape).copy()
    new, FC0, ks = bu.sink_column(Hz, z_w, qc, cff)
    before, after = (qc * Hz).sum(axis=-1), (new * Hz).sum(axis=-1)
    # rounding: a flux is a sum of up to 18 products of the size of the column inventory (2^-53 relative each); a cell
    # takes the difference of two fluxes times 1 / Hz
    dFC = 32 * 2.0 ** -53 * before.max()
    dq = 2.0 * dFC / Hz.min()
    assert np.abs(before - after - FC0).max() <= dFC                  # the inventory falls by exactly FC(0)
    assert (ks > np.arange(1, 19) + 2).any() and new.min() >= -dq     # nothing goes negative
    if cff > Hz.sum(axis=-1).max():                                   # everything left through the open bottom
        assert np.all(ks == 18) and np.abs(FC0 - before).max() <= dFC and np.abs(new).max() <= dq
    else:
        assert np.all(np.diff(new, axis=-1) <= 2.0 * dq)              # a monotone profile stays monotone
        assert (np.diff(new, axis=-1) < -2.0 * dq).any() and (ks < 18).any()


# ----------------------------------------------------------------------------------------------- 5. positivity --
def test_positivity_outcomes():
    M = bu.MINVAL
    v = np.array([[5.0, 1.0, 0.5, 0.2],                               # no negatives
                  [5.0, -0.3, 0.5, -0.1],                             # the deficit comes out of the largest pool
                  [3.0e-7, -2.0e-7, 1.0e-7, 5.0e-7],                  # the largest pool is too small: nothing is deducted
                  [2.0, -0.5, 2.0, 0.1]])                             # equal largest pools: the first pays
    got = bu.positive(v)
    assert np.array_equal(got[0], v[0])
    deficit = (M + 0.3) + (M + 0.1)
    assert np.array_equal(got[1], [5.0 - deficit, M, 0.5, M])
    assert np.array_equal(got[2], [M, M, M, M])
    assert np.array_equal(got[3], [2.0 - (M + 0.5), M, 2.0, 0.1])
    # t(nnew) * Hz_inv goes through the same step and nothing of it reaches the result (:256-260)
    Hz, z_w, pools = _columns(seed=8)
    par = bio.PowellPar()
    sr = np.full(Hz.shape[:-1], 5.0e-5)
    tN = pools * Hz[..., None]
    a = bu.npzd_powell(par, DT, RHO0, Hz, z_w, sr, pools, tN)
    b = bu.npzd_powell(par, DT, RHO0, Hz, z_w, sr, pools, -tN)
    assert np.allclose(a - tN, b + tN, rtol=1e-12, atol=0.0)


# -------------------------------------------------------------------------------------------------- 6. no jumps --
@pytest.mark.parametrize("case", bu.PARITY_CASES, ids=bu.case_id)
def test_no_parity_point_sits_on_a_jump(case):
    """Every input of the parity case moved by a relative 1e-13 (random signs): the result moves by less than 1e-10 of
    each field's maximum, so no branch of the limiters, weights, cu or the departure search decides a compared cell."""
    grid, mask, pset = case
    st = bu.bio_state(grid, mask)
    par = bu.params(pset, st.p.dt)
    rng = np.random.default_rng(11)
    base = bu.expected(st, par)
    moved = bu.expected(st, par, perturb=lambda shape: 1.0 + 1.0e-13 * rng.choice([-1.0, 1.0], size=shape))
    I = bu.interior(st.b)
    for q, itrc in enumerate(par.tracers(st.b)):
        a, b = base[I][:, :, :, 1, itrc - 1], moved[I][:, :, :, 1, itrc - 1]
        ratio = np.abs(a - b).max() / np.abs(a).max()
        print(f"{bio.POOLS[q]}: {ratio:.3e}")
        assert ratio < 1.0e-10, (bio.POOLS[q], ratio)


# ------------------------------------------------------------------------------------------ 7. table and struct --
def test_table_round_trips(tmp_path):
    members = abi.STRUCTS["roms_bio_powell_t"]
    assert [n for _, n, _ in members] == bio.MEMBERS and len(members) == 21
    assert [(t, e) for t, n, e in members if n == "idbio"] == [("int", (4,))]
    assert ctypes.sizeof(abi.BioPowell) == 6 * 4 + 18 * 8
    (tmp_path / "off.c").write_text("""#include <stddef.h>
#include <stdio.h>
#include "roms_hip.h"
#define ROMS_MEMBER(type, name) printf(#type " " #name " %zu %zu\\n", offsetof(roms_bio_powell_t, name), sizeof(((roms_bio_powell_t *)0)->name));
#define ROMS_MEMBER_A(type, name, n) ROMS_MEMBER(type, name)
int main(void)
{
  printf("struct %zu\\n", sizeof(roms_bio_powell_t));
#include "roms_bio.def"
  return 0;
}
""")
    r = subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "off.c", "-o", "off"],
                       cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(tmp_path / "off")], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].split() == ["struct", "168"]
    got = [(w[0], w[1], int(w[2]), int(w[3])) for w in (ln.split() for ln in out[1:])]
    want = []
    for name, t in abi.BioPowell._fields_:
        f = getattr(abi.BioPowell, name)
        while hasattr(t, "_length_"):
            t = t._type_
        want.append(({ctypes.c_int: "int", ctypes.c_double: "double"}[t], name, f.offset, f.size))
    assert got == want
    # the defaults are the values the table documents, and the model ids are the header's and the Fortran module's
    blk = bio.PowellPar().c_struct(type("B", (), {"NAT": 2, "NT": 6})())
    assert list(blk.idbio) == [3, 4, 5, 6] and blk.wDet == 8.0 and blk.BioIter == 1 and blk.Cp == 3985.0
    assert abi.BIO_MODEL == {"NONE": 0, "NPZD_POWELL": 1, "NPZD_FRANKS": 2, "NPZD_IRON": 3, "FENNEL": 4, "NEMURO": 5,
                             "ECOSIM": 6, "HYPOXIA_SRM": 7, "RED_TIDE": 8}
    src = open(os.path.join(ROOT, "roms_trunk_mgh_amd", "fortran", "roms_hip_mod.F90")).read()
    fort = {n: int(v) for n, v in re.findall(r"\bROMS_BIO_(\w+) = (\d+)", src)}
    assert fort == abi.BIO_MODEL
    assert "roms_hip_set_biology" in src and "roms_hip_biology" in src


def test_analytic_biology_fills_time_level_one():
    from roms_trunk_mgh_amd import ana
    st = ana.make_tile("UPWELLING", NT=6)
    before = st["t"].copy()
    bio.analytic_biology(st)
    for q, value in enumerate(bio.BIO_INI):
        assert np.all(st["t"][:, :, :, 0, 2 + q] == value)
    assert np.array_equal(st["t"][..., :2], before[..., :2]) and np.array_equal(st["t"][:, :, :, 1:, :], before[:, :, :, 1:, :])
    with pytest.raises(ValueError):
        bio.analytic_biology(ana.make_tile("UPWELLING"))
