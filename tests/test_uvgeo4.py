"""The numpy restatement of the viscosity rotated to geopotentials (tests/uvgeo4_util.py) pinned without a GPU: it is
one of the two yardsticks of tests/test_gpu_uvgeo4.py for uv3dmix4_geo.h (UV_VIS4 + MIX_GEO_UV, roms_params_t.uv_vis4 =
2).  The other is the C oracle's uv3dmix4_geo (oracle/oracle_uvmix_geo.c), written separately; both are pinned bit for
bit to the reference built with the option (oracle/_ref/*_GEOUV4: tests/test_ref_pinning.py, and the fixture
tests/golden/ref_geouv4.npz in tests/test_golden.py), and to each other here."""
import numpy as np
import pytest

import util
import uvgeo4_util as G
from roms_trunk_mgh_amd import ana

EPS = np.finfo(np.float64).eps
VISC2 = {"SEAMOUNT": {"visc2": 50.0}}
VIS4 = {"UPWELLING": {"uv_vis4": 2, "visc4": 4.0e7}, "SEAMOUNT": {"uv_vis4": 2, "visc4": 1.0e8},
        "BENCHMARK_TINY": {"uv_vis4": 2, "visc4": 2.0e10}}          # the viscosities of tests/test_gpu_biharmonic.py
OUT = ("u", "v", "rufrc", "rvfrc")


def _idx():
    return util.step_idx(iic=5, iif=1, pred=0, knew=2, krhs=3)


@pytest.mark.parametrize("config", ["UPWELLING", "SEAMOUNT", "BENCHMARK_TINY"])
@pytest.mark.parametrize("variant", ["periodic", "closed", "mask", "wet"])
def test_harmonic_form_is_the_oracles(config, variant):
    """the level body with visc2, Hz inside the fluxes and the increment added is uv3dmix2_geo.h: identical bits to the
    oracle's uv3dmix2 at uv_vis2 = 2 (pinned to four reference builds), on the states of tests/test_gpu_uvgeo.py"""
    import oracle
    ov = {"uv_vis2": 2, **VISC2.get(config, {})}
    if variant == "closed":
        ov["EWperiodic"] = False
    st0 = util.prepared_state(config, overrides=ov, mask="island" if variant == "mask" else None, wet=(variant == "wet") or None)
    st_o, st_n = st0.copy(), st0.copy()
    s = _idx()
    oracle.Oracle(st_o).call("uv3dmix2", s)
    G.uv3dmix2_geo(st_n, s)
    for name in OUT:
        assert np.array_equal(st_n[name], st_o[name]), (name, float(np.abs(st_n[name] - st_o[name]).max()))
    assert not np.array_equal(st_o["u"], st0["u"]) and not np.array_equal(st_o["rvfrc"], st0["rvfrc"])


@pytest.mark.parametrize("config", ["UPWELLING", "SEAMOUNT", "BENCHMARK_TINY"])
@pytest.mark.parametrize("variant", ["periodic", "closed", "open", "mask", "mask_closed", "mask_open", "wet"])
def test_biharmonic_form_is_the_oracles(config, variant):
    """the two statements of uv3dmix4_geo.h -- numpy here, C in the oracle at uv_vis2 = uv_vis4 = 2 -- give identical bits
    on the states of tests/test_gpu_uvgeo4.py, BENCHMARK_TINY (which no reference build covers) and gradient conditions
    on a masked basin included; u, v, rufrc, rvfrc change and the oracle changes nothing else"""
    import oracle
    from roms_trunk_mgh_amd import abi
    ov = {"uv_vis2": 2, **VISC2.get(config, {}), **VIS4[config]}
    if variant.endswith(("closed", "open")):
        ov["EWperiodic"] = False
    st0 = util.prepared_state(config, overrides=ov, mask="island" if variant.startswith("mask") else None,
                              wet=(variant == "wet") or None)
    if variant.endswith("open"):
        for sd in ("west", "east", "south", "north"):
            for var in ("u", "v"):
                st0.p.lbc[abi.LBS[sd]][abi.LBV[var]] = abi.LBC["Gra"]
    st_o, st_n = st0.copy(), st0.copy()
    s = _idx()
    oracle.Oracle(st_o).call("uv3dmix4", s)
    G.uv3dmix4_geo(st_n, s)
    for name in OUT:
        assert np.array_equal(st_n[name], st_o[name]), (name, float(np.abs(st_n[name] - st_o[name]).max()))
    assert sorted(util.compare_states(st_o, st0)) == sorted(OUT)


@pytest.mark.parametrize("pair", [(1, 2), (2, 1)])
@pytest.mark.parametrize("kernel", ["uv3dmix2", "uv3dmix4", "rhs3d"])
def test_oracle_refuses_a_mixed_pair(pair, kernel):
    """MIX_GEO_UV is one switch for both operators: the oracle refuses (uv_vis2, uv_vis4) = (1, 2) and (2, 1) by name, as
    the device does, changes nothing, and never runs the s-surface operator in the rotated one's place"""
    import oracle
    st = util.prepared_state("UPWELLING", overrides=dict(VIS4["UPWELLING"], uv_vis2=2))
    st.p.uv_vis2, st.p.uv_vis4 = pair
    st0 = st.copy()
    with pytest.raises(RuntimeError) as e:
        oracle.Oracle(st).call(kernel, _idx())
    assert "MIX_GEO_UV" in str(e.value)
    assert util.compare_states(st, st0) == {}


def test_oracle_rotates_on_sloping_levels():
    """the oracle at uv_vis4 = 2 differs from uv_vis4 = 1 on SEAMOUNT: the s-surface operator is not what runs"""
    import oracle
    out = []
    for vis in (1, 2):
        st = util.prepared_state("SEAMOUNT", overrides=dict(VIS4["SEAMOUNT"], uv_vis2=0, uv_vis4=vis))
        s = _idx()
        oracle.Oracle(st).call("uv3dmix4", s)
        out.append(st["u"][:, :, :, s.nnew - 1].copy())
    assert util.max_rel_diff(out[1], out[0]) > 1e-9


def test_uniform_velocities_are_left_alone():
    """u and v uniform in space over the sloping levels of SEAMOUNT (uniform pm, pn): every gradient is exactly zero,
    so the biharmonic operator changes no bit of u(nnew), v(nnew), rufrc, rvfrc"""
    st0 = util.prepared_state("SEAMOUNT", overrides=VIS4["SEAMOUNT"])
    assert float(np.ptp(st0["pm"])) == 0.0 and float(np.ptp(st0["pn"])) == 0.0
    assert float(np.ptp(st0["z_r"][:, :, 0])) > 100.0
    s = _idx()
    st0["u"][:, :, :, s.nrhs - 1] = 0.125
    st0["v"][:, :, :, s.nrhs - 1] = -0.0625
    st = st0.copy()
    keep = {}
    G.uv3dmix4_geo(st, s, keep)
    for name in OUT:
        assert np.array_equal(st[name], st0[name]), name
    assert not keep["LapU"].any() and not keep["LapV"].any()


def _diagonal_state(Lm=14, Mm=9, N=6):
    """a closed rectangular basin (dx != dy) whose fields are functions of (i + j, k) -- see test_transposition"""
    st = util.prepared_state("SEAMOUNT", overrides=dict(VIS4["SEAMOUNT"], EWperiodic=False, Lm=Lm, Mm=Mm, N=N))
    b = st.b
    assert (b.Lm, b.Mm, b.N) == (Lm, Mm, N) and not b.EWperiodic
    d = (np.arange(b.LBi, b.UBi + 1, dtype=np.float64)[:, None] + np.arange(b.LBj, b.UBj + 1, dtype=np.float64)[None, :])
    H = 900.0 + 350.0 * np.sin(0.37 * d) + 11.0 * d
    kk = np.arange(1, N + 1, dtype=np.float64)[None, None, :]
    st["Hz"][:] = (H[:, :, None] / N) * (0.6 + 0.8 * kk / N)
    zw = np.concatenate([np.zeros_like(H)[:, :, None], np.cumsum(st["Hz"], axis=2)], axis=2) - st["Hz"].sum(axis=2)[:, :, None]
    st["z_r"][:] = 0.5 * (zw[:, :, :-1] + zw[:, :, 1:])
    for lev in range(2):
        st["u"][:, :, :, lev] = 0.2 * np.sin(0.41 * d + 0.3 + lev)[:, :, None] * (0.3 + kk / N)
        st["v"][:, :, :, lev] = 0.1 * np.cos(0.29 * d + 0.1 * lev)[:, :, None] * (1.3 - kk / N)
    st["rufrc"][:] = 1.0e-3 * np.sin(0.2 * d)
    st["rvfrc"][:] = 2.0e-3 * np.cos(0.3 * d)
    st["visc4_r"][:] = 1.0e4 * (1.0 + 0.1 * np.sin(0.5 * d))
    st["visc4_p"][:] = 1.0e4 * (1.0 + 0.1 * np.sin(0.5 * (d - 1.0)))
    st["pm"][:] = 1.0 / 4000.0
    st["pn"][:] = 1.0 / 2500.0
    for a, val in (("om_r", 4000.0), ("om_p", 4000.0), ("om_u", 4000.0), ("om_v", 4000.0),
                   ("on_r", 2500.0), ("on_p", 2500.0), ("on_u", 2500.0), ("on_v", 2500.0)):
        st[a][:] = val
    return st


SWAP = {"u": "v", "v": "u", "pm": "pn", "pn": "pm", "om_r": "on_r", "on_r": "om_r", "om_p": "on_p", "on_p": "om_p",
        "om_u": "on_v", "on_v": "om_u", "on_u": "om_v", "om_v": "on_u", "rufrc": "rvfrc", "rvfrc": "rufrc",
        "umask": "vmask", "vmask": "umask", "umask_wet": "vmask_wet", "vmask_wet": "umask_wet"}


def _transposed(st):
    b = st.b
    bt = ana.make_bounds(b.Mm, b.Lm, b.N, b.NT, b.NAT, 1, 1, 0, EWperiodic=False, NSperiodic=False, NghostPoints=b.NghostPoints)
    tt = st.copy()
    tt.b, tt.ni, tt.nj = bt, st.nj, st.ni
    assert (bt.UBi - bt.LBi + 1, bt.UBj - bt.LBj + 1) == (st.nj, st.ni)
    tt.arr = {}
    for name, a in st.arr.items():
        if a.ndim >= 2 and a.shape[:2] == (st.ni, st.nj):
            tt.arr[SWAP.get(name, name)] = np.asfortranarray(np.swapaxes(a, 0, 1))
        else:
            tt.arr[name] = a.copy(order="F")
    return tt


def test_transposition():
    """i <-> j, u <-> v, pm <-> pn (and the metrics accordingly) of a closed rectangular basin: the output is the
    transposed output, so a slip in one of the separately written u- and v-halves shows.

    u(nnew), v(nnew) and LapU, LapV: equal bits.  Negation and commuted two-term sums are exact; the statements whose
    association transposition does change are the four-term sums 0.25*(Hz + Hz + Hz + Hz) at psi-points and
    0.25*(dVdz + ...) / 0.25*(dUdz + ...) of the vertical fluxes, where it exchanges the values at (i-1, j+1) and (i, j)
    [or (i-1, j) and (i, j-1)].  The state's fields are functions of (i + j, k), for which those two are the same
    number, with dx != dy, u != v and walls on all four sides; a general state would differ in the last bits there.

    rufrc, rvfrc: `rufrc - cff1 - cff2 - cff3 - cff4` becomes `rvfrc + cff2 - cff1 - cff4 - cff3` against the
    reference's `rvfrc - cff1 + cff2 - cff3 - cff4`: 4 additions per level on either side, 8 N roundings in all, each
    at most eps/2 of a partial sum that |rufrc| + sum |cff| bounds."""
    st0 = _diagonal_state()
    s = _idx()
    a, ka = st0.copy(), {}
    G.uv3dmix4_geo(a, s, ka)
    t, kt = _transposed(st0), {}
    G.uv3dmix4_geo(t, s, kt)
    back = _transposed(t)
    assert not np.array_equal(a["u"], st0["u"]) and not np.array_equal(a["v"], st0["v"])
    assert np.array_equal(np.swapaxes(kt["LapV"], 0, 1), ka["LapU"]) and np.array_equal(np.swapaxes(kt["LapU"], 0, 1), ka["LapV"])
    for name in ("u", "v"):
        assert np.array_equal(back[name], a[name]), (name, float(np.abs(back[name] - a[name]).max()))
    N = st0.b.N
    for name in ("rufrc", "rvfrc"):
        mag = np.abs(st0[name]) + G.forcing_magnitude(st0, s)[name]          # bounds every partial sum
        bound = 8 * N * (EPS / 2) * mag
        d = np.abs(back[name] - a[name])
        print(name, "largest difference", float(d.max()), "largest bound", float(bound.max()))
        assert (d <= bound).all(), (name, float((d - bound).max()))


def _flat(config, variant):
    import oracle
    ov = dict(VIS4[config])
    if variant == "closed":
        ov["EWperiodic"] = False
    st = util.prepared_state(config, overrides=ov, mask="island" if variant == "mask" else None)
    st["h"][:] = float(st["h"].max())
    st["zeta"][:] = 0.0
    st["Zt_avg1"][:] = 0.0
    oracle.Oracle(st).call("set_depth", util.step_idx())
    return st


@pytest.mark.parametrize("config,variant", [("UPWELLING", "periodic"), ("UPWELLING", "closed"), ("SEAMOUNT", "periodic"),
                                            ("BENCHMARK_TINY", "periodic")])
def test_level_geopotentials_reduce_to_s_surfaces(config, variant):
    """Flat bottom and zeta = 0: z_r and Hz do not vary in i, j, every slope is exactly zero, the vertical fluxes vanish
    and uv3dmix4_geo.h states the operator of uv3dmix4_s.h (the oracle's uv3dmix4 at uv_vis4 = 1, pinned).  On an
    unmasked grid the two files agree on such a state: neither has Hz in the first operator's fluxes (the geo file
    divides only the vertical part, which is zero, by Hz), both have it inside the second operator's.  They round
    differently -- the geo file forms on_r*(0.5*pm*(..)) where the s file forms 0.5*pmon_r*(..), and
    on_r*on_r*visc4*cff where the s file has visc4 inside cff.

    Under MASKING they do NOT agree, so no masked case is here: the geo file multiplies the psi-point gradients by
    pmask and the psi-point flux by pmask again (uv3dmix4_geo.h:397, :557), the s file the flux only; pmask is 2 on a
    no-slip coast (gamma2 = -1).  Measured on masked BENCHMARK_TINY: 1.0e-5 in u next to the island.

    The bound.  The longer (geo) chain to u(nnew) has about 110 roundings: 6 per gradient, 18 per flux, 50 per operator,
    2 x 50 + 10 for the time step; with a factor of two of room 2 * 110 * eps/2 = 110 eps times a magnitude.  The
    roundings of the increment are relative to the terms it is made of, not to u(nnew) at the point -- where u crosses
    zero a bound by |u(nnew)| alone fails (measured: 2.8e-17 against 2.5e-17) -- and those terms come from the
    velocities of the whole stencil through an operator whose gain visc4^2 dt (pm^2 + pn^2)^2 is below 1 (asserted): the
    magnitude is the larger of the point's own value and the largest velocity of the field.  For rufrc, rvfrc it is the
    largest |rufrc| + sum over the levels of the flux magnitudes of the field (uvgeo4_util.forcing_magnitude: cff1 ..
    cff4 are differences of fluxes, and the roundings they inherit are relative to the fluxes; a bound by |cff1| + ..
    alone fails on BENCHMARK_TINY, 7.8e-13 against 3.5e-13).

    Measured (largest difference against the smallest bound; the excess is negative everywhere): UPWELLING u 2.8e-17
    against 5.4e-15, v 1.2e-17, rufrc 8.3e-14 against 2.4e-12, rvfrc 7.4e-14 against 2.7e-12; SEAMOUNT u 1.4e-17,
    rufrc 2.3e-13 against 6.8e-12; BENCHMARK_TINY u 1.4e-20, rufrc 7.8e-13 against 1.9e-12 (all printed)."""
    import oracle
    st0 = _flat(config, variant)
    b = st0.b
    T = (st0.I(b.IstrT, b.IendT), st0.J(b.JstrT, b.JendT))          # the points set_depth fills: all the operator reads
    assert float(np.ptp(st0["z_r"][T], axis=(0, 1)).max()) == 0.0 and float(np.ptp(st0["Hz"][T], axis=(0, 1)).max()) == 0.0
    gain = float((st0["visc4_r"] ** 2 * st0.p.dt * (st0["pm"] ** 2 + st0["pn"] ** 2) ** 2).max())
    assert 0.0 < gain < 1.0, gain
    s = _idx()
    st_g = st0.copy()
    G.uv3dmix4_geo(st_g, s)
    st_s = st0.copy()
    st_s.p = type(st0.p).from_buffer_copy(st0.p)
    st_s.p.uv_vis4 = 1
    oracle.Oracle(st_s).call("uv3dmix4", s)
    assert not np.array_equal(st_s["u"], st0["u"])
    vmax = max(float(np.abs(st0["u"]).max()), float(np.abs(st0["v"]).max()))
    mag = G.forcing_magnitude(st0, s)
    for name in OUT:
        a, b_ = st_g[name], st_s[name]
        scale = vmax if name in ("u", "v") else float((np.abs(st0[name]) + mag[name]).max())
        bound = 110.0 * EPS * np.maximum(np.maximum(np.abs(a), np.abs(b_)), scale)
        ex = np.abs(a - b_) - bound
        print(config, variant, name, "largest difference", float(np.abs(a - b_).max()), "bound", float(bound.min()), "excess", float(ex.max()))
        assert float(ex.max()) <= 0.0, (name, float(ex.max()))


def test_sloping_levels_differ_from_s_surfaces():
    """on SEAMOUNT the rotation acts: the restated geo result is more than 1e-9 relative from the s-surface one"""
    import oracle
    st0 = util.prepared_state("SEAMOUNT", overrides=VIS4["SEAMOUNT"])
    s = _idx()
    st_g = st0.copy()
    G.uv3dmix4_geo(st_g, s)
    st_s = st0.copy()
    st_s.p = type(st0.p).from_buffer_copy(st0.p)
    st_s.p.uv_vis4 = 1
    oracle.Oracle(st_s).call("uv3dmix4", s)
    assert util.max_rel_diff(st_g["u"][:, :, :, s.nnew - 1], st_s["u"][:, :, :, s.nnew - 1]) > 1e-9
    assert util.max_rel_diff(st_g["v"][:, :, :, s.nnew - 1], st_s["v"][:, :, :, s.nnew - 1]) > 1e-9
