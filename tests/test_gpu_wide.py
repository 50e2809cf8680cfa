"""-m gpu: parity on grids several workgroups wide in x, across every option family.

Every kernel is launched in 64 x 4 workgroups (BLK_X, BLK_Y of csrc/roms_dev.h).  The grids of the other parity tests
are one workgroup wide over Istr:Iend, so the seams between workgroups of the LDS halo tiles, the renumbering of
xcd_block() (gridDim.x a multiple of 8), the strip branch of decode_tile_tracer() (nbx >= 8, unequal strips and surplus
workgroups when nbx % 8 != 0) and decode_tile_level() only ran on the periodic, unmasked, default-option BENCHMARK
grids of tests/test_gpu_fullsize.py.  Here: four shapes that are wide and otherwise tiny (SHAPES; the geometry each is
chosen for is asserted, check_geometry), with land, dry cells, physical edges and point sources placed at the first
seam (columns Istr+62 .. Istr+66; asserted, check_seam).

  1. test_wide_kernels: single calls, HIP against the CPU oracle, 1e-12 of each field's maximum on every registered
     field (the bound of tests/test_basin.py), for every kernel family (FAMILIES) -- at w8 in every variant (VARIANTS),
     at w3, w10 and thin on the periodic island grid and on one basin variant (BASIN_OF).
     test_wide_clima: the climatology terms (the oracle has none): the null case and the numpy mirror of
     tests/test_gpu_clima.py.
  2. test_wide_runs: 10 whole steps with physics and diagnostics, 1e-10 relative RMS (test_gpu_fullsize._check_prognostic).
  3. test_wide_shift_equivariance: rolling every input by q columns rolls the result, bit for bit.

thin has N = 3.  pre_step3d, rhs3d_tile (so rhs3d) and step3d_t need N >= 4 -- their columns read k-1 .. k+2 -- and
refuse fewer levels (include/roms_hip.h); on thin the test asserts the refusal for them and parity for the others.

tests/test_wide_shapes.py checks the same states without a GPU: geometry, seam conditions, the oracle's calls finite
and not trivial."""
import numpy as np
import pytest

import clima_util as cu
import util
from roms_trunk_mgh_amd import abi, ana, main3d
from test_basin import OPEN, RADNUD, _open_all
from test_gpu_mpdata import MIXED

pytestmark = pytest.mark.gpu
BLK_X, BLK_Y = 64, 4                    # csrc/roms_dev.h
TOL = 1e-12
SHAPES = {"w3": dict(Lm=130, Mm=9, N=5), "w8": dict(Lm=500, Mm=6, N=4), "w10": dict(Lm=590, Mm=7, N=5),
          "thin": dict(Lm=66, Mm=3, N=3)}
CONFIG = {"w3": "UPWELLING", "w8": "UPWELLING", "w10": "BENCHMARK_TINY", "thin": "BENCHMARK_TINY"}
# periodic channel with the island; basin: closed / open edges and the island / radiation + nudging with RADIATION_2D
VARIANTS = ["island", "closed", "open_island", "radnud"]
BASIN_OF = {"w3": "closed", "w10": "open_island", "thin": "radnud"}      # the basin variant of the shapes other than w8
NEEDS_4_LEVELS = ("pre_step3d", "rhs3d_tile", "rhs3d", "step3d_t")
I0 = 1                                  # Istr of the one-tile grids


def shape_of(shape):
    """(dimensions, configuration) of a shape: a name of SHAPES, or that pair itself where the caller brings its own
    shape (tests/test_gpu_levels.py)"""
    return (SHAPES[shape], CONFIG[shape]) if isinstance(shape, str) else shape


def dims(shape):
    return shape_of(shape)[0]


def config_of(shape):
    return shape_of(shape)[1]
SEAM = range(I0 + 62, I0 + 67)          # the columns around the first seam (Istr+63 | Istr+64)
LAND_ROW = 2


def nblk(lo, hi, blk=BLK_X):
    return (hi - lo + 1 + blk - 1) // blk


def strips(nbx):
    """widths of the tile-column strips of the eight XCDs, decode_tile_tracer() with nbx >= 8"""
    return [(((x + 1) * nbx) >> 3) - ((x * nbx) >> 3) for x in range(8)]


def x_ranges(b):
    return {"interior": (b.Istr, b.Iend), "R": (b.IstrR, b.IendR), "T": (b.IstrT, b.IendT), "U-2:p2": (b.IstrU - 2, b.Iendp2),
            "allocated": (b.LBi, b.UBi)}


def check_geometry(shape, b):
    """The launch geometry the shape is there for, from the state's bounds."""
    sh = SHAPES[shape]
    assert (b.Lm, b.Mm, b.N) == (sh["Lm"], sh["Mm"], sh["N"]) and b.Istr == I0
    nbx = {k: nblk(*r) for k, r in x_ranges(b).items()}
    nby = nblk(b.Jstr, b.Jend, BLK_Y)
    live_x = b.Iend - b.Istr + 1 - BLK_X * (nbx["interior"] - 1)
    live_y = b.Jend - b.Jstr + 1 - BLK_Y * (nby - 1)
    if shape == "w3":
        assert set(nbx.values()) == {3} and live_x == 2 and nby == 3 and live_y == 1
    elif shape == "w8":
        assert set(nbx.values()) == {8}                                  # xcd_block() renumbers in every grid2d kernel
        assert strips(8) == [1] * 8                                      # the tracer decode: strips one tile wide
    elif shape == "w10":
        assert nbx["interior"] == 10 and all(v % 8 for v in nbx.values())        # xcd_block() is off
        w = strips(10)
        assert sum(w) == 10 and len(set(w)) > 1                          # unequal strips
        assert 8 * ((10 + 7) // 8) * nby > 10 * nby                      # grid_tile_tracer launches surplus workgroups
    else:
        assert b.Mm < BLK_Y and nby == 1 and set(nbx.values()) == {2} and live_x == 2 and b.N == 3
    return nbx


def check_seam(st, variant, wet=False):
    """No case passes vacuously: land (dry cells) and water on both sides of the first seam with u-faces of every mask
    value; in a basin the eastern edge in another workgroup than the western."""
    b = st.b
    cols = st.I(SEAM[0], SEAM[-1])
    rows = st.J(b.Jstr, b.Jend)
    if "island" in variant:
        assert st.p.masking == 1
        assert set(np.unique(st["rmask"][cols, rows])) == {0.0, 1.0}
        assert set(np.unique(st["umask"][cols, rows])) == {0.0, 1.0}
        for side in (st.I(SEAM[0], I0 + 63), st.I(I0 + 64, SEAM[-1])):           # land on either side of the seam
            assert (st["rmask"][side, rows] == 0.0).any() and (st["rmask"][side, rows] == 1.0).any()
    if wet:
        assert st.p.wet_dry == 1
        assert set(np.unique(st["rmask_wet"][cols, rows])) == {0.0, 1.0}
        assert {-1.0, 0.0, 1.0, 2.0} <= set(np.unique(st["umask_wet"][cols, rows]))
    if variant != "island":
        assert b.EWperiodic == 0 and (b.Iend - b.Istr) // BLK_X > 0
    else:
        assert b.EWperiodic == 1


# ---------------------------------------------------------------------------------------------- the states --
def seam_land(shape):
    return [(I0 + 63, LAND_ROW), (I0 + 64, LAND_ROW)]


def seam_dry(shape):
    row = 3 if dims(shape)["Mm"] > 3 else 1        # dry | wet | dry dry: u-faces -1, 1, 0 at Istr+62 .. Istr+64
    return [(I0 + 61, row), (I0 + 63, row), (I0 + 64, row)]


def _edges(st, variant):
    """the open / RadNud edges of tests/test_basin.py::_state with its boundary data"""
    if variant in ("open_island", "radnud"):
        _open_all(st, OPEN if variant == "open_island" else RADNUD)
        rng = np.random.default_rng(5)
        for name in ("zeta_bry", "ubar_bry", "vbar_bry", "u_bry", "v_bry"):
            st[name][:] = 1.0e-2 * rng.standard_normal(st[name].shape)
        st["t_bry"][:] = st["t"][:, :, :, 0, :] * (1.0 + 1.0e-3 * rng.standard_normal(st["t_bry"].shape))
        if variant == "radnud":
            st.p.radiation_2d = 1
    return st


def _kw(shape, variant, ov=None, wet=False):
    o = dict(dims(shape), **(ov or {}))
    if variant != "island":
        o["EWperiodic"] = False
    masked = "island" in variant
    return dict(overrides=o, mask="island" if masked else None, land=seam_land(shape) if masked else (),
                wet=wet, dry=seam_dry(shape) if wet else ())


def prepared(shape, variant, ov=None, NT=None, wet=False, config=None):
    st = util.prepared_state(config or config_of(shape), NT=NT, **_kw(shape, variant, ov, wet))
    return _edges(st, variant)


def tile(shape, variant, ov=None, NT=None, config=None):
    """ana.make_tile for the whole-step runs, with the seam's land"""
    kw = _kw(shape, variant, ov)
    st = ana.make_tile(config or config_of(shape), perturb=1.0, NT=NT, overrides=kw["overrides"], mask=kw["mask"])
    if kw["land"]:
        util.add_land(st, kw["land"])
    if variant in ("open_island", "radnud"):
        _open_all(st, OPEN if variant == "open_island" else RADNUD)
    return st


def _s(iic=5, iif=1, pred=0):
    return util.step_idx(iic=iic, iif=iif, pred=pred, knew=3 if pred else 2, krhs=1 if pred else 3)


S_INI = dict(iic=1, iif=1, pred=0, kstp=1, krhs=1, knew=1)


def _calls(kernel):
    if kernel == "step2d":                                   # the sequence of tests/test_basin.py
        return [(kernel, _s(5, 1, 1)), (kernel, _s(5, 2, 1)), (kernel, _s(5, 2, 0))]
    if kernel in ("ini_zeta", "ini_fields"):
        return [(kernel, util.step_idx(**S_INI))]
    return [(kernel, _s())]


def _mix_ov(config):
    return {"tnu2": 300.0} if config == "SEAMOUNT" else {"tnu2": 300.0, "visc2": 800.0}


def _detune(st):
    for name, f in (("Zt_avg1", 1.3), ("u", 1.1), ("v", 0.9), ("Huon", 1.05), ("Hvom", 0.95)):
        st[name] *= f


def _detune_forcing(st):
    st["stflux"][:, :, 0] += 1.0e-6
    st["Vwind"] += 0.3 * st["Uwind"] - 2.0
    st["rain"] += 2.0e-5
    if st.b.NT > 1:
        st["stflux"][:, :, 1] = 2.0e-8
        st["btflx"][:, :, 1] = 1.0e-9


def _base(label, shape, variant):
    ov = _mix_ov(config_of(shape)) if label in ("t3dmix2", "uv3dmix2", "rhs3d") else None
    st = prepared(shape, variant, ov)
    if label == "step3d_t":
        util.hz_weighted_tnew(st)
    if label in ("set_massflux", "omega", "set_depth", "set_zeta"):
        _detune(st)
    return st, _calls(label)


def _prsgrd(label, shape, variant):
    return prepared(shape, variant, {"pgf": label.split(":")[1]}), _calls("prsgrd")


DIF4 = {"UPWELLING": {"ts_dif4": 1, "uv_vis4": 1, "tnu4": 2.0e7, "visc4": 4.0e7},
        "BENCHMARK_TINY": {"ts_dif4": 1, "uv_vis4": 1, "tnu4": 1.0e10, "visc4": 2.0e10}}       # tests/test_gpu_biharmonic.py


def _dif4(label, shape, variant):
    st = prepared(shape, variant, DIF4[config_of(shape)])
    assert st.b.NghostPoints == 3 and st.p.uv_vis4 == 1
    return st, _calls(label.split(":")[0])


VISC4_GEO = {"UPWELLING": 4.0e7, "BENCHMARK_TINY": 2.0e10}      # tests/test_gpu_uvgeo4.py


def _geo(label, shape, variant):
    """MIX_GEO_UV: uv3dmix2_geo.h (":geo"), and uv3dmix4_geo.h as well ("uv3dmix4:geo", "rhs3d:geo4": uv_vis2 = uv_vis4 = 2,
    one CPP switch for both operators)"""
    kernel, opt = label.split(":")
    ov = {"uv_vis2": 2}
    if kernel == "uv3dmix4" or opt == "geo4":
        ov.update(uv_vis4=2, visc4=VISC4_GEO[config_of(shape)])
    st = prepared(shape, variant, ov)
    assert st.p.uv_vis2 == 2 and st.p.uv_vis4 == ov.get("uv_vis4", 0)
    assert st.b.NghostPoints == 3 or not st.p.uv_vis4
    return st, _calls(kernel)


def _iso(label, shape, variant):
    """tests/ref_worker.py::iso_state with TS_MIX_STABILITY and TS_MIX_MIN_STRAT: a weakly and a strongly stratified band
    of columns; nrhs = 3 and nstp = 1 distinct, so that the 1/4 part of the stability form counts"""
    import oracle
    ov = dict(DIF4[config_of(shape)], mix_iso_ts=1, tnu2=300.0, ts_mix_stability=1, ts_mix_min_strat=1)
    st = prepared(shape, variant, ov)
    assert st.p.mix_iso_ts == 1 and st.p.ts_mix_stability == 1 and st.p.ts_mix_min_strat == 1
    oracle.Oracle(st).call("rho_eos", util.step_idx())
    b, pd = st.b, st["pden"]
    mid = pd[:, :, b.N // 2][:, :, None]
    band = slice(b.Lm // 3 - b.LBi, b.Lm // 2 - b.LBi)
    pd[band] = mid[band] + 0.02 * (pd[band] - mid[band])
    strong = slice(b.Lm // 2 - b.LBi, 3 * b.Lm // 4 - b.LBi)
    pd[strong] = mid[strong] + 60.0 * (pd[strong] - mid[strong])
    return st, [(label.split(":")[0], util.step_idx(iic=5, nstp=1, nnew=2, nrhs=3))]


def _gls(label, shape, variant):
    kernel, gset = label.split(":")
    kw = _kw(shape, variant)
    st = util.gls_state(config_of(shape), gls=gset, mask=kw["mask"], extra=kw["overrides"], land=kw["land"])
    _edges(st, variant)
    if variant == "open_island":                             # tkebc: the tracers' condition, closed or gradient only
        for sd in range(4):
            st.p.lbc[sd][abi.LBV["t"]] = abi.LBC["Gra"]
    s = util.step_idx(iic=5)
    if kernel == "gls_corstep":                              # tests/test_gpu_gls.py::_hz_weight
        hzw = np.zeros_like(st["Akv"])
        hzw[:, :, 1:-1] = 0.5 * (st["Hz"][:, :, :-1] + st["Hz"][:, :, 1:])
        hzw[:, :, 0] = hzw[:, :, 1]
        hzw[:, :, -1] = hzw[:, :, -2]
        for n in ("tke", "gls"):
            st[n][:, :, :, s.nnew - 1] = hzw * st[n][:, :, :, s.nstp - 1]
    return st, [(kernel, s)]


SCHEMES = {"MPDATA": {"Hadv": "MPDATA", "Vadv": "MPDATA"}, "HSIMT": {"Hadv": "HSIMT", "Vadv": "HSIMT"}, "MIXED": MIXED}


def _adv3(label, shape, variant):
    kernel, scheme = label.split(":")
    st = prepared(shape, variant, SCHEMES[scheme], NT=6)
    assert st.b.NghostPoints == 3 and st.b.NT == 6
    if kernel == "step3d_t":
        util.hz_weighted_tnew(st)
    return st, _calls(kernel)


def _classic(label, shape, variant):
    kernel = label.split(":")[0]
    st = prepared(shape, variant, {"splines_vdiff": 0, "splines_vvisc": 0})
    if kernel == "step3d_t":
        util.hz_weighted_tnew(st)
    return st, _calls(kernel)


def _physics(label, shape, variant):
    if label.startswith("set_vbc"):
        drag = int(label.split(":")[1])
        st = prepared(shape, variant, {"uv_drag": drag})
        assert st.p.uv_drag == drag
        b = st.b
        ii = np.arange(b.LBi, b.UBi + 1, dtype=np.float64)[:, None] / b.Lm
        jj = np.arange(b.LBj, b.UBj + 1, dtype=np.float64)[None, :] / b.Mm
        st["ZoBot"][:] = 1.0e-4 * 10.0 ** (2.0 * ii + 1.5 * jj)           # tests/ref_worker.py::logdrag_state
        _detune_forcing(st)
        return st, _calls("set_vbc")
    if label == "bulk_flux":
        st = prepared(shape, variant, config="BENCHMARK_TINY")
        _detune_forcing(st)
        return st, _calls("bulk_flux")
    if label == "lmd_vmix":
        kw = _kw(shape, variant)
        st = util.kpp_state("BENCHMARK_TINY", mask=kw["mask"], overrides=kw["overrides"], land=kw["land"])
        return _edges(st, variant), [("lmd_vmix", util.step_idx())]
    st = prepared(shape, variant)
    _detune(st)
    return st, [("wvelocity", util.step_idx()), ("diag", util.step_idx())]


def _wet(label, shape, variant):
    """tests/test_gpu_wetdry.py: the kernels with a WET_DRY block on synthetic wet/dry masks that hold 0, 1, 2 and -1"""
    kernel = label.split(":")[0]
    st = prepared(shape, variant, _mix_ov("UPWELLING"), wet=True, config="UPWELLING")
    st["h"][st.I(7), st.J(2)] = 0.0
    if kernel.startswith("ini"):
        st["h"][:, :2][::3] = 0.16                           # shallow stretches so that the Dcrit floor of ini_zeta acts
    if kernel == "step2d":                                   # test_gpu_wetdry._prep2d
        b = st.b
        ii = np.arange(b.LBi, b.UBi + 1, dtype=np.float64)[:, None]
        jj = np.arange(b.LBj, b.UBj + 1, dtype=np.float64)[None, :]
        w = np.sin(2.0 * np.pi * 3 * ii / b.Lm + 0.4) * np.cos(np.pi * 2 * jj / b.Mm)
        for lev in range(2):
            st["rzeta"][:, :, lev] = (1.0 + 0.3 * lev) * 1.0e-2 * w
            st["rubar"][:, :, lev] = (1.0 - 0.2 * lev) * 3.0e-1 * w
            st["rvbar"][:, :, lev] = (1.0 + 0.1 * lev) * 2.0e-1 * np.roll(w, 5, axis=0)
        st["rufrc"][:] = 4.0e-1 * np.roll(w, 3, axis=0)
        st["rvfrc"][:] = 2.5e-1 * np.roll(w, 9, axis=0)
        st["h"][((ii // 4) % 3 == 0) & ((jj // 2) % 2 == 1)] = 0.16      # some cells fall dry in the call
        st["rmask_wet_avg"][:] = np.floor(3.0 * (1.0 + w))
    return st, _calls(kernel)


def seam_sources(shape):
    """(I, J, Dsrc, fraction): a u-face and a cell-centred source in the first column of the second workgroup, a v-face
    source in the last column of the first, a v-face and a cell-centred one further into the second; none on the seam's
    land or dry cells"""
    Mm = dims(shape)["Mm"]
    if Mm < 4:
        return [(I0 + 64, 1, 0, 0.5), (I0 + 63, 1, 1, 0.4), (I0 + 65, 1, 1, 0.3), (I0 + 64, 1, 2, 0.3), (I0 + 66, 3, 2, -0.2)]
    jm = Mm // 2 + 1
    return [(I0 + 64, jm, 0, 0.5), (I0 + 63, 1, 1, 0.4), (I0 + 65, 1, 1, 0.3), (I0 + 64, jm + 1, 2, 0.3), (I0 + 65, 1, 2, -0.2)]


def check_sources(src, b):
    wg = [((i - b.Istr) // BLK_X, (i - b.Istr) % BLK_X, int(d)) for i, d in zip(src.Isrc, src.Dsrc)]
    for d in (0, 1, 2):
        assert any(g > 0 and dd == d for g, _, dd in wg), (d, wg)
    assert any(loc in (0, BLK_X - 1) for _, loc, _ in wg), wg


def _sources(label, shape, variant):
    kernel = label.split(":")[0]
    wet = kernel == "wetdry"
    st = prepared(shape, variant, wet=wet, config="UPWELLING")
    src = util.river_sources(st, "walls", at=seam_sources(shape))
    check_sources(src, st.b)
    assert st.p.point_sources == 3
    q = src.qsrc()                                           # tests/test_gpu_sources.py::_prepared
    for n, (i, j, d) in enumerate(zip(src.Isrc, src.Jsrc, src.Dsrc)):
        if int(d) < 2:
            st["Huon" if int(d) == 0 else "Hvom"][st.I(i), st.J(j), :] = q[n]
    if kernel == "step3d_t":
        util.hz_weighted_tnew(st)
    return st, _calls(kernel)


FAMILIES = {
    "base": (_base, ["set_depth", "set_massflux", "omega", "set_zeta", "rho_eos", "prsgrd", "t3dmix2", "uv3dmix2", "rhs3d_tile",
                     "pre_step3d", "rhs3d", "step2d", "step3d_uv", "step3d_t", "set_vbc", "wvelocity", "ini_zeta",
                     "ini_fields", "step2d_loop"]),
    "prsgrd": (_prsgrd, ["prsgrd:STANDARD", "prsgrd:WJ_GRADP", "prsgrd:PJ_GRADP"]),         # prsgrd31 x 2, prsgrd40
    "dif4": (_dif4, ["t3dmix4:dif4", "uv3dmix4:dif4", "step2d:dif4"]),
    "geo": (_geo, ["uv3dmix2:geo", "rhs3d:geo", "uv3dmix4:geo", "rhs3d:geo4"]),
    "iso": (_iso, ["t3dmix2:iso", "t3dmix4:iso"]),
    "gls": (_gls, ["gls_prestep:k-epsilon", "gls_corstep:k-epsilon", "gls_prestep:my25", "gls_corstep:my25"]),
    "adv3": (_adv3, [k + ":" + sc for sc in ("MPDATA", "HSIMT", "MIXED") for k in ("pre_step3d", "step3d_t")]),
    "classic": (_classic, ["step3d_uv:classic", "step3d_t:classic"]),
    "physics": (_physics, ["set_vbc:1", "set_vbc:2", "set_vbc:3", "bulk_flux", "lmd_vmix", "wvelocity+diag"]),
    "wet": (_wet, [k + ":wet" for k in ("set_depth", "prsgrd", "t3dmix2", "uv3dmix2", "pre_step3d", "rhs3d", "step3d_uv",
                                        "ini_zeta", "ini_fields", "wetdry", "step2d")]),
    "sources": (_sources, [k + ":src" for k in ("step2d", "step3d_uv", "pre_step3d", "step3d_t", "rhs3d", "omega", "wetdry")]),
}


# the closure's boundary rule (tkebc) takes closed and gradient edges only: no RadNud variant
APPLIES = {"gls": ["island", "closed", "open_island"]}


def variants_of(fam, shape):
    """every variant that applies at w8; the periodic island grid and one basin variant at the other shapes"""
    ok = APPLIES.get(fam, VARIANTS)
    if shape == "w8":
        return ok
    return ["island", BASIN_OF[shape] if BASIN_OF[shape] in ok else "closed"]


def kernel_cases():
    out = []
    for fam, (_, labels) in FAMILIES.items():
        for shape in SHAPES:
            for variant in variants_of(fam, shape):
                for label in labels:
                    out.append(pytest.param(fam, label, shape, variant, id=f"{label}-{shape}-{variant}"))
    return out


def build(fam, label, shape, variant):
    st0, calls = FAMILIES[fam][0](label, shape, variant)
    check_geometry(shape, st0.b)
    check_seam(st0, variant, wet=bool(st0.p.wet_dry))
    return st0, calls


def run_calls(be, calls):
    """the calls on one backend (oracle or HIP); returns what the entries return beside the state"""
    out = []
    for kernel, s in calls:
        if kernel == "step2d_loop":
            out.append(be.step2d_loop(util.step_idx(iic=4), 1))
        elif kernel == "diag":
            out.append(be.diag(s))
        else:
            be.call(kernel, s)
    return out


def refused(shape, calls):
    return dims(shape)["N"] < 4 and any(k in NEEDS_4_LEVELS for k, _ in calls)


def run_oracle(st0, calls):
    import oracle
    st_o = st0.copy()
    return st_o, run_calls(oracle.Oracle(st_o), calls)


def vacuous_ok(label, variant):
    # Chapman / radiation edges: ini_zeta applies no condition (tests/test_basin.py)
    return label.startswith("ini_zeta") and variant in ("open_island", "radnud")


# ---------------------------------------------------------------------------- 1. single calls against the oracle --
@pytest.mark.parametrize("fam,label,shape,variant", kernel_cases())
def test_wide_kernels(fam, label, shape, variant):
    from roms_trunk_mgh_amd import hip
    st0, calls = build(fam, label, shape, variant)
    st_h = st0.copy()
    h = hip.RomsHip(st_h)
    try:
        if refused(shape, calls):
            with pytest.raises(RuntimeError, match="N >= 4"):
                run_calls(h, calls)
            return
        r_h = run_calls(h, calls)
        h.to_host()
        h.check_guards()
    finally:
        h.close()
    st_o, r_o = run_oracle(st0, calls)
    diffs = util.compare_states(st_h, st_o)
    print(label, shape, variant, "max relative differences:", diffs)
    assert all(v <= TOL for v in diffs.values()), diffs
    for a, o in zip(r_h, r_o):
        assert np.array_equal(a, o), (a, o)
    assert vacuous_ok(label, variant) or util.compare_states(st_o, st0), "kernel did not modify anything: test is vacuous"


def clima_state(shape, variant, entry):
    st0 = prepared(shape, variant, config="UPWELLING")
    if entry == "step3d_t":
        util.hz_weighted_tnew(st0)
    check_geometry(shape, st0.b)
    check_seam(st0, variant)
    return st0


def clima_cases():
    return [pytest.param(shape, variant, id=f"{shape}-{variant}") for shape in SHAPES
            for variant in (VARIANTS if shape == "w8" else ["island", BASIN_OF[shape]])]


@pytest.mark.parametrize("shape,variant", clima_cases())
def test_wide_clima(shape, variant):
    """The climatology terms of rhs3d, step2d and step3d_t (tests/test_gpu_clima.py; the oracle has none).  Momentum:
    random coefficients with uclm = u(nrhs), ubarclm = ubar(krhs) -- the difference the term multiplies is zero at every
    point, so the result equals the run without, bit for bit, unless climatology, coefficient and field are indexed
    apart (at a seam, say).  Tracers: t(nnew) = mask(t0 + (dt c)(tclm - t0)) on the whole R range, mirrored in numpy."""
    s3, sp, sc = util.step_idx(iic=5), util.step_idx(iic=5, iif=3, pred=1, kstp=2, knew=3, krhs=1), \
        util.step_idx(iic=5, iif=3, pred=0, kstp=1, knew=2, krhs=3)
    for entry, s in (("rhs3d_tile", s3), ("step2d", sp), ("step2d", sc)):
        if refused(shape, [(entry, s)]):
            continue
        st0 = clima_state(shape, variant, entry)
        b = st0.b
        c = cu.random_clima(st0)
        if variant == "radnud":          # the edges read tau from the coefficients: those of the parameters there
            inner = (st0.I(2, b.Lm - 1), st0.J(2, b.Mm - 1))
            keep = c["M2nudgcof"][inner].copy()
            c["M2nudgcof"][:] = 2.0e-4
            c["M2nudgcof"][inner] = keep
            for sd in range(4):          # obc_in as the library computes it from obcfac
                for var in cu.NUDGED:
                    st0.p.obc_in[sd][abi.LBV[var]] = c.obcfac * 2.0e-4
        if entry == "rhs3d_tile":
            c["uclm"][:] = st0["u"][:, :, :, s.nrhs - 1]
            c["vclm"][:] = st0["v"][:, :, :, s.nrhs - 1]
        else:
            c["ubarclm"][:] = st0["ubar"][:, :, s.krhs - 1]
            c["vbarclm"][:] = st0["vbar"][:, :, s.krhs - 1]
        a = cu.run_hip(st0, [(entry, s)])
        w = cu.run_hip(st0, [(entry, s)], c)
        assert cu.differing(a, w) == [], (entry, s.predictor_2d_step)
        assert cu.differing(a, st0) != []
    if refused(shape, [("step3d_t", s3)]) or variant == "radnud":      # (RadNud edges: tau itself changes with the arrays)
        return
    st0 = clima_state(shape, variant, "step3d_t")
    b, p, nnew = st0.b, st0.p, s3.nnew - 1
    c = cu.random_clima(st0, tracers=[0, 1])
    a = cu.run_hip(st0, [("step3d_t", s3)])
    w = cu.run_hip(st0, [("step3d_t", s3)], c)
    R = (st0.I(b.IstrR, b.IendR), st0.J(b.JstrR, b.JendR))
    assert cu.differing(a, w) == ["t"]
    assert cu.same(a["t"][:, :, :, nnew, 0], w["t"][:, :, :, nnew, 0])
    t0, tw = a["t"][:, :, :, nnew, 1][R], w["t"][:, :, :, nnew, 1][R]
    want = t0 + (p.dt * c["Tnudgcof"][R + (slice(None), 0)]) * (c["tclm"][R + (slice(None), 0)] - t0)
    if st0.p.masking:
        want = want * st0["rmask"][R][:, :, None]
    assert np.array_equal(tw, want), float(np.abs(tw - want).max())
    assert not np.array_equal(tw, t0)


# ------------------------------------------------------------------------------------------- 2. whole steps --
BEACH = {"wet_dry": 1, "beach": 1, "zeta_amp": 0.3}          # tests/test_gpu_wetdry.py
GEO4_RUN = {"uv_vis2": 2, "uv_vis4": 2, "visc4": VISC4_GEO["UPWELLING"]}
RUNS = {
    "w8-island": ("w8", "island", {}), "w8-open": ("w8", "open_island", {}),
    "w10-island": ("w10", "island", {}), "w10-open": ("w10", "open_island", {}),
    "w8-mpdata6": ("w8", "island", dict(ov=SCHEMES["MPDATA"], NT=6, config="BENCHMARK_TINY")),
    "w8-beach": ("w8", "island", dict(ov=BEACH, config="UPWELLING")),
    "w3-sources": ("w3", "closed", dict(config="UPWELLING")),
    # both viscosities rotated to geopotentials (uv_vis2 = uv_vis4 = 2): uv3dmix4_geo's two passes inside whole steps
    "w3-geo4-island": ("w3", "island", dict(ov=GEO4_RUN, config="UPWELLING")),
    "w3-geo4-open": ("w3", "open_island", dict(ov=GEO4_RUN, config="UPWELLING")),
}


def check_geo4_run(st):
    """a whole-step state of the rotated pair: both switches at 2 and, with prsgrd32 and lambda = 1, the momentum start
    fused into the pressure-gradient kernel (csrc/k_rhs3d.hip: rhs3d_fuses_uvstart) while uv3dmix4_geo runs"""
    assert (st.p.uv_vis2, st.p.uv_vis4) == (2, 2) and st.b.NghostPoints == 3
    assert st.p.pgf == abi.PGF["DJ_GRADPS"] and st.p.lambda_ == 1.0
    assert float(np.abs(st["visc4_r"]).max()) > 0.0 and float(np.abs(st["visc2_r"]).max()) > 0.0


def run_state(name):
    shape, variant, kw = RUNS[name]
    st = tile(shape, variant, **kw)
    check_geometry(shape, st.b)
    check_seam(st, variant)
    if name == "w3-sources":
        check_sources(util.river_sources(st, "walls", at=seam_sources(shape)), st.b)
    if "geo4" in name:
        check_geo4_run(st)
    return st


def run_steps(be, nsteps=10):
    m = main3d.Main3D(be, physics=True, diagnostics=True)
    m.initial()
    m.run(nsteps)
    return m


@pytest.mark.parametrize("name", list(RUNS))
def test_wide_runs(name):
    import oracle
    from roms_trunk_mgh_amd import hip
    from test_gpu_fullsize import _check_prognostic
    st_o = run_state(name)
    st_h = st_o.copy()
    be = hip.RomsHip(st_h)
    try:
        run_steps(be)
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    mo = run_steps(oracle.Oracle(st_o))
    _check_prognostic(st_h, st_o, mo)
    if name == "w8-beach":
        assert 0 < st_o["rmask_wet"].sum() < st_o["rmask_wet"].size
        for n in ("rmask_wet", "umask_wet", "vmask_wet", "pmask_wet"):
            assert np.array_equal(st_h[n], st_o[n]), n


# ------------------------------------------------------------------------- 3. placement independence --
def shift_state(shape):
    st = tile(shape, "island", ov=SCHEMES["MPDATA"], NT=6, config="BENCHMARK_TINY")
    check_geometry(shape, st.b)
    check_seam(st, "island")
    return st


@pytest.mark.parametrize("shape", ["w8", "w10"])
def test_wide_shift_equivariance(shape):
    """tests/test_gpu_fullsize.py::test_benchmark3_periodic_shift_equivariance with the island and MPDATA for six
    tracers: every input, masks included, rolled by q columns gives the rolled result bit for bit after 3 steps of hot
    path + wvelocity + diag (KPP stays out: lmd_finish_tile copies column Iend to Iend-1 whatever the periodicity).
    q = 1 and 37 move the seams over the data, q = 64 moves every cell to the next workgroup -- at w8, through the
    renumbering of xcd_block() and the one-tile strips, to another XCD."""
    from roms_trunk_mgh_amd import hip
    from test_gpu_fullsize import _roll_i
    names = ("zeta", "ubar", "vbar", "u", "v", "t", "wvel")

    def run(st):
        be = hip.RomsHip(st)
        try:
            m = main3d.Main3D(be, physics=False, diagnostics=True)
            m.initial()
            m.run(3)
            be.to_host()
        finally:
            be.close()
        return m
    st_a = _roll_i(shift_state(shape), 0)                    # ghost columns = periodic images
    b = st_a.b
    i0 = 1 - b.LBi
    rolled = {q: _roll_i(st_a, q) for q in (1, 37, 64)}
    for q, st_b in rolled.items():
        assert np.array_equal(np.roll(st_a["rmask"][i0:i0 + b.Lm], q, axis=0), st_b["rmask"][i0:i0 + b.Lm])
    da = run(st_a).last_diag
    assert float(np.abs(st_a["u"]).max()) > 1e-6 and np.isfinite(st_a["t"]).all()
    for q, st_b in rolled.items():
        db = run(st_b).last_diag
        for name in names:
            assert np.array_equal(np.roll(st_a[name][i0:i0 + b.Lm], q, axis=0), st_b[name][i0:i0 + b.Lm]), (q, name)
        assert da[5] == db[5] and da[10:12].tolist() == db[10:12].tolist()      # same Courant maximum, same (j, k)
        assert (int(da[9]) - 1 + q) % b.Lm + 1 == int(db[9])                    # ... q columns further east
