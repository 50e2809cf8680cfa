"""The helpers of the tiling tests (tests/tiling_util.py) have teeth: the comparison sees a changed owned point and a
changed rho ghost point and nothing else, the variant table sets what its options say and refuses what it does not know,
and spawn_ranks fails at once on a failed rank and leaves nothing running.  No GPU, no oracle."""
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest

import tiling_util as tu

LM, MM, NG, N = 7, 5, 2, 2


def _bounds(ntI=1, ntJ=1, tile=0):
    """the bounds of get_bounds.F for an even split of an E-W periodic LM x MM grid with NG ghost points, restated:
    7 = 4 + 3 columns, 5 = 3 + 2 rows; the R range takes in the boundary row at a physical (N-S) edge only"""
    it, jt = tile % ntI, tile // ntI
    ci, cj = -(-LM // ntI), -(-MM // ntJ)
    Istr, Iend = 1 + it * ci, min(LM, (it + 1) * ci)
    Jstr, Jend = 1 + jt * cj, min(MM, (jt + 1) * cj)
    return SimpleNamespace(Istr=Istr, Iend=Iend, Jstr=Jstr, Jend=Jend, IstrR=Istr, IendR=Iend,
                           JstrR=Jstr - (jt == 0), JendR=Jend + (jt == ntJ - 1),
                           LBi=Istr - NG, UBi=Iend + NG, LBj=Jstr - NG if jt else 0, UBj=Jend + NG if jt < ntJ - 1 else MM + 1,
                           Lm=LM, Mm=MM, NghostPoints=NG)


@pytest.fixture
def tiled(tmp_path):
    """global rho-type, u-type and 3-D rho-type arrays of distinct values, cut into 2 x 2 tile files"""
    gb = _bounds()
    shape = (gb.UBi - gb.LBi + 1, gb.UBj - gb.LBj + 1)
    want = {"zeta": 1.0 + np.arange(shape[0] * shape[1], dtype=float).reshape(shape),
            "ubar": 1000.0 + np.arange(shape[0] * shape[1], dtype=float).reshape(shape),
            "t": 5000.0 + np.arange(shape[0] * shape[1] * N, dtype=float).reshape(shape + (N,))}
    cut = []
    for r in range(4):
        b = _bounds(2, 2, r)
        I, J = slice(b.LBi - gb.LBi, b.UBi - gb.LBi + 1), slice(b.LBj - gb.LBj, b.UBj - gb.LBj + 1)
        cut.append((b, {k: v[I, J].copy() for k, v in want.items()}))
        tu.write_tile(tmp_path, r, b, cut[-1][1])
    return SimpleNamespace(path=tmp_path, gb=gb, want=want, cut=cut)


def _rewrite(tiled, rank, name, i, j):
    """tile `rank` again with the point (i, j) (global indices) of `name` changed"""
    b, arrays = tiled.cut[rank]
    arrays = {k: v.copy() for k, v in arrays.items()}
    arrays[name][i - b.LBi, j - b.LBj] += 0.5
    tu.write_tile(tiled.path, rank, b, arrays)


OWNED = pytest.mark.parametrize("owned", ["Istr:Iend", "IstrR:IendR"])
NAMES = ("zeta", "ubar", "t")


@OWNED
def test_equal_tiles_pass(tiled, owned):
    tu.assert_tiles_equal(tiled.path, 4, tiled.want, tiled.gb, NAMES, owned=owned, rho_ghosts=("zeta", "t"))
    seen = [(r, sorted(k for k in d if k not in tu.BOUNDS)) for r, d, _, _ in tu.tiles(tiled.path, 4, tiled.gb, owned)]
    assert seen == [(r, ["t", "ubar", "zeta"]) for r in range(4)]


@OWNED
@pytest.mark.parametrize("name", NAMES)
def test_changed_owned_point_names_field_and_rank(tiled, owned, name):
    b = tiled.cut[3][0]
    _rewrite(tiled, 3, name, b.Iend, b.Jstr)
    with pytest.raises(AssertionError) as e:
        tu.assert_tiles_equal(tiled.path, 4, tiled.want, tiled.gb, NAMES, owned=owned)
    assert f"field {name}, rank 3" in str(e.value) and "0.5" in str(e.value)
    tu.assert_tiles_equal(tiled.path, 4, tiled.want, tiled.gb, [n for n in NAMES if n != name], owned=owned)


@OWNED
@pytest.mark.parametrize("name", ["zeta", "t"])
def test_changed_rho_ghost_point_is_seen_only_in_rho_ghosts(tiled, owned, name):
    b = tiled.cut[2][0]
    _rewrite(tiled, 2, name, b.Iend + 2, b.Jstr - 1)          # a ghost point inside the grid: defined
    tu.assert_tiles_equal(tiled.path, 4, tiled.want, tiled.gb, NAMES, owned=owned)
    tu.assert_tiles_equal(tiled.path, 4, tiled.want, tiled.gb, NAMES, owned=owned, rho_ghosts=[n for n in ("zeta", "t") if n != name])
    with pytest.raises(AssertionError) as e:
        tu.assert_tiles_equal(tiled.path, 4, tiled.want, tiled.gb, NAMES, owned=owned, rho_ghosts=("zeta", "t"))
    assert f"field {name}, rank 2" in str(e.value) and "ghost" in str(e.value)


@OWNED
def test_changed_u_ghost_point_is_not_seen(tiled, owned):
    """today's behaviour, pinned: outside the owned range only the rho_ghosts are compared"""
    b = tiled.cut[0][0]
    _rewrite(tiled, 0, "ubar", b.Iend + 1, b.Jend + 1)
    tu.assert_tiles_equal(tiled.path, 4, tiled.want, tiled.gb, NAMES, owned=owned, rho_ghosts=("zeta", "t"))


def test_legacy_positional_bounds_are_read(tmp_path):
    b = _bounds(2, 2, 1)
    np.savez(os.path.join(tmp_path, "tile0.npz"), bounds=np.array([b.Istr, b.Iend, b.Jstr, b.Jend, b.LBi, b.LBj]), zeta=np.zeros((3, 3)))
    d = tu.read_tile(os.path.join(tmp_path, "tile0.npz"))
    assert [d[k] for k in ("Istr", "Iend", "Jstr", "Jend", "LBi", "LBj")] == [b.Istr, b.Iend, b.Jstr, b.Jend, b.LBi, b.LBj]
    assert "bounds" not in d and d["zeta"].shape == (3, 3)


# ----------------------------------------------------------------------------------------- the variant table --
def _adv(st):
    return sorted({int(v) for v in st.p.Hadv[:st.b.NT]}), sorted({int(v) for v in st.p.Vadv[:st.b.NT]})


# BENCHMARK_TINY and UPWELLING as ana.py ships them: two tracers, U3 (3) / C4 (1) advection, harmonic viscosity along
# s-surfaces, an E-W periodic channel of water with SPLINES_VDIFF and no closure, rivers or drying
DEFAULT = dict(NT=2, Hadv=3, Vadv=1, ts_dif4=0, uv_vis2=1, uv_vis4=0, EWperiodic=1, wet_dry=0, splines_vdiff=1,
               gls_mixing=0, masking=0, sources=False)
MPDATA, HSIMT = dict(NT=6, Hadv=6, Vadv=6), dict(Hadv=7, Vadv=7)
# every variant string of the suite (run options left out: they are the caller's): config, what differs from DEFAULT
VARIANTS = {"": ("BENCHMARK_TINY", {}),
            "mpdata": ("BENCHMARK_TINY", MPDATA),
            "hsimt": ("BENCHMARK_TINY", HSIMT),
            "mask": ("BENCHMARK_TINY", dict(masking=1)),
            "basin": ("UPWELLING", dict(EWperiodic=0)),
            "mpdata+basin+mask": ("BENCHMARK_TINY", dict(MPDATA, EWperiodic=0, masking=1)),
            "hsimt+basin+mask": ("BENCHMARK_TINY", dict(HSIMT, EWperiodic=0, masking=1)),
            "gls": ("UPWELLING", dict(gls_mixing=1)),
            "gls+basin+mask": ("BENCHMARK_TINY", dict(gls_mixing=1, EWperiodic=0, masking=1)),
            "my25": ("UPWELLING", dict(gls_mixing=2)),
            "my25+basin+mask": ("BENCHMARK_TINY", dict(gls_mixing=2, EWperiodic=0, masking=1)),
            # SEAMOUNT: one tracer, A4 (2) advection, no viscosity as shipped; geouv gives it visc2 = 50
            "geouv": ("SEAMOUNT", dict(NT=1, Hadv=2, Vadv=2, uv_vis2=2, visc2=50.0)),
            "geouv+basin+mask": ("BENCHMARK_TINY", dict(uv_vis2=2, EWperiodic=0, masking=1, visc2=5000.0)),
            # WET_DRY needs MASKING: without a mask option, a mask of water everywhere
            "geouv+wet": ("BENCHMARK_TINY", dict(uv_vis2=2, wet_dry=1, masking=1)),
            "wet": ("UPWELLING", dict(wet_dry=1, masking=1)),
            "wet+basin+mask": ("UPWELLING", dict(wet_dry=1, EWperiodic=0, masking=1)),
            "dif4": ("BENCHMARK_TINY", dict(ts_dif4=1, uv_vis4=1)),
            "dif4+basin+mask": ("BENCHMARK_TINY", dict(ts_dif4=1, uv_vis4=1, EWperiodic=0, masking=1)),
            "river": ("BENCHMARK_TINY", dict(sources=True)),
            "river+basin+mask": ("UPWELLING", dict(sources=True, EWperiodic=0, masking=1)),
            "river+mpdata+basin+mask": ("BENCHMARK_TINY", dict(MPDATA, sources=True, EWperiodic=0, masking=1)),
            "river+wells+basin+mask": ("UPWELLING", dict(sources=True, EWperiodic=0, masking=1)),
            "river+wells+mpdata": ("BENCHMARK_TINY", dict(MPDATA, sources=True)),
            "river+wells+wet+basin+mask": ("UPWELLING", dict(sources=True, wet_dry=1, EWperiodic=0, masking=1)),
            "classic": ("BENCHMARK_TINY", dict(splines_vdiff=0)),
            "classic+river+wells+basin+mask": ("UPWELLING", dict(splines_vdiff=0, sources=True, EWperiodic=0, masking=1)),
            "curv": ("UPWELLING", {}), "curveast": ("UPWELLING", {}),
            "dif4+edge": ("BENCHMARK_TINY", dict(ts_dif4=1, uv_vis4=1))}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variant_table_sets_what_the_old_tables_set(variant):
    config, differs = VARIANTS[variant]
    want = dict(DEFAULT, **differs)
    st = tu.make_variant_tile(config, variant)
    b, p = st.b, st.p
    assert b.NT == want["NT"] and _adv(st) == ([want["Hadv"]], [want["Vadv"]])
    assert int(b.EWperiodic) == want["EWperiodic"]
    for key in ("ts_dif4", "uv_vis2", "uv_vis4", "wet_dry", "splines_vdiff", "gls_mixing", "masking"):
        assert int(getattr(p, key)) == want[key], key
    assert bool(p.point_sources) == want["sources"]
    if "visc2" in want:
        assert float(st["visc2_r"].max()) == want["visc2"]
    if "mask" in variant:
        assert (st["rmask"] == 0.0).any()                      # the island
    # the changes after make_tile: curv_util touches the metrics, and only where the option says
    opts = set(variant.split("+"))
    straight = tu.make_variant_tile(config, "+".join(sorted(opts - {"curv", "curveast", "edge", ""})))
    differ = np.argwhere(st["pn"] != straight["pn"])
    assert bool(len(differ)) == bool(opts & {"curv", "curveast", "edge"})
    if "curveast" in opts:
        assert differ[:, 0].min() > st["pn"].shape[0] // 2     # in the eastern half only
    if "edge" in opts:                                         # column 30 of 64: Istr - 3 of the eastern of two tiles
        assert set(differ[:, 0]) == {30 - b.LBi}


def test_hsimt_replaces_what_mpdata_set():
    st = tu.make_variant_tile("BENCHMARK_TINY", "mpdata+hsimt")
    assert st.b.NT == 2 and _adv(st) == _adv(tu.make_variant_tile("BENCHMARK_TINY", "hsimt"))


def test_tile_arguments_reach_make_tile():
    st = tu.make_variant_tile("BENCHMARK_TINY", "mask", 2, 2, 3)
    full = tu.make_variant_tile("BENCHMARK_TINY", "mask")
    assert (st.b.Iend, st.b.Jend) == (full.b.Iend, full.b.Jend) and st.b.Istr > 1 and st.b.Jstr > 1


@pytest.mark.parametrize("variant", ["mpdta", "mask+bassin", "physics"])
def test_unknown_option_is_an_error(variant):
    with pytest.raises(ValueError, match="unknown option"):
        tu.make_variant_tile("BENCHMARK_TINY", variant)


def test_run_options_are_the_callers():
    assert tu.options("mask+physics+rccl", run_options=("physics", "rccl", "slim")) == {"mask", "physics", "rccl"}
    with pytest.raises(ValueError, match="rcl"):
        tu.options("mask+rcl", run_options=("physics", "rccl", "slim"))


# ------------------------------------------------------------------------------------------------ launching --
def test_spawn_ranks_fails_on_the_failed_rank_and_kills_the_rest(tmp_path):
    """rank 1 exits with 1 while rank 0 would sleep for a minute: the call fails within seconds and rank 0 is dead"""
    pidfile = os.path.join(tmp_path, "pid")
    child = ("import os, sys, time\n"
             "if sys.argv[1] == '1':\n"
             "    while not os.path.exists(sys.argv[4] + '.done'):\n"
             "        time.sleep(0.01)\n"
             "    sys.exit(1)\n"
             "open(sys.argv[4], 'w').write(str(os.getpid()))\n"
             "os.rename(sys.argv[4], sys.argv[4] + '.done')\n"
             "time.sleep(60)\n")
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match="rank 1"):
        tu.spawn_ranks(["-c", child], 2, [pidfile], timeout=30)
    assert time.monotonic() - t0 < 10.0
    pid = int(open(pidfile + ".done").read())
    with pytest.raises(ProcessLookupError):                  # killed and waited for: the pid is gone
        os.kill(pid, 0)


def test_spawn_ranks_returns_when_every_rank_exits_0():
    tu.spawn_ranks(["-c", "import sys; assert len(sys.argv) == 5 and sys.argv[2] == '3' and int(sys.argv[3]) > 0"], 3, ["x"],
                   timeout=30)
