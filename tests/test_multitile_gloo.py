"""CPU, multi-process: the N>1 path.  The oracle runs one tile per process
(world_size 2 and 4, gloo) with the halo-exchange protocol of mp_exchange.F
restated in roms_trunk_mgh_amd/halo.py; after 3 full steps every tile's owned
points AND ghost points must equal the single-tile run bit for bit -- the
reference's own acceptance rule ("identical results across tilings")."""
import os
import subprocess
import sys

import pytest

import mp_worker as worker
import tiling_util

HERE = os.path.dirname(os.path.abspath(__file__))


def _single(config, nsteps, variant=""):
    import oracle
    st = worker.tiled_state(config, variant)
    return st, worker.run(oracle.Oracle(st), st, nsteps)


@pytest.mark.parametrize("ntI,ntJ,config,variant", [(2, 1, "UPWELLING", ""), (1, 2, "UPWELLING", ""),
                                                    (2, 2, "SEAMOUNT", ""), (2, 1, "BENCHMARK_TINY", ""),
                                                    # MPDATA on 6 tracers: three ghost points, extended flux ranges
                                                    (2, 2, "BENCHMARK_TINY", "mpdata"),
                                                    # HSIMT: three ghost points, limiter reaching two faces upwind
                                                    (2, 2, "BENCHMARK_TINY", "hsimt"),
                                                    # a basin: physical edges on all four sides, corners
                                                    (2, 2, "UPWELLING", "basin"), (2, 1, "BENCHMARK_TINY", "basin"),
                                                    # MPDATA / HSIMT on a basin with land: Ta's boundary values and
                                                    # corners, the edge rule of Ua / Va, masks -- across tile edges
                                                    (2, 2, "BENCHMARK_TINY", "mpdata+basin+mask"),
                                                    (2, 2, "BENCHMARK_TINY", "hsimt+basin+mask"),
                                                    # the GLS closure across tile edges (smoothed shear, five-point advection of
                                                    # tke / gls, the Akv / Akt edge rule of gls_corstep.F)
                                                    (2, 2, "UPWELLING", "gls"), (2, 1, "BENCHMARK_TINY", "gls+basin+mask"),
                                                    (2, 2, "UPWELLING", "my25"), (1, 2, "BENCHMARK_TINY", "my25+basin+mask"),
                                                    # UV_VIS2 rotated to geopotentials (uv3dmix2_geo.h) across tile edges
                                                    (2, 2, "SEAMOUNT", "geouv"),
                                                    # WET_DRY: the wet/dry masks, their fast-time sum and the drying
                                                    # shoreline across tile edges; with land and on a basin
                                                    (2, 2, "UPWELLING", "wet"), (2, 2, "UPWELLING", "wet+basin+mask"),
                                                    # biharmonic mixing: the first operator's one-point-wider range
                                                    # and its edge rule across tile edges, channel and basin
                                                    (2, 2, "BENCHMARK_TINY", "dif4"), (2, 2, "BENCHMARK_TINY", "dif4+basin+mask"),
                                                    # point sources (LuvSrc): rivers in the walls and on the island's
                                                    # coast, every rank holding the whole table; MPDATA's wider range
                                                    (2, 2, "UPWELLING", "river+basin+mask"), (2, 1, "BENCHMARK_TINY", "river"),
                                                    (2, 2, "BENCHMARK_TINY", "river+mpdata+basin+mask"),
                                                    # ... and cell-centred sources (LwSrc) beside them
                                                    (2, 2, "UPWELLING", "river+wells+basin+mask"), (2, 2, "BENCHMARK_TINY", "river+wells+mpdata"),
                                                    (2, 2, "UPWELLING", "river+wells+wet+basin+mask"),
                                                    # without SPLINES_VVISC / SPLINES_VDIFF
                                                    (2, 2, "UPWELLING", "classic+river+wells+basin+mask"), (2, 1, "BENCHMARK_TINY", "classic")])
def test_tiled_equals_single(tmp_path, ntI, ntJ, config, variant):
    nsteps = 3
    world = ntI * ntJ
    tiling_util.spawn_ranks("mp_worker.py", world, [ntI, ntJ, tmp_path, config, nsteps, variant], timeout=600)
    ref, want = _single(config, nsteps, variant)
    tiling_util.assert_tiles_equal(tmp_path, world, want, ref.b, tiling_util.FIELDS, owned="Istr:Iend",
                                   rho_ghosts=("zeta", "t", "Hz", "W", "rmask_wet"))


MPIEXEC = "/opt/conda/bin/mpiexec"


@pytest.mark.skipif(not os.path.exists(MPIEXEC), reason="no MPI in this image")
@pytest.mark.parametrize("ntI,ntJ,config", [(2, 2, "SEAMOUNT"), (4, 2, "BENCHMARK_TINY")])
def test_mpi_baseline_layer_equals_single(tmp_path, ntI, ntJ, config):
    """The arrangement bench.py's cpu_baseline leg times -- one oracle process per tile under mpiexec, halos
    through oracle/mpi/oracle_mpi.c (mp_exchange.F:290-902 restated on MPI) -- against the one-tile run: 1 + 2
    steps, every tile bit-equal incl. ghost points.  (4x2 = the tiling of the 8-GPU run.)"""
    root = os.path.dirname(HERE)
    world = ntI * ntJ
    r = subprocess.run([MPIEXEC, "-n", str(world), sys.executable, os.path.join(root, "bench.py"), "--cpu-worker",
                        config, "2", "0", str(ntI), str(ntJ), str(tmp_path)],
                       env=dict(os.environ, OMP_NUM_THREADS="1", PYTHONPATH=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    ref, want = _single(config, 3)
    tiling_util.assert_tiles_equal(tmp_path, world, want, ref.b,
                                   ("zeta", "ubar", "vbar", "u", "v", "t", "Huon", "W", "Hz", "Akv", "tke"),
                                   owned="Istr:Iend", rho_ghosts=("zeta", "t", "Hz", "W"))
