"""GPU, multi-process: the N>1 device path.  One process per tile (2 and 4 tiles, all on
the one GPU of the test box), halos through the library's host-relay transport over gloo.
After 3 full steps every tile's owned AND ghost points must equal the single-tile HIP run
bit for bit -- the reference's acceptance rule "identical results across tilings" -- which
exercises the general (multi-tile) branch of every kernel, the pack/unpack kernels, the
neighbour table incl. the periodic Nghost+1 rule and the corner messages of the one-phase exchange
(2x2: each tile's W and E, and its two diagonal neighbours, are the same rank -- four messages per pair,
paired by order as RCCL does).
The RCCL calls themselves need one GPU per rank and run only in bench.py --gpus N."""
import pytest

import mp_gpu_worker as worker
import tiling_util

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ntI,ntJ,config,variant", [(2, 1, "BENCHMARK_TINY", ""), (1, 2, "UPWELLING", ""),
                                                    (2, 2, "SEAMOUNT", ""), (4, 1, "BENCHMARK_TINY", ""),
                                                    # ragged tiles (64 = 22 + 21 + 21 columns), three different neighbours
                                                    (3, 1, "BENCHMARK_TINY", ""),
                                                    # three ghost points, MPDATA's extended ranges across tile edges
                                                    (2, 2, "BENCHMARK_TINY", "mpdata"),
                                                    # bulk fluxes, KPP, wvelocity, diag on every tile
                                                    (2, 2, "BENCHMARK_TINY", "physics"),
                                                    # MASKING: an island across the tile corner, a headland on the wall
                                                    (2, 2, "BENCHMARK_TINY", "mask"), (2, 1, "UPWELLING", "mask"),
                                                    # no periodic direction: physical edges on the outer tile sides, corners
                                                    (2, 2, "UPWELLING", "basin"), (2, 1, "BENCHMARK_TINY", "basin+physics"),
                                                    # MPDATA on a basin with land, across tile edges
                                                    (2, 2, "BENCHMARK_TINY", "mpdata+basin+mask"),
                                                    # the GLS closure: smoothed shear, five-point advection of tke / gls and
                                                    # the Akv / Akt edge rule of gls_corstep.F across tile edges
                                                    (2, 2, "UPWELLING", "gls"), (2, 1, "BENCHMARK_TINY", "gls+basin+mask"),
                                                    (2, 2, "UPWELLING", "my25"), (1, 2, "BENCHMARK_TINY", "my25+basin+mask"),
                                                    # UV_VIS2 rotated to geopotentials: the LDS patches of k_uv3dmix2_geo against tile edges
                                                    (2, 2, "SEAMOUNT", "geouv"), (2, 1, "BENCHMARK_TINY", "geouv+basin+mask"), (3, 1, "BENCHMARK_TINY", "geouv+wet"),
                                                    # WET_DRY: masks, their fast-time sum and the drying shoreline across
                                                    # tile edges
                                                    (2, 2, "UPWELLING", "wet"), (2, 2, "UPWELLING", "wet+basin+mask"),
                                                    # biharmonic mixing across tile edges
                                                    (2, 2, "BENCHMARK_TINY", "dif4"), (2, 2, "BENCHMARK_TINY", "dif4+basin+mask"),
                                                    # point sources (LuvSrc): rivers in the walls and on the island's coast
                                                    (2, 2, "UPWELLING", "river+basin+mask"), (2, 1, "BENCHMARK_TINY", "river+physics"),
                                                    (2, 2, "BENCHMARK_TINY", "river+mpdata+basin+mask"),
                                                    (2, 2, "UPWELLING", "river+wells+basin+mask"), (2, 2, "BENCHMARK_TINY", "river+wells+mpdata"),
                                                    (2, 2, "UPWELLING", "river+wells+wet+basin+mask"),
                                                    # without SPLINES_VVISC / SPLINES_VDIFF
                                                    (2, 2, "UPWELLING", "classic+river+wells+basin+mask"), (2, 1, "BENCHMARK_TINY", "classic+physics"),
                                                    # BASELINE.json configurations 4 and 5 at FULL size (2048x256x30): the
                                                    # 512-column tiles of the 8-GPU run (4x1), both tile rows (2x2), the
                                                    # deferred-flux step2d path and, with six MPDATA tracers, three ghost points
                                                    (4, 1, "BENCHMARK3", "physics+slim"), (2, 2, "BENCHMARK3", "physics+slim"),
                                                    (2, 2, "BENCHMARK3", "mpdata+slim"),
                                                    # a curvilinear grid (tests/curv_util.py): metrics and mixing
                                                    # coefficients varying in i and j, the general barotropic kernel
                                                    (2, 1, "UPWELLING", "curv"), (1, 2, "UPWELLING", "curv"),
                                                    # ... in the eastern tile's columns only: the western tile takes its
                                                    # metrics from the row table, the eastern one from the arrays
                                                    (2, 1, "UPWELLING", "curveast"),
                                                    # pn differs along the one column that is Istr-3 of the eastern
                                                    # tile: read there with three ghost points, so that tile must not
                                                    # use the row table either
                                                    (2, 1, "BENCHMARK_TINY", "dif4+edge")])
def test_tiled_hip_equals_single_hip(tmp_path, ntI, ntJ, config, variant):
    nsteps = 2 if "slim" in variant else 3
    world = ntI * ntJ
    ref, want = worker.single_tile(config, nsteps, variant)     # before the children start: at most `world` + 1 GPU processes
    tiling_util.spawn_ranks("mp_gpu_worker.py", world, [ntI, ntJ, tmp_path, config, nsteps, variant], timeout=600)
    for r, d, _, _ in tiling_util.tiles(tmp_path, world, ref.b):
        if "curveast" in variant:        # row_metrics_state(): the table on the western tile, the arrays on the eastern
            assert (int(d["rowm"]) in (1, 3)) == (r == 0) and (int(d["rowm"]) == 2) == (r == 1), (r, int(d["rowm"]))
        if "edge" in variant or "curv" in variant.split("+"):
            assert int(d["rowm"]) == 2, (r, int(d["rowm"]))
    tiling_util.assert_tiles_equal(tmp_path, world, want, ref.b, tiling_util.FIELDS, owned="Istr:Iend",
                                   rho_ghosts=("zeta", "t", "Hz", "W"))
