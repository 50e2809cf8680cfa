"""GPU: the RCCL leg of the halo exchange (halo.hip: ncclCommInitRank, one ncclGroupStart/End with the
ncclSend/ncclRecv of an exchange) executed on hardware.

* loopback (runs on the one-GPU test box): ONE tile initialised WITH an RCCL id -- the tile is its own W and
  E neighbour, its periodic wrap goes out and comes back through RCCL (two sends to and two receives from
  the same peer per exchange, paired by order: the assumption the 2x1 and 2x2 periodic tilings rely on) and
  every kernel takes its multi-tile branch incl. the deferred-flux step2d call.  Result = the plain
  one-tile run, bit for bit.
* 2x1 on two devices: skipped with an explicit reason when the box has one GPU (RCCL refuses two ranks on
  one device); otherwise one rank per device through RCCL, bit-equal to the one-tile run.
mp_exchange2d/3d/4d: ROMS/Utility/mp_exchange.F:73-286, 290-902."""
import pytest

import mp_gpu_worker as worker
import tiling_util

pytestmark = pytest.mark.gpu
FIELDS = ("zeta", "ubar", "vbar", "u", "v", "t", "Huon", "W", "Hz")


def _rccl_equals_single(tmp_path, world, ntI, ntJ, config, variant):
    nsteps = 3
    ref, want = worker.single_tile(config, nsteps, variant.replace("+rccl", "").replace("rccl", ""))
    tiling_util.spawn_ranks("mp_gpu_worker.py", world, [ntI, ntJ, tmp_path, config, nsteps, variant], timeout=240)
    tiling_util.assert_tiles_equal(tmp_path, world, want, ref.b, FIELDS, owned="Istr:Iend",
                                   rho_ghosts=("zeta", "t", "Hz", "W"))


@pytest.mark.parametrize("config,variant", [("BENCHMARK_TINY", "physics+rccl"), ("UPWELLING", "rccl"),
                                            ("BENCHMARK_TINY", "mpdata+rccl"), ("SEAMOUNT", "mask+rccl")])
def test_rccl_loopback_equals_local_periodic_copy(tmp_path, config, variant):
    _rccl_equals_single(tmp_path, 1, 1, 1, config, variant)


def test_rccl_two_devices(tmp_path):
    import torch
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip(f"needs 2 GPUs for one RCCL rank per device (this box has {ndev}); the transport itself "
                    "runs in the loopback test above")
    _rccl_equals_single(tmp_path, 2, 2, 1, "BENCHMARK_TINY", "physics+rccl")
