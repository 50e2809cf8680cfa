"""Worker of tests/test_gpu_uvgeo4.py::test_tilings: one rank per tile of masked BENCHMARK_TINY as a closed basin with
both viscosities rotated to geopotentials (uv_vis2 = 2, uv_vis4 = 2), whole steps of Main3D, the halo exchange through
the library's host-relay transport over gloo (as tests/mp_gpu_worker.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OVERRIDES = {"EWperiodic": False, "uv_vis2": 2, "uv_vis4": 2, "visc4": 2.0e10}
FIELDS = ("zeta", "ubar", "vbar", "u", "v", "t", "rufrc", "rvfrc")


def make(ntI=1, ntJ=1, tile=0):
    from roms_trunk_mgh_amd import ana
    return ana.make_tile("BENCHMARK_TINY", ntileI=ntI, ntileJ=ntJ, tile=tile, perturb=1.0, overrides=dict(OVERRIDES), mask="island")


def run_rank(rank, world, ntI, ntJ, nsteps, port, outdir):
    import torch
    import torch.distributed as dist
    from roms_trunk_mgh_amd import hip, main3d
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    st = make(ntI, ntJ, rank)
    b = st.b
    be = hip.RomsHip(st, rank=rank, device=rank % max(torch.cuda.device_count(), 1), nccl_unique_id=None)
    be.set_halo_relay_gloo(dist, torch)
    m = main3d.Main3D(be)
    m.initial()
    m.run(nsteps)
    be.to_host()
    be.close()
    np.savez(os.path.join(outdir, f"tile{rank}.npz"), bounds=np.array([b.Istr, b.Iend, b.Jstr, b.Jend, b.LBi, b.LBj]),
             **{k: st[k] for k in FIELDS})
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv
    run_rank(int(a[1]), int(a[2]), int(a[3]), int(a[4]), int(a[5]), int(a[6]), a[7])
