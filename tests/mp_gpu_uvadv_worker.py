"""Worker of the tiling-invariance test of the momentum advection schemes (tests/test_gpu_uvadv.py): one rank = one tile
of ana.make_tile under the scheme pair through the HIP library, halos over the gloo relay."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

FIELDS = ("zeta", "ubar", "vbar", "u", "v", "t", "Huon", "W", "Hz")


def run_rank(rank, world, ntI, ntJ, config, nsteps, port, outdir, hadv, vadv):
    import torch
    import torch.distributed as dist
    from roms_trunk_mgh_amd import ana, hip, main3d
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    st = ana.make_tile(config, ntI, ntJ, rank, perturb=1.0, overrides={"uv_hadv": hadv, "uv_vadv": vadv})
    be = hip.RomsHip(st, rank=rank, device=rank % max(torch.cuda.device_count(), 1), nccl_unique_id=None)
    be.set_halo_relay_gloo(dist, torch)
    m = main3d.Main3D(be)
    m.initial()
    m.run(nsteps)
    be.to_host()
    be.check_guards()
    be.close()
    b = st.b
    np.savez(os.path.join(outdir, f"tile{rank}.npz"), bounds=np.array([b.Istr, b.Iend, b.Jstr, b.Jend, b.LBi, b.LBj]),
             **{k: st[k] for k in FIELDS})
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv
    run_rank(int(a[1]), int(a[2]), int(a[3]), int(a[4]), a[5], int(a[6]), int(a[7]), a[8], a[9], a[10])
