"""Worker for tests/test_gpu_rhs3d_fused.py::test_tiling_invariance: one rank per tile (all on one GPU), halos through
the library's host-relay transport over gloo as in tests/mp_gpu_worker.py.  One full step brings the fields away from
the initial state; then rhs3d ALONE runs on the rotated time indices and its outputs are saved."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OVERRIDES = {"tnu2": 300.0}
FIELDS = ("t", "u", "v", "ru", "rv", "rufrc", "rvfrc")


def rotated_geo(st):
    """UPWELLING mixes along s-surfaces; the fused path needs the rotated operator"""
    st.p = type(st.p).from_buffer_copy(st.p)
    st.p.mix_geo_ts, st.p.mix_s_ts = 1, 0
    return st


def one_step_then_rhs3d(be):
    from roms_trunk_mgh_amd import main3d
    m = main3d.Main3D(be)
    m.initial()
    m.run(1)
    m._rotate()
    be.call("rhs3d", m.s)
    be.to_host()
    return m.s


def run_rank(rank, world, ntI, ntJ, config, port, outdir):
    import torch
    import torch.distributed as dist
    from roms_trunk_mgh_amd import ana, hip
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    st = rotated_geo(ana.make_tile(config, ntileI=ntI, ntileJ=ntJ, tile=rank, perturb=1.0, overrides=OVERRIDES))
    b = st.b
    be = hip.RomsHip(st, rank=rank, device=rank % max(torch.cuda.device_count(), 1), nccl_unique_id=None)
    be.set_halo_relay_gloo(dist, torch)
    one_step_then_rhs3d(be)
    be.close()
    np.savez(os.path.join(outdir, f"tile{rank}.npz"), bounds=np.array([b.Istr, b.Iend, b.Jstr, b.Jend, b.LBi, b.LBj]),
             **{k: st[k] for k in FIELDS})
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv
    run_rank(int(a[1]), int(a[2]), int(a[3]), int(a[4]), a[5], int(a[6]), a[7])
