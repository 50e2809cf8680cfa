"""Worker of the tiling-invariance test of the climatology nudging (tests/test_gpu_clima.py): one rank = one tile of
clima_util.tiled_state through the HIP library, halos over the gloo relay or (variant "...+rccl", one rank) through
RCCL in loopback -- the transports of tests/mp_gpu_worker.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

FIELDS = ("zeta", "ubar", "vbar", "u", "v", "t", "Huon", "W", "Hz")


def run_rank(rank, world, ntI, ntJ, config, nsteps, port, outdir, variant=""):
    import torch
    import torch.distributed as dist
    import clima_util
    from roms_trunk_mgh_amd import hip, main3d
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    opts = set(variant.split("+")) if variant else set()
    st = clima_util.tiled_state(config, "basin" if "basin" in opts else "", ntI, ntJ, rank)
    ndev = torch.cuda.device_count()
    if "rccl" in opts:
        import ctypes
        assert world <= max(ndev, 1)
        buf = ctypes.create_string_buffer(128)
        if rank == 0:
            assert hip.load().roms_hip_get_unique_id(buf) == 0
        t = torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8).clone()
        dist.broadcast(t, src=0)
        be = hip.RomsHip(st, rank=rank, device=rank, nccl_unique_id=bytes(t.numpy().tobytes()))
    else:
        be = hip.RomsHip(st, rank=rank, device=rank % max(ndev, 1), nccl_unique_id=None)
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
    run_rank(int(a[1]), int(a[2]), int(a[3]), int(a[4]), a[5], int(a[6]), int(a[7]), a[8], a[9] if len(a) > 9 else "")
