"""Worker of the tiling-invariance test of the time-averaged fields (tests/test_gpu_avg.py): one rank = one tile through
the HIP library with averages selected, halos over the gloo relay or (variant "...+rccl", one rank) through RCCL in
loopback -- the transports of tests/mp_gpu_clima_worker.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

SHAPE = dict(Lm=130, Mm=10, N=5)
NAVG, NSTEPS = 3, 4                       # the window closes at iic = 4
SELECT = [("avgzeta", 0), ("avgu2d", 0), ("avgv3d", 0), ("avgw3d", 0), ("avgAKv", 0), ("avgUV", 0), ("avgHuon", 0),
          ("avgt", 1), ("avgUT", 2), ("avgVT", 1), ("avgHvomT", 2)]


def tiled_state(variant, ntI=1, ntJ=1, tile=0):
    from roms_trunk_mgh_amd import ana
    ov = dict(SHAPE)
    if "basin" in variant:
        ov["EWperiodic"] = False
    return ana.make_tile("UPWELLING", ntI, ntJ, tile, perturb=1.0, overrides=ov)


def run(be, st):
    """NSTEPS steps with the averages on; {(name, itrc): array}"""
    import avg_util
    from roms_trunk_mgh_amd import main3d
    av = avg_util.averages_of(st.b, SELECT, nAVG=NAVG)
    m = main3d.Main3D(be, averages=av)
    m.initial()
    m.run(NSTEPS)
    out = {f"{n}:{it}": be.get_average(n, it) for n, it in SELECT}
    be.check_guards()
    return out


def run_rank(rank, world, ntI, ntJ, port, outdir, variant=""):
    import torch
    import torch.distributed as dist
    from roms_trunk_mgh_amd import hip
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    opts = set(variant.split("+")) if variant else set()
    st = tiled_state(variant, ntI, ntJ, rank)
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
    try:
        out = run(be, st)
    finally:
        be.close()
    b = st.b
    np.savez(os.path.join(outdir, f"tile{rank}.npz"),
             bounds=np.array([b.IstrR, b.IendR, b.JstrR, b.JendR, b.LBi, b.LBj, b.UBi]), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv
    run_rank(int(a[1]), int(a[2]), int(a[3]), int(a[4]), int(a[5]), a[6], a[7] if len(a) > 7 else "")
