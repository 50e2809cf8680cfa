"""Worker of the tiling-invariance test of the tidal boundary forcing (tests/test_gpu_tides.py): one rank = one tile
through the HIP library under Main3D(tides=...), halos over the gloo relay or (variant "...+rccl", one rank) through RCCL
in loopback -- the transports of tests/mp_gpu_avg_worker.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

SHAPE = dict(Lm=16, Mm=10, N=4, EWperiodic=False)
NSTEPS = 7
FIELDS = ("zeta_bry", "ubar_bry", "vbar_bry", "zeta", "ubar", "vbar", "u", "v", "t")


def tiled_state(variant, ntI=1, ntJ=1, tile=0):
    """(state, tides): the open basin; variant "ssh" = SSH_TIDES alone (the reduced-physics boundary value), otherwise
    SSH_TIDES + UV_TIDES"""
    import tides_util as tu
    from roms_trunk_mgh_amd import ana
    st = ana.make_tile("UPWELLING", ntI, ntJ, tile, perturb=1.0, overrides=dict(SHAPE))
    tu.open_all(st)
    td = ana.analytic_tides(st, ntc=3, mtc=4, uv="ssh" not in variant, tide_start=-0.2, ramp=True, dstart=-1.0)
    return st, td


def run(be, st, td):
    """NSTEPS steps with the tides on; {field: array}, the boundary arrays as the last step's call left them"""
    from roms_trunk_mgh_amd import main3d
    m = main3d.Main3D(be, tides=td)
    m.initial()
    m.run(NSTEPS)
    be.to_host()
    be.check_guards()
    return {name: st[name].copy() for name in FIELDS}


def run_rank(rank, world, ntI, ntJ, port, outdir, variant=""):
    import torch
    import torch.distributed as dist
    from roms_trunk_mgh_amd import hip
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    opts = set(variant.split("+")) if variant else set()
    st, td = tiled_state(variant, ntI, ntJ, rank)
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
        out = run(be, st, td)
    finally:
        be.close()
    b = st.b
    np.savez(os.path.join(outdir, f"tile{rank}.npz"),
             bounds=np.array([b.IstrR, b.IendR, b.JstrR, b.JendR, b.LBi, b.LBj]), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv
    run_rank(int(a[1]), int(a[2]), int(a[3]), int(a[4]), int(a[5]), a[6], a[7] if len(a) > 7 else "")
