"""What every tiling-invariance test ("N tiles equal one tile, bit for bit") shares, once:

    free_port()          a free TCP port for the gloo rendezvous
    make_variant_tile()  the variant table: a "+"-separated variant string -> the state of one tile.  The one-tile
                         reference and the ranks call it with the same string and differ in (ntI, ntJ, tile) only
    Rank                 the rank harness of a worker (tests/mp_*_worker.py): gloo start-up, the backend of the tile
                         (HIP over the gloo relay, HIP over RCCL, the CPU oracle with the exchange hook), the tile file
    spawn_ranks()        one child process per rank, all dead when it returns
    assert_tiles_equal() the comparison of the tile files with the one-tile run; tiles() for what a test asserts on top

A scenario module (a worker) provides tiled_state(..., ntI, ntJ, tile) and run(be, st, ...) -> {name: array}; its test
calls both for the one-tile reference and its __main__ calls both for one tile inside `with Rank(sys.argv)`."""
import os
import socket
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _path in (os.path.dirname(HERE), HERE):          # a worker is started as a script: the package and tests/ by hand
    if _path not in sys.path:
        sys.path.insert(0, _path)

BOUNDS = ("Istr", "Iend", "Jstr", "Jend", "IstrR", "IendR", "JstrR", "JendR", "LBi", "UBi", "LBj", "UBj")
OWNED = {"Istr:Iend": ("Istr", "Iend", "Jstr", "Jend"), "IstrR:IendR": ("IstrR", "IendR", "JstrR", "JendR")}
# the fields of the general multitile tests (tests/mp_worker.py, tests/mp_gpu_worker.py)
FIELDS = ("zeta", "ubar", "vbar", "u", "v", "t", "Huon", "W", "Hz", "Akv", "tke", "rmask_wet", "umask_wet", "vmask_wet",
          "pmask_wet", "rmask_wet_avg")
STATE_OPTIONS = frozenset(("mpdata", "hsimt", "mask", "dif4", "basin", "wet", "classic", "gls", "my25", "geouv", "curv",
                           "curveast", "edge", "river", "wells"))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ----------------------------------------------------------------------------------------- the variant table --
def options(variant, run_options=()):
    """the set of options of a variant string; one that neither the table nor the caller (run_options: what concerns
    the run, not the state -- rccl, physics, slim) knows is an error, not a run of the default state"""
    opts = set(variant.split("+")) if variant else set()
    unknown = opts - STATE_OPTIONS - set(run_options)
    if unknown:
        raise ValueError(f"variant {variant!r}: unknown option(s) {sorted(unknown)}")
    return opts


def make_variant_tile(config, variant, ntI=1, ntJ=1, tile=0, perturb=1.0, run_options=()):
    """The state of tile `tile` of an ntI x ntJ tiling of `config` under the options of `variant`.  The order is part of
    the table: hsimt replaces what mpdata set."""
    import curv_util as cv
    import util
    from roms_trunk_mgh_amd import ana
    opts = options(variant, run_options)
    kw = dict(NT=6, overrides={"Hadv": "MPDATA", "Vadv": "MPDATA"}) if "mpdata" in opts else {}
    if "hsimt" in opts:
        kw = dict(overrides={"Hadv": "HSIMT", "Vadv": "HSIMT"})
    ov = kw.setdefault("overrides", {})
    if "mask" in opts:
        kw["mask"] = "island"
    if "dif4" in opts:                   # biharmonic mixing (three ghost points with UV_VIS4)
        ov.update({"ts_dif4": 1, "uv_vis4": 1, "tnu4": 1.0e10, "visc4": 2.0e10})
    if "basin" in opts:                  # no periodic direction
        ov["EWperiodic"] = False
    if "wet" in opts:                    # WET_DRY on the beach bathymetry of ana.py (the shoreline crosses tile edges)
        ov.update({"wet_dry": 1, "beach": 1, "zeta_amp": 0.3})
    if "classic" in opts:                # without SPLINES_VVISC / SPLINES_VDIFF: the tridiagonal systems for u, v, t themselves
        ov.update({"splines_vdiff": 0, "splines_vvisc": 0})
    if "gls" in opts:                    # GLS_MIXING (k-epsilon, Kantha-Clayson, N2S2_HORAVG, RI_SPLINES)
        ov["gls"] = "k-epsilon"
    if "my25" in opts:                   # MY25_MIXING (Kantha-Clayson, N2S2_HORAVG, RI_SPLINES)
        ov["gls"] = "my25"
    if "geouv" in opts:                  # UV_VIS2 with MIX_GEO_UV (uv3dmix2_geo.h)
        ov.update({"uv_vis2": 2, **({"visc2": 50.0} if config == "SEAMOUNT" else {})})
    if not ov:
        del kw["overrides"]
    st = ana.make_tile(config, ntileI=ntI, ntileJ=ntJ, tile=tile, perturb=perturb, **kw)
    if "edge" in opts:                   # pn differs along one column that the eastern tile holds as ghost column Istr-3 only
        cv.ghost_only_column(st)
    elif opts & {"curv", "curveast"}:    # a curvilinear grid; curveast: in the eastern tile's columns only
        cv.curvilinear(st, columns=cv.east_columns(st.b) if "curveast" in opts else None)
    if "river" in opts:                  # point sources (LuvSrc) in the walls and, with a mask, on the island's coast
        util.river_sources(st, "all" if "wells" in opts else "both" if "mask" in opts else "walls")
    return st


# ------------------------------------------------------------------------------------------ the rank harness --
def rccl_unique_id(dist=None, torch=None, rank=0):
    """an RCCL id from the library; with a process group, rank 0's id on every rank"""
    import ctypes
    from roms_trunk_mgh_amd import hip
    buf = ctypes.create_string_buffer(128)
    if rank == 0:
        assert hip.load().roms_hip_get_unique_id(buf) == 0
    if dist is None:
        return bytes(buf.raw)
    t = torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8).clone()
    dist.broadcast(t, src=0)
    return bytes(t.numpy().tobytes())


def write_tile(outdir, rank, b, arrays):
    """tile{rank}.npz: the arrays and the bounds of the tile BY NAME (BOUNDS), one layout for every comparison"""
    assert not set(BOUNDS) & set(arrays)
    np.savez(os.path.join(outdir, f"tile{rank}.npz"), **{k: np.array(getattr(b, k)) for k in BOUNDS}, **arrays)


class Rank:
    """One rank of a tiling test, from the command line spawn_ranks() gives a worker:
    rank world port ntI ntJ outdir [the scenario's own arguments -> .args].

        with Rank(sys.argv) as rk:
            st = tiled_state(..., rk.ntI, rk.ntJ, rk.rank)
            rk.save(st.b, run(rk.hip(st), st, ...))

    Entering sets the environment and the thread count and joins the gloo group; leaving closes the backend (also on an
    exception), then writes the tile file, waits at the barrier and leaves the group."""

    def __init__(self, argv):
        self.rank, self.world, self.port, self.ntI, self.ntJ = (int(x) for x in argv[1:6])
        self.outdir, self.args = argv[6], list(argv[7:])
        self._close, self._tile = [], None

    def __enter__(self):
        import torch
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(self.port)
        torch.set_num_threads(1)
        dist.init_process_group("gloo", rank=self.rank, world_size=self.world)
        self.torch, self.dist = torch, dist
        return self

    def hip(self, st, rccl=False):
        """the HIP library on this tile (all ranks may share one GPU), halos through the host-relay transport
        (roms_hip_set_halo_relay) over gloo -- the same pack/unpack kernels, neighbour table and phase order as RCCL --
        or, rccl=True, through RCCL itself: one device per rank (RCCL refuses two ranks on one device); with ONE rank
        the library runs in loopback (the tile is its own W/E neighbour, roms_hip.h)"""
        from roms_trunk_mgh_amd import hip
        ndev = self.torch.cuda.device_count()
        if rccl:
            assert self.world <= max(ndev, 1)
            be = hip.RomsHip(st, rank=self.rank, device=self.rank,
                             nccl_unique_id=rccl_unique_id(self.dist, self.torch, self.rank))
        else:
            be = hip.RomsHip(st, rank=self.rank, device=self.rank % max(ndev, 1), nccl_unique_id=None)
            be.set_halo_relay_gloo(self.dist, self.torch)
        self._close.append(be.close)
        return be

    def oracle(self, st):
        """the CPU oracle on this tile, halos through its exchange hook: the Python mirror of mp_exchange over gloo"""
        import ctypes as C
        import oracle
        from roms_trunk_mgh_amd import halo
        b, ni, nj = st.b, st.ni, st.nj
        sr = halo.gloo_sendrecv(self.dist, self.torch)
        HOOK = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int, C.c_int)

        def hook(ptr, nk, gtype):
            A = np.ctypeslib.as_array(ptr, shape=(nk * nj * ni,)).reshape((ni, nj, nk), order="F")
            halo.exchange(A, b, self.rank, sr)

        cb = HOOK(hook)
        lib = oracle.lib()
        lib.oracle_set_exchange_hook.argtypes = [HOOK]
        lib.oracle_set_exchange_hook(cb)
        self._close.append(lambda keep=cb: lib.oracle_set_exchange_hook(HOOK(0)))
        return oracle.Oracle(st)

    def save(self, b, arrays):
        """what the tile file is to hold; written on leaving, after the backend is closed"""
        self._tile = (b, dict(arrays))

    def __exit__(self, etype, exc, tb):
        for close in reversed(self._close):
            close()
        if etype is None:
            write_tile(self.outdir, self.rank, *self._tile)
            self.dist.barrier()
            self.dist.destroy_process_group()
        return False


# ------------------------------------------------------------------------------------------------ launching --
def spawn_ranks(worker_file, world, args, timeout):
    """`world` children `python worker_file rank world port *args` (worker_file: a path under tests/, or the list of
    python's own arguments), OMP_NUM_THREADS=1.  Every rank must exit 0 within `timeout` seconds; the first that does
    not fails the call at once, and whatever still runs is killed and waited for.  Nothing is started again."""
    head = [sys.executable] + ([os.path.join(HERE, worker_file)] if isinstance(worker_file, str) else list(worker_file))
    port = free_port()
    env = dict(os.environ, OMP_NUM_THREADS="1")
    procs = [subprocess.Popen(head + [str(r), str(world), str(port)] + [str(a) for a in args], env=env) for r in range(world)]
    deadline = time.monotonic() + timeout
    try:
        pending = dict(enumerate(procs))
        while pending:
            for r, p in list(pending.items()):
                if p.poll() is not None:
                    assert p.returncode == 0, f"rank {r} of {worker_file} exited with status {p.returncode}"
                    del pending[r]
            if pending:
                assert time.monotonic() < deadline, f"ranks {sorted(pending)} of {worker_file} still run after {timeout} s"
                time.sleep(0.02)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()


# ------------------------------------------------------------------------------------------------ comparing --
def read_tile(path):
    """{name: array} of a tile file, the bounds as ints by name"""
    with np.load(path) as d:
        out = {k: d[k] for k in d.files}
    if "bounds" in out and "Istr" not in out:
        # the one legacy layout: bench.py --cpu-worker (test_mpi_baseline_layer_equals_single) writes the positional
        # bounds = [Istr, Iend, Jstr, Jend, LBi, LBj]
        out.update(zip(("Istr", "Iend", "Jstr", "Jend", "LBi", "LBj"), out.pop("bounds")))
    out.update({k: int(out[k]) for k in BOUNDS if k in out})
    return out


def tiles(tmp_path, world, gb, owned="Istr:Iend"):
    """(rank, arrays, own_slices, global_slices) of every tile file: the tile's owned range `owned` in the tile's arrays
    and in the arrays of the one-tile run with bounds gb"""
    i0, i1, j0, j1 = OWNED[owned]
    for r in range(world):
        d = read_tile(os.path.join(tmp_path, f"tile{r}.npz"))
        own = (slice(d[i0] - d["LBi"], d[i1] - d["LBi"] + 1), slice(d[j0] - d["LBj"], d[j1] - d["LBj"] + 1))
        glob = (slice(d[i0] - gb.LBi, d[i1] - gb.LBi + 1), slice(d[j0] - gb.LBj, d[j1] - gb.LBj + 1))
        yield r, d, own, glob


def _assert_equal(a, want, what):
    if not np.array_equal(a, want):
        worst = float(np.abs(a - want).max()) if a.shape == want.shape else f"shapes {a.shape} and {want.shape}"
        raise AssertionError(f"{what}, largest difference {worst}")


def assert_tiles_equal(tmp_path, world, want, gb, names, owned="Istr:Iend", rho_ghosts=()):
    """Every field `names` of every tile file equals want[name], the one-tile run with bounds gb, bit for bit on the
    tile's owned range; the names in rho_ghosts (rho-type: every ghost point is defined) also on the whole allocated
    tile -- not the reference's spare padding column/row of even-sized grids, Im=Lm+1/Jm=Mm+1."""
    for r, d, own, glob in tiles(tmp_path, world, gb, owned):
        for name in names:
            a, full = d[name], want[name]
            _assert_equal(a[own], full[glob], f"field {name}, rank {r}: owned points differ")
            if name in rho_ghosts:
                i0, j0 = d["LBi"] - gb.LBi, d["LBj"] - gb.LBj
                iv = min(a.shape[0], gb.Lm + gb.NghostPoints - d["LBi"] + 1)
                jv = min(a.shape[1], gb.Mm + 1 - d["LBj"] + 1)
                _assert_equal(a[:iv, :jv], full[i0:i0 + iv, j0:j0 + jv], f"field {name}, rank {r}: ghost points differ")
