"""ctypes binding of libroms_hip.so -- the Python stand-in for the Fortran
ISO_C_BINDING shims (fortran/roms_hip_mod.F90).  Method names mirror the
reference's module procedures (`step3d_t(ng,tile)` -> `call("step3d_t", s)`).

There is NO CPU fallback: if the shared library is missing, or no HIP device is
present, construction fails loudly.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libroms_hip.so")
_LIB = None


def use_library(path):
    """Developer A/B tools only (tools/bench_kernel.py --lib): load another build of the same ABI instead of the
    in-tree product library.  Must be called before the first load(); nothing in tests/, bench.py or
    __graft_entry__.py calls it, and no environment variable can redirect the product path."""
    global LIB_PATH
    if _LIB is not None:
        raise RuntimeError("use_library() after the library was loaded")
    LIB_PATH = os.path.abspath(path)

ENTRIES = ["set_massflux", "rho_eos", "omega", "set_zeta", "set_depth", "rhs3d",
           "pre_step3d", "prsgrd", "t3dmix2", "rhs3d_tile", "uv3dmix2", "step2d",
           "step3d_uv", "step3d_t", "bulk_flux", "set_vbc", "lmd_vmix", "wvelocity", "ini_zeta", "ini_fields",
           "t3dmix4", "uv3dmix4", "gls_prestep", "gls_corstep", "wetdry", "set_avg", "set_diags", "biology"]

# every symbol include/roms_hip.h declares
DECLARED_SYMBOLS = (
    ["roms_hip_init", "roms_hip_finalize", "roms_hip_get_unique_id", "roms_hip_set_bounds",
     "roms_hip_set_params", "roms_hip_register_field", "roms_hip_sync_to_device",
     "roms_hip_sync_to_host", "roms_hip_sync_all_to_device", "roms_hip_sync_all_to_host",
     "roms_hip_device_ptr", "roms_hip_device_synchronize", "roms_hip_last_error",
     "roms_hip_step2d_loop", "roms_hip_exchange", "roms_hip_timing_enable",
     "roms_hip_timing_last_ms", "roms_hip_calib_stream", "roms_hip_set_halo_relay", "roms_hip_diag",
     "roms_hip_snapshot_begin", "roms_hip_snapshot_end", "roms_hip_halo_plan",
     "roms_hip_ana_srflux", "roms_hip_check_guards", "roms_hip_guarded_arrays", "roms_hip_row_metrics_state",
     "roms_hip_graph_exchanges", "roms_hip_graph_exchanges_state", "roms_hip_set_sources",
     "roms_hip_set_clima", "roms_hip_set_averages", "roms_hip_get_average", "roms_hip_average_device_ptr",
     "roms_hip_avg_phase", "roms_hip_set_floats", "roms_hip_floats_put", "roms_hip_floats_get",
     "roms_hip_step_floats", "roms_hip_set_tides", "roms_hip_tides", "roms_hip_set_diagnostics",
     "roms_hip_get_diagnostic", "roms_hip_dia_index", "roms_hip_set_data_record", "roms_hip_set_data_point",
     "roms_hip_set_data", "roms_hip_set_data_factors", "roms_hip_get_clima",
     "roms_hip_set_kpp", "roms_hip_get_kpp", "roms_hip_set_biology", "roms_hip_set_ddmix"] + ["roms_hip_" + e for e in ENTRIES])


_DP = C.POINTER(C.c_double)
class HaloMsg(C.Structure):
    """roms_halo_msg_t of include/roms_hip.h"""
    _fields_ = [("peer", C.c_int), ("tag", C.c_int), ("count", C.c_long), ("buf", _DP)]


RELAY_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(HaloMsg), C.c_int, C.POINTER(HaloMsg))


def load():
    """dlopen libroms_hip.so (does not touch the GPU)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -m roms_trunk_mgh_amd._build` "
            "(there is no CPU fallback for the HIP path)")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    abi.check_abi(lib)
    lib.roms_hip_init.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.roms_hip_set_bounds.argtypes = [C.POINTER(abi.Bounds)]
    lib.roms_hip_set_params.argtypes = [C.POINTER(abi.Params)]
    lib.roms_hip_register_field.argtypes = [C.c_int, C.c_void_p, C.c_long]
    lib.roms_hip_last_error.restype = C.c_char_p
    lib.roms_hip_device_ptr.restype = C.c_void_p
    lib.roms_hip_device_ptr.argtypes = [C.c_int]
    lib.roms_hip_timing_last_ms.restype = C.c_double
    lib.roms_hip_timing_last_ms.argtypes = [C.c_char_p]
    lib.roms_hip_get_unique_id.argtypes = [C.c_void_p]
    for e in ENTRIES:
        fn = getattr(lib, "roms_hip_" + e, None)
        if fn is not None:
            fn.restype = C.c_int
            fn.argtypes = [C.POINTER(abi.StepIdx)]
    if hasattr(lib, "roms_hip_step2d_loop"):
        lib.roms_hip_step2d_loop.argtypes = [C.POINTER(abi.StepIdx), C.POINTER(C.c_int)]
    lib.roms_hip_calib_stream.argtypes = [C.c_long]
    lib.roms_hip_guarded_arrays.restype = C.c_long
    lib.roms_hip_guarded_arrays.argtypes = [C.c_char_p, C.c_long]
    _ip = C.POINTER(C.c_int)
    lib.roms_hip_set_sources.argtypes = [C.c_int, _ip, _ip, _DP, _DP, _DP, _DP, _ip]
    lib.roms_hip_set_clima.argtypes = [C.c_int, _DP, _DP, _DP, C.c_int, _DP, _DP, _DP, _ip, _DP, _DP, C.c_double]
    lib.roms_hip_set_averages.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip]
    lib.roms_hip_get_average.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_long]
    lib.roms_hip_average_device_ptr.restype = C.c_void_p
    lib.roms_hip_average_device_ptr.argtypes = [C.c_int, C.c_int]
    lib.roms_hip_avg_phase.argtypes = [C.c_int] * 5
    lib.roms_hip_set_floats.argtypes = [C.c_int, _ip, _DP, _DP, _DP, _DP]
    lib.roms_hip_floats_put.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    lib.roms_hip_floats_get.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    lib.roms_hip_step_floats.argtypes = [C.POINTER(abi.StepIdx), C.c_double, _ip]
    lib.roms_hip_set_tides.argtypes = ([C.c_int, C.c_int] + [_DP] * 8 + [C.c_double, C.c_int, C.c_double, C.c_int, _DP,
                                        C.c_int, _DP, _DP])
    lib.roms_hip_tides.argtypes = [C.c_double]
    lib.roms_hip_set_diagnostics.argtypes = [C.c_int] * 4
    lib.roms_hip_get_diagnostic.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    lib.roms_hip_dia_index.argtypes = [C.c_int] * 3
    lib.roms_hip_set_data_record.argtypes = [C.c_int] * 4 + [C.c_double, C.c_int, C.c_void_p, C.c_long]
    lib.roms_hip_set_data_point.argtypes = [C.c_int] * 3 + [C.c_double, C.c_int, C.c_double]
    lib.roms_hip_set_data.argtypes = [C.c_double, C.c_double, _ip]
    lib.roms_hip_set_data_factors.argtypes = [C.c_double] * 4 + [C.c_int, C.c_int, _DP, _DP, _ip]
    lib.roms_hip_set_kpp.argtypes = [C.c_int, C.c_void_p]
    lib.roms_hip_get_kpp.argtypes = [C.c_char_p, C.c_void_p, C.c_long]
    lib.roms_hip_set_biology.argtypes = [C.c_int, C.c_void_p, C.c_long]
    lib.roms_hip_set_ddmix.argtypes = [C.c_int]
    if lib.roms_abi_sizeof(5) != C.sizeof(abi.BioPowell):
        raise RuntimeError(f"ABI struct size mismatch: roms_bio_powell_t python={C.sizeof(abi.BioPowell)} "
                           f"C={lib.roms_abi_sizeof(5)}")
    lib.roms_hip_set_halo_relay.argtypes = [RELAY_FN, C.c_void_p]
    if hasattr(lib, "roms_hip_tile_neighbors"):
        lib.roms_hip_tile_neighbors.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_int)]
    _LIB = lib
    return lib


def set_data_factors(time, dt, T1, T2, Tindex, onerec=False):
    """Host-only helper of the library (roms_hip_set_data_factors; needs no GPU): the weights of set_2dfld.F:90-120 for
    Tintrp(1:2) = T1, T2 as (fac1, fac2, synchro), or None where the reference takes its error branch."""
    f1, f2, syn = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
    rc = load().roms_hip_set_data_factors(float(time), float(dt), float(T1), float(T2), int(Tindex), int(bool(onerec)),
                                          C.byref(f1), C.byref(f2), C.byref(syn))
    return None if rc else (f1.value, f2.value, syn.value)


KPP_ARRAYS = {"hbbl": np.float64, "kbbl": np.int32, "ksbl": np.int32}


def kpp_args(state, lmd_bkpp, hbbl=None):
    """The arguments of roms_hip_set_kpp for the tile `state`, checked on the host: lmd_bkpp is a bool (or 0 / 1); hbbl
    is None (zero, as mod_mixing.F leaves it) or an array of the tile's (LBi:UBi, LBj:UBj), and only goes with the switch
    on.  Returns (int, array or None); the array is a Fortran-ordered float64 copy the caller keeps alive over the call."""
    if isinstance(lmd_bkpp, (bool, np.bool_)):
        lmd_bkpp = int(lmd_bkpp)
    if not isinstance(lmd_bkpp, (int, np.integer)) or lmd_bkpp not in (0, 1):
        raise ValueError(f"set_kpp: lmd_bkpp is False / True (0 / 1), not {lmd_bkpp!r}")
    if hbbl is None:
        return int(lmd_bkpp), None
    if not lmd_bkpp:
        raise ValueError("set_kpp: hbbl goes with lmd_bkpp = True only")
    a = np.asfortranarray(hbbl, dtype=np.float64)
    if a.shape != (state.ni, state.nj):
        raise ValueError(f"set_kpp: hbbl has shape {a.shape}, the tile's rho points are {(state.ni, state.nj)}")
    if not np.isfinite(a).all():
        raise ValueError("set_kpp: hbbl is not finite")
    return 1, a


def tile_neighbors(rank, ntileI, ntileJ, Nghost, NghostPoints, EWperiodic, NSperiodic):
    """Host-only helper of the library (mp_exchange.F:73-286); needs no GPU."""
    out = (C.c_int * 12)()
    load().roms_hip_tile_neighbors(rank, ntileI, ntileJ, Nghost, NghostPoints,
                                   int(EWperiodic), int(NSperiodic), out)
    keys = ["Wtile", "Etile", "Stile", "Ntile", "GsendW", "GsendE", "GrecvW", "GrecvE",
            "GsendS", "GsendN", "GrecvS", "GrecvN"]
    return dict(zip(keys, list(out)))


def halo_plan(bounds, rank):
    """Host-only helper of the library: the (sends, recvs) of one halo update of tile `rank`, each a list
    of dicts peer, tag, i0, wi, j0, wj (include/roms_hip.h, roms_hip_halo_plan); needs no GPU."""
    out = (C.c_int * 98)()
    lib = load()
    lib.roms_hip_halo_plan.argtypes = [C.POINTER(abi.Bounds), C.c_int, C.POINTER(C.c_int)]
    lib.roms_hip_halo_plan(C.byref(bounds), rank, out)
    ns, nr = out[0], out[1]
    keys = ["peer", "tag", "i0", "wi", "j0", "wj"]
    msgs = [dict(zip(keys, out[2 + 6 * m: 8 + 6 * m])) for m in range(ns + nr)]
    return msgs[:ns], msgs[ns:]


class RomsHip:
    """One tile on one GPU.  Owns nothing on the host: the TileState arrays stay
    the caller's (as the Fortran module arrays do)."""

    name = "hip"
    _live = None

    def __init__(self, state, rank=0, device=0, nccl_unique_id=None, leave_unregistered=()):
        """leave_unregistered: names of fields an application without the option does not have (the land/sea masks
        without MASKING, visc4_p / visc4_r / diff4 without UV_VIS4 / TS_DIF4): the library keeps defaults for them."""
        self.st = state
        self.l = load()
        if RomsHip._live is not None:
            RomsHip._live.close()
        RomsHip._live = self
        b = state.b
        uid = None
        if nccl_unique_id is not None:
            self._uid = C.create_string_buffer(bytes(nccl_unique_id), 128)
            uid = C.cast(self._uid, C.c_void_p)
        try:
            self._chk(self.l.roms_hip_init(rank, b.ntileI, b.ntileJ, device, uid), "init")
            self._chk(self.l.roms_hip_set_bounds(C.byref(b)), "set_bounds")
            self._chk(self.l.roms_hip_set_params(C.byref(state.p)), "set_params")
            for name, _, _ in abi.FIELDS:
                if name in leave_unregistered:
                    continue
                a = state.arr[name]
                self._chk(self.l.roms_hip_register_field(abi.FIELD_ID[name], a.ctypes.data, a.size),
                          "register_field " + name)
            self._chk(self.l.roms_hip_sync_all_to_device(), "sync_all_to_device")
            if getattr(state, "sources", None) is not None:
                self.set_sources(state.sources)
            if getattr(state, "clima", None) is not None:
                self.set_clima(state.clima)
            if getattr(state, "tides", None) is not None:
                self.set_tides(state.tides)
        except Exception:
            # a refused set-up (more levels than ROMS_MAXN, say) leaves no half-made context behind: the next
            # RomsHip() would otherwise fail while closing it (check_guards without bounds)
            RomsHip._live = None
            self.l.roms_hip_finalize()
            raise

    def set_sources(self, src):
        """SOURCES(ng) with LuvSrc (roms_trunk_mgh_amd/sources.py) -> roms_hip_set_sources"""
        self._chk(self.l.roms_hip_set_sources(*src.c_args()), "set_sources")

    def set_clima(self, clima, only=None):
        """CLIMA(ng) with LnudgeM2CLM / LnudgeM3CLM / LnudgeTCLM (roms_trunk_mgh_amd/clima.py) -> roms_hip_set_clima;
        only = names of the arrays to hand over again (the others keep their device copy)."""
        self._chk(self.l.roms_hip_set_clima(*clima.c_args(only)), "set_clima")

    def get_clima(self, clima, name):
        """The library's device copy of one array of `clima` as a host array of its extents (roms_hip_get_clima)."""
        out = np.zeros(clima.arr[name].shape, dtype=np.float64, order="F")
        self.l.roms_hip_get_clima.argtypes = [C.c_char_p, C.c_void_p, C.c_long]
        self._chk(self.l.roms_hip_get_clima(name.encode(), out.ctypes.data, out.size), "get_clima " + name)
        return out

    def set_averages(self, averages):
        """The selection of time-averaged fields (roms_trunk_mgh_amd/avg.py) -> roms_hip_set_averages; None switches
        the averages off (nAVG = 0)."""
        self.averages = averages
        args = averages.c_args() if averages is not None else (0, 0, 0, 0, None, None)
        self._chk(self.l.roms_hip_set_averages(*args), "set_averages")

    def get_average(self, name, itrc=0):
        """One average (itrc = the 1-based tracer of a per-tracer one) or WET_DRY counter of roms_avg.def as a host
        array with the tile's extents (roms_hip_get_average)."""
        from . import avg
        if getattr(self, "averages", None) is None:
            raise RuntimeError("roms_hip get_average: no averages selected (set_averages)")
        out = np.zeros(self.averages.shape(name), dtype=np.float64, order="F")
        self._chk(self.l.roms_hip_get_average(avg.AVG_ID[name], int(itrc), out.ctypes.data, out.size), "get_average " + name)
        return out

    def set_diagnostics(self, diags):
        """nDIA / ntsDIA of the tracer budget diagnostics (roms_trunk_mgh_amd/diags.py) -> roms_hip_set_diagnostics; None
        switches them off (nDIA = 0) and releases the arrays."""
        args = diags.c_args() if diags is not None else (0, 0, 0, 0)
        self._chk(self.l.roms_hip_set_diagnostics(*args), "set_diagnostics")      # (refused: the set in force stays)
        self.diags = diags

    def set_diags(self, s):
        """set_diags (main3d.F:491): initialise or accumulate DiaTrc, avgzeta and the counter, roms_hip_set_diags"""
        self.call("set_diags", s)

    def get_diagnostic(self, name, itrc=1, accumulated=False):
        """The plane (LBi:UBi, LBj:UBj, N) of term `name` of roms_dia.def and tracer itrc (1-based), DiaTwrk or with
        accumulated DiaTrc; "avgzeta" / "rmask_dia": those 2-D arrays (roms_hip_get_diagnostic)."""
        from . import diags as _diags
        if getattr(self, "diags", None) is None:
            raise RuntimeError("roms_hip get_diagnostic: diagnostics are off (set_diagnostics)")
        out = np.zeros(self.diags.shape(name), dtype=np.float64, order="F")
        self._chk(self.l.roms_hip_get_diagnostic(_diags.DIA_ID[name], int(itrc), int(bool(accumulated)), out.ctypes.data,
                                                 out.size), "get_diagnostic " + name)
        return out

    def set_kpp(self, lmd_bkpp=True, hbbl=None):
        """LMD_BKPP, the KPP bottom boundary layer inside lmd_vmix -> roms_hip_set_kpp; hbbl = the depth of a restart
        file on the tile's rho points, None = zero; False releases hbbl, kbbl, ksbl (kpp_args checks the arguments)."""
        on, a = kpp_args(self.st, lmd_bkpp, hbbl)
        self._chk(self.l.roms_hip_set_kpp(on, None if a is None else a.ctypes.data), "set_kpp")
        self.bkpp = bool(on)

    def get_kpp(self, name):
        """"hbbl" (float64), "kbbl" or "ksbl" (int32) of the bottom boundary layer on the tile's rho points, or
        "alfaobeta" (float64, W-levels 0:N) of LMD_DDMIX (roms_hip_get_kpp)."""
        if name not in KPP_ARRAYS and name != "alfaobeta":
            raise ValueError(f"get_kpp: {name!r} is not one of {sorted(KPP_ARRAYS) + ['alfaobeta']}")
        if name == "alfaobeta":
            out = np.zeros((self.st.ni, self.st.nj, self.st.b.N + 1), dtype=np.float64, order="F")
        else:
            out = np.zeros((self.st.ni, self.st.nj), dtype=KPP_ARRAYS[name], order="F")
        self._chk(self.l.roms_hip_get_kpp(name.encode(), out.ctypes.data, out.size), "get_kpp " + name)
        return out

    def set_ddmix(self, lmd_ddmix=True):
        """LMD_DDMIX, the double-diffusive mixing of KPP -> roms_hip_set_ddmix: rho_eos stores alfaobeta (library-owned,
        get_kpp("alfaobeta")) and lmd_vmix adds nu_ddt / nu_dds to the interior Akt; False releases alfaobeta."""
        if isinstance(lmd_ddmix, (bool, np.bool_)):
            lmd_ddmix = int(lmd_ddmix)
        if not isinstance(lmd_ddmix, (int, np.integer)) or lmd_ddmix not in (0, 1):
            raise ValueError(f"set_ddmix: lmd_ddmix is False / True (0 / 1), not {lmd_ddmix!r}")
        self._chk(self.l.roms_hip_set_ddmix(int(lmd_ddmix)), "set_ddmix")
        self.ddmix = bool(lmd_ddmix)

    def set_biology(self, model="NPZD_POWELL", par=None):
        """BIOLOGY -> roms_hip_set_biology.  model: a name of abi.BIO_MODEL or its code, None / "NONE" drops the
        setting; par: a bio.PowellPar (or an abi.BioPowell), None = the values of npzd_Powell.in with the tracers
        NAT+1 .. NAT+4.  A refused call leaves the setting in force."""
        from . import bio as _bio
        code = 0 if model is None else abi.BIO_MODEL[model] if isinstance(model, str) else int(model)
        if code == 0:
            self._chk(self.l.roms_hip_set_biology(0, None, 0), "set_biology")
            self.biology = None
            return
        if par is None:
            par = _bio.PowellPar()
        blk = par.c_struct(self.st.b) if hasattr(par, "c_struct") else par
        self._chk(self.l.roms_hip_set_biology(code, C.byref(blk), C.sizeof(blk)), "set_biology")
        self.biology = par

    def set_floats(self, floats):
        """DRIFTER(ng) (roms_trunk_mgh_amd/floats.py) -> roms_hip_set_floats; None releases the floats (Nfloats = 0)."""
        self.floats = floats
        args = floats.c_args() if floats is not None else (0, None, None, None, None, None)
        self._chk(self.l.roms_hip_set_floats(*args), "set_floats")

    def floats_put(self, track, bounded):
        """track(NFV,0:NFT,Nfloats) and bounded(Nfloats) to the device (restart), roms_hip_floats_put"""
        t = np.asfortranarray(track, dtype=np.float64)
        bd = np.ascontiguousarray(bounded, dtype=np.int32)
        self._chk(self.l.roms_hip_floats_put(t.ctypes.data, t.size, bd.ctypes.data, bd.size), "floats_put")

    def floats_get(self):
        """(track(NFV,0:NFT,Nfloats), bounded(Nfloats)) from the device, roms_hip_floats_get"""
        if getattr(self, "floats", None) is None:
            raise RuntimeError("roms_hip floats_get: no floats set (set_floats)")
        t = np.zeros(self.floats.track_shape(), dtype=np.float64, order="F")
        bd = np.zeros(self.floats.n, dtype=np.int32)
        self._chk(self.l.roms_hip_floats_get(t.ctypes.data, t.size, bd.ctypes.data, bd.size), "floats_get")
        return t, bd.astype(bool)

    def step_floats(self, s, time, nfl):
        """step_floats (main3d.F:894) with nfl = (nfm3, nfm2, nfm1, nf, nfp1), roms_hip_step_floats"""
        v = (C.c_int * 5)(*nfl)
        self._chk(self.l.roms_hip_step_floats(C.byref(s), float(time), v), "step_floats")

    def set_tides(self, tides, only=None):
        """TIDES(ng) (roms_trunk_mgh_amd/tides.py) -> roms_hip_set_tides; None releases the tides (NTC = 0); only = names
        of the sub-tidal base arrays to hand over again (the others keep their device copy)."""
        from . import tides as _tides
        args = tides.c_args(only) if tides is not None else _tides.NO_TIDES
        self._chk(self.l.roms_hip_set_tides(*args), "set_tides")

    def tides(self, time):
        """set_tides (main3d.F:396) at time = time(ng): writes zeta_bry, ubar_bry, vbar_bry on the device, roms_hip_tides"""
        self._chk(self.l.roms_hip_tides(float(time)), "tides")

    def set_data_record(self, name, slot, Tintrp, record, index=0, side=None, onerec=False):
        """One time record of a target of roms_data.def (roms_trunk_mgh_amd/data.py) -> roms_hip_set_data_record; side =
        a name of data.SIDES or its code."""
        from . import data as _data
        a = np.asfortranarray(record, dtype=np.float64)
        sd = 0 if side is None else _data.SIDES.index(side) if isinstance(side, str) else int(side)
        self._chk(self.l.roms_hip_set_data_record(_data.DATA_ID.get(name, -1) if isinstance(name, str) else int(name), int(index),
                                                  sd, int(slot), float(Tintrp), int(bool(onerec)), a.ctypes.data, a.size),
                  f"set_data_record {name}")

    def set_data_point(self, name, slot, Tintrp, value, index=0, onerec=False):
        """Point data Fpoint(slot) of a set_2dfld target -> roms_hip_set_data_point"""
        from . import data as _data
        self._chk(self.l.roms_hip_set_data_point(_data.DATA_ID.get(name, -1) if isinstance(name, str) else int(name), int(index),
                                                 int(slot), float(Tintrp), int(bool(onerec)), float(value)),
                  f"set_data_point {name}")

    def set_data(self, time, dt):
        """set_data (main3d.F:222) at time = time(ng): interpolates every target with records on the device; returns the
        synchro flag (set_2dfld.F:139-141), roms_hip_set_data"""
        syn = C.c_int(0)
        self._chk(self.l.roms_hip_set_data(float(time), float(dt), C.byref(syn)), "set_data")
        return syn.value

    set_data_factors = staticmethod(set_data_factors)

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.l.roms_hip_last_error()
            raise RuntimeError(f"roms_hip {what} failed rc={rc}: {msg.decode() if msg else ''}")

    def call(self, kernel, s):
        self._chk(getattr(self.l, "roms_hip_" + kernel)(C.byref(s)), kernel)

    def snapshot_begin(self, names):
        """Start an asynchronous device-to-host snapshot of the named fields (roms_hip.h)."""
        ids = (C.c_int * len(names))(*[abi.FIELD_ID[n] for n in names])
        self.l.roms_hip_snapshot_begin.argtypes = [C.POINTER(C.c_int), C.c_int]
        self._chk(self.l.roms_hip_snapshot_begin(ids, len(names)), "snapshot_begin")

    def snapshot_end(self):
        self._chk(self.l.roms_hip_snapshot_end(), "snapshot_end")

    def ana_srflux(self, yday, hour):
        """ana_srflux (ALBEDO branch) for the day of the year and hour caldate gives; writes srflx."""
        self.l.roms_hip_ana_srflux.argtypes = [C.c_double, C.c_double]
        self._chk(self.l.roms_hip_ana_srflux(float(yday), float(hour)), "ana_srflux")

    def diag(self, s):
        """Tile-local sums and maxima of diag_tile (diag.F:190-290) as a 12-vector, see roms_hip.h."""
        import numpy as np
        out = np.zeros(12)
        self.l.roms_hip_diag.argtypes = [C.POINTER(abi.StepIdx), _DP]
        self._chk(self.l.roms_hip_diag(C.byref(s), out.ctypes.data_as(_DP)), "diag")
        return out

    def step2d_loop(self, s, indx1):
        ii = C.c_int(indx1)
        self._chk(self.l.roms_hip_step2d_loop(C.byref(s), C.byref(ii)), "step2d_loop")
        return ii.value

    def to_device(self, names=None):
        if names is None:
            self._chk(self.l.roms_hip_sync_all_to_device(), "sync_all_to_device")
        else:
            for n in names:
                self._chk(self.l.roms_hip_sync_to_device(abi.FIELD_ID[n]), "sync_to_device")

    def to_host(self, names=None):
        if names is None:
            self._chk(self.l.roms_hip_sync_all_to_host(), "sync_all_to_host")
        else:
            for n in names:
                self._chk(self.l.roms_hip_sync_to_host(abi.FIELD_ID[n]), "sync_to_host")
        return self.st

    def sync(self):
        self._chk(self.l.roms_hip_device_synchronize(), "device_synchronize")

    def timing(self, on=True):
        self.l.roms_hip_timing_enable(int(on))

    def set_halo_relay_gloo(self, dist, torch):
        """Route the halo exchange through torch.distributed (gloo, host memory) instead of
        RCCL: roms_hip_set_halo_relay with a callback doing the isend/irecv of one exchange.  Used to
        rehearse N tiles on fewer GPUs and as the pattern for a host-MPI relay.  Deliberately WITHOUT
        message tags: like RCCL, gloo then pairs the k-th send to a rank with the k-th receive from it,
        so the multi-process tests also check the order in which the library lists its messages (two
        tiles in a periodic direction exchange up to four messages per call)."""
        def cb(_user, nsend, send, nrecv, recv):
            try:
                reqs = []
                view = lambda m: torch.from_numpy(np.ctypeslib.as_array(m.buf, shape=(m.count,)))
                for q in range(nsend):
                    reqs.append(dist.isend(view(send[q]), dst=send[q].peer))
                for q in range(nrecv):
                    reqs.append(dist.irecv(view(recv[q]), src=recv[q].peer))
                for r in reqs:
                    r.wait()
                return 0
            except Exception as e:      # an exception must not unwind through the C frame
                import sys
                print(f"halo relay failed: {e!r}", file=sys.stderr, flush=True)
                return 1
        self._relay = RELAY_FN(cb)      # keep the thunk alive
        self._chk(self.l.roms_hip_set_halo_relay(self._relay, None), "set_halo_relay")

    def calib_stream(self, n_doubles):
        self._chk(self.l.roms_hip_calib_stream(n_doubles), "calib_stream")

    def last_ms(self, entry):
        return self.l.roms_hip_timing_last_ms(entry.encode())

    def row_metrics_state(self):
        """roms_hip_row_metrics_state: 0 not examined, 1 metric arrays independent of i (row table), 2 not."""
        self.l.roms_hip_row_metrics_state.restype = C.c_int
        return int(self.l.roms_hip_row_metrics_state())

    def graph_exchanges(self, on=True):
        """Several tiles over RCCL: replay LOOP_2D with its exchanges as one hipGraph (roms_hip.h)."""
        self._chk(self.l.roms_hip_graph_exchanges(int(on)), "graph_exchanges")

    def graph_exchanges_state(self):
        self.l.roms_hip_graph_exchanges_state.restype = C.c_int
        return int(self.l.roms_hip_graph_exchanges_state())

    def check_guards(self):
        """Raise if a kernel stored outside one of the device arrays (roms_hip_check_guards)."""
        self._chk(self.l.roms_hip_check_guards(), "check_guards")

    def guarded_arrays(self):
        """The names of the arrays check_guards looks at, in allocation order: NAME, or NAME[q] for the scratch arrays
        (roms_hip_guarded_arrays)."""
        n = self.l.roms_hip_guarded_arrays(None, 0)
        if n < 0:
            self._chk(8, "guarded_arrays")
        buf = C.create_string_buffer(64 * n + 1)
        assert self.l.roms_hip_guarded_arrays(buf, len(buf)) == n
        return buf.value.decode().split("\n")[:-1] if n else []

    def close(self):
        # the library holds ONE context per process: only its current owner may tear it down
        # (a stale object being garbage-collected must not finalize its successor's context)
        if RomsHip._live is self:
            import sys
            import warnings
            RomsHip._live = None
            rc = self.l.roms_hip_check_guards()
            msg = self.l.roms_hip_last_error() if rc else None
            self.l.roms_hip_finalize()
            if rc:
                text = msg.decode() if msg else ""
                what = ("guard band damaged: " if "store outside" in text else "guard bands could not be checked: ") + text
                if sys.exc_info()[0] is not None:
                    # close() in a `finally:` while the body's exception is propagating: do not replace it
                    warnings.warn("roms_hip: " + what)
                else:
                    raise RuntimeError("roms_hip: " + what)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
