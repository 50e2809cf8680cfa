"""Tidal boundary forcing: the host-side image of TIDES(ng) (ROMS/Modules/mod_tides.F) with the CPP choices SSH_TIDES,
UV_TIDES, RAMP_TIDES, ADD_FSOBC, ADD_M2OBC as run-time switches, as an application's tidal forcing file fills it.
`RomsHip.set_tides` hands it to the library (roms_hip_set_tides); `Main3D(tides=...)` then issues `tides(time)` every
step directly after set_vbc (main3d.F:395-397), which writes zeta_bry, ubar_bry, vbar_bry on the device.

Only the HIP path consumes it.  The CPU oracle has no set_tides: a test that compares against it writes the boundary
arrays itself before each step (tests/tides_util.py)."""
import ctypes as C

import numpy as np

_DP = C.POINTER(C.c_double)

SSH = ("SSH_Tamp", "SSH_Tphase")
UV = ("UV_Tangle", "UV_Tphase", "UV_Tmajor", "UV_Tminor")
BASES = ("zeta_base", "ubar_base", "vbar_base")


class Tides:
    def __init__(self, bounds, Tperiod, NTC=None, SSH_Tamp=None, SSH_Tphase=None, UV_Tangle=None, UV_Tphase=None,
                 UV_Tmajor=None, UV_Tminor=None, angler=None, tide_start=0.0, ramp=False, dstart=0.0,
                 add_fsobc=False, zeta_base=None, add_m2obc=False, ubar_base=None, vbar_base=None):
        """bounds: the tile's abi.Bounds.  Tperiod (MTC) in seconds; NTC <= MTC constituents are used (default MTC).
        The harmonic arrays have the tile's extents and MTC planes, (ni, nj, MTC) with ni = UBi-LBi+1, nj = UBj-LBj+1,
        ghost points filled; amplitudes in m, semi-axes in m/s, phases, inclinations and angler (ni, nj) in radians.
        SSH_Tamp with SSH_Tphase = SSH_TIDES; the four UV arrays = UV_TIDES.  tide_start and dstart in days; ramp =
        RAMP_TIDES.  add_fsobc / add_m2obc with the sub-tidal boundary data zeta_base / ubar_base, vbar_base (ni, nj), in
        the point convention of zeta_bry / ubar_bry / vbar_bry."""
        b = bounds
        ni, nj = b.UBi - b.LBi + 1, b.UBj - b.LBj + 1
        self.Tperiod = np.ascontiguousarray(Tperiod, dtype=np.float64).reshape(-1)
        self.MTC = int(self.Tperiod.size)
        self.NTC = self.MTC if NTC is None else int(NTC)
        self.tide_start, self.dstart, self.ramp = float(tide_start), float(dstart), bool(ramp)
        self.add_fsobc, self.add_m2obc = bool(add_fsobc), bool(add_m2obc)
        given = dict(SSH_Tamp=SSH_Tamp, SSH_Tphase=SSH_Tphase, UV_Tangle=UV_Tangle, UV_Tphase=UV_Tphase,
                     UV_Tmajor=UV_Tmajor, UV_Tminor=UV_Tminor, angler=angler, zeta_base=zeta_base, ubar_base=ubar_base,
                     vbar_base=vbar_base)
        self.arr = {}
        for name, a in given.items():
            if a is None:
                continue
            want = (ni, nj, self.MTC) if name in SSH + UV else (ni, nj)
            a = np.asarray(a, dtype=np.float64)
            if a.shape != want:
                raise ValueError(f"{name} has shape {a.shape}, wanted {want}")
            self.arr[name] = np.asfortranarray(a).copy(order="F")

    @property
    def ssh(self):
        return all(n in self.arr for n in SSH)

    @property
    def uv(self):
        return all(n in self.arr for n in UV)

    def __getitem__(self, name):
        return self.arr[name]

    def c_args(self, only=None):
        """The arguments of roms_hip_set_tides; only = names of the base arrays to pass (the others go as NULL: "keep
        the copy you have")."""
        def ptr(name):
            if name not in self.arr or (only is not None and name in BASES and name not in only):
                return None
            return self.arr[name].ctypes.data_as(_DP)
        return (self.NTC, self.MTC, self.Tperiod.ctypes.data_as(_DP), ptr("SSH_Tamp"), ptr("SSH_Tphase"),
                ptr("UV_Tangle"), ptr("UV_Tphase"), ptr("UV_Tmajor"), ptr("UV_Tminor"), ptr("angler"),
                self.tide_start, int(self.ramp), self.dstart, int(self.add_fsobc), ptr("zeta_base"),
                int(self.add_m2obc), ptr("ubar_base"), ptr("vbar_base"))


NO_TIDES = (0, 0, None, None, None, None, None, None, None, None, 0.0, 0, 0.0, 0, None, 0, None, None)
