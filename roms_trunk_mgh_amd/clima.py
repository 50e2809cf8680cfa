"""Climatology nudging: the host-side image of CLIMA(ng) (ROMS/Modules/mod_clima.F:190-261) with the run-time switches
LnudgeM2CLM, LnudgeM3CLM and LnudgeTCLM of a roms_*.in, as an application's ana_nudgcoef.h / set_data.F fill it.  A
TileState carries one as `state.clima`; RomsHip hands it to the library when it is built and whenever `set_clima` is
called again (the reference re-interpolates tclm / uclm / ... in set_data every step).

Only the HIP path consumes it.  The CPU oracle has no climatology: `oracle.Oracle` ignores `state.clima`, so a state
that carries one cannot be compared against the oracle (tests/test_gpu_clima.py compares against the HIP path without
climatology and against closed forms instead)."""
import ctypes as C

import numpy as np

_IP = C.POINTER(C.c_int)
_DP = C.POINTER(C.c_double)

ARRAYS = ("M2nudgcof", "ubarclm", "vbarclm", "M3nudgcof", "uclm", "vclm", "Tnudgcof", "tclm")


class Clima:
    def __init__(self, bounds, LnudgeM2CLM=False, M2nudgcof=None, ubarclm=None, vbarclm=None,
                 LnudgeM3CLM=False, M3nudgcof=None, uclm=None, vclm=None,
                 LnudgeTCLM=None, Tnudgcof=None, tclm=None, obcfac=1.0):
        """bounds: the tile's abi.Bounds.  Arrays have the tile's extents: M2nudgcof, ubarclm, vbarclm (ni, nj);
        M3nudgcof, uclm, vclm (ni, nj, N); Tnudgcof, tclm (ni, nj, N, NTCLM) with ni = UBi-LBi+1, nj = UBj-LBj+1.
        LnudgeTCLM (NT) = LtracerCLM .and. LnudgeTCLM per tracer; NTCLM = the number of set flags, the compact index
        counting them in the order of the tracers (step3d_t.F:1551-1560).  Coefficients in 1/s, ghost points filled.
        obcfac: obc_in = obcfac * obc_out on RadNud edges."""
        b = bounds
        ni, nj, N, NT = b.UBi - b.LBi + 1, b.UBj - b.LBj + 1, b.N, b.NT
        self.LnudgeM2CLM, self.LnudgeM3CLM = bool(LnudgeM2CLM), bool(LnudgeM3CLM)
        self.LnudgeTCLM = np.zeros(NT, dtype=np.int32)
        if LnudgeTCLM is not None:
            flags = np.asarray(LnudgeTCLM)
            if flags.shape != (NT,):
                raise ValueError(f"LnudgeTCLM has shape {flags.shape}, the tile has NT = {NT} tracers")
            self.LnudgeTCLM[:] = flags != 0
        self.obcfac = float(obcfac)
        if not self.obcfac >= 0.0:
            raise ValueError("obcfac < 0")
        ntclm = self.NTCLM
        want = {"M2nudgcof": (ni, nj), "ubarclm": (ni, nj), "vbarclm": (ni, nj),
                "M3nudgcof": (ni, nj, N), "uclm": (ni, nj, N), "vclm": (ni, nj, N),
                "Tnudgcof": (ni, nj, N, ntclm), "tclm": (ni, nj, N, ntclm)}
        on = {"M2nudgcof": self.LnudgeM2CLM, "ubarclm": self.LnudgeM2CLM, "vbarclm": self.LnudgeM2CLM,
              "M3nudgcof": self.LnudgeM3CLM, "uclm": self.LnudgeM3CLM, "vclm": self.LnudgeM3CLM,
              "Tnudgcof": ntclm > 0, "tclm": ntclm > 0}
        given = dict(M2nudgcof=M2nudgcof, ubarclm=ubarclm, vbarclm=vbarclm, M3nudgcof=M3nudgcof, uclm=uclm, vclm=vclm,
                     Tnudgcof=Tnudgcof, tclm=tclm)
        self.arr = {}
        for name in ARRAYS:
            a = given[name]
            if not on[name]:
                if a is not None:
                    raise ValueError(f"{name} given but its switch is off")
                continue
            if a is None:
                raise ValueError(f"{name}: the switch is on but the array is missing")
            a = np.asarray(a, dtype=np.float64)
            if a.shape != want[name]:
                what = " (NTCLM = %d set flags)" % ntclm if name in ("Tnudgcof", "tclm") else ""
                raise ValueError(f"{name} has shape {a.shape}, wanted {want[name]}{what}")
            self.arr[name] = np.asfortranarray(a).copy(order="F")

    @property
    def NTCLM(self):
        return int(self.LnudgeTCLM.sum())

    def ic(self, itrc):
        """compact index (1-based) of tracer itrc (1-based), 0 when it is not nudged"""
        return int(self.LnudgeTCLM[:itrc].sum()) if self.LnudgeTCLM[itrc - 1] else 0

    def __getitem__(self, name):
        return self.arr[name]

    def c_args(self, only=None):
        """The arguments of roms_hip_set_clima; only = names of the arrays to pass (the others go as NULL: "keep the
        copy you have")."""
        def ptr(name):
            if name not in self.arr or (only is not None and name not in only):
                return None
            return self.arr[name].ctypes.data_as(_DP)
        return (int(self.LnudgeM2CLM), ptr("M2nudgcof"), ptr("ubarclm"), ptr("vbarclm"),
                int(self.LnudgeM3CLM), ptr("M3nudgcof"), ptr("uclm"), ptr("vclm"),
                self.LnudgeTCLM.ctypes.data_as(_IP), ptr("Tnudgcof"), ptr("tclm"), self.obcfac)
