"""Tracer budget diagnostics (DIAGNOSTICS_TS): the host-side image of nDIA / ntsDIA of a roms_*.in, the table of the
terms (include/roms_dia.def, the file the C side compiles) with the reference's numbering of them
(ROMS/Modules/mod_scalars.F:4027-4043, mod_param.F:1380-1389), and the schedule of set_diags
(ROMS/Utility/set_diags.F:121-124, :244), which is the initialise / accumulate part of avg.phase.

Only the HIP path computes the terms: main3d.Main3D(backend, diags=Diags(...)) issues set_diags after set_zeta and before
set_avg (main3d.F:490-492); the host fetches planes with RomsHip.get_diagnostic and scales the accumulated ones by the
window length at output time, as for the averages.  The momentum half, DIAGNOSTICS_UV, is not built."""
import re

from . import abi, avg


def _lines():
    """The lines of roms_dia.def in the order of enum roms_dia_id: the terms, then the reserved ids."""
    terms, reserved = [], []
    for kind, args in re.findall(r"\bROMS_DIA(_RESERVED|)\(([^()]*)\)", abi._read("roms_dia.def")):
        a = [x.strip() for x in args.split(",")]
        if kind == "":
            terms.append(dict(name=a[0], group=a[1], what=", ".join(a[2:])))
        else:
            reserved.append(dict(name=a[0], what=", ".join(a[1:])))
    return terms, reserved


TERMS, RESERVED = _lines()
DIA_COUNT = len(TERMS)
DIA_ID = {d["name"]: i for i, d in enumerate(TERMS)}
DIA_ID.update({d["name"]: DIA_COUNT + 1 + i for i, d in enumerate(RESERVED)})       # DIA_COUNT itself asks for NDT


def _present(d, hdif, rotated):
    return d["group"] == "DIA_ALWAYS" or (d["group"] == "DIA_HDIF" and hdif) or (d["group"] == "DIA_ROT" and hdif and rotated)


def indices(hdif, rotated=False):
    """{name: idiag} (1-based, as mod_scalars.F numbers them) of the terms present in a build with / without TS_DIF2 or
    TS_DIF4 and rotated mixing, plus "NDT"; mirrors roms_hip_dia_index."""
    out, n = {}, 0
    for d in TERMS:
        if _present(d, hdif, rotated):
            n += 1
            out[d["name"]] = n
    out["NDT"] = n
    return out


def phase(iic, nDIA, ntsDIA, ntstart, nrrec):
    """What set_diags does at time step iic: avg.SET (initialise), avg.ADD (accumulate) or 0."""
    return avg.phase(iic, nDIA, ntsDIA, ntstart, nrrec) & (avg.SET | avg.ADD)


class Diags:
    """nDIA, ntsDIA, ntstart, nrrec of a tile with bounds `bounds`."""

    def __init__(self, bounds, nDIA, ntsDIA=1, ntstart=1, nrrec=0):
        self.b = bounds
        self.nDIA, self.ntsDIA, self.ntstart, self.nrrec = int(nDIA), int(ntsDIA), int(ntstart), int(nrrec)

    def phase(self, iic):
        return phase(iic, self.nDIA, self.ntsDIA, self.ntstart, self.nrrec)

    def shape(self, name):
        """Extents of the host array of a term's plane or of a reserved id."""
        b = self.b
        ni, nj = b.UBi - b.LBi + 1, b.UBj - b.LBj + 1
        return (ni, nj, b.N) if DIA_ID[name] < DIA_COUNT else (ni, nj)

    def c_args(self):
        """The arguments of roms_hip_set_diagnostics."""
        return (self.nDIA, self.ntsDIA, self.ntstart, self.nrrec)
