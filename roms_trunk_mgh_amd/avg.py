"""Time-averaged fields (AVERAGES): the host-side image of what an application selects with the Aout switches of its
roms_*.in and nAVG / ntsAVG, the table of the averages (include/roms_avg.def, the file the C side compiles) and the
schedule of set_avg_tile (ROMS/Nonlinear/set_avg.F:237-240, :1264, :2298-2301) with that of set_avg_masks
(ROMS/Utility/set_masks.F:466-468).  `phase` mirrors roms_hip_avg_phase of csrc/k_avg.hip; tests/test_avg.py holds both
against a table written out by hand.

Only the HIP path computes averages: main3d.Main3D(backend, averages=Averages(...)) issues set_avg after set_zeta
(main3d.F:493-495), and the host fetches the closed windows with RomsHip.get_average."""
import ctypes as C
import re

import numpy as np

from . import abi

_IP = C.POINTER(C.c_int)
SET, ADD, CLOSE, MASKS = 1, 2, 4, 8          # the bits of roms_hip_avg_phase


def _lines():
    """The lines of roms_avg.def in the order of enum roms_avg_id."""
    out = []
    for kind, args in re.findall(r"\bROMS_AVG(_NOT_BUILT|_COUNTER|)\(([^()]*)\)", abi._read("roms_avg.def")):
        a = [x.strip() for x in args.split(",")]
        if kind == "":
            keys = ("name", "aout", "grid", "shape", "mask", "range", "expr", "srcA", "srcB", "plane")
            d = dict(zip(keys, a), kind="avg")
            d["plane"] = int(d["plane"])
        elif kind == "_NOT_BUILT":
            d = dict(name=a[0], aout=a[1], why=", ".join(a[2:]), kind="not_built")
        else:
            d = dict(name=a[0], grid=a[1], shape="AVS_2D", kind="counter")
        out.append(d)
    return out


LINES = _lines()
AVG_ID = {d["name"]: i for i, d in enumerate(LINES)}
AVG_COUNT = len(LINES)
BUILT = [d["name"] for d in LINES if d["kind"] == "avg"]
NOT_BUILT = [d["name"] for d in LINES if d["kind"] == "not_built"]
COUNTERS = [d["name"] for d in LINES if d["kind"] == "counter"]
TRACER_KINDS = [d["name"] for d in LINES if d["kind"] == "avg" and d["shape"] == "AVS_NT"]     # the rows of AoutT
assert len(TRACER_KINDS) == abi.CONSTANTS["ROMS_AVG_NTKINDS"]


def phase(iic, nAVG, ntsAVG, ntstart, nrrec):
    """What set_avg does at time step iic: a sum of SET (initialise), ADD (accumulate), CLOSE (scale) and MASKS (clamp
    the WET_DRY counters); 0 with nAVG = 0."""
    if nAVG <= 0:                                                                       # set_avg.F:189
        return 0
    ph = 0
    restart = nrrec > 0 and iic == ntstart
    if (iic > ntsAVG and (iic - 1) % nAVG == 1) or (iic >= ntsAVG and nAVG == 1) or restart:       # :237-240
        ph |= SET
    elif iic > ntsAVG:                                                                  # :1264
        ph |= ADD
    window_end = iic > ntsAVG and (iic - 1) % nAVG == 0 and not restart
    if window_end or (iic >= ntsAVG and nAVG == 1):                                     # :2298-2301
        ph |= CLOSE
    if window_end:                                                                      # set_masks.F:466-468
        ph |= MASKS
    return ph


class Averages:
    """The selection: nAVG, ntsAVG, ntstart, nrrec and the averages switched on.  select: names of roms_avg.def that
    are not per tracer; tracers: {per-tracer name: tracers (1-based)}.  A name the library does not build may be
    selected here -- roms_hip_set_averages refuses it by name, as it refuses an average whose source is missing."""

    def __init__(self, bounds, nAVG, ntsAVG=1, ntstart=1, nrrec=0, select=(), tracers=None):
        b = bounds
        self.b = b
        self.nAVG, self.ntsAVG, self.ntstart, self.nrrec = int(nAVG), int(ntsAVG), int(ntstart), int(nrrec)
        self.Aout = np.zeros(AVG_COUNT, dtype=np.int32)
        self.AoutT = np.zeros((len(TRACER_KINDS), b.NT), dtype=np.int32)
        for name in select:
            if name not in AVG_ID or name in COUNTERS:
                raise ValueError(f"{name} is not an average of roms_avg.def")
            if name in TRACER_KINDS:
                raise ValueError(f"{name} is selected per tracer: tracers={{'{name}': [...]}}")
            self.Aout[AVG_ID[name]] = 1
        for name, its in (tracers or {}).items():
            if name not in TRACER_KINDS:
                raise ValueError(f"{name} is not a per-tracer average of roms_avg.def")
            for it in its:
                if not 1 <= it <= b.NT:
                    raise ValueError(f"{name}: tracer {it} outside 1..{b.NT}")
                self.AoutT[TRACER_KINDS.index(name), it - 1] = 1

    def selected(self):
        """[(name, itrc)] in the order of the library's arrays; itrc = 0 for an average that is not per tracer."""
        out = []
        for d in LINES:
            if d["kind"] == "counter":
                continue
            name = d["name"]
            if name in TRACER_KINDS:
                out += [(name, it + 1) for it in range(self.b.NT) if self.AoutT[TRACER_KINDS.index(name), it]]
            elif self.Aout[AVG_ID[name]]:
                out.append((name, 0))
        return out

    def shape(self, name):
        """Extents of the library's array of an average or a counter."""
        b = self.b
        ni, nj = b.UBi - b.LBi + 1, b.UBj - b.LBj + 1
        trail = {"AVS_2D": (), "AVS_N": (b.N,), "AVS_W": (b.N + 1,), "AVS_NT": (b.N,)}[LINES[AVG_ID[name]].get("shape", "AVS_2D")]
        return (ni, nj) + trail

    def phase(self, iic):
        return phase(iic, self.nAVG, self.ntsAVG, self.ntstart, self.nrrec)

    def c_args(self):
        """The arguments of roms_hip_set_averages."""
        assert self.AoutT.flags["C_CONTIGUOUS"]              # AoutT[kind][NT]
        return (self.nAVG, self.ntsAVG, self.ntstart, self.nrrec, self.Aout.ctypes.data_as(_IP),
                self.AoutT.ctypes.data_as(_IP))
