"""Forcing, climatology and open-boundary snapshots (set_data, ROMS/Nonlinear/set_data.F): the table of the targets the
library interpolates in time on the device (include/roms_data.def, the file the C side compiles) and `Data`, the
host-side image of what get_data keeps per field: the two time records Finp(..., 1:2), their times Tintrp(1:2), the slot
of the latest read Tindex = Iinfo(8) and Lonerec = Linfo(3).

Only the HIP path interpolates records: main3d.Main3D(backend, data=Data(...)) hands every record over
(RomsHip.set_data_record / set_data_point) and issues set_data at the place of main3d.F:222; a record loaded during the
run goes through Data.load(...), which hands it over as well."""
import re

import numpy as np

from . import abi

SIDES = ("west", "east", "south", "north")          # enum roms_lbc_side


def _lines():
    """The lines of roms_data.def in the order of enum roms_data_id."""
    keys = ("name", "routine", "grid", "shape", "dest")
    return [dict(zip(keys, (x.strip() for x in args.split(","))))
            for args in re.findall(r"\bROMS_DATA\(([^()]*)\)", abi._read("roms_data.def"))]


LINES = _lines()
DATA_ID = {d["name"]: i for i, d in enumerate(LINES)}
DATA_COUNT = len(LINES)
GRIDDED = [d["name"] for d in LINES if d["dest"] == "DD_FIELD"]
CLIMA = [d["name"] for d in LINES if d["dest"] == "DD_CLIMA"]
BOUNDARY = [d["name"] for d in LINES if d["dest"] == "DD_BRY"]
INDEXED = [d["name"] for d in LINES if d["shape"] in ("DS_2DT", "DS_NC", "DS_ENT")]


def record_shape(bounds, name, side=None):
    """Extents of one record of target `name` (side: a name of SIDES or its code, for an open-boundary target)."""
    b = bounds
    ni, nj = b.UBi - b.LBi + 1, b.UBj - b.LBj + 1
    shape = LINES[DATA_ID[name]]["shape"]
    if shape in ("DS_2D", "DS_2DT"):
        return (ni, nj)
    if shape in ("DS_N", "DS_NC"):
        return (ni, nj, b.N)
    sd = SIDES.index(side) if isinstance(side, str) else int(side)
    along = nj if sd <= 1 else ni
    return (along,) if shape == "DS_E" else (along, b.N)


class Data:
    """The records of a run.  A key is (name, index, side): index = itrc (1-based) of stflux / btflux / t_bry or the
    compact index ic of tclm, 0 otherwise; side = a name of SIDES for an open-boundary target, None otherwise."""

    def __init__(self, bounds):
        self.b = bounds
        self.rec = {}            # key -> dict(slot={1: array or float, 2: ...}, Tintrp={1: s, 2: s}, Tindex, onerec, point)
        self.backend = None

    @staticmethod
    def key(name, index=0, side=None):
        if name not in DATA_ID:
            raise ValueError(f"{name} is not a target of roms_data.def")
        return (name, int(index) if name in INDEXED else 0, side if name in BOUNDARY else None)

    def load(self, name, slot, Tintrp, record, index=0, side=None, onerec=False, point=False):
        """What get_data leaves after reading one record: Finp(..., slot) (or Fpoint(slot) with point=True),
        Tintrp(slot), Tindex = slot.  With a backend attached (Main3D does that) the record goes to the device too."""
        k = self.key(name, index, side)
        r = self.rec.setdefault(k, dict(slot={}, Tintrp={}, Tindex=slot, onerec=False, point=bool(point)))
        if point:
            value = float(record)
        else:
            value = np.asfortranarray(record, dtype=np.float64)
            want = record_shape(self.b, name, side)
            if value.shape != want:
                raise ValueError(f"{name}: a record has the extents {want}, not {value.shape}")
        r["slot"][slot], r["Tintrp"][slot], r["Tindex"], r["onerec"], r["point"] = value, float(Tintrp), slot, bool(onerec), bool(point)
        if self.backend is not None:
            self._hand_over(self.backend, k, slot)

    def _hand_over(self, be, k, slot):
        name, index, side = k
        r = self.rec[k]
        if r["point"]:
            be.set_data_point(name, slot, r["Tintrp"][slot], r["slot"][slot], index=index, onerec=r["onerec"])
        else:
            be.set_data_record(name, slot, r["Tintrp"][slot], r["slot"][slot], index=index, side=side, onerec=r["onerec"])

    def attach(self, backend):
        """Hand every record over, the slot of the latest read last (it becomes Tindex)."""
        self.backend = backend
        for k, r in self.rec.items():
            for slot in sorted(r["slot"], key=lambda s: s == r["Tindex"]):
                self._hand_over(backend, k, slot)
