"""ctypes mirror of include/roms_hip.h (the C ABI).

The field table (roms_fields.def), the members of the three structs (roms_bounds.def, roms_params.def,
roms_step_idx.def) and the limits ROMS_MAXN ... are parsed from the files the C side compiles, so that the C side
and the Python side cannot drift apart; the struct sizes are checked at load time against ``roms_abi_sizeof``
exported by both shared libraries, every member's offset by tests/test_abi.py.
"""
import ctypes as C
import keyword
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE_DIR = os.path.join(ROOT, "include")


def _read(name):
    """A file of include/ without its C comments."""
    with open(os.path.join(INCLUDE_DIR, name)) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def _constants():
    """The integer constants of roms_hip.h: its `#define NAME integer` lines and the enumerators of its enums
    (roms_field_id, which expands roms_fields.def, is FIELD_ID below)."""
    txt = _read("roms_hip.h")
    out = {n: int(v) for n, v in re.findall(r"^#define\s+(\w+)\s+(\d+)\s*$", txt, flags=re.M)}
    for body in re.findall(r"\benum\s+\w+\s*\{([^{}#]*)\}", txt):
        nxt = 0
        for item in body.split(","):
            name, _, val = (x.strip() for x in item.partition("="))
            out[name] = nxt = int(val) if val else nxt
            nxt += 1
    return out


CONSTANTS = _constants()
ROMS_MAXN, ROMS_MAXNT, ROMS_MAXFAST = (CONSTANTS[n] for n in ("ROMS_MAXN", "ROMS_MAXNT", "ROMS_MAXFAST"))
LBV_COUNT = CONSTANTS["LBV_COUNT"]

KINDS = ["K_2D", "K_2D_T2", "K_2D_T3", "K_2D_NT", "K_3DR", "K_3DW",
         "K_3DR_T2", "K_3DW_T2", "K_3DW_NAT", "K_4DT", "K_3DR_NT", "K_3DW_T3"]

# enum roms_adv (T_ADV logical records, ROMS/Modules/mod_param.F:382-394)
ADV = {"C2": 0, "C4": 1, "A4": 2, "U3": 3, "SU3": 4, "SPLINES": 5,
       "MPDATA": 6, "HSIMT": 7}
GLS_STAB = {"GALPERIN": 0, "KANTHA_CLAYSON": 1, "CANUTO_A": 2, "CANUTO_B": 3}            # enum roms_gls_stab
PGF = {"DJ_GRADPS": 0, "STANDARD": 1, "WJ_GRADP": 2, "PJ_GRADP": 3}         # enum roms_pgf (prsgrd.F:16-26)
LBC_PERIODIC, LBC_CLOSED, LBC_GRADIENT, LBC_CLAMPED, LBC_CHAPMAN_IMPLICIT, LBC_FLATHER, LBC_RADIATION = range(7)
LBC = {"Per": 0, "Clo": 1, "Gra": 2, "Cla": 3, "Cha": 4, "Fla": 5, "Rad": 6, "RadNud": 7, "Che": 8, "Shc": 9, "Red": 10}      # the keywords of roms_*.in
UV_HADV = {"U3": 0, "C2": 1, "C4": 2}                     # enum roms_uv_hadv
UV_VADV = {"C4W": 0, "C2": 1, "C4": 2, "SPLINES": 3}      # enum roms_uv_vadv
# the pairs the reference can be compiled to (none; UV_SADVECTION; UV_C2ADVECTION [+ S]; UV_C4ADVECTION [+ S])
UV_ADV_PAIRS = [("U3", "C4W"), ("U3", "SPLINES"), ("C2", "C2"), ("C2", "SPLINES"), ("C4", "C4"), ("C4", "SPLINES")]


def uv_adv(h="U3", v="C4W"):
    """ROMS_UV_ADV(h, v) of roms_hip.h: the value of roms_params_t.uv_adv for a horizontal and a vertical scheme
    (names of UV_HADV / UV_VADV, or their codes); uv_adv() = 1 is the default pair."""
    return 1 | (UV_HADV.get(h, h) << 4) | (UV_VADV.get(v, v) << 8)


LBV = {"zeta": 0, "ubar": 1, "vbar": 2, "u": 3, "v": 4, "t": 5}
LBS = {"west": 0, "east": 1, "south": 2, "north": 3}


FIELDS = re.findall(r"\bROMS_FIELD\(\s*(\w+)\s*,\s*(\w+)\s*,\s*(\w+)\s*\)", _read("roms_fields.def"))   # [(name, kind, owner)]
FIELD_ID = {n: i for i, (n, _, _) in enumerate(FIELDS)}
FIELD_KIND = {n: k for n, k, _ in FIELDS}


def trailing_shape(kind, N, NT, NAT):
    """Trailing dimensions (after LBi:UBi,LBj:UBj) of a field kind."""
    return {
        "K_2D": (), "K_2D_T2": (2,), "K_2D_T3": (3,), "K_2D_NT": (NT,),
        "K_3DR": (N,), "K_3DW": (N + 1,), "K_3DR_T2": (N, 2),
        "K_3DW_T2": (N + 1, 2), "K_3DW_NAT": (N + 1, NAT), "K_4DT": (N, 3, NT), "K_3DR_NT": (N, NT),
        "K_3DW_T3": (N + 1, 3),
    }[kind]


def _extent(text):
    """An array extent of a member table: an integer, a constant of roms_hip.h, or a constant + an integer."""
    m = re.fullmatch(r"(\w+)(?:\s*\+\s*(\d+))?", text.strip())
    if not m:
        raise ValueError(f"array extent {text!r}: expected INTEGER, NAME or NAME + INTEGER")
    base = m.group(1)
    return (int(base) if base.isdigit() else CONSTANTS[base]) + int(m.group(2) or 0)


def _parse_members(def_file):
    """[(C type, C name, extents)] of one struct from its X-macro table: ROMS_MEMBER(type, name),
    ROMS_MEMBER_A(type, name, n), ROMS_MEMBER_A2(type, name, n1, n2)."""
    out = []
    for args in re.findall(r"\bROMS_MEMBER(?:_A2?)?\(([^()]*)\)", _read(def_file)):
        ctype, name, *ext = (a.strip() for a in args.split(","))
        out.append((ctype, name, tuple(_extent(e) for e in ext)))
    return out


# the structs of the C ABI, member for member as include/roms_hip.h declares them: the three of the boundary and the
# parameter block of the NPZD_POWELL biology (roms_hip_set_biology)
STRUCTS = {"roms_bounds_t": _parse_members("roms_bounds.def"),
           "roms_params_t": _parse_members("roms_params.def"),
           "roms_step_idx_t": _parse_members("roms_step_idx.def"),
           "roms_bio_powell_t": _parse_members("roms_bio.def"),
           "roms_bio_fennel_t": _parse_members("roms_bio_fennel.def")}
_CTYPES = {"int": C.c_int, "double": C.c_double}


def py_name(c_name):
    """Python spelling of a C member name (`lambda` is a keyword: `lambda_`)."""
    return c_name + "_" if keyword.iskeyword(c_name) else c_name


def _ctypes_fields(members):
    out = []
    for ctype, name, ext in members:
        t = _CTYPES[ctype]
        for n in reversed(ext):                 # int lbc[4][6] = (c_int * 6) * 4
            t = t * n
        out.append((py_name(name), t))
    return out


class Bounds(C.Structure):
    """roms_bounds_t -- ROMS/Include/set_bounds.h:20-79, tile.h:21-45."""
    _fields_ = _ctypes_fields(STRUCTS["roms_bounds_t"])
    _names = [n for n, _ in _fields_]

    def as_dict(self):
        return {n: getattr(self, n) for n in self._names}


class Params(C.Structure):
    """roms_params_t -- scalars of mod_scalars.F / mod_param.F used on the path."""
    _fields_ = _ctypes_fields(STRUCTS["roms_params_t"])


class StepIdx(C.Structure):
    """roms_step_idx_t -- mod_stepping.F indices, main3d.F:189-191,597-662."""
    _fields_ = _ctypes_fields(STRUCTS["roms_step_idx_t"])


class BioPowell(C.Structure):
    """roms_bio_powell_t -- the parameters of npzd_Powell_mod.h / npzd_Powell.in, idbio and Cp (roms_bio.def)."""
    _fields_ = _ctypes_fields(STRUCTS["roms_bio_powell_t"])


class BioFennel(C.Structure):
    """roms_bio_fennel_t -- the switches, idbio, the parameters of fennel_mod.h / bio_Fennel.in and Cp (roms_bio_fennel.def); the
    library does not take it yet."""
    _fields_ = _ctypes_fields(STRUCTS["roms_bio_fennel_t"])


# enum roms_bio_model: the ecosystem models of the reference; only NPZD_POWELL is built
BIO_MODEL = {n[len("ROMS_BIO_"):]: v for n, v in CONSTANTS.items() if n.startswith("ROMS_BIO_")}


class Fields(C.Structure):
    """roms_fields_t -- one double* per module array."""
    _fields_ = [(n, C.POINTER(C.c_double)) for n, _, _ in FIELDS]


def check_abi(lib):
    """Compare struct sizes with the C side (0=bounds 1=params 2=step 3=fields)."""
    lib.roms_abi_sizeof.restype = C.c_int
    lib.roms_abi_sizeof.argtypes = [C.c_int]
    want = [C.sizeof(Bounds), C.sizeof(Params), C.sizeof(StepIdx), C.sizeof(Fields)]
    got = [lib.roms_abi_sizeof(i) for i in range(4)]
    if want != got:
        raise RuntimeError(f"ABI struct size mismatch python={want} C={got}")
    lib.roms_abi_sizeof.argtypes = [C.c_int]
    if lib.roms_abi_sizeof(4) != len(FIELDS):
        raise RuntimeError("ABI field-count mismatch")
