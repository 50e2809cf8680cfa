"""CPU: the ISO_C_BINDING shim module compiles with flang (when present); its field-id constants agree with
include/roms_fields.def and its three TYPE, BIND(C) mirrors agree member for member with the tables of
include/ (roms_bounds.def, roms_params.def, roms_step_idx.def)."""
import os
import re
import shutil
import subprocess

import pytest

from roms_trunk_mgh_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "roms_trunk_mgh_amd", "fortran", "roms_hip_mod.F90")


def test_field_ids_match_def_file():
    pairs = re.findall(r"FID_(\w+)=(\d+)", open(SRC).read())
    assert len(pairs) == len(abi.FIELDS)
    assert all(abi.FIELD_ID[n] == int(v) for n, v in pairs)


def _split_top(text):
    """Split at the commas that are not inside parentheses."""
    out, depth, cur = [], 0, ""
    for ch in text:
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    return [x.strip() for x in out + [cur]]


def fortran_types(text):
    """{type name: [(C type, member name, C extents)]} of the TYPE, BIND(C) blocks of a Fortran source.  Named
    extents are resolved with the module's own INTEGER, PARAMETER constants; the extents come back in C order
    (lbc(6,4) = lbc[4][6]).  Every line of a block has to be a declaration this parser understands."""
    code = [ln.split("!")[0].strip() for ln in text.splitlines()]
    const = {}
    for ln in code:
        m = re.match(r"INTEGER, PARAMETER, PUBLIC :: (.*)", ln)
        if m:
            const.update((k.strip(), int(v)) for k, v in (x.split("=") for x in m.group(1).split(",")))

    def extent(e):
        m = re.fullmatch(r"(\w+)(?:\s*\+\s*(\d+))?", e)
        assert m, e
        return (int(m.group(1)) if m.group(1).isdigit() else const[m.group(1)]) + int(m.group(2) or 0)

    kinds = {"INTEGER(c_int)": "int", "REAL(c_double)": "double"}
    out, cur = {}, None
    for ln in code:
        m = re.match(r"TYPE, BIND\(C\)(?:, PUBLIC)? :: (\w+)$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif re.match(r"END TYPE\b", ln):
            cur = None
        elif cur is not None and ln:
            kind, sep, decls = ln.partition(" :: ")
            assert sep and "&" not in ln, ln
            for d in _split_top(decls):
                m = re.fullmatch(r"(\w+)(?:\((.*)\))?", d)
                assert m, ln
                ext = tuple(extent(e) for e in reversed(_split_top(m.group(2)))) if m.group(2) else ()
                cur.append((kinds.get(kind.strip(), kind.strip()), m.group(1), ext))
    return out, const


def test_struct_mirrors_match_the_member_tables():
    """TYPE(roms_bounds_t), TYPE(roms_params_t), TYPE(roms_step_idx_t) of roms_hip_mod declare the members of the C
    structs (abi.STRUCTS = the tables roms_hip.h expands) in the same order, with the same kind, the same name
    (case-sensitively: an integrator fills them by name) and the same extents; the module's limits are the header's."""
    types, const = fortran_types(open(SRC).read())
    assert const == {n: abi.CONSTANTS[n] for n in ("ROMS_MAXN", "ROMS_MAXNT", "ROMS_MAXFAST")}
    for name, members in abi.STRUCTS.items():
        assert types[name] == members, name
    assert [len(types[n]) for n in ("roms_params_t", "roms_bounds_t", "roms_step_idx_t")] == [90, 63, 10]
    # the check sees what a size comparison cannot: two neighbours swapped, a member missing, an extent changed
    txt = open(SRC).read()
    for old, new in [("uv_adv, uv_cor", "uv_cor, uv_adv"), (":: nstp, nnew, nrhs", ":: nstp, nrhs"),
                     ("Hadv(ROMS_MAXNT)", "Hadv(ROMS_MAXN)"), ("lbc(6,4)", "lbc(4,6)"), ("Tcoef", "TCoef")]:
        assert txt.count(old) == 1, old
        bad, _ = fortran_types(txt.replace(old, new))
        assert any(bad[n] != abi.STRUCTS[n] for n in abi.STRUCTS), (old, new)


def test_reference_wrapper_mirrors_match_the_member_tables():
    """oracle/ref_wrap.F90, which hands the same blocks to the reference's own routines and reads them by name,
    keeps a copy of the bounds and the parameter block too: same members, same order, same extents."""
    types, _ = fortran_types(open(os.path.join(ROOT, "oracle", "ref_wrap.F90")).read())
    assert types["bounds_t"] == abi.STRUCTS["roms_bounds_t"]
    assert types["params_t"] == abi.STRUCTS["roms_params_t"]
    assert [(k, e) for k, _, e in types["stepidx_t"]] == [(k, e) for k, _, e in abi.STRUCTS["roms_step_idx_t"]]


@pytest.mark.skipif(shutil.which("flang") is None, reason="flang not installed")
def test_shim_compiles(tmp_path):
    r = subprocess.run(["flang", "-c", SRC, "-o", str(tmp_path / "m.o"), "-module-dir", str(tmp_path)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(shutil.which("flang") is None, reason="flang not installed")
def test_fortran_struct_mirrors_have_the_abi_sizes(tmp_path):
    """TYPE(roms_bounds_t), TYPE(roms_params_t), TYPE(roms_step_idx_t), TYPE(roms_halo_msg_t) of roms_hip_mod
    occupy exactly the bytes the C structs do (roms_abi_sizeof / ctypes mirror)."""
    import ctypes
    from roms_trunk_mgh_amd import hip
    prog = tmp_path / "sz.F90"
    prog.write_text("""program sz
  use, intrinsic :: iso_c_binding
  use roms_hip_mod
  type(roms_bounds_t) :: b
  type(roms_params_t) :: p
  type(roms_step_idx_t) :: s
  type(roms_halo_msg_t) :: m
  print '(4(i0,1x))', c_sizeof(b), c_sizeof(p), c_sizeof(s), c_sizeof(m)
end program
""")
    r = subprocess.run(["flang", "-c", SRC, "-o", "m.o"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["flang", str(prog), "m.o", "-o", "sz"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(abi.Bounds), ctypes.sizeof(abi.Params), ctypes.sizeof(abi.StepIdx),
                                     ctypes.sizeof(hip.HaloMsg)]
