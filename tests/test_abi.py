"""CPU: the C-ABI library loads without a GPU and exports every symbol
include/roms_hip.h declares; struct layouts match the ctypes mirror; the HIP
path fails loudly (no fallback) when no device is present.  The three structs of the boundary are compared member
for member (offset, size, type) and the enum mirrors value for value with what a C compiler makes of the header."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from roms_trunk_mgh_amd import abi, ana, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "roms_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(roms_hip_\w+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    lib = hip.load()
    names = _declared()
    assert len(names) >= 30
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(hip.DECLARED_SYMBOLS) <= set(names)


def test_struct_layouts_match():
    abi.check_abi(hip.load())
    import oracle
    abi.check_abi(oracle.lib())
    assert len(abi.FIELDS) == len(set(n for n, _, _ in abi.FIELDS))


_STRUCTS = [("roms_bounds_t", "roms_bounds.def", abi.Bounds), ("roms_params_t", "roms_params.def", abi.Params),
            ("roms_step_idx_t", "roms_step_idx.def", abi.StepIdx)]


def test_member_offsets_match_the_c_compiler(tmp_path):
    """A C program that includes roms_hip.h expands the member tables into offsetof / sizeof of every member of the
    three structs; name, offset, size and element type equal those of the ctypes classes, in order.  The sizes are
    asserted literally: a layout change cannot pass by changing both sides at once.  The same program prints every
    constant abi.py parsed out of the header (limits, enumerators)."""
    sections = "".join(f"""
  printf("struct {s} %zu\\n", sizeof({s}));
#define S {s}
#include "{d}"
#undef S""" for s, d, _ in _STRUCTS)
    consts = "".join(f'  printf("const {n} %d\\n", (int){n});\n' for n in abi.CONSTANTS)
    (tmp_path / "off.c").write_text(f"""#include <stddef.h>
#include <stdio.h>
#include "roms_hip.h"
#define ROMS_MEMBER(type, name) printf(#type " " #name " %zu %zu\\n", offsetof(S, name), sizeof(((S *)0)->name));
#define ROMS_MEMBER_A(type, name, n) ROMS_MEMBER(type, name)
#define ROMS_MEMBER_A2(type, name, n1, n2) ROMS_MEMBER(type, name)
int main(void)
{{{sections}
{consts}  return 0;
}}
""")
    r = subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "off.c", "-o", "off"],
                       cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(tmp_path / "off")], capture_output=True, text=True, check=True).stdout.splitlines()
    got, sizes, consts = {}, {}, {}
    for line in out:
        w = line.split()
        if w[0] == "struct":
            cur = got.setdefault(w[1], [])
            sizes[w[1]] = int(w[2])
        elif w[0] == "const":
            consts[w[1]] = int(w[2])
        else:
            cur.append((w[0], w[1], int(w[2]), int(w[3])))
    assert consts == abi.CONSTANTS and len(consts) >= 50
    assert sizes == {"roms_bounds_t": 252, "roms_params_t": 7376, "roms_step_idx_t": 40}
    n_members = 0
    for s, _, cls in _STRUCTS:
        want = []
        for name, t in cls._fields_:
            f = getattr(cls, name)
            while hasattr(t, "_length_"):
                t = t._type_
            want.append(({ctypes.c_int: "int", ctypes.c_double: "double"}[t], name, f.offset, f.size))
        assert [(t, abi.py_name(n), o, z) for t, n, o, z in got[s]] == want, s
        assert ctypes.sizeof(cls) == sizes[s]
        n_members += len(want)
    print(f"{n_members} members, sizeof = {sizes}")
    assert n_members == 163
    assert abi.Bounds._names == [n for _, n, _ in abi.STRUCTS["roms_bounds_t"]] and "lambda_" in dict(abi.Params._fields_)


def test_enum_mirrors_equal_the_header():
    """abi.ADV, PGF, GLS_STAB, KINDS, LBV, LBS and the LBC_* constants carry the values of the enumerators of
    roms_hip.h (abi.CONSTANTS, which test_member_offsets_match_the_c_compiler checks against the C compiler), and
    no enumerator is left without its mirror."""
    def enum(prefix):
        return {n[len(prefix):]: v for n, v in abi.CONSTANTS.items() if n.startswith(prefix)}
    assert {k.upper(): v for k, v in abi.ADV.items()} == enum("ADV_") and len(abi.ADV) == 8
    assert abi.PGF == enum("PGF_") and len(abi.PGF) == 4
    assert abi.GLS_STAB == enum("GLS_") and len(abi.GLS_STAB) == 4
    assert {k: i for i, k in enumerate(abi.KINDS)} == {"K_" + k: v for k, v in enum("K_").items()} and len(abi.KINDS) == 12
    lbv = enum("LBV_")
    assert lbv.pop("COUNT") == abi.LBV_COUNT == len(abi.LBV) == 6
    assert {k.upper(): v for k, v in abi.LBV.items()} == lbv
    assert {k.upper(): v for k, v in abi.LBS.items()} == enum("LBS_") and len(abi.LBS) == 4
    lbc = enum("LBC_")
    for name in ("PERIODIC", "CLOSED", "GRADIENT", "CLAMPED", "CHAPMAN_IMPLICIT", "FLATHER", "RADIATION"):
        assert getattr(abi, "LBC_" + name) == lbc[name], name
    assert sorted(abi.LBC.values()) == sorted(lbc.values()) == list(range(11))
    assert (abi.ROMS_MAXN, abi.ROMS_MAXNT, abi.ROMS_MAXFAST) == (64, 16, 256)


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_no_cpu_fallback():
    st = ana.make_tile("SEAMOUNT")
    with pytest.raises(RuntimeError) as e:
        hip.RomsHip(st)
    assert "init" in str(e.value)


def test_entries_refuse_uninitialised_library():
    lib = hip.load()
    s = abi.StepIdx(iic=1, ntfirst=1, nstp=1, nnew=2, nrhs=1, kstp=1, krhs=1, knew=2, iif=1, predictor_2d_step=0)
    lib.roms_hip_finalize()
    rc = lib.roms_hip_step3d_t(ctypes.byref(s))
    assert rc != 0
    assert b"not initialised" in lib.roms_hip_last_error()


def test_guarded_arrays_is_exported_and_refuses_uninitialised_library():
    lib = hip.load()
    assert hasattr(lib, "roms_hip_guarded_arrays") and "roms_hip_guarded_arrays" in hip.DECLARED_SYMBOLS
    lib.roms_hip_finalize()
    buf = ctypes.create_string_buffer(64)
    assert lib.roms_hip_guarded_arrays(None, 0) < 0
    assert b"roms_hip_guarded_arrays" in lib.roms_hip_last_error() and b"not initialised" in lib.roms_hip_last_error()
    assert lib.roms_hip_guarded_arrays(buf, len(buf)) < 0 and buf.value == b""


def test_tile_neighbors_matches_python_mirror():
    from roms_trunk_mgh_amd import halo
    for (nI, nJ) in [(1, 1), (2, 1), (4, 1), (4, 2), (2, 2), (1, 2), (3, 3)]:
        for ng in (2, 3):
            for ew in (True, False):
                for ns in (True, False):
                    for r in range(nI * nJ):
                        a = hip.tile_neighbors(r, nI, nJ, ng, ng, ew, ns)
                        bq = halo.tile_neighbors(r, nI, nJ, ng, ng, ew, ns)
                        assert a == bq, (nI, nJ, ng, ew, ns, r, a, bq)
    # the documented BENCHMARK3 4x2 case: rank 3 -> east neighbour 0
    n = hip.tile_neighbors(3, 4, 2, 2, 2, True, False)
    assert (n["Etile"], n["Wtile"], n["Ntile"], n["Stile"]) == (0, 2, 7, -1)
    assert n["GsendE"] == 3 and hip.tile_neighbors(0, 4, 2, 2, 2, True, False)["GrecvW"] == 3


@pytest.mark.parametrize("nI,nJ,ng", [(4, 2, 2), (4, 2, 3), (2, 2, 2), (3, 3, 2), (2, 1, 2), (1, 2, 2), (4, 1, 3), (3, 2, 2)])
def test_halo_plan_fills_every_ghost_point(nI, nJ, ng):
    """Play one halo update of a whole tiling on the host with the library's own message plan (one phase,
    up to eight messages per tile, corners from the diagonal tiles): k-th send of A to B pairs with the
    k-th receive of B from A (RCCL's rule, no tags), counts agree, and afterwards every ghost point of every
    tile holds the owner's value -- including across the periodic seam (Nghost+1 rule) and in the corners."""
    from roms_trunk_mgh_amd import bounds as B
    Lm, Mm = 48, 20
    G = np.arange((Lm + 1) * (Mm + 2), dtype=np.float64).reshape(Lm + 1, Mm + 2) + 0.5     # G[i, j], i = 1..Lm
    wrap = lambda i: (i - 1) % Lm + 1
    tiles = []
    for r in range(nI * nJ):
        b = B.make_bounds(Lm, Mm, 4, 2, 2, ntileI=nI, ntileJ=nJ, tile=r, NghostPoints=ng)
        a = np.full((b.UBi - b.LBi + 1, b.UBj - b.LBj + 1), np.nan)
        jlo = b.Jstr - 1 if b.south_edge else b.Jstr            # wall rows 0 and Mm+1 belong to the edge tiles
        jhi = b.Jend + 1 if b.north_edge else b.Jend
        for i in range(b.Istr, b.Iend + 1):
            a[i - b.LBi, jlo - b.LBj:jhi - b.LBj + 1] = G[i, jlo:jhi + 1]
        if nI == 1:                                             # one tile column: periodic copy is local
            for i in list(range(b.LBi, 1)) + list(range(Lm + 1, Lm + ng + 1)):
                a[i - b.LBi, :] = a[wrap(i) - b.LBi, :]
        tiles.append((b, a, *hip.halo_plan(b, r)))
    # post: queues per (src, dst) in list order
    queues = {}
    for r, (b, a, sends, recvs) in enumerate(tiles):
        for m in sends:
            blk = a[m["i0"] - b.LBi:m["i0"] - b.LBi + m["wi"], m["j0"] - b.LBj:m["j0"] - b.LBj + m["wj"]].copy()
            queues.setdefault((r, m["peer"]), []).append((m["tag"], blk))
    for r, (b, a, sends, recvs) in enumerate(tiles):
        assert len(sends) == len(recvs) <= 8
        for m in recvs:
            tag, blk = queues[(m["peer"], r)].pop(0)
            assert tag == m["tag"], (r, m, tag)
            assert blk.shape == (m["wi"], m["wj"]), (r, m, blk.shape)
            a[m["i0"] - b.LBi:m["i0"] - b.LBi + m["wi"], m["j0"] - b.LBj:m["j0"] - b.LBj + m["wj"]] = blk
    assert all(len(q) == 0 for q in queues.values())
    for r, (b, a, _, _) in enumerate(tiles):
        # periodic images the reference defines: i = -2..0 (three, whatever NghostPoints) and Lm+1..Lm+ng
        for i in range(max(b.LBi, -2), min(b.UBi, Lm + ng) + 1):
            for j in range(max(b.LBj, 0), min(b.UBj, Mm + 1) + 1):
                assert a[i - b.LBi, j - b.LBj] == G[wrap(i), j], (r, i, j)


def test_reduce_diag_and_host_clock():
    """Host-side helpers of main3d.py: the reduction of the tile-local diag vectors (diag.F:398-420) and the
    clock handed to ana_srflux (caldate with TIME_REF = 0; pinned against the reference in test_ref_pinning.py)."""
    from roms_trunk_mgh_amd import main3d
    a = np.array([10.0, 2.0, 3.0, 0.5, 27.0, 0.10, 0.04, 0.05, 0.01, 7, 8, 9])
    b = np.array([20.0, 1.0, 5.0, 0.7, 26.0, 0.30, 0.10, 0.15, 0.05, 17, 18, 19])
    r = main3d.reduce_diag([a, b])
    assert list(r[0:3]) == [30.0, 3.0, 8.0] and list(r[3:5]) == [0.7, 27.0]
    assert list(r[5:12]) == list(b[5:12])                      # MAXLOC: the tile with the larger Courant number
    assert main3d.host_clock(0.0) == (1.0, 0.0)
    yd, hr = main3d.host_clock(150.0 / 86400.0)                # one BENCHMARK step later
    assert abs(yd - (1.0 + 150.0 / 86400.0)) < 1e-12 and abs(hr - 150.0 / 3600.0) < 1e-12
    yd, hr = main3d.host_clock(10.5)
    assert abs(yd - 11.5) < 1e-12 and hr == 12.0
    with pytest.raises(ValueError):
        main3d.host_clock(400.0)
