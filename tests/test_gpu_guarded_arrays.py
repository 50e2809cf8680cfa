"""-m gpu: every guarded device array registers itself (roms_hip_guarded_arrays, csrc/capi.hip).

roms_hip_check_guards walks one table that guarded_alloc fills and guarded_free empties, so an option store cannot own
a guarded array that the check does not see.  These cases read the table through RomsHip.guarded_arrays() -- nothing is
stored outside an array -- on the one-tile 66 x 9 x 5 state of tests/reuse_util.py (a beach: MASKING and WET_DRY, so
that the averages' four counters and rmask_dia exist).  Per-tracer averages carry the name of their line once per
selected tracer, as the messages of roms_hip_check_guards always have; the lists are compared as multisets."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import avg_util as au
import reuse_util as ru
from roms_trunk_mgh_amd import abi, ana, avg, diags, hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NWS3 = int(re.search(r"#define ROMS_NWS3 (\d+)", open(os.path.join(ROOT, "roms_trunk_mgh_amd", "csrc", "roms_dev.h")).read()).group(1))

FIELDS = [name for name, _, _ in abi.FIELDS]
SCRATCH = [f"ws3[{q}]" for q in range(NWS3)] + [f"ws2[{q}]" for q in range(32)]
CLIMA = ["M2nudgcof", "ubarclm", "vbarclm", "M3nudgcof", "uclm", "vclm", "Tnudgcof", "tclm"]
AVERAGES = [("avgzeta", 0), ("avgw3d", 0), ("avgt", 1), ("avgt", 2)]        # a 2-D line, a W line, a per-tracer line
COUNTERS = ["pmask_avg", "rmask_avg", "umask_avg", "vmask_avg"]
DIAGS = ["DiaTwrk", "DiaTrc", "avgzeta (diagnostics)", "rmask_dia"]
KPP = ["hbbl", "kbbl", "ksbl"]
OPTIONS = {"clima": CLIMA, "averages": [n for n, _ in AVERAGES] + COUNTERS, "diagnostics": DIAGS, "kpp": KPP}


def beach():
    st = ru.family_tile("UPWELLING", "beach")[0]
    assert st.p.wet_dry == 1 and st.p.masking == 1 and st.b.NT == 2
    ana.analytic_clima(st, tracers=[1] * st.b.NT)
    assert st.clima.LnudgeM2CLM and st.clima.LnudgeM3CLM and all(st.clima.LnudgeTCLM)
    return st


def switch(be, option, on):
    st = be.st
    if option == "clima":
        if on:
            be.set_clima(st.clima)
        else:
            be._chk(be.l.roms_hip_set_clima(0, None, None, None, 0, None, None, None, None, None, None, 1.0), "set_clima")
    elif option == "averages":
        be.set_averages(au.averages_of(st.b, AVERAGES, nAVG=2) if on else None)
    elif option == "diagnostics":
        be.set_diagnostics(diags.Diags(st.b, 3) if on else None)
    else:
        be.set_kpp(bool(on))


def listed(be):
    names = be.guarded_arrays()
    assert len(names) == be.l.roms_hip_guarded_arrays(None, 0)
    return sorted(names)


def test_every_guarded_array_is_listed_and_each_option_takes_its_own_away():
    st = beach()                                   # (st.clima is set: RomsHip hands it over)
    be = hip.RomsHip(st)
    try:
        on = {"clima"}
        assert listed(be) == sorted(FIELDS + SCRATCH + CLIMA)
        for option in ("averages", "diagnostics", "kpp"):
            switch(be, option, True)
            on.add(option)
            assert listed(be) == sorted(FIELDS + SCRATCH + sum((OPTIONS[o] for o in on), []))
        everything = listed(be)
        assert len(everything) == len(FIELDS) + NWS3 + 32 + 8 + 4 + 4 + 4 + 3
        assert len(set(everything)) == len(everything) - 1                   # avgt twice: tracers 1 and 2
        # in allocation order: the scratch arrays of set_bounds, the fields as registered, then the options
        assert be.guarded_arrays()[:NWS3 + 32 + len(FIELDS)] == SCRATCH + FIELDS
        for option in OPTIONS:                     # each off in turn, and on again
            switch(be, option, False)
            assert listed(be) == sorted(FIELDS + SCRATCH + sum((OPTIONS[o] for o in on - {option}), [])), option
            switch(be, option, True)
            assert listed(be) == everything, option
        be.check_guards()
    finally:
        be.close()


def test_after_a_bounds_change_only_the_scratch_arrays_remain():
    st = beach()
    be = hip.RomsHip(st)
    lib = be.l
    try:
        for option in ("averages", "diagnostics", "kpp"):
            switch(be, option, True)
        assert len(listed(be)) > len(FIELDS) + NWS3 + 32
        be._chk(lib.roms_hip_set_bounds(C.byref(st.b)), "set_bounds")
        assert be.guarded_arrays() == SCRATCH
        be.check_guards()
        buf = np.zeros(st.ni * st.nj * (st.b.N + 1))
        lib.roms_hip_get_clima.argtypes = [C.c_char_p, C.c_void_p, C.c_long]
        assert lib.roms_hip_get_clima(b"ubarclm", buf.ctypes.data, st.ni * st.nj) != 0
        assert b"the library has no copy of ubarclm" in lib.roms_hip_last_error()
        assert lib.roms_hip_get_average(avg.AVG_ID["avgzeta"], 0, buf.ctypes.data, st.ni * st.nj) != 0
        assert b"avgzeta is not selected" in lib.roms_hip_last_error()
        assert lib.roms_hip_get_diagnostic(0, 1, 0, buf.ctypes.data, st.ni * st.nj * st.b.N) != 0
        assert b"diagnostics: not switched on" in lib.roms_hip_last_error()
        assert lib.roms_hip_get_kpp(b"hbbl", buf.ctypes.data, st.ni * st.nj) != 0
        assert b"LMD_BKPP is not switched on" in lib.roms_hip_last_error()
        assert be.guarded_arrays() == SCRATCH      # a refused call leaves the library as it was
    finally:
        be.close()


def test_library_defaults_appear_with_the_first_entry_and_go_with_the_parameters():
    st = ru.tile("UPWELLING")
    assert st.p.masking == 0
    masks = ("rmask", "umask", "vmask", "pmask")
    be = hip.RomsHip(st, leave_unregistered=masks)
    try:
        registered = [n for n in FIELDS if n not in masks]
        assert be.guarded_arrays() == SCRATCH + registered
        be.calib_stream(64)                        # the first kernel entry: roms_entry_check makes the defaults
        assert be.guarded_arrays() == SCRATCH + registered + [n for n in FIELDS if n in masks]
        be.check_guards()
        p = type(st.p).from_buffer_copy(st.p)
        p.masking = 1                              # all-water defaults are no masks of a MASKING application
        be._chk(be.l.roms_hip_set_params(C.byref(p)), "set_params")
        assert be.guarded_arrays() == SCRATCH + registered
        be._chk(be.l.roms_hip_set_params(C.byref(st.p)), "set_params")
        be.check_guards()
    finally:
        be.close()


def test_a_new_context_starts_from_an_empty_table():
    st = beach()
    be = hip.RomsHip(st)
    try:
        switch(be, "kpp", True)
        assert len(be.guarded_arrays()) == NWS3 + 32 + len(FIELDS) + 8 + 3
        be.check_guards()
    finally:
        be.close()
    lib = hip.load()
    assert lib.roms_hip_guarded_arrays(None, 0) < 0 and b"not initialised" in lib.roms_hip_last_error()
    try:
        assert lib.roms_hip_init(0, st.b.ntileI, st.b.ntileJ, 0, None) == 0, lib.roms_hip_last_error()
        assert lib.roms_hip_guarded_arrays(None, 0) == 0
        assert lib.roms_hip_set_bounds(C.byref(st.b)) == 0, lib.roms_hip_last_error()
        assert lib.roms_hip_guarded_arrays(None, 0) == NWS3 + 32
        assert lib.roms_hip_check_guards() == 0, lib.roms_hip_last_error()
    finally:
        lib.roms_hip_finalize()
