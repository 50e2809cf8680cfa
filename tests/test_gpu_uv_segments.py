"""-m gpu: parity of k_uv_column at the joints of its Thomas segments and at the clamped look-ahead of its first sweep.

k_uv_column keeps the coefficients of its tridiagonal solve at every SEG-th row only and re-runs a segment of SEG rows
from its checkpoint in the back substitution; its first sweep requests the inputs AHEAD levels ahead with the level
clamped to N, the back substitution a segment's Akv pairs, the coupling the whole Hflx column, clamped alike
(csrc/k_step3d_uv.hip).  What can go wrong there depends on N against the multiples of SEG and against NMAX - AHEAD, not
on the grid: a row on the wrong side of a joint, a checkpoint of the wrong row, a top segment dropped or run one row
too far, a clamped level used.  So the grid is the 66 x 5 of tests/test_gpu_levels.py (two workgroups in x and two in y,
the second partly live; builders of tests/test_gpu_wide.py) and N runs over LEVELS.  The rungs 17 ... 64 are
tests/test_gpu_levels.py's.

  1. test_uv_segments_kernels: one step3d_uv call per label, variant and N, HIP against the CPU oracle at 1e-12 of each
     field's maximum on every registered field, equal return values, guard bands, and the top level changed by the
     reference (a dropped or truncated top segment fails).
  2. test_uv_segments_run: 10 whole steps at N = 2 SEG + 1 with physics and diagnostics, 1e-10 relative RMS.

tests/test_uv_segments_shapes.py checks the case list and the reference's side of these cases without a GPU."""
import numpy as np
import pytest

import test_gpu_levels as tl
import test_gpu_wide as tw
import util

pytestmark = pytest.mark.gpu
TOL = tw.TOL
SEG = 5          # UV_SEG, csrc/k_step3d_uv.hip:30: rows of the tridiagonal system per segment
AHEAD = 4        # UV_AHEAD, csrc/k_step3d_uv.hip:33: levels the first sweep requests ahead
NMIN = 1         # the smallest N the builders accept (tests/test_uv_segments_shapes.py::test_smallest_n)
# row j of the system couples the levels j and j + 1, the top row is N - 1: N = SEG + 1 fills the first segment,
# N = SEG + 2 and 2 SEG + 2 = 16 - AHEAD start a segment of one row
LEVELS = tuple(sorted({NMIN, SEG - 1, SEG, SEG + 1, SEG + 2, 2 * SEG, 2 * SEG + 1, 16 - AHEAD, 16, 30}))
LABELS = {"step3d_uv": "base", "step3d_uv:wet": "wet", "step3d_uv:src": "sources"}      # label -> family of test_gpu_levels
VARIANTS = tl.VARIANTS
RUN_N = 2 * SEG + 1


def kernel_cases():
    return [pytest.param(fam, label, N, variant, id=f"{label}-N{N}-{variant}")
            for label, fam in LABELS.items() for N in LEVELS for variant in VARIANTS]


@pytest.mark.parametrize("fam,label,N,variant", kernel_cases())
def test_uv_segments_kernels(fam, label, N, variant):
    from roms_trunk_mgh_amd import hip
    st0, calls = tl.build(fam, label, N, variant)
    st_h = st0.copy()
    h = hip.RomsHip(st_h)
    try:
        r_h = tw.run_calls(h, calls)
        h.to_host()
        h.check_guards()
    finally:
        h.close()
    st_r, r_r = tl.run_reference(fam, st0, calls)
    diffs = util.compare_states(st_h, st_r)
    print(label, N, variant, "max relative differences:", diffs)
    assert all(v <= TOL for v in diffs.values()), diffs
    assert len(r_h) == len(r_r)
    for a, o in zip(r_h, r_r):
        assert np.array_equal(a, o), (a, o)
    assert tl.top_level_changed(label, st_r, st0), "the reference left the top level alone"


def run_state(variant):
    st = tw.tile(tl.shape(RUN_N, "BENCHMARK_TINY"), variant)
    tl.check_geometry(st.b, RUN_N)
    tw.check_seam(st, variant)
    return st


def test_uv_segments_run():
    import oracle
    from roms_trunk_mgh_amd import hip
    from test_gpu_fullsize import _check_prognostic
    st_o = run_state("island")
    st_h = st_o.copy()
    be = hip.RomsHip(st_h)
    try:
        tw.run_steps(be)
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    mo = tw.run_steps(oracle.Oracle(st_o))
    _check_prognostic(st_h, st_o, mo)
