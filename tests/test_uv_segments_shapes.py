"""The inputs of tests/test_gpu_uv_segments.py checked without a GPU: the case list stands on both sides of the segment
joints of k_uv_column and at its clamped look-ahead, the builders accept the smallest N of the list and nothing below
it, and the reference's calls on these states are finite and change the top level -- so that no GPU case passes on
NaN == NaN or on a top level nobody touched."""
import re
from pathlib import Path

import numpy as np
import pytest

import test_gpu_levels as tl
import test_gpu_uv_segments as ts
import test_gpu_wide as tw
from roms_trunk_mgh_amd import abi

S, D = ts.SEG, ts.AHEAD


def _finite(st):
    return all(np.isfinite(st[name]).all() for name, _, _ in abi.FIELDS)


def test_constants_are_the_kernels():
    """SEG and AHEAD restate the two constants of csrc/k_step3d_uv.hip"""
    src = (Path(tl.__file__).resolve().parents[1] / "roms_trunk_mgh_amd" / "csrc" / "k_step3d_uv.hip").read_text()
    assert int(re.search(r"^#define UV_SEG (\d+)$", src, re.M).group(1)) == S
    assert int(re.search(r"^#define UV_AHEAD (\d+)$", src, re.M).group(1)) == D


def test_case_list():
    """the top row of the tridiagonal system is N - 1 and segment m holds the rows m S + 1 .. m S + S.  For the joints
    S and 2 S: a case whose top row is the last before the joint's row, one whose top row is the joint's (a full
    segment) and one whose top row is the first of the next segment (a segment of one row).  Every joint below N = 30 is
    crossed by a case; the rung of 16 levels is met at N == NMAX and at the first N whose look-ahead is clamped at
    level 1 already (N = 16 - AHEAD: the request of level 1 + AHEAD ... is the last unclamped one)."""
    top_rows = {N - 1 for N in ts.LEVELS}
    for m in (1, 2):
        assert {m * S - 1, m * S, m * S + 1} <= top_rows, m
    for joint in range(S, 30 - 1, S):
        assert any(N - 1 >= joint + 1 for N in ts.LEVELS), joint
    assert {ts.NMIN, S - 1, S, S + 1, 2 * S, 2 * S + 1, 16 - D, 16, 30} <= set(ts.LEVELS)
    assert all(tl.nmax("k_uv_column", N) == (16 if N <= 16 else 32) for N in ts.LEVELS)
    have = {(p.values[1], p.values[2], p.values[3]) for p in ts.kernel_cases()}
    assert have == {(lb, N, v) for lb in tl.LAUNCHED_BY["k_uv_column"][0] for N in ts.LEVELS for v in tl.VARIANTS}
    assert {tl.MASKED[v] for v in ts.VARIANTS} == {True, False}
    ids = [p.id for p in ts.kernel_cases()]
    assert len(ids) == len(set(ids))
    assert ts.RUN_N == 2 * S + 1


def test_smallest_n():
    """N = NMIN builds in every family and variant (test_reference_on_the_segment_states runs it); N = NMIN - 1 does not"""
    for label, fam in ts.LABELS.items():
        with pytest.raises(Exception):
            tl.build(fam, label, ts.NMIN - 1, "closed")


@pytest.mark.parametrize("fam,label,N,variant", ts.kernel_cases())
def test_reference_on_the_segment_states(fam, label, N, variant):
    st0, calls = tl.build(fam, label, N, variant)              # asserts geometry and seam conditions
    assert _finite(st0)
    if "src" in label:
        tw.check_sources(st0.sources, st0.b)
    st_r, _ = tl.run_reference(fam, st0, calls)
    assert _finite(st_r), [n for n, _, _ in abi.FIELDS if not np.isfinite(st_r[n]).all()]
    assert tl.top_level_changed(label, st_r, st0), "top level untouched"


def test_oracle_run_on_the_segment_state():
    import oracle
    st = ts.run_state("island")
    m = tw.run_steps(oracle.Oracle(st), 10)
    assert np.isfinite(st["t"]).all() and np.isfinite(st["u"]).all()
    assert float(np.abs(st["u"]).max()) > 1e-6 and m.last_diag is not None
