"""The inputs of tests/test_gpu_levels.py checked without a GPU: the case list covers every rung of every ladder of
RUNGS, the geometry and the seam conditions of the 66 x 5 shape (build() asserts them), the reference's single calls
finite with a changed top level -- so that no GPU case passes on NaN == NaN or on a top level nobody touched -- and the
oracle's 10-step runs finite and moving."""
import numpy as np
import pytest

import test_gpu_levels as tl
import test_gpu_wide as tw
from roms_trunk_mgh_amd import abi


def _finite(st):
    return all(np.isfinite(st[name]).all() for name, _, _ in abi.FIELDS)


def test_nmax():
    assert [tl.nmax("k_uv_column", N) for N in (16, 17, 32, 33, 48, 49, 64)] == [16, 32, 32, 48, 48, 64, 64]
    assert [tl.nmax("k_omega", N) for N in (16, 17, 32, 33, 48, 49, 64)] == [16, 32, 32, 64, 64, 64, 64]
    assert [tl.nmax("k_lmd_vmix", N) for N in (17, 32, 33, 64)] == [32, 32, 64, 64]
    assert all(tl.nmax("k_step3d_t_pipe:src", N) == 64 for N in tl.LEVELS)
    assert all(max(r) == 64 and r == tuple(sorted(r)) for r in tl.RUNGS.values())
    with pytest.raises(ValueError):
        tl.nmax("k_omega", 65)


def test_required_coverage():
    """for every family and every rung above 16 of its ladder the case list holds N == rung and, where the ladder has a
    rung below, N == that rung + 1 (the first N the rung is handed), for every label that launches the family, in a
    masked variant and an unmasked one (the two MASK instantiations of k_step3d_t_pipe are families of their own: one
    variant each)"""
    have = {(p.values[1], p.values[2], p.values[3]) for p in tl.kernel_cases()}
    assert set(tl.LAUNCHED_BY) == set(tl.RUNGS)
    ladder_labels = {label for _, labels in tl.LADDER.values() for label in labels}
    for family, rungs in tl.RUNGS.items():
        labels, variants = tl.LAUNCHED_BY[family]
        assert labels and set(labels) <= ladder_labels, family
        if ":masked" not in family and ":unmasked" not in family:
            assert {tl.MASKED[v] for v in variants} == {True, False}, family
        for q, rung in enumerate(rungs):
            if rung == 16:
                continue
            edges = [rung] + ([rungs[q - 1] + 1] if q else [])
            for N in edges:
                assert tl.nmax(family, N) == rung
                for label in labels:
                    for v in variants:
                        assert (label, N, v) in have, (family, label, N, v)
    # the families' own variants: MASK = true on the island grid, MASK = false in the basin
    assert tl.LAUNCHED_BY["k_step3d_t_pipe:masked"][1] == ("island",)
    assert tl.LAUNCHED_BY["k_step3d_t_pipe:unmasked"][1] == ("closed",)
    # the level loops without a ladder: every label at 33 and 64 in both variants
    for _, labels in tl.PLAIN.values():
        assert all((label, N, v) in have for label in labels for N in tl.PLAIN_LEVELS for v in tl.VARIANTS)
    ids = [p.id for p in tl.kernel_cases()]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("N", tl.LEVELS)
def test_geometry(N):
    """the shape for the two and the three ghost-point layouts, periodic and not"""
    for variant in tl.VARIANTS:
        for ov in (None, tw.SCHEMES["MPDATA"]):
            st = tw.tile(tl.shape(N), variant, ov=ov)
            assert st.b.NghostPoints == (3 if ov else 2)
            nbx = tl.check_geometry(st.b, N)
            tw.check_seam(st, variant)
            assert nbx["interior"] == 2
            assert bool(st.p.masking) == tl.MASKED[variant]


@pytest.mark.parametrize("fam,label,N,variant", tl.kernel_cases())
def test_reference_on_the_level_states(fam, label, N, variant):
    st0, calls = tl.build(fam, label, N, variant)              # asserts geometry and seam conditions
    assert _finite(st0)
    if "src" in label:
        tw.check_sources(st0.sources, st0.b)
        assert st0.sources.Tsrc.shape[1] == N
    st_r, _ = tl.run_reference(fam, st0, calls)
    assert _finite(st_r), [n for n, _, _ in abi.FIELDS if not np.isfinite(st_r[n]).all()]
    assert tl.top_level_changed(label, st_r, st0), "top level untouched"


@pytest.mark.parametrize("name", list(tl.RUNS))
def test_oracle_runs_on_the_level_states(name):
    import oracle
    st = tl.run_state(name)
    m = tw.run_steps(oracle.Oracle(st), 10)
    assert np.isfinite(st["t"]).all() and np.isfinite(st["u"]).all()
    assert float(np.abs(st["u"]).max()) > 1e-6 and m.last_diag is not None
    if name.endswith("beach"):
        assert 0 < st["rmask_wet"].sum() < st["rmask_wet"].size
