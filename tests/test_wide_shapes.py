"""The inputs of tests/test_gpu_wide.py checked without a GPU: the launch geometry each shape is chosen for (from the
bounds and the 64 x 4 workgroup), the seam conditions of every state builder the GPU cases use (build() asserts them),
and the oracle's calls on those states finite and not trivial."""
import numpy as np
import pytest

import test_gpu_wide as tw
import util
from roms_trunk_mgh_amd import abi


def _finite(st):
    return all(np.isfinite(st[name]).all() for name, _, _ in abi.FIELDS)


@pytest.mark.parametrize("shape", list(tw.SHAPES))
def test_geometry_table(shape):
    """the table of the shapes, for the two and the three ghost-point layouts, periodic and not"""
    for variant in ("island", "closed"):
        for ov in (None, tw.SCHEMES["MPDATA"]):
            st = tw.tile(shape, variant, ov=ov)
            nbx = tw.check_geometry(shape, st.b)
            tw.check_seam(st, variant)
            assert nbx["interior"] == {"w3": 3, "w8": 8, "w10": 10, "thin": 2}[shape]
    assert tw.strips(10) == [1, 1, 1, 2, 1, 1, 1, 2] and tw.strips(16) == [2] * 8


def test_required_coverage():
    """every family at w8 in every variant, at the other shapes on the island grid and in a basin"""
    have = {(p.values[0], p.values[1], p.values[2], p.values[3]) for p in tw.kernel_cases()}
    for fam, (_, labels) in tw.FAMILIES.items():
        for label in labels:
            assert all((fam, label, "w8", v) in have for v in tw.APPLIES.get(fam, tw.VARIANTS))
            for shape in ("w3", "w10", "thin"):
                assert (fam, label, shape, "island") in have
                assert any((fam, label, shape, v) in have for v in tw.VARIANTS[1:])


@pytest.mark.parametrize("fam,label,shape,variant", tw.kernel_cases())
def test_oracle_on_the_wide_states(fam, label, shape, variant):
    st0, calls = tw.build(fam, label, shape, variant)          # asserts geometry and seam conditions
    assert _finite(st0)
    st_o, _ = tw.run_oracle(st0, calls)
    assert _finite(st_o), [n for n, _, _ in abi.FIELDS if not np.isfinite(st_o[n]).all()]
    assert tw.vacuous_ok(label, variant) or util.compare_states(st_o, st0)


@pytest.mark.parametrize("shape,variant", tw.clima_cases())
def test_clima_states(shape, variant):
    for entry in ("rhs3d_tile", "step3d_t"):
        assert _finite(tw.clima_state(shape, variant, entry))


@pytest.mark.parametrize("name", list(tw.RUNS))
def test_oracle_runs_on_the_wide_states(name):
    import oracle
    st = tw.run_state(name)
    m = tw.run_steps(oracle.Oracle(st), 10)
    assert np.isfinite(st["t"]).all() and np.isfinite(st["u"]).all()
    assert float(np.abs(st["u"]).max()) > 1e-6 and m.last_diag is not None


@pytest.mark.parametrize("shape", ["w8", "w10"])
def test_shift_states(shape):
    import oracle
    from roms_trunk_mgh_amd import main3d
    st = tw.shift_state(shape)
    m = main3d.Main3D(oracle.Oracle(st), physics=False, diagnostics=True)
    m.initial()
    m.run(3)
    assert np.isfinite(st["t"]).all() and float(np.abs(st["u"]).max()) > 1e-6
