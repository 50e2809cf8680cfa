"""roms_hip_diag's two reduction kernels (csrc/k_diag.hip: k_diag_rows walks the rows serially in j, 16 at a time;
k_diag_final adds the per-i partials serially in i out of LDS, a wavefront per sum, and finds the maxima with a butterfly
in a fourth): the twelve numbers against the oracle's diag, bit for bit, on random states.

The sizes nI x nJ are the corners and three mixed cases of nI in {1, 63, 65, 130, 513} (one lane, a wavefront less and
more than one, three workgroups, more than one pass of the candidates of a lane) and nJ in {1, 15, 17, 33} (one row, a
group of 16 rows less and more than one row, more than two groups).  N = 3, the least diag accepts.
  * "random": the prepared state with every input of diag perturbed at random;
  * "mixed": every input of mixed magnitude (each 1e-4 .. 1e4, their products 1e-8 .. 1e8 and beyond), so that any change
    of the order of the additions shows in the last bits -- test_mixed_magnitudes_separate_orders checks that without a GPU;
  * "tie": the same Courant number everywhere: the location is the smallest j, then the largest k, then the smallest i;
  * "rest": a state at rest: maximum 0 at (0, 0, 0)."""
import numpy as np
import pytest

import util
from roms_trunk_mgh_amd import hip

SIZES = [(1, 1), (1, 33), (513, 1), (513, 33), (63, 15), (65, 17), (130, 33)]
N = 3
_STATES = {}


def _base(nI, nJ):
    """the prepared closed basin of nI x nJ interior points (built once per size; callers copy)"""
    if (nI, nJ) not in _STATES:
        st = util.prepared_state("UPWELLING", overrides=dict(Lm=nI, Mm=nJ, N=N, EWperiodic=False))
        b = st.b
        assert (b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1, b.N) == (nI, nJ, N)
        _STATES[(nI, nJ)] = st
    return _STATES[(nI, nJ)].copy()


def _state(nI, nJ, kind):
    st = _base(nI, nJ)
    rng = np.random.default_rng(1000 * nI + nJ)

    def mag(shape, lo=-4.0, hi=4.0):
        return 10.0 ** rng.uniform(lo, hi, shape)

    def sign(shape):
        return np.where(rng.random(shape) < 0.5, -1.0, 1.0)

    if kind == "random":
        for name in ("u", "v", "rho", "wvel"):
            st[name][:] = st[name] * (1.0 + 0.3 * rng.standard_normal(st[name].shape)) + 1.0e-3 * rng.standard_normal(st[name].shape)
        st["Hz"][:] = st["Hz"] * (1.0 + 0.3 * rng.random(st["Hz"].shape))
    elif kind == "mixed":
        for name in ("u", "v", "wvel", "rho", "z_r", "z_w"):
            st[name][:] = sign(st[name].shape) * mag(st[name].shape)
        for name in ("Hz", "omn", "pm", "pn"):
            st[name][:] = mag(st[name].shape)
    elif kind == "tie":
        st["u"][:] = 0.125
        st["v"][:] = 0.0625
        st["wvel"][:] = 0.0
        st["pm"][:] = 1.0e-3
        st["pn"][:] = 2.0e-3
    elif kind == "rest":
        for name in ("u", "v", "wvel"):
            st[name][:] = 0.0
    else:
        raise KeyError(kind)
    return st


def _both(st0):
    import oracle
    s = util.step_idx()
    d_o = oracle.Oracle(st0.copy()).diag(s)
    h = hip.RomsHip(st0.copy())
    try:
        d_h = h.diag(s)
    finally:
        h.close()
    return d_h, d_o


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "mixed"])
@pytest.mark.parametrize("nI,nJ", SIZES)
def test_twelve_numbers_bit_for_bit(nI, nJ, kind):
    d_h, d_o = _both(_state(nI, nJ, kind))
    assert np.isfinite(d_o).all() and d_o[5] > 0.0, d_o
    assert np.array_equal(d_h, d_o), (d_h, d_o)


@pytest.mark.gpu
@pytest.mark.parametrize("nI,nJ", [(130, 33), (513, 17)])
def test_ties_go_to_the_first_in_loop_order(nI, nJ):
    st = _state(nI, nJ, "tie")
    d_h, d_o = _both(st)
    b = st.b
    assert d_o[5] > 0.0 and tuple(d_o[9:12]) == (b.Istr, b.Jstr, b.N), d_o
    assert np.array_equal(d_h, d_o), (d_h, d_o)


@pytest.mark.gpu
@pytest.mark.parametrize("nI,nJ", [(130, 33), (1, 1)])
def test_state_at_rest(nI, nJ):
    d_h, d_o = _both(_state(nI, nJ, "rest"))
    assert tuple(d_o[5:12]) == (0.0,) * 7, d_o
    assert np.array_equal(d_h, d_o), (d_h, d_o)


def test_mixed_magnitudes_separate_orders():
    """Without a GPU: on the mixed-magnitude state the per-column kinetic-energy terms (diag.F:268-278, formed here in
    numpy) summed in the reference's order -- j ascending inside i ascending -- differ from the same terms summed
    pairwise, and from the j-partials summed pairwise over i: a reduction that reorders either stage cannot pass."""
    st = _state(130, 33, "mixed")
    b = st.b
    I = slice(b.Istr - b.LBi, b.Iend - b.LBi + 1)
    I1 = slice(b.Istr - b.LBi + 1, b.Iend - b.LBi + 2)
    J = slice(b.Jstr - b.LBj, b.Jend - b.LBj + 1)
    J1 = slice(b.Jstr - b.LBj + 1, b.Jend - b.LBj + 2)
    u, v = st["u"][:, :, :, 0], st["v"][:, :, :, 0]
    u2v2 = u[I, J] ** 2 + u[I1, J] ** 2 + v[I, J] ** 2 + v[I, J1] ** 2
    term = st["omn"][I, J] * (st["Hz"][I, J] * 0.25 * u2v2).sum(axis=2)
    part = np.zeros(term.shape[0])
    for j in range(term.shape[1]):
        part = part + term[:, j]
    serial = 0.0
    for x in part:
        serial = serial + x

    def pairwise(x):
        x = list(x)
        while len(x) > 1:
            x = [x[q] + x[q + 1] if q + 1 < len(x) else x[q] for q in range(0, len(x), 2)]
        return x[0]

    assert pairwise(part) != serial
    assert pairwise([pairwise(row) for row in term]) != serial
