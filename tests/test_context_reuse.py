"""The inputs of tests/test_gpu_context_reuse.py checked without a GPU, on the oracle: every scenario's run is finite and
moving, its (k, m) meets the key-repeat condition (a captured LOOP_2D graph is replayed before the change and, for
either nstp, after it), and the change is one the model feels -- the state after k + m steps with it differs from the
state without it by more than 100 x the parity bound in a compared field.  The oracle restarted with ntstart = 5 is
compared with ntstart = 1 on the same state (scenario 2)."""
import numpy as np
import pytest

import reuse_util as ru
import util
from roms_trunk_mgh_amd import abi

SCEN = ru.scenarios()


def _finite(st):
    return all(np.isfinite(st[name]).all() for name, _, _ in abi.FIELDS)


def test_shape():
    for app in ru.APPS:
        for fam in ru.FAMILIES:
            st, _ = ru.family_tile(app, fam)           # asserts the geometry
            assert bool(st.p.wet_dry) == (fam == "beach")
            if fam == "beach":
                assert st.p.masking == 1 and 0 < (st["rmask"] == 0.0).sum()
            if fam == "mpdata6":
                assert st.b.NT == 6 and st.b.NghostPoints == 3
            if fam == "gls":
                assert st.p.gls_mixing == 1
        assert ru.tile(app, ru.DIF4[app]).b.NghostPoints == 3


@pytest.mark.parametrize("name", list(SCEN))
def test_oracle_scenario(name):
    sc = SCEN[name]
    st0 = sc["state"]()
    mkw = sc.get("mkw")
    st_m, m, keys, _ = ru.run_continued(st0, sc["changes"], False, mkw=mkw)
    assert _finite(st_m), [n for n, _, _ in abi.FIELDS if not np.isfinite(st_m[n]).all()]
    assert float(np.abs(st_m["u"]).max()) > 1e-6
    # the key-repeat condition, for the first change and for every later one
    k = ru.K
    for _, steps in sc["changes"]:
        ru.assert_replays(keys[:k + steps], k)
        k += steps
    assert k == len(keys)
    if sc.get("vacuous") or sc.get("oracle") is False:       # (non-vacuity of those: in the GPU module)
        return
    # each change is felt: the run that stops changing after the first q changes ends elsewhere
    total = sum(steps for _, steps in sc["changes"])
    prev = None
    for q in range(len(sc["changes"]) + 1):
        done = sc["changes"][:q]
        rest = total - sum(steps for _, steps in done)
        st_q, m_q, _, _ = ru.run_continued(st0, done + ([(ru.m_none, rest)] if rest else []), False, mkw=mkw)
        if prev is not None:
            assert ru.felt(st_q, prev, m_q), (name, "change", q, "without effect", ru.parity(st_q, prev, m_q))
        prev = st_q


@pytest.mark.parametrize("app", ru.APPS)
def test_oracle_ntstart_5_equals_ntstart_1(app):
    """the step counter enters the oracle only through iic == ntfirst and iic - ntstart: a run restarted with
    ntstart = 5 is the run with ntstart = 1, bit for bit -- so the GPU module asserts the same for the library"""
    st0 = ru.restart_state(app)
    out = {}
    for nt in (1, 5):
        st, m, keys, _ = ru.run_continued(st0, [], False, k=8, ntstart=nt)
        assert m.iic == nt + 8 and m.ntfirst == nt
        assert {q % 4 for q, _ in keys} == {0, 1, 2}              # the three start-up phases of the key
        seen = [q for q, _ in keys]
        assert len(set(seen)) < len(seen)
        out[nt] = st
    assert _finite(out[5]) and float(np.abs(out[5]["u"]).max()) > 1e-6
    assert ru.differing(out[5], out[1]) == []
    assert ru.differing(out[5], st0) != []


def test_graph_key_and_single_calls_follow_the_oracle_loop():
    """loop_by_single_calls restates LOOP_2D: on the oracle it equals oracle_step2d_loop bit for bit, indx1 included"""
    import oracle
    st_a = util.prepared_state("UPWELLING", overrides=dict(ru.SHAPE))
    st_b = st_a.copy()
    s_a, s_b = util.step_idx(iic=5), util.step_idx(iic=5)
    ia = oracle.Oracle(st_a).step2d_loop(s_a, 1)
    ib = ru.loop_by_single_calls(oracle.Oracle(st_b), s_b, 1)
    assert ia == ib and ru.differing(st_a, st_b) == []
    assert bytes(s_a) == bytes(s_b)
    assert ru.graph_key(1, util.step_idx(iic=1, nstp=1, nnew=2)) == ((1 * 4 + 1) * 4 + 2) * 4 + 0
    assert ru.graph_key(2, util.step_idx(iic=2, nstp=2, nnew=1)) == ((2 * 4 + 2) * 4 + 1) * 4 + 1
    assert ru.graph_key(2, util.step_idx(iic=9, ntfirst=5, nstp=1, nnew=2)) == ((2 * 4 + 1) * 4 + 2) * 4 + 2
