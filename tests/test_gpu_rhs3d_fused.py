"""-m gpu: roms_hip_rhs3d with the start of the corrector t(nnew) = Hz*t(nstp) + explicit vertical flux divergence moved
out of k_pre_t into the rotated harmonic mixing kernel (csrc/k_rhs3d.hip: rhs3d_fuses_tstart; k_pre_t<.., DEFER>,
k_t3dmix_geo<0, ISO, false, START>), and with two tracers per thread in k_pre_t.

* the driver against its own pieces called one entry at a time (which keep the two kernels): bit for bit;
* the driver against the oracle's rhs3d at the per-call tolerance of tests/test_gpu_kernels.py;
* the combinations that keep the two kernels (mixing along s-surfaces, lambda < 1, diagnostics, a run length of one);
* 2x1 and 2x2 tiles against one tile, bit for bit.
Every case checks that t(nnew) moved, and that it differs from the result without mixing: the start value and the
mixing term both reached the one store."""
import numpy as np
import pytest

import mp_gpu_rhs3d_worker as worker
import tiling_util
import util
from roms_trunk_mgh_amd import abi, hip

pytestmark = pytest.mark.gpu
TOL = 1e-12
PIECES = ("pre_step3d", "prsgrd", "t3dmix2", "rhs3d_tile", "uv3dmix2")


def _state(config, mix="geo", NT=None, overrides=None, mask=None, **params):
    """prepared_state with tnu2 = 300 and the tracer mixing option `mix` (geo / iso / s); params: members of the
    parameter block set afterwards (lambda_, lmd_nonlocal, solar_source)"""
    import oracle
    ov = dict(overrides or {}, tnu2=300.0)
    if mix == "iso":
        ov["mix_iso_ts"] = 1
    st = util.prepared_state(config, NT=NT, overrides=ov, mask=mask)
    st.p = type(st.p).from_buffer_copy(st.p)
    if mix == "geo":
        st.p.mix_geo_ts, st.p.mix_s_ts = 1, 0
    elif mix == "s":
        st.p.mix_geo_ts, st.p.mix_s_ts = 0, 1
    if mix == "iso":
        oracle.Oracle(st).call("rho_eos", util.step_idx())     # the potential density the slopes come from
    for k, v in params.items():
        setattr(st.p, k, v)
    assert st.p.ts_dif2 == 1 and (st.p.mix_geo_ts, st.p.mix_iso_ts, st.p.mix_s_ts) == \
        {"geo": (1, 0, 0), "iso": (0, 1, 0), "s": (0, 0, 1)}[mix]
    return st


def _surface_forcing(st):
    """non-zero KPP non-local transport and short-wave flux: the two terms of the explicit vertical flux that moved"""
    b = st.b
    ii = np.arange(b.LBi, b.UBi + 1, dtype=np.float64)[:, None, None]
    jj = np.arange(b.LBj, b.UBj + 1, dtype=np.float64)[None, :, None]
    kk = (np.arange(0, b.N + 1, dtype=np.float64) / b.N)[None, None, :]
    wob = 1.0 + 0.5 * np.sin(2.0 * np.pi * 2 * (ii - 0.5) / b.Lm) * np.cos(np.pi * (jj - 0.5) / b.Mm)
    for it in range(b.NAT):
        st["ghats"][:, :, :, it] = 2.0e-2 * (1.0 + 0.3 * it) * wob * kk * (1.0 - kk) * 4.0
        st["Akt"][:, :, :, it] += 1.0e-3 * wob * kk * (1.0 - kk) * 4.0
    st["srflx"][:] = 1.0e-4 * wob[:, :, 0]
    st["stflx"][:, :, 0] = 2.0e-5 * wob[:, :, 0]
    st["btflx"][:, :, 0] = -1.0e-7 * wob[:, :, 0]
    if st.p.masking:
        st["srflx"] *= st["rmask"]
        st["stflx"] *= st["rmask"][:, :, None]
        st["btflx"] *= st["rmask"][:, :, None]
    st.p.lmd_nonlocal = st.p.solar_source = 1
    assert np.abs(st["ghats"]).max() > 0.0 and np.abs(st["srflx"]).max() > 0.0
    return st


def _hip(st0, s, entries=("rhs3d",), with_diags=False):
    st = st0.copy()
    be = hip.RomsHip(st)
    try:
        if with_diags:
            from roms_trunk_mgh_amd import diags
            be.set_diagnostics(diags.Diags(st.b, 1))
        for e in entries:
            if e == "uv3dmix2" and not st.p.uv_vis2:
                continue
            be.call(e, s)
        be.to_host()
        be.check_guards()
    finally:
        be.close()
    return st


def _oracle(st0, s, no_mixing=False):
    import oracle
    st = st0.copy()
    if no_mixing:
        st["diff2"][:] = 0.0
    oracle.Oracle(st).call("rhs3d", s)
    return st


def _check_against_oracle(st0, s, st_h):
    st_o = _oracle(st0, s)
    diffs = util.compare_states(st_h, st_o)
    assert all(v <= TOL for v in diffs.values()), diffs
    # not vacuous: t(nnew) moved (the start value), and the mixing term is in it as well
    lev = s.nnew - 1
    new, old = st_o["t"][:, :, :, lev], st0["t"][:, :, :, lev]
    assert util.max_rel_diff(new, old) > 1e-6
    plain = _oracle(st0, s, no_mixing=True)["t"][:, :, :, lev]
    assert util.max_rel_diff(plain, old) > 1e-6
    assert util.max_rel_diff(new, plain) > 1e-9
    return st_o


@pytest.mark.parametrize("iic", [1, 2, 5])
@pytest.mark.parametrize("config,mix", [("UPWELLING", "geo"), ("BENCHMARK_TINY", "geo"), ("UPWELLING", "iso")])
def test_driver_equals_its_pieces_bit_for_bit(config, mix, iic):
    """The three time weightings of the predictor (first step, second step, LF-AM3).  The entries on their own keep the
    two kernels and the stored intermediate t(nnew); the driver must leave the same bits in every field."""
    st0 = _state(config, mix)
    if config == "BENCHMARK_TINY":
        _surface_forcing(st0)
    s = util.step_idx(iic=iic)
    fused = _hip(st0, s)
    pieces = _hip(st0, s, PIECES)
    for name, _, _ in abi.FIELDS:
        assert np.array_equal(fused[name], pieces[name]), name
    _check_against_oracle(st0, s, fused)


ORACLE_CASES = {
    # pairs plus a single tracer (NT = 3: a passive tracer beyond NAT), and one tracer alone
    "nt3": dict(config="UPWELLING", NT=3),
    "nt1": dict(config="SEAMOUNT"),
    # MASKING through both kernels, closed walls on all four sides
    "island": dict(config="UPWELLING", mask="island"),
    "island_iso": dict(config="BENCHMARK_TINY", mask="island", mix="iso", forcing=True),
    "basin": dict(config="UPWELLING", overrides={"EWperiodic": False}),
    # the moved terms on a grid that does not have them by default, three tracers
    "forcing_nt3": dict(config="UPWELLING", NT=3, forcing=True),
    # the rungs of kernel_for_n
    "n16": dict(config="BENCHMARK_TINY", overrides={"N": 16}, forcing=True),
    "n17": dict(config="UPWELLING", overrides={"N": 17}),
    "n33": dict(config="UPWELLING", overrides={"N": 33}),
    # the other scheme pairs with two tracers per thread
    "c4": dict(config="UPWELLING", overrides={"Hadv": "C4", "Vadv": "C4"}),
    "c2_nt3": dict(config="UPWELLING", NT=3, overrides={"Hadv": "C2", "Vadv": "C2"}),
}


@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_driver_against_oracle(case):
    kw = dict(ORACLE_CASES[case])
    forcing = kw.pop("forcing", False)
    st0 = _state(kw.pop("config"), kw.pop("mix", "geo"), **kw)
    if forcing:
        _surface_forcing(st0)
    if "mask" in kw:
        assert st0.p.masking == 1 and (st0["rmask"] == 0).any()
    if case == "basin":
        assert not st0.b.EWperiodic
    if case.startswith("n") and case[1:].isdigit():
        assert st0.b.N == int(case[1:])
    if case == "nt1":
        assert st0.b.NT == 1
    s = util.step_idx(iic=5)
    _check_against_oracle(st0, s, _hip(st0, s))


FALLBACKS = {
    "mix_s": dict(mix="s"),
    "lambda": dict(lambda_=0.5),
    "diagnostics": dict(mix="s", with_diags=True),
    # a run length of one: tracer 1 U3 / C4, tracer 2 A4 / A4
    "mixed_schemes": dict(overrides={"Hadv_list": ["U3", "A4"], "Vadv_list": ["C4", "A4"]}),
    "mpdata_six": dict(NT=6, overrides={"Hadv": "MPDATA", "Vadv": "MPDATA"}),
}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_other_paths_against_oracle(case):
    """What keeps the two kernels (s-surfaces, an explicit share of the vertical diffusion, diagnostics), tracers whose
    schemes differ (every run has length one), and six tracers of the upstream predictor (three pairs)"""
    kw = dict(FALLBACKS[case])
    with_diags = kw.pop("with_diags", False)
    st0 = _state("UPWELLING", kw.pop("mix", "geo"), **kw)
    if case == "lambda":
        assert st0.p.lambda_ == 0.5
    if case == "mixed_schemes":
        assert st0.p.Hadv[0] != st0.p.Hadv[1]
    s = util.step_idx(iic=5)
    _check_against_oracle(st0, s, _hip(st0, s, with_diags=with_diags))


@pytest.mark.parametrize("ntI,ntJ", [(2, 1), (2, 2)])
def test_tiling_invariance(tmp_path, ntI, ntJ):
    """rhs3d alone after one full step, 2x1 and 2x2 tiles of UPWELLING over the host relay: every owned point equal to
    the one-tile run bit for bit (both loops cover Istr:Iend, Jstr:Jend on every tile)"""
    ref = worker.tiled_state("UPWELLING")
    t_in = ref["t"].copy()
    be = hip.RomsHip(ref)
    try:
        want = worker.run(be, ref)
    finally:
        be.close()
    lev = int(want["nnew"]) - 1
    assert util.max_rel_diff(ref["t"][:, :, :, lev], t_in[:, :, :, lev]) > 1e-6
    world = ntI * ntJ
    tiling_util.spawn_ranks("mp_gpu_rhs3d_worker.py", world, [ntI, ntJ, tmp_path, "UPWELLING"], timeout=300)
    tiling_util.assert_tiles_equal(tmp_path, world, want, ref.b, worker.FIELDS, owned="Istr:Iend")
