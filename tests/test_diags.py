"""Tracer budget diagnostics (DIAGNOSTICS_TS) without a GPU: the recovery of the expected terms from the oracle's
per-routine entry points closes on the oracle alone (tests/diags_util.py), the term table and its numbering follow
mod_scalars.F:4027-4043, the three entries are in the ABI, and the schedule of set_diags.F:121-124 / :244 is the
initialise / accumulate part of the averages' schedule."""
import numpy as np
import pytest

import diags_util as du
import util
from roms_trunk_mgh_amd import avg, diags, hip

SHAPE = dict(Lm=70, Mm=6)                     # two workgroups wide in x and two in y


def _state(N, ov=None, mask=None, config="UPWELLING"):
    st = util.prepared_state(config, overrides=dict(SHAPE, N=N, **(ov or {})), mask=mask)
    st["diff2"][:] = 40.0 * (1.0 + 0.3 * np.cos(0.2 * np.arange(st.ni))[:, None, None])       # UPWELLING ships tnu2 = 0
    return st


@pytest.mark.parametrize("ov,mask", [({}, None), ({"splines_vdiff": 0}, None), ({"ts_dif2": 0}, None), ({}, "island"),
                                     ({"Hadv": "A4", "Vadv": "SPLINES"}, None)],
                         ids=["plain", "classic", "ndt6", "masked", "A4-SPLINES"])
def test_the_recovery_closes_on_the_oracle_alone(ov, mask):
    st = _state(17, ov, mask)
    r = du.recover(st, util.step_idx())
    w = np.broadcast_to(du.water(st), r["iTrate"].val.shape)
    total = r["iThadv"] + r["iTvadv"] + r["iTvdif"]
    if st.p.ts_dif2:
        total = total + r["iThdif"]
        assert np.abs(r["iThdif"].val[w]).max() > 0.0
    # hadv + vadv + hdif + vdif = rate
    ex = np.abs(total.val - r["iTrate"].val) - (total.bound + r["iTrate"].bound)
    assert ex[w].max() <= 0.0, float(ex[w].max())
    # xadv + yadv = hadv, hadv + vadv = the advection of the run with every transport, xdif + ydif = hdif
    pairs = [(("iTxadv", "iTyadv"), "iThadv"), (("iThadv", "iTvadv"), "adv")]
    if st.p.ts_dif2:                                  # xdif + ydif = hdif, each direction with the other's metric zeroed
        pairs.append((("iTxdif", "iTydif"), "iThdif"))
        assert np.abs(r["iTxdif"].val[w]).max() > 0.0 and np.abs(r["iTydif"].val[w]).max() > 0.0
    for parts, whole in pairs:
        s = r[parts[0]] + r[parts[1]]
        ex = np.abs(s.val - r[whole].val) - (s.bound + r[whole].bound)
        assert ex[w].max() <= 0.0, (whole, float(ex[w].max()))
    for name in ("iTxadv", "iTyadv", "iTvadv", "iTvdif", "iTrate"):
        assert np.abs(r[name].val[w]).max() > 10.0 * r[name].bound[np.broadcast_to(du.water(st), r[name].bound.shape)].max(), name


def test_x_and_y_diffusion_recovered_from_uniform_fields():
    """a tracer uniform in y has no eta-diffusion, one uniform in x no xi-diffusion: the whole of t3dmix2 is then one
    direction's term, and neither is trivially zero"""
    import oracle
    s = util.step_idx()
    st = _state(17)
    I, J = du.interior(st)
    for axis in ("y", "x"):
        v = du.uniform_along(st, axis)
        before = v["t"][:, :, :, s.nnew - 1, :].copy()
        oracle.Oracle(v).call("t3dmix2", s)
        hdif = du.diff(v["t"][:, :, :, s.nnew - 1, :], before, 1.0 / np.where(v["Hz"] > 0.0, v["Hz"], 1.0)[:, :, :, None])
        assert np.abs(hdif.val[I, J]).max() > 100.0 * hdif.bound[I, J].max(), axis


def test_the_term_table_follows_mod_scalars():
    lib = hip.load()
    names = [d["name"] for d in diags.TERMS]
    assert names == ["iThadv", "iTxadv", "iTyadv", "iTvadv", "iThdif", "iTxdif", "iTydif", "iTsdif", "iTvdif", "iTrate"]
    assert diags.DIA_COUNT == 10 and diags.DIA_ID["avgzeta"] == 11 and diags.DIA_ID["rmask_dia"] == 12
    # mod_scalars.F:4027-4043 written out by hand: NDT = 6, 9, 10 (mod_param.F:1380-1389)
    table = {(0, 0): dict(iThadv=1, iTxadv=2, iTyadv=3, iTvadv=4, iTvdif=5, iTrate=6, NDT=6),
             (1, 0): dict(iThadv=1, iTxadv=2, iTyadv=3, iTvadv=4, iThdif=5, iTxdif=6, iTydif=7, iTvdif=8, iTrate=9, NDT=9),
             (1, 1): dict(iThadv=1, iTxadv=2, iTyadv=3, iTvadv=4, iThdif=5, iTxdif=6, iTydif=7, iTsdif=8, iTvdif=9, iTrate=10,
                          NDT=10)}
    for (hdif, rot), want in table.items():
        assert diags.indices(hdif, rot) == want
        for name in names:
            assert lib.roms_hip_dia_index(diags.DIA_ID[name], hdif, rot) == want.get(name, 0), (name, hdif, rot)
        assert lib.roms_hip_dia_index(diags.DIA_COUNT, hdif, rot) == want["NDT"]
    assert diags.indices(0, 1) == table[(0, 0)]                       # MIX_GEO_TS without TS_DIF2 / TS_DIF4: no iTsdif
    assert lib.roms_hip_dia_index(-1, 1, 1) == 0 and lib.roms_hip_dia_index(diags.DIA_COUNT + 1, 1, 1) == 0


def test_the_abi_exposes_the_three_entries():
    lib = hip.load()
    for name in ("roms_hip_set_diagnostics", "roms_hip_set_diags", "roms_hip_get_diagnostic", "roms_hip_dia_index"):
        assert hasattr(lib, name) and name in hip.DECLARED_SYMBOLS, name
    assert "set_diags" in hip.ENTRIES
    # refused without a context, through the error path
    assert lib.roms_hip_set_diagnostics(3, 1, 1, 0) != 0 and b"come first" in lib.roms_hip_last_error()
    buf = np.zeros(4)
    assert lib.roms_hip_get_diagnostic(0, 1, 0, buf.ctypes.data, buf.size) != 0


# (nDIA, ntsDIA, ntstart, nrrec): the phases of iic = ntstart .. ntstart + 7, I = initialise, A = accumulate, - = nothing
PHASES = {(1, 0, 1, 0): "IIIIIIII", (1, 2, 1, 0): "-IIIIIII", (3, 0, 1, 0): "AIAAIAAI", (3, 2, 1, 0): "--AAIAAI",
          (3, 0, 7, 1): "IIAAIAAI", (3, 2, 6, 1): "IAIAAIAA"}


@pytest.mark.parametrize("sched", sorted(PHASES))
def test_the_phase_sequence(sched):
    nDIA, ntsDIA, ntstart, nrrec = sched
    lib = hip.load()
    b = _state(17).b
    ref = du.DiaRef(b, False, nDIA, ntsDIA, ntstart, nrrec)
    rng = np.random.default_rng(3)
    total, seen = 0.0, ""                       # (the arrays are allocated zeroed: a first accumulation adds to zero)
    I, J = ref.I, ref.J
    for iic in range(ntstart, ntstart + 8):
        ph = diags.phase(iic, *sched)
        assert ph == lib.roms_hip_avg_phase(iic, *sched) & (avg.SET | avg.ADD)
        assert (bool(ph & avg.SET), bool(ph & avg.ADD)) == du.schedule(iic, *sched)
        seen += "I" if ph & avg.SET else "A" if ph & avg.ADD else "-"
        plane = np.asfortranarray(rng.standard_normal((ref.avgzeta.shape[0], ref.avgzeta.shape[1], b.N)))
        zeta = np.asfortranarray(rng.standard_normal(ref.avgzeta.shape))
        ref.set_diags(iic, {("iTrate", 1): plane}, zeta)
        if ph & avg.SET:
            total = plane[I, J].copy()
        elif ph & avg.ADD:
            total = total + plane[I, J]
        if ph:
            assert np.array_equal(ref.trc[("iTrate", 1)][I, J], total)
    assert seen == PHASES[sched]
    assert diags.phase(5, 0, 0, 1, 0) == 0 and du.schedule(5, 0, 0, 1, 0) == (False, False)
