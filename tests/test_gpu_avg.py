"""-m gpu: the time-averaged fields on the device (AVERAGES: roms_hip_set_averages, roms_hip_set_avg, csrc/k_avg.hip).

set_avg.F needs the I/O layer, so the reference cannot make a vector for this routine: the yardstick is the numpy
restatement tests/avg_util.py, whose known answers tests/test_avg.py checks without a GPU.  Bit for bit throughout
(np.array_equal): the kernel performs the reference's operations in the reference's order and the build does not
contract multiply-adds.
  1. per-call parity of every average and counter on the whole allocated array, over two windows and the restart case
  2. seven whole steps through main3d; nothing else changes
  3. tiling invariance over the relay, and one tile in RCCL loopback
  4. the refusals"""
import numpy as np
import pytest

import avg_util as au
import tiling_util
import util
from roms_trunk_mgh_amd import abi, ana, avg, hip, main3d
from test_gpu_wide import SHAPES, seam_dry, seam_land

pytestmark = pytest.mark.gpu

SOURCES = ("zeta", "ubar", "vbar", "u", "v", "t", "W", "wvel", "rho", "Akv", "Akt", "hsbl", "sustr", "svstr", "bustr", "bvstr",
           "Pair", "Tair", "Uwind", "Vwind", "stflx", "srflx", "lhflx", "lrflx", "shflx", "evap", "rain", "Huon", "Hvom")
# (nAVG, ntsAVG, ntstart, nrrec)
SCHEDULES = [(1, 1, 1, 0), (1, 3, 1, 0), (3, 1, 1, 0), (3, 3, 1, 0), (3, 1, 7, 1)]


def _state(shape, nghost, periodic, wet):
    ov = dict(SHAPES[shape])
    if nghost == 3:
        ov["uv_vis4"] = 1                                 # three ghost points (inp_par.F:264-278)
    if not periodic:
        ov["EWperiodic"] = False
    kw = dict(mask="island", land=seam_land(shape), wet=True, dry=seam_dry(shape)) if wet else {}
    st = util.prepared_state("BENCHMARK_TINY", overrides=ov, **kw)
    assert st.b.NghostPoints == nghost and bool(st.b.EWperiodic) == periodic and st.p.wet_dry == int(wet)
    return st


def _randomise(st, rng):
    for name in SOURCES:
        st[name][:] = rng.standard_normal(st[name].shape)


def _compare(be, ref, tag):
    for (name, it), want in ref.avg.items():
        got = be.get_average(name, it)
        assert np.array_equal(got, want), (tag, name, it, float(np.abs(got - want).max()))
    for name, want in ref.cnt.items():
        got = be.get_average(name)
        assert np.array_equal(got, want), (tag, name, float(np.abs(got - want).max()))


@pytest.mark.parametrize("wet", [False, True])
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nghost", [2, 3])
@pytest.mark.parametrize("shape", ["w3", "thin"])
def test_every_call_equals_the_restatement(shape, nghost, periodic, wet):
    st = _state(shape, nghost, periodic, wet)
    b = st.b
    sel = au.all_in_scope(b.NT)
    rng = np.random.default_rng(7)
    be = hip.RomsHip(st)
    try:
        for nAVG, ntsAVG, ntstart, nrrec in SCHEDULES:
            kw = dict(nAVG=nAVG, ntsAVG=ntsAVG, ntstart=ntstart, nrrec=nrrec)
            be.set_averages(au.averages_of(b, sel, **kw))
            ref = au.AvgRef(b, wet, nAVG, ntsAVG, ntstart, nrrec, sel)
            seen = 0
            for k, iic in enumerate(range(ntstart, ntstart + 2 * nAVG + 2)):
                _randomise(st, rng)
                be.to_device(SOURCES)
                s = util.step_idx(iic=iic, kstp=1 + k % 3, nrhs=1 + k % 2)
                be.call("set_avg", s)
                ph = ref.set_avg(st, s)
                seen |= sum(1 << q for q in range(4) if ph[q])
                _compare(be, ref, (kw, iic))
            assert seen & 5 == 5 and (nAVG == 1 or seen & 2)            # initialised, closed, and accumulated
            assert any(np.abs(a).max() > 0.0 for a in ref.avg.values())
        be.check_guards()
        # a small selection: nothing else is allocated, nothing else is touched
        few = [("avgzeta", 0), ("avgt", 2), ("avgUT", 1)]
        be.set_averages(au.averages_of(b, few, nAVG=2))
        ref = au.AvgRef(b, wet, 2, 1, 1, 0, few)
        for k, iic in enumerate(range(1, 6)):
            _randomise(st, rng)
            be.to_device(SOURCES)
            s = util.step_idx(iic=iic, kstp=1 + k % 3, nrhs=1 + k % 2)
            be.call("set_avg", s)
            ref.set_avg(st, s)
            _compare(be, ref, ("few", iic))
        lib = be.l
        for name, it in sel:
            ptr = lib.roms_hip_average_device_ptr(avg.AVG_ID[name], it)
            assert bool(ptr) == ((name, it) in few), (name, it)
        be.check_guards()
    finally:
        be.close()


# ------------------------------------------------------------------------------------------- 2. end to end --
class _Proxy:
    """forwards every call; on set_avg it also pulls the state and feeds the restatement"""

    def __init__(self, be, ref):
        self._be, self._ref, self.closed = be, ref, []

    def __getattr__(self, name):
        return getattr(self._be, name)

    def call(self, kernel, s):
        self._be.call(kernel, s)
        if kernel == "set_avg":
            self._be.to_host()
            if self._ref.set_avg(self._be.st, s)[2]:
                _compare(self._be, self._ref, ("main3d", s.iic))
                self.closed.append(s.iic)


PROGNOSTIC = ("zeta", "ubar", "vbar", "u", "v", "t", "Hz", "W", "Huon", "Hvom", "rho", "Zt_avg1", "DU_avg1", "DV_avg2")


def test_seven_steps_through_main3d():
    st0 = ana.make_tile("UPWELLING", perturb=1.0, overrides=SHAPES["w3"])
    sel = au.all_in_scope(st0.b.NT)
    out = {}
    for key in ("with", "without"):
        st = st0.copy()
        be = hip.RomsHip(st)
        try:
            if key == "with":
                ref = au.AvgRef(st.b, 0, 3, 1, 1, 0, sel)
                proxy = _Proxy(be, ref)
                m = main3d.Main3D(proxy, averages=au.averages_of(st.b, sel, nAVG=3))
            else:
                m = main3d.Main3D(be)
            m.initial()
            m.run(7)
            be.to_host()
            be.check_guards()
        finally:
            be.close()
        out[key] = st
    assert proxy.closed == [4, 7]
    assert np.abs(ref.avg[("avgUT", 1)]).max() > 0.0 and np.abs(ref.avg[("avgzeta", 0)]).max() > 0.0
    for name in PROGNOSTIC:
        assert np.array_equal(out["with"][name], out["without"][name], equal_nan=True), name
    assert not np.array_equal(out["with"]["t"], st0["t"])


# ------------------------------------------------------------------------------------- 3. tiling invariance --
def _tiles_equal_single(tmp_path, world, ntI, ntJ, variant):
    import mp_gpu_avg_worker as worker
    st = worker.tiled_state(variant)
    be = hip.RomsHip(st)
    try:
        want = worker.run(be, st)
    finally:
        be.close()
    assert all(np.abs(a).max() > 0.0 for a in want.values())
    tiling_util.spawn_ranks("mp_gpu_avg_worker.py", world, [ntI, ntJ, tmp_path, variant], timeout=600)
    gb = st.b
    tiling_util.assert_tiles_equal(tmp_path, world, want, gb, list(want), owned="IstrR:IendR")
    if "basin" not in variant:
        for r, d, (_, J), (_, Jg) in tiling_util.tiles(tmp_path, world, gb, owned="IstrR:IendR"):
            LBi, UBi = d["LBi"], d["UBi"]
            # the periodic ghost columns, filled after the close
            cols = [i for i in list(range(-2, 1)) + list(range(gb.Lm + 1, gb.Lm + gb.NghostPoints + 1)) if LBi <= i <= UBi]
            for key, glob in want.items():
                a = d[key]
                for i in cols:
                    assert np.array_equal(a[i - LBi, J], glob[i - gb.LBi, Jg]), (key, r, i)
                    assert np.array_equal(a[i - LBi, J], glob[(i - 1) % gb.Lm + 1 - gb.LBi, Jg]), (key, r, i, "image")


@pytest.mark.parametrize("ntI,ntJ,variant", [(2, 1, ""), (1, 2, ""), (2, 1, "basin"), (1, 2, "basin")])
def test_tiled_averages_equal_the_single_tile_run(tmp_path, ntI, ntJ, variant):
    _tiles_equal_single(tmp_path, ntI * ntJ, ntI, ntJ, variant)


def test_rccl_loopback_equals_the_single_tile_run(tmp_path):
    _tiles_equal_single(tmp_path, 1, 1, 1, "rccl")


# ---------------------------------------------------------------------------------------------- 4. refusals --
def test_refusals_use_the_error_path_and_leave_the_library_usable():
    lib = hip.load()
    st = util.prepared_state("UPWELLING")
    b = st.b
    ok = au.averages_of(b, [("avgzeta", 0), ("avgt", 1)], nAVG=2)
    s = util.step_idx(iic=2)
    assert hip.RomsHip._live is None
    assert lib.roms_hip_init(0, 1, 1, 0, None) == 0
    try:                                                       # before bounds / params
        assert lib.roms_hip_set_averages(*ok.c_args()) != 0 and b"come first" in lib.roms_hip_last_error()
    finally:
        assert lib.roms_hip_finalize() == 0
    be = hip.RomsHip(st, leave_unregistered=("lhflx",))        # an application without BULK_FLUXES has no lhflx
    try:
        with pytest.raises(RuntimeError, match="lhflx"):
            be.set_averages(au.averages_of(b, [("avglhf", 0)], nAVG=2))
    finally:
        be.close()
    be = hip.RomsHip(st)
    try:
        be.call("set_avg", s)                                  # nothing configured: returns 0, writes nothing
        be.check_guards()
        assert not lib.roms_hip_average_device_ptr(avg.AVG_ID["avgzeta"], 0)
        for name in ("avgu2dE", "avgpvor3d", "avghbbl", "avgu3Sd", "avgbedldv", "avgDV_avg2"):
            bad = avg.Averages(b, 2, select=["avgzeta", name])
            assert lib.roms_hip_set_averages(*bad.c_args()) != 0
            msg = lib.roms_hip_last_error()
            assert name.encode() in msg and b"not built" in msg, msg
            assert not lib.roms_hip_average_device_ptr(avg.AVG_ID["avgzeta"], 0)       # left as it was
        neg = list(ok.c_args())
        neg[0] = -1
        assert lib.roms_hip_set_averages(*neg) != 0 and b"nAVG < 0" in lib.roms_hip_last_error()
        be.set_averages(ok)
        be.call("set_avg", s)
        z = be.get_average("avgzeta")
        assert np.array_equal(z[st.I(b.IstrR, b.IendR), st.J(b.JstrR, b.JendR)],
                              st["zeta"][:, :, s.kstp - 1][st.I(b.IstrR, b.IendR), st.J(b.JstrR, b.JendR)])
        with pytest.raises(RuntimeError, match="avgrho is not selected"):
            be.get_average("avgrho")
        with pytest.raises(RuntimeError, match="not selected"):
            be.get_average("avgt", 2)
        with pytest.raises(RuntimeError, match="not selected"):
            be.get_average("rmask_avg")                        # no wet_dry: no counters
        buf = np.zeros(z.size + 1)
        assert lib.roms_hip_get_average(avg.AVG_ID["avgzeta"], 0, buf.ctypes.data, buf.size) != 0
        assert b"doubles" in lib.roms_hip_last_error() and not buf.any()
        assert lib.roms_hip_get_average(avg.AVG_COUNT, 0, buf.ctypes.data, buf.size) != 0
        # a refused selection keeps the one in force
        bad = avg.Averages(b, 2, select=["avgu2dE"])
        assert lib.roms_hip_set_averages(*bad.c_args()) != 0
        assert np.array_equal(be.get_average("avgzeta"), z)
        be.set_averages(None)                                  # nAVG = 0 releases everything
        assert not lib.roms_hip_average_device_ptr(avg.AVG_ID["avgzeta"], 0)
        be.call("set_avg", s)
        be.check_guards()
    finally:
        be.close()
