"""Worker of tests/test_gpu_context_reuse.py: the scenarios that need a process of their own -- ONE rank initialised with
an RCCL id (loopback: the tile is its own W / E neighbour and every kernel takes its several-tiles branch).

    bounds    a second roms_hip_set_bounds in one loopback context (scenario 10); saves the second state
    single    LOOP_2D by the loop, by single calls and interleaved, each in a loopback context with graph_exchanges(1)
              (scenario 11); saves the three states
    two_ctx   a loopback context with graph_exchanges(1), sources and climatology, closed; then a loopback context that
              asks for nothing (scenario 12); saves its state and both graph_exchanges_state() values"""
import sys

import numpy as np

from tiling_util import rccl_unique_id as unique_id


def main(mode, app, out):
    import reuse_util as ru
    from roms_trunk_mgh_amd import abi, ana, hip, main3d
    extra = {}
    if mode == "bounds":
        st, _, _ = ru.second_bounds_run(app, be_kw=dict(nccl_unique_id=unique_id()))
    elif mode == "single":
        states, indx1, fields = [], [], {}
        for pattern in ("LLLLLLL", "SSSSSSS", "LLLSLLL"):
            st, m, state = ru.mixed_run(ru.tile(app), pattern, be_kw=dict(nccl_unique_id=unique_id()), graph_exchanges=True)
            states.append(state)
            indx1.append(m.indx1)
            fields.update({f"{pattern}:{name}": st[name] for name, _, _ in abi.FIELDS})
        np.savez(out, states=np.array(states), indx1=np.array(indx1), **fields)
        return
    elif mode == "two_ctx":
        st1 = ru.tile(app)
        st1.p.point_sources = 1
        st1.sources = ru.source_table(st1, 3, "river")
        ana.analytic_clima(st1)
        be = hip.RomsHip(st1, nccl_unique_id=unique_id())
        try:
            be.graph_exchanges(1)
            m = main3d.Main3D(be)
            m.initial()
            m.run(ru.K)
            extra["first_state"] = np.array(be.graph_exchanges_state())
            be.check_guards()
        finally:
            be.close()
        st = ru.tile(app)
        be = hip.RomsHip(st, nccl_unique_id=unique_id())
        try:
            m = main3d.Main3D(be)
            m.initial()
            m.run(ru.K)
            extra["second_state"] = np.array(be.graph_exchanges_state())
            be.to_host()
            be.check_guards()
        finally:
            be.close()
    else:
        raise SystemExit(f"unknown mode {mode}")
    np.savez(out, **{name: st[name] for name, _, _ in abi.FIELDS}, **extra)


if __name__ == "__main__":
    main(*sys.argv[1:4])
