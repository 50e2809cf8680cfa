"""Generates tests/golden/ref_geouv4.npz from the REFERENCE's own uv3dmix4 built with MIX_GEO_UV and UV_VIS4
(uv3dmix4_geo.h; oracle/_ref/UPWELLING_GEOUV4, SEAMOUNT_GEOUV4, UPWELLING_MASK_GEOUV4, UPWELLING_MASK_WET_GEOUV4 built by
oracle/build_ref.sh) on the states of tests/ref_worker.geouv4_state (those of tests/test_gpu_uvgeo4.py, uv_vis2 =
uv_vis4 = 2): channel, the seamount (steep slopes), closed basins and gradient conditions on u, v on all sides (the
LapU / LapV edge and corner rule), the island grid, the island grid with gradient conditions, the island grid with
WET_DRY masks.  Stored per case, with the sampling of make_golden_geouv.py: u, v at every second point of three levels,
rufrc, rvfrc in full, and a SHA-256 of the whole arrays.  Run where the reference builds are:

    python tests/golden/make_golden_geouv4.py
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from make_golden_geouv import NAMES, results  # noqa: E402,F401

CASES = {
    "channel": dict(config="UPWELLING", basin=None, mask=None, wet=False),
    "seamount": dict(config="SEAMOUNT", basin=None, mask=None, wet=False),
    "closed": dict(config="UPWELLING", basin="closed", mask=None, wet=False),
    "seamount_closed": dict(config="SEAMOUNT", basin="closed", mask=None, wet=False),
    "open": dict(config="UPWELLING", basin="open", mask=None, wet=False),
    "seamount_open": dict(config="SEAMOUNT", basin="open", mask=None, wet=False),
    "island": dict(config="UPWELLING", basin=None, mask="island", wet=False),
    "island_open": dict(config="UPWELLING", basin="open", mask="island", wet=False),
    "island_wet": dict(config="UPWELLING", basin=None, mask="island", wet=True),
}


def prepare(case):
    import ref_worker
    import util
    c = CASES[case]
    was = util.WET
    util.WET = c["wet"]
    try:
        return ref_worker.geouv4_state(c["config"], c["basin"], c["mask"])
    finally:
        util.WET = was


def child(case):
    from oracle import ref
    st, s = prepare(case)
    ref.Ref(st).call("uv3dmix4", s)
    np.savez_compressed(os.path.join(HERE, f"_geouv4_{case}.npz"), **results(st, s, case))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        child(sys.argv[1])
    else:
        out = {}
        for case in CASES:           # one process per case: each loads another build of the reference
            subprocess.run([sys.executable, os.path.abspath(__file__), case], check=True)
            f = os.path.join(HERE, f"_geouv4_{case}.npz")
            out.update(dict(np.load(f)))
            os.remove(f)
        np.savez_compressed(os.path.join(HERE, "ref_geouv4.npz"), **out)
        print(os.path.getsize(os.path.join(HERE, "ref_geouv4.npz")) // 1024, "KiB")
