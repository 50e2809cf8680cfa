"""Generates tests/golden/ref_bkpp.npz from the REFERENCE's own lmd_vmix(ng, tile) built with LMD_BKPP (lmd_vmix_tile,
lmd_skpp, lmd_bkpp, lmd_finish; oracle/_ref/BENCHMARK_BKPP and BENCHMARK_MASK_BKPP, built by oracle/build_ref.sh) on
states of tests/bkpp_util.bkpp_state -- those tests/test_gpu_bkpp.py runs: N = 4, 32, 33, with and without the island, as
a channel and as a basin.  Stored per case (pack):

    <case>/sha           SHA-256 of the inputs (every array lmd_vmix reads, hbbl of the previous step, the switches)
    <case>/kbbl, /ksbl   int8, every interior column
    <case>/hbbl          float64, every interior column (the boundary values are bc_r2d_tile of these)
    <case>/cols          the interior columns (i - Istr, j - Jstr) whose whole profiles are stored: the first column of each
                         census entry of bkpp_util.lmd_bkpp_tile (crossing, no crossing with the Ekman limit, clipped to
                         the bottom, overlap of the two layers, ksbl = 0, land) and the columns Iend-1, Iend of the middle
                         row (lmd_finish's eastern edge rule)
    <case>/profiles      Akv, Akt(itemp), Akt(isalt) at those columns, W-levels 1 .. N-1 (float64)
    <case>/ksum          per column the sum of the three over the W-levels 1 .. N-1, at the interior columns with i + j
                         even (float64)

Run where the reference builds are:

    python tests/golden/make_golden_bkpp.py
"""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {f"{g}-{m}-{bs}": (g, None if m == "plain" else m, bs == "basin")
         for g in ("PARTIAL", "N32", "N33") for m in ("plain", "island") for bs in ("channel", "basin")}
INPUTS = ("Hz", "z_r", "z_w", "h", "f", "u", "v", "rho", "pden", "bvf", "alpha", "beta", "srflx", "stflx", "btflx", "sustr", "svstr",
          "bustr", "bvstr", "Akv", "Akt", "ghats", "hsbl", "rmask")


def prepare(case):
    import bkpp_util as bk
    grid, mask, basin = CASES[case]
    return bk.bkpp_state(grid, mask, basin, False)


def inputs_sha(st, hprev):
    h = hashlib.sha256()
    for name in INPUTS:
        h.update(np.ascontiguousarray(st[name]).tobytes())
    h.update(np.ascontiguousarray(hprev).tobytes())
    h.update(repr([int(st.p.masking), int(st.b.EWperiodic), int(st.b.N), st.p.g, st.p.rho0]).encode())
    return h.hexdigest()


def fixture_columns(st, hprev):
    import bkpp_util as bk
    import oracle
    import util
    sa = st.copy()
    oracle.Oracle(sa).call("lmd_vmix", util.step_idx())
    census = bk.expected(st, sa["Akv"], sa["Akt"], sa["hsbl"], hprev)["census"]
    ni, nj = census["land"].shape
    picks = [(ni - 2, nj // 2), (ni - 1, nj // 2)]
    for name in ("crossing", "no_crossing_ekman", "clipped_to_bottom", "overlap", "ksbl_zero", "land"):
        where = np.argwhere(census[name])
        if len(where):
            picks.append(where[0])
    return np.array(sorted({(int(i), int(j)) for i, j in picks}), dtype=np.int32)


def pack(case, st, hprev, res, cols=None):
    """the stored quantities of one case from hbbl, kbbl, ksbl, Akv, Akt on the tile's extents (the reference's, the
    restatement's or the device's)"""
    import bkpp_util as bk
    b, N = st.b, st.b.N
    I = bk.interior(b)
    cols = fixture_columns(st, hprev) if cols is None else np.asarray(cols)
    K = np.stack([res["Akv"][I][:, :, 1:N], res["Akt"][I][:, :, 1:N, 0], res["Akt"][I][:, :, 1:N, 1]], axis=-1)
    ii, jj = np.meshgrid(np.arange(K.shape[0]), np.arange(K.shape[1]), indexing="ij")
    return {f"{case}/sha": np.array(inputs_sha(st, hprev)), f"{case}/cols": cols.astype(np.int32),
            f"{case}/kbbl": res["kbbl"][I].astype(np.int8), f"{case}/ksbl": res["ksbl"][I].astype(np.int8),
            f"{case}/hbbl": np.ascontiguousarray(res["hbbl"][I], dtype=np.float64),
            f"{case}/profiles": np.ascontiguousarray(K[cols[:, 0], cols[:, 1]]),
            f"{case}/ksum": K.sum(axis=(2, 3))[(ii + jj) % 2 == 0]}


if __name__ == "__main__":
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case, (grid, mask, basin) in CASES.items():          # one process per case: ref_setup is once per process
            path = os.path.join(tmp, case + ".npz")
            subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ref_worker.py"), "bkpp", grid, mask or "plain",
                            "basin" if basin else "channel", "stable", path], check=True, stdout=subprocess.DEVNULL)
            st, hprev = prepare(case)
            out.update(pack(case, st, hprev, dict(np.load(path))))
    out["cases"] = np.array(list(CASES))
    dest = os.path.join(HERE, "ref_bkpp.npz")
    np.savez_compressed(dest, **out)
    print(os.path.getsize(dest) // 1024, "KiB")
