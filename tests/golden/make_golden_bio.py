"""Generates tests/golden/ref_bio.npz from the REFERENCE's own biology(ng, tile) built with NPZD_POWELL (biology.F with
npzd_Powell.h; oracle/_ref/UPWELLING_BIO and, for the constpar set, UPWELLING_BIO_CPAR, built by oracle/build_ref.sh) on
states of tests/bio_util.bio_state -- those tests/test_gpu_bio.py runs.  Stored per case (pack):

    <case>/sha       SHA-256 of the inputs (Hz, z_w, srflx, t, the parameters, dt, rho0): a drifted state builder fails
    <case>/cols      the interior columns (i - Istr, j - Jstr) whose whole profiles are stored: a day and a night column
                     with a negative pool, a column where no pool can pay, the shallowest and the deepest column, the last
                     column of the tile, and with the island a land column
    <case>/profiles  t(nnew) of the four pools at those columns, every level (float64)
    <case>/colsum    per column the sum of t(nnew) over the levels and the four pools, at the interior columns with
                     i + j even (float64): every second column of the tile is checked through its inventory

Run where the reference builds are:

    python tests/golden/make_golden_bio.py
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

CASES = {f"{g}-{m}-{ps}": (g, None if m == "plain" else m, ps)
         for g, ps in (("PARTIAL", "sink"), ("N17", "sink"), ("N33", "sink"), ("N33", "default"), ("TINY", "constpar"))
         for m in ("plain", "island")}
NNEW = 2


def prepare(case):
    import bio_util as bu
    grid, mask, pset = CASES[case]
    st = bu.bio_state(grid, mask)
    return st, bu.params(pset, st.p.dt)


def inputs_sha(st, par):
    from roms_trunk_mgh_amd import bio
    h = hashlib.sha256()
    for name in ("Hz", "z_w", "srflx", "t"):
        h.update(np.ascontiguousarray(st[name]).tobytes())
    h.update(repr([(n, getattr(par, n)) for n in sorted(bio.DEFAULTS)] + [par.tracers(st.b), st.p.dt, st.p.rho0]).encode())
    return h.hexdigest()


def fixture_columns(st, par):
    import bio_util as bu
    b = st.b
    I = bu.interior(b)
    a = bu.columns(st, par)
    day = a["srflx"] > 0.0
    neg = (a["tS"][..., bu.iPhyt] < 0.0).any(axis=-1)
    low = (a["tS"].max(axis=-1) < bu.MINVAL).any(axis=-1)
    depth = -a["z_w"][..., 0]
    picks = [np.argwhere(day & neg)[0], np.argwhere(~day & neg)[0], np.argwhere(low)[0],
             np.unravel_index(depth.argmin(), depth.shape), np.unravel_index(depth.argmax(), depth.shape),
             (depth.shape[0] - 1, depth.shape[1] - 1)]
    if st.p.masking:
        picks.append(np.argwhere(st["rmask"][I] == 0.0)[0])
    return np.array(sorted({(int(i), int(j)) for i, j in picks}), dtype=np.int32)


def pack(case, st, par, t, cols=None):
    """the stored quantities of one case from a whole t array (the reference's, the restatement's or the device's)"""
    import bio_util as bu
    b = st.b
    I = bu.interior(b)
    it0 = par.tracers(b)[0] - 1
    new = t[I][:, :, :, NNEW - 1, it0:it0 + 4]
    cols = fixture_columns(st, par) if cols is None else np.asarray(cols)
    ii, jj = np.meshgrid(np.arange(new.shape[0]), np.arange(new.shape[1]), indexing="ij")
    return {f"{case}/sha": np.array(inputs_sha(st, par)), f"{case}/cols": cols.astype(np.int32),
            f"{case}/profiles": np.ascontiguousarray(new[cols[:, 0], cols[:, 1]]),
            f"{case}/colsum": new.sum(axis=(2, 3))[(ii + jj) % 2 == 0]}


if __name__ == "__main__":
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case, (grid, mask, pset) in CASES.items():           # one process per case: ref_setup is once per process
            path = os.path.join(tmp, case + ".npz")
            subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ref_worker.py"), "bio", grid, mask or "plain", pset, path],
                           check=True, stdout=subprocess.DEVNULL)
            st, par = prepare(case)
            out.update(pack(case, st, par, np.load(path)["t"]))
    out["cases"] = np.array(list(CASES))
    dest = os.path.join(HERE, "ref_bio.npz")
    np.savez_compressed(dest, **out)
    print(os.path.getsize(dest) // 1024, "KiB")
