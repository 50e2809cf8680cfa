"""Generates tests/golden/ref_ddmix.npz from the REFERENCE's own rho_eos.F and lmd_vmix(ng, tile) (lmd_vmix_tile, lmd_skpp,
lmd_swfrac, lmd_bkpp, lmd_finish) built with the BENCHMARK option set plus -DLMD_DDMIX: plain, with -DMASKING, and each
again with -DLMD_BKPP.  No build of oracle/build_ref.sh defines LMD_DDMIX, so this script builds its own four, by the
recipe that script documents (cpp -P -traditional, flang -O2 -fPIC -ffp-contract=off, the file list and the CPP
definitions read from the script, oracle/ref_wrap.F90 as the bind(C) front end), into the git-ignored

    oracle/_ref/BENCHMARK_DDMIX, BENCHMARK_MASK_DDMIX, BENCHMARK_DDMIX_BKPP, BENCHMARK_MASK_DDMIX_BKPP

which oracle.ref.Ref(state, build=TAG) loads.  MIXING(ng)%alfaobeta is no member of roms_fields_t: the few lines of
ACCESSOR below, compiled into each of the four, copy it out.  The states are those of tests/ddmix_util.ddmix_state and
the sequence the one of ddmix_util.run_device: rho_eos, the builder's density profiles back in place, lmd_vmix.  The
plain builds BENCHMARK / BENCHMARK_MASK of oracle/build_ref.sh give Akt without the option on the same states.  Stored
per case <grid>-<plain|island>-<skpp|bkpp> (pack):

    <case>/sha              SHA-256 of the inputs: a drifted state builder fails
    <case>/cols             the interior columns (i - Istr, j - Jstr) whose whole profiles are stored
    <case>/prof/<field>     one array per field -- alfaobeta, Akt1, Akt2 (itemp, isalt), Akv, ghats1, ghats2 -- at those
                            columns, W-levels 1 .. N (level 0 of alfaobeta is never written; of the others it is an input);
                            each field is compared on its own, within the bound times its own maximum
    <case>/sum/<field>      per column the sum of the field over those levels, at the interior columns with
                            (i + j) % STRIDE == 0 (not for PARTIAL)
    <case>/hsbl             at the columns of cols; with bkpp also <case>/hbbl
    <case>/plain/<field>, /plainsum/<field>   (skpp cases) Akt1, Akt2 of the build without LMD_DDMIX, laid out alike

PARTIAL (Lm = 67, Mm = 6, N = 4, the partial-workgroup shape) stores whole fields: cols is every interior column.  A
departure from the plan: whole fields of BENCHMARK_TINY are 3 MB a case, twelve times the size limit of a committed file
for the four cases, so TINY stores whole profiles at 18 columns spread over the tile (every workgroup column and row of
the launch) and column sums at every 16th column; N32 / N33 store 6 columns and every 8th column's sums.

Run where the reference and flang are:

    python tests/golden/make_golden_ddmix.py <path of the reference's root directory>
"""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRIDS = ("TINY", "PARTIAL", "N32", "N33")
CASES = {f"{g}-{m}-{l}": (g, None if m == "plain" else m, l == "bkpp")
         for g in GRIDS for m in ("plain", "island") for l in ("skpp", "bkpp")}
STRIDE = {"TINY": 16, "PARTIAL": None, "N32": 8, "N33": 8}        # None: whole fields, no sums
INPUTS = ("Hz", "z_r", "z_w", "h", "f", "u", "v", "t", "rho", "pden", "bvf", "alpha", "beta", "srflx", "stflx", "btflx", "sustr",
          "svstr", "bustr", "bvstr", "Akv", "Akt", "ghats", "hsbl", "rmask")
FIELDS = ("alfaobeta", "Akt1", "Akt2", "Akv", "ghats1", "ghats2")

ACCESSOR = """subroutine ref_get_alfaobeta (n, out) bind(C, name='ref_get_alfaobeta')
  use iso_c_binding
  use mod_mixing, only : MIXING
  integer(c_long), value :: n
  real(c_double), intent(out) :: out(n)
  out = reshape(MIXING(1)%alfaobeta, (/ n /))
end subroutine ref_get_alfaobeta
"""


def tag_of(mask, bkpp, ddmix=True):
    return "BENCHMARK" + ("_MASK" if mask else "") + ("_DDMIX" if ddmix else "") + ("_BKPP" if bkpp else "")


def build_tag(ref_root, tag):
    """one build of the reference with LMD_DDMIX, by the recipe of oracle/build_ref.sh (read, not changed)"""
    odir = os.path.join(ROOT, "oracle")
    dest = os.path.join(odir, "_ref", tag)
    if os.path.exists(os.path.join(dest, "libref.so")):
        return
    script = open(os.path.join(odir, "build_ref.sh")).read()
    files = re.search(r'^FILES="(.*?)"', script, re.S | re.M).group(1).split()
    fflags = re.search(r'^FFLAGS="(.*?)"', script, re.M).group(1).split()
    assert fflags == ["-O2", "-fPIC", "-ffp-contract=off"], fflags
    masking, bkpp = "_MASK" in tag, tag.endswith("_BKPP")
    xdef = (["-DMASKING"] if masking else []) + ["-DLMD_DDMIX"] + (["-DLMD_BKPP"] if bkpp else [])
    wdef = ["-DREF_BKPP"] if bkpp else []
    if bkpp:
        files.insert(files.index("Nonlinear/lmd_vmix"), "Nonlinear/lmd_bkpp")
    if masking:                                  # (ana_mask.h stops the compilation on purpose: build_ref.sh says why)
        files.remove("Functionals/analytical")
    os.makedirs(dest, exist_ok=True)
    roms = os.path.join(ref_root, "ROMS")
    hdr = "benchmark.h"
    cppf = ["-P", "-traditional", "-w", "-DBENCHMARK"] + xdef + [f'-DROMS_HEADER="{hdr}"', f'-DROOT_DIR="{ref_root}"'] + \
        [f'-D{n}="x"' for n in ("HOST_NAME", "SVN_URL", "SVN_REV", "ANALYTICAL_DIR", "HEADER_DIR", "MY_ANALYTICAL_DIR", "MY_HEADER_DIR",
                                "MY_ROOT_DIR", "MY_ANALYTICAL")] + \
        ['-DMY_OS="Linux"', '-DMY_CPU="x86_64"', '-DMY_FORT="flang"', '-DMY_FC="flang"', '-DMY_FFLAGS="-O2"', f'-DHEADER="{hdr}"',
         f'-DMY_HEADER="{hdr}"', "-I" + os.path.join(odir, "ref_headers")] + \
        ["-I" + os.path.join(roms, d) for d in ("Include", "Functionals", "Nonlinear", "Utility", "Modules")]
    run = lambda cmd, **kw: subprocess.run(cmd, check=True, cwd=dest, **kw)
    objs = []
    for f in files:
        bn = os.path.basename(f)
        with open(os.path.join(dest, bn + ".f90"), "w") as out:
            run(["cpp"] + cppf + [os.path.join(roms, f + ".F")], stdout=out)
        run(["flang"] + fflags + ["-c", bn + ".f90", "-o", bn + ".o"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        objs.append(bn + ".o")
    with open(os.path.join(dest, "ref_wrap_pp.f90"), "w") as out:
        run(["cpp", "-P", "-traditional", "-w", "-DBENCHMARK"] + xdef + wdef + [os.path.join(odir, "ref_wrap.F90")], stdout=out)
    run(["flang"] + fflags + ["-c", "ref_wrap_pp.f90", "-o", "ref_wrap.o"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    open(os.path.join(dest, "ddmix_accessor.f90"), "w").write(ACCESSOR)
    run(["flang"] + fflags + ["-c", "ddmix_accessor.f90", "-o", "ddmix_accessor.o"])
    run(["flang", "-shared", "-o", "libref.so"] + objs + ["ref_wrap.o", "ddmix_accessor.o"])
    for f in os.listdir(dest):                   # keep no preprocessed reference text around
        if f.endswith(".f90"):
            os.remove(os.path.join(dest, f))
    print("built", dest, flush=True)


def prepare(case):
    import ddmix_util as dd
    grid, mask, bkpp = CASES[case]
    return dd.ddmix_state(grid, mask)


def inputs_sha(st, hprev):
    h = hashlib.sha256()
    for name in INPUTS:
        h.update(np.ascontiguousarray(st[name]).tobytes())
    h.update(np.ascontiguousarray(hprev).tobytes())
    h.update(repr([int(st.p.masking), int(st.p.nonlin_eos), int(st.b.EWperiodic), int(st.b.N), st.p.g, st.p.rho0]).encode())
    return h.hexdigest()


def fixture_columns(st, grid):
    """PARTIAL: every interior column.  TINY: a 4 x 4 lattice over the tile, N32 / N33: 4 columns; each with Iend-1, Iend
    of the middle row (lmd_finish's eastern edge rule)"""
    b = st.b
    ni, nj = b.Iend - b.Istr + 1, b.Jend - b.Jstr + 1
    if STRIDE[grid] is None:
        picks = [(i, j) for i in range(ni) for j in range(nj)]
    elif grid == "TINY":
        picks = [(i, j) for i in range(3, ni, 16) for j in range(1, nj, 8)]
    else:
        picks = [((3 + 17 * q) % ni, (1 + 2 * q) % nj) for q in range(4)]
    return np.array(sorted(set(picks + [(ni - 2, nj // 2), (ni - 1, nj // 2)])), dtype=np.int32)


def _field(st, res, name):
    """one field on the interior columns, W-levels 1 .. N"""
    import ddmix_util as dd
    I = dd.interior(st.b)
    a = {"alfaobeta": lambda: res["alfaobeta"][I], "Akv": lambda: res["Akv"][I], "Akt1": lambda: res["Akt"][I][..., 0],
         "Akt2": lambda: res["Akt"][I][..., 1], "ghats1": lambda: res["ghats"][I][..., 0], "ghats2": lambda: res["ghats"][I][..., 1]}[name]()
    return a[:, :, 1:]


def pack(case, st, hprev, res, plain=None, cols=None):
    """the stored quantities of one case from alfaobeta, Akv, Akt, ghats, hsbl[, hbbl] on the tile's extents (the
    reference's or the device's); plain: dict(Akt) of the run without the option (skpp cases)"""
    import ddmix_util as dd
    grid, mask, bkpp = CASES[case]
    I = dd.interior(st.b)
    cols = fixture_columns(st, grid) if cols is None else np.asarray(cols)
    ci, cj = cols[:, 0], cols[:, 1]
    ni, nj = res["hsbl"][I].shape
    ii, jj = np.meshgrid(np.arange(ni), np.arange(nj), indexing="ij")
    sel = None if STRIDE[grid] is None else (ii + jj) % STRIDE[grid] == 0
    out = {f"{case}/sha": np.array(inputs_sha(st, hprev)), f"{case}/cols": cols.astype(np.int32),
           f"{case}/hsbl": np.ascontiguousarray(res["hsbl"][I][ci, cj])}
    if bkpp:
        out[f"{case}/hbbl"] = np.ascontiguousarray(res["hbbl"][I][ci, cj])
    for tag, stag, src, names in (("prof", "sum", res, FIELDS), ("plain", "plainsum", plain, ("Akt1", "Akt2"))):
        if src is None:
            continue
        for name in names:
            K = _field(st, src, name)
            out[f"{case}/{tag}/{name}"] = np.ascontiguousarray(K[ci, cj])
            if sel is not None:
                out[f"{case}/{stag}/{name}"] = K.sum(axis=2)[sel]
    return out


def child(case, ddmix, path):
    """one process per reference configuration: the sequence of ddmix_util.run_device on the reference"""
    import ddmix_util as dd
    import util
    from oracle import ref
    grid, mask, bkpp = CASES[case]
    st, hprev = dd.ddmix_state(grid, mask)
    s = util.step_idx()
    st_r = st.copy()
    R = ref.Ref(st_r, build=tag_of(mask, bkpp, ddmix))
    if bkpp:
        R.kpp_layers(hprev)
    out = {}
    if ddmix:
        R.call("rho_eos", s)
        aob = np.zeros(st["z_w"].shape, order="F")
        R.l.ref_get_alfaobeta.argtypes = [C.c_long, C.c_void_p]
        R.l.ref_get_alfaobeta(aob.size, aob.ctypes.data)
        aob[:, :, 0] = 0.0                       # never written by rho_eos: whatever the allocation held
        out["alfaobeta"] = aob
        for name in dd.RHO_EOS_OUT:
            st_r[name][...] = st[name]
    R.physics("lmd_vmix", s)
    out.update({n: st_r[n] for n in dd.OUT})
    if bkpp:
        out.update(R.kpp_layers())
    np.savez(path, **out)


def compare(case, st, res, plain):
    """the restatement against the reference: alfaobeta bit for bit on the computed range, the increment recovered as
    Akt(LMD_DDMIX) - Akt(plain) at the levels the surface layer leaves alone"""
    import bkpp_util as bk
    import ddmix_util as dd
    b, N = st.b, st.b.N
    T = (slice(b.IstrT - b.LBi, b.IendT - b.LBi + 1), slice(b.JstrT - b.LBj, b.JendT - b.LBj + 1))
    want = dd.alfaobeta(st)
    same = bool(np.array_equal(res["alfaobeta"][T][:, :, 1:], want[T][:, :, 1:]))
    msg = f"{case}: alfaobeta bit for bit {same}"
    if plain is not None:
        I = dd.interior(b)
        nt, ns, reg, info = dd.state_increment(st)
        ks = bk.ksbl_from_hsbl(st, res["hsbl"])[I]
        alone = np.arange(1, N)[None, None, :] <= ks[:, :, None]
        if b.east_edge:
            alone[-2] = False                    # column Iend-1 receives column Iend (lmd_vmix.F:560-575)
        worst = 0.0
        for it, nu in ((0, nt), (1, ns)):
            got = (res["Akt"][I][:, :, 1:N, it] - plain["Akt"][I][:, :, 1:N, it])[alone]
            worst = max(worst, float(np.abs(got - nu[I][alone]).max()) / float(np.abs(res["Akt"][I][:, :, 1:N, it]).max()))
        msg += f", increment within {worst:.3e} of Akt's maximum over {int(alone.sum())} points"
    print(msg, flush=True)
    assert same, case


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3] == "1", sys.argv[4])
        sys.exit(0)
    ref_root = sys.argv[1]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(4) as ex:
        list(ex.map(lambda t: build_tag(ref_root, t), [tag_of(m, l) for m in (None, "island") for l in (False, True)]))
    out = {}
    me = os.path.abspath(__file__)
    with tempfile.TemporaryDirectory() as tmp:
        for case, (grid, mask, bkpp) in CASES.items():
            st, hprev = prepare(case)
            path = os.path.join(tmp, case + ".npz")
            subprocess.run([sys.executable, me, "--child", case, "1", path], check=True)
            res, plain = dict(np.load(path)), None
            if not bkpp:
                subprocess.run([sys.executable, me, "--child", case, "0", path], check=True)
                plain = dict(np.load(path))
            compare(case, st, res, plain)
            out.update(pack(case, st, hprev, res, plain))
    out["cases"] = np.array(list(CASES))
    dest = os.path.join(HERE, "ref_ddmix.npz")
    np.savez_compressed(dest, **out)
    print(os.path.getsize(dest) // 1024, "KiB")
