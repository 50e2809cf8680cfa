"""BIOLOGY on the device: the host side of roms_hip_set_biology / roms_hip_biology (include/roms_hip.h).

    PowellPar          the parameters of the NPZD_POWELL model (ROMS/Nonlinear/Biology/npzd_Powell_mod.h), the defaults
                       the values of ROMS/External/npzd_Powell.in; the members are those of include/roms_bio.def
    BIO_INI            BioIni of npzd_Powell.in:54-57
    analytic_biology   ana_biology.h:197-212 (NPZD_FRANKS / NPZD_POWELL): uniform initial pools
"""
from . import abi

# the values of ROMS/External/npzd_Powell.in (lines 49-131); Cp of mod_scalars.F:431; const_par = the CPP option CONST_PAR
DEFAULTS = dict(BioIter=1, const_par=0, AttSW=0.067, AttPhy=0.0095, PhyIS=0.025, Vm_NO3=1.5, PhyMRD=0.1, PhyMRN=0.0,
                K_NO3=1.0, Ivlev=0.84, ZooGR=0.52, ZooEED=0.0, ZooEEN=0.3, ZooMRD=0.145, ZooMRN=0.0, DetRR=1.03,
                wPhy=0.0, wDet=8.0, PARfrac=0.43, Cp=3985.0)
POOLS = ("iNO3_", "iPhyt", "iZoop", "iSDet")          # the order of idbio (npzd_Powell_mod.h:259-274)
BIO_INI = (17.0, 1.0, 1.0, 1.0)                       # BioIni(iNO3_ .. iSDet), npzd_Powell.in:54-57
MEMBERS = [n for _, n, _ in abi.STRUCTS["roms_bio_powell_t"]]
assert sorted(MEMBERS) == sorted(list(DEFAULTS) + ["idbio"])


class PowellPar:
    """The NPZD_POWELL parameters; every member of roms_bio.def is an attribute.  idbio = None: the four tracers
    behind the active ones, NAT+1 .. NAT+4, as npzd_Powell_mod.h:259-274 numbers them."""

    model = "NPZD_POWELL"

    def __init__(self, idbio=None, **kw):
        unknown = set(kw) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"PowellPar: unknown parameter(s) {sorted(unknown)}")
        self.idbio = None if idbio is None else tuple(int(x) for x in idbio)
        if self.idbio is not None and len(self.idbio) != 4:
            raise ValueError("PowellPar: idbio names four tracers (iNO3_, iPhyt, iZoop, iSDet)")
        for name, value in DEFAULTS.items():
            setattr(self, name, type(value)(kw.get(name, value)))

    def replace(self, **kw):
        """a copy with some members changed"""
        cur = {n: getattr(self, n) for n in DEFAULTS}
        idbio = kw.pop("idbio", self.idbio)
        cur.update(kw)
        return PowellPar(idbio=idbio, **cur)

    def tracers(self, b):
        """idbio for a tile with bounds b (1-based)"""
        return self.idbio if self.idbio is not None else tuple(b.NAT + 1 + q for q in range(4))

    def c_struct(self, b):
        """the roms_bio_powell_t block for a tile with bounds b"""
        blk = abi.BioPowell()
        for name in DEFAULTS:
            setattr(blk, name, getattr(self, name))
        for q, it in enumerate(self.tracers(b)):
            blk.idbio[q] = it
        return blk


def analytic_biology(st, BioIni=BIO_INI, par=None):
    """ana_biology.h:197-212: t(:,:,:,1,idbio) = BioIni on every point of the tile (IstrT:IendT, JstrT:JendT)."""
    idbio = (par or PowellPar()).tracers(st.b)
    if max(idbio) > st.b.NT:
        raise ValueError(f"analytic_biology: the tile has NT = {st.b.NT} tracers, idbio = {idbio}")
    for it, value in zip(idbio, BioIni):
        st["t"][:, :, :, 0, it - 1] = float(value)
    return st
