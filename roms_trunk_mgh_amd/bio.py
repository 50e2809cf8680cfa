"""BIOLOGY on the device: the host side of roms_hip_set_biology / roms_hip_biology (include/roms_hip.h).

    PowellPar          the parameters of the NPZD_POWELL model (ROMS/Nonlinear/Biology/npzd_Powell_mod.h), the defaults
                       the values of ROMS/External/npzd_Powell.in; the members are those of include/roms_bio.def
    BIO_INI            BioIni of npzd_Powell.in:54-57
    FennelPar          the switches and the parameters of the BIO_FENNEL model (ROMS/Nonlinear/Biology/fennel_mod.h),
                       the defaults the values of ROMS/External/bio_Fennel.in; the members are those of
                       include/roms_bio_fennel.def
    analytic_biology   ana_biology.h:197-212 (NPZD_FRANKS / NPZD_POWELL): uniform initial pools; ana_biology.h:112-155
                       (BIO_FENNEL)
"""
import numpy as np

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


# the values of ROMS/External/bio_Fennel.in (lines 49-207); Cp of mod_scalars.F:431; the switches = the CPP options of
# the BIO_TOY application (bio_toy.h:56-68: CARBON, DENITRIFICATION, BIO_SEDIMENT), bulk_fluxes as the application has it
FENNEL_SWITCHES = ("bio_sediment", "denitrification", "oxygen", "carbon", "bulk_fluxes")
FENNEL_DEFAULTS = dict(BioIter=1, bio_sediment=1, denitrification=1, oxygen=0, carbon=1, bulk_fluxes=0,
                       AttSW=0.04, AttChl=0.02486, PARfrac=0.43, Vp0=1.0, I_thNH4=0.0095, D_p5NH4=0.1, NitriR=0.05,
                       K_NO3=2.0, K_NH4=2.0, K_Phy=2.0, Chl2C_m=0.0535, ChlMin=0.001, PhyCN=6.625, PhyIS=0.025,
                       PhyMin=0.001, PhyMR=0.15, ZooAE_N=0.75, ZooBM=0.1, ZooCN=6.625, ZooER=0.1, ZooGR=0.6,
                       ZooMin=0.001, ZooMR=0.025, LDeRRN=0.01, LDeRRC=0.01, CoagR=0.005, SDeRRN=0.03, SDeRRC=0.03,
                       wPhy=0.1, wLDet=1.0, wSDet=0.1, pCO2air=370.0, Cp=3985.0)
# the order of idbio (fennel_mod.h:497-527 without the pools that are not built)
FENNEL_POOLS = ("iNO3_", "iNH4_", "iChlo", "iPhyt", "iZoop", "iLDeN", "iSDeN", "iLDeC", "iSDeC", "iTIC_", "iTAlk", "iOxyg")
FENNEL_MEMBERS = [n for _, n, _ in abi.STRUCTS["roms_bio_fennel_t"]]
assert sorted(FENNEL_MEMBERS) == sorted(list(FENNEL_DEFAULTS) + ["idbio"])


class FennelPar:
    """The BIO_FENNEL switches and parameters (the library refuses the model by name until its kernel is built); every
    member of roms_bio_fennel.def is an attribute.  idbio = None: the
    active pools behind the active tracers, NAT+1 .., in the order fennel_mod.h:497-527 numbers them; otherwise twelve
    entries in the order of FENNEL_POOLS, 0 for a pool that is switched off."""

    model = "FENNEL"

    def __init__(self, idbio=None, **kw):
        unknown = set(kw) - set(FENNEL_DEFAULTS)
        if unknown:
            raise TypeError(f"FennelPar: unknown parameter(s) {sorted(unknown)}")
        self.idbio = None if idbio is None else tuple(int(x) for x in idbio)
        if self.idbio is not None and len(self.idbio) != 12:
            raise ValueError(f"FennelPar: idbio has twelve entries {FENNEL_POOLS}, 0 for a pool that is off")
        for name, value in FENNEL_DEFAULTS.items():
            setattr(self, name, type(value)(kw.get(name, value)))

    def replace(self, **kw):
        """a copy with some members changed"""
        cur = {n: getattr(self, n) for n in FENNEL_DEFAULTS}
        idbio = kw.pop("idbio", self.idbio)
        cur.update(kw)
        return FennelPar(idbio=idbio, **cur)

    def active(self):
        """which of the twelve pools are switched on"""
        return tuple(q <= 6 or (bool(self.carbon) and 7 <= q <= 10) or (bool(self.oxygen) and q == 11) for q in range(12))

    def tracers(self, b):
        """idbio for a tile with bounds b (1-based), twelve entries, 0 for a pool that is off"""
        if self.idbio is not None:
            return self.idbio
        out, nxt = [], b.NAT + 1
        for on in self.active():
            out.append(nxt if on else 0)
            nxt += bool(on)
        return tuple(out)

    def c_struct(self, b):
        """the roms_bio_fennel_t block for a tile with bounds b"""
        blk = abi.BioFennel()
        for name in FENNEL_DEFAULTS:
            setattr(blk, name, getattr(self, name))
        for q, it in enumerate(self.tracers(b)):
            blk.idbio[q] = it
        return blk


def _analytic_fennel(st, par):
    """ana_biology.h:112-155: NO3 from the temperature, the other pools uniform"""
    idbio = par.tracers(st.b)
    if max(idbio) > st.b.NT:
        raise ValueError(f"analytic_biology: the tile has NT = {st.b.NT} tracers, idbio = {idbio}")
    t = st["t"]
    temp = t[:, :, :, 0, 0]
    cff1, cff2 = 20.0 / 3.0, 2.0 / 3.0
    SiO4 = np.where(temp < 8.0, 30.0,
                    np.where(temp <= 11.0, 30.0 - ((temp - 8.0) * cff1),
                             np.where(temp <= 13.0, 10.0 - ((temp - 11.0) * 4.0),
                                      np.where(temp <= 16.0, 2.0 - ((temp - 13.0) * cff2), 0.0))))
    value = dict(iNO3_=1.67 + 0.5873 * SiO4 + 0.0144 * SiO4 ** 2 + 0.0003099 * SiO4 ** 3, iPhyt=0.08, iZoop=0.06, iNH4_=0.1,
                 iLDeN=0.02, iSDeN=0.04, iChlo=0.02, iTIC_=2100.0, iTAlk=2350.0, iLDeC=0.002, iSDeC=0.06,
                 iOxyg=10.0 / 0.02241)
    for name, it in zip(FENNEL_POOLS, idbio):
        if it:
            t[:, :, :, 0, it - 1] = value[name]
    return st


def analytic_biology(st, BioIni=BIO_INI, par=None):
    """ana_biology.h:197-212: t(:,:,:,1,idbio) = BioIni on every point of the tile (IstrT:IendT, JstrT:JendT); with a
    FennelPar ana_biology.h:112-155 (BioIni is not read)."""
    if isinstance(par, FennelPar):
        return _analytic_fennel(st, par)
    idbio = (par or PowellPar()).tracers(st.b)
    if max(idbio) > st.b.NT:
        raise ValueError(f"analytic_biology: the tile has NT = {st.b.NT} tracers, idbio = {idbio}")
    for it, value in zip(idbio, BioIni):
        st["t"][:, :, :, 0, it - 1] = float(value)
    return st
