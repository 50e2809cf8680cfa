"""Lagrangian floats (FLOATS) on the host side: the index constants of mod_floats.F:80-90, the five time-level indices
of mod_stepping.F with their initial values (initial.F:146-149) and rotation (main3d.F:899-903), and the container
handed to roms_hip_set_floats (RomsHip.set_floats, Main3D(floats=...))."""
import ctypes as C

import numpy as np

# rows of track(NFV,0:NFT,Nfloats) and of Tinfo(0:izrhs,Nfloats), mod_floats.F:80-90
itstr, ixgrd, iygrd, izgrd, iflon, iflat, idpth, ixrhs, iyrhs, izrhs, ifden = range(11)
NFT = 4                                    # time levels 0:NFT
flt_Lagran, flt_Isobar, flt_Geopot = 1, 2, 3          # mod_floats.F:125-127
INITIAL_LEVELS = dict(nfp1=1, nf=0, nfm1=4, nfm2=3, nfm3=2)
SPVAL = 1.0e37


def NFV(NT):
    """number of float variables without FLOAT_VWALK / FLOAT_BIOLOGY: ifTvar(itrc) = 10 + itrc"""
    return NT + 10


def ifTvar(itrc):
    return 10 + itrc


class Floats:
    """DRIFTER(ng) as the library takes it.  Ftype(Nfloats); Tinfo(0:izrhs, Nfloats); Fz0(Nfloats); xcoord, ycoord:
    lonr, latr (spherical) or xr, yr with the tile's extents."""

    def __init__(self, bounds, Ftype, Tinfo, Fz0, xcoord, ycoord):
        self.b = bounds
        self.Ftype = np.ascontiguousarray(Ftype, dtype=np.int32)
        self.n = int(self.Ftype.size)
        self.Tinfo = np.asfortranarray(Tinfo, dtype=np.float64)
        self.Fz0 = np.ascontiguousarray(Fz0, dtype=np.float64)
        shape = (bounds.UBi - bounds.LBi + 1, bounds.UBj - bounds.LBj + 1)
        self.xcoord = np.asfortranarray(xcoord, dtype=np.float64)
        self.ycoord = np.asfortranarray(ycoord, dtype=np.float64)
        if self.Tinfo.shape != (izrhs + 1, self.n) or self.Fz0.shape != (self.n,):
            raise ValueError("floats: Tinfo is (0:izrhs, Nfloats) and Fz0 (Nfloats)")
        if self.xcoord.shape != shape or self.ycoord.shape != shape:
            raise ValueError("floats: the coordinate arrays have the tile's extents (LBi:UBi, LBj:UBj)")
        self.NFV = NFV(bounds.NT)
        self.levels = dict(INITIAL_LEVELS)

    def nfl(self):
        """{nfm3, nfm2, nfm1, nf, nfp1} as roms_hip_step_floats takes them"""
        L = self.levels
        return (L["nfm3"], L["nfm2"], L["nfm1"], L["nf"], L["nfp1"])

    def rotate(self):
        """main3d.F:899-903"""
        for k in self.levels:
            self.levels[k] = (self.levels[k] + 1) % (NFT + 1)

    def track_shape(self):
        return (self.NFV, NFT + 1, self.n)

    def c_args(self):
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        return (self.n, self.Ftype.ctypes.data_as(ip), self.Tinfo.ctypes.data_as(dp), self.Fz0.ctypes.data_as(dp),
                self.xcoord.ctypes.data_as(dp), self.ycoord.ctypes.data_as(dp))
