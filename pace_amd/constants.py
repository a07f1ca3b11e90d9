"""Physical constants used on the acoustic path.

The reference selects a constant set with ``PACE_CONSTANTS`` (GFDL | GFS | GEOS)
[REF README.md:88-93]; the values themselves live in the un-vendored NDSL
submodule (``ndsl/constants.py``), so the numbers below are restated from the
public FV3 / NDSL sources.  Every kernel takes them as run-time parameters
(see ``include/fv3_mi355x.h: fv3_constants``) so a different set is a data change.
"""
import math
import os
from dataclasses import dataclass

N_HALO_DEFAULT = 3  # [REF driver/pace/driver/driver.py:21,177]

X_DIM = "x"
X_INTERFACE_DIM = "x_interface"
Y_DIM = "y"
Y_INTERFACE_DIM = "y_interface"
Z_DIM = "z"
Z_INTERFACE_DIM = "z_interface"


@dataclass(frozen=True)
class ConstantSet:
    name: str
    RADIUS: float
    OMEGA: float
    GRAV: float
    RDGAS: float
    RVGAS: float
    CP_AIR: float
    DZ_MIN: float
    PI: float = math.pi
    SECONDS_PER_DAY: float = 86400.0
    CNST_0P20: float = 0.20

    @property
    def RGRAV(self):
        return 1.0 / self.GRAV

    @property
    def KAPPA(self):
        return self.RDGAS / self.CP_AIR

    @property
    def CV_AIR(self):
        return self.CP_AIR - self.RDGAS

    @property
    def RDG(self):
        return -self.RDGAS / self.GRAV

    @property
    def ZVIR(self):
        return self.RVGAS / self.RDGAS - 1.0


GFS = ConstantSet(
    name="GFS",
    RADIUS=6.3712e6,
    OMEGA=7.2921e-5,
    GRAV=9.80665,
    RDGAS=287.05,
    RVGAS=461.50,
    CP_AIR=1004.6,
    DZ_MIN=2.0,
)
GFDL = ConstantSet(
    name="GFDL",
    RADIUS=6371.0e3,
    OMEGA=7.292e-5,
    GRAV=9.80,
    RDGAS=287.04,
    RVGAS=461.50,
    CP_AIR=287.04 / (2.0 / 7.0),
    DZ_MIN=2.0,
)
GEOS = ConstantSet(
    name="GEOS",
    RADIUS=6.371e6,
    OMEGA=2.0 * math.pi / 86164.0,
    GRAV=9.80665,
    RDGAS=8314.47 / 28.965,
    RVGAS=8314.47 / 18.015,
    CP_AIR=(8314.47 / 28.965) / (2.0 / 7.0),
    DZ_MIN=6.0,
)

# Heat capacities of the water species in moist_cv (J/kg/K), restated from FV3's fv_mapz.F90: cv_vap = 3 rvgas, c_liq, c_ice.  They are
# run-time data of the moist entries (``fv3_water`` in include/fv3_mi355x.h), not part of ``fv3_constants``.  Newer FV3 branches carry
# c_liq = 4218, c_ice = 2106 ("Uncertain restatements").
CV_VAP = 3.0 * 461.50
C_LIQ = 4185.5
C_ICE = 1972.0
# Latent heats of vaporisation and fusion (J/kg) and the freezing point (K) of neg_adj3 (fv_sg.F90), run-time data of ``fv3_neg_adj3``
# (``fv3_latent`` in include/fv3_mi355x.h).  Restated from memory like the heat capacities ("Uncertain restatements").
HLV = 2.5e6
HLF = 3.3358e5
T_ICE = 273.16
# Namelist defaults of the saturation adjustment (FV3 fv_cmp.F90 / gfdl_cloud_microphys.F90; ``fv3_sat_params`` in include/fv3_mi355x.h):
# the time scales tau_* in seconds, the thresholds in kg/kg, t_sub in K.  Restated from memory ("Uncertain restatements").
SAT_ADJ_DEFAULTS = dict(
    tau_i2s=1000.0, tau_v2l=150.0, tau_l2v=300.0, tau_imlt=600.0, tau_r2g=900.0, tau_smlt=900.0, tau_l2r=900.0,
    ql_gen=1.0e-3, qi_gen=1.82e-6, qi_lim=1.0, ql_mlt=2.0e-3, qs_mlt=1.0e-6, ql0_max=2.0e-3, qi0_max=1.0e-4, sat_adj0=0.9, t_sub=184.0,
)

_SETS = {"GFS": GFS, "GFDL": GFDL, "GEOS": GEOS}


def get_constants(name: str | None = None) -> ConstantSet:
    """Constant set named by ``PACE_CONSTANTS`` (default GFS)."""
    if name is None:
        name = os.environ.get("PACE_CONSTANTS", "GFS")
    try:
        return _SETS[name.upper()]
    except KeyError:
        raise ValueError(f"unknown PACE_CONSTANTS set {name!r}; expected one of {sorted(_SETS)}")


def float_precision_bits() -> int:
    """``PACE_FLOAT_PRECISION`` (32 | 64, default 64) [REF README.md:94]."""
    bits = int(os.environ.get("PACE_FLOAT_PRECISION", "64"))
    if bits not in (32, 64):
        raise ValueError("PACE_FLOAT_PRECISION must be 32 or 64")
    return bits
