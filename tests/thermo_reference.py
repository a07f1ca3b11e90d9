"""numpy restatement of the thermodynamic bookends (fv3_pt_from_temperature / fv3_temperature_from_pt in include/fv3_mi355x.h),
written from the formulas of the header, in the arrays' own dtype: every product and quotient is one rounded numpy operation, in
the order the formulas are written (left to right).  exp / log are numpy's: a different implementation from the device's, each
within a few ulp (tests/test_device_math.py)."""
import numpy as np

from pace_amd.constants import get_constants


def constants(dtype):
    c = get_constants()
    return dtype(-c.RDGAS / c.GRAV), dtype(c.RVGAS / c.RDGAS - 1.0)


def fac(q_con, qvapor):
    dt = q_con.dtype.type
    _, zvir = constants(dt)
    zq = zvir * qvapor if qvapor is not None else dt(0.0)
    return (dt(1.0) + zq) * (dt(1.0) - q_con)


def pt_from_temperature(pt, delp, delz, q_con, cappa, qvapor=None):
    """T -> (pt, pkz) of the loop's form."""
    rrg, _ = constants(pt.dtype.type)
    tv = pt * fac(q_con, qvapor)
    pz = np.exp(cappa * np.log(rrg * delp / delz * tv))
    return tv / pz, pz


def temperature_from_pt(pt, pkz, delp, delz, q_con, cappa, w, qvapor=None, recompute_pkz=False):
    """the loop's form -> (T, pkz, omga); pkz is returned as given unless recompute_pkz."""
    dt = pt.dtype.type
    rrg, _ = constants(dt)
    if recompute_pkz:
        r = rrg * delp / delz
        tv = pt * np.exp(cappa / (dt(1.0) - cappa) * np.log(r * pt))
        pkz = np.exp(cappa * np.log(r * tv))
    else:
        tv = pt * pkz
    return tv / fac(q_con, qvapor), pkz, delp / delz * w
