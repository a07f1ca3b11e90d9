"""numpy restatement of FV3's ``moist_cv`` for six water species (``fv3_moist_cv`` in include/fv3_mi355x.h), written from the formulas
of the header, in the arrays' own dtype: every sum, product and quotient is one rounded numpy operation, in the order the formulas
are written.  A species given as None is a field of zeros.  The arithmetic is only + - * /, so the device result is compared bitwise.

    qv = qvapor;  ql = qliquid + qrain;  qs = (qice + qsnow) + qgraupel
    q_con = ql + qs
    cvm   = (((1 - (qv + q_con)) * cv_air + qv * cv_vap) + ql * c_liq) + qs * c_ice
    cappa = rdgas / (rdgas + cvm / (1 + zvir * qv))
"""
import numpy as np

from pace_amd import constants as _c

ROLES = ("qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel")


def moist_cv(qvapor, qliquid=None, qrain=None, qice=None, qsnow=None, qgraupel=None, cv_vap=_c.CV_VAP, c_liq=_c.C_LIQ, c_ice=_c.C_ICE):
    """(q_con, cappa, cvm) in qvapor's dtype."""
    dt = qvapor.dtype.type
    c = _c.get_constants()
    rdgas, zvir, cv_air = dt(c.RDGAS), dt(c.RVGAS / c.RDGAS - 1.0), dt(c.CP_AIR - c.RDGAS)
    cv_vap, c_liq, c_ice = dt(cv_vap), dt(c_liq), dt(c_ice)
    z = np.zeros_like(qvapor)
    f = lambda a: z if a is None else a  # noqa: E731
    qv = qvapor
    ql = f(qliquid) + f(qrain)
    qs = (f(qice) + f(qsnow)) + f(qgraupel)
    q_con = ql + qs
    cvm = (((dt(1.0) - (qv + q_con)) * cv_air + qv * cv_vap) + ql * c_liq) + qs * c_ice
    cappa = rdgas / (rdgas + cvm / (dt(1.0) + zvir * qv))
    assert q_con.dtype == cappa.dtype == cvm.dtype == qvapor.dtype
    return q_con, cappa, cvm
