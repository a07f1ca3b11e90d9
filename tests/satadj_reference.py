"""numpy restatement of the saturation adjustment (fv3_sat_adj in include/fv3_mi355x.h; FV3 fv_cmp.F90, fv_sat_adj): cell-vectorised and
dtype-generic, one rounded operation per numpy call in the order the specification writes them, the saturation tables an argument (the test
hands over the entries the kernel holds, so both interpolate the very same numbers).  Every conditional of the 17 steps is evaluated for
all cells and applied through masks.  Beside the result it returns, per cell, the bitmask of the branches taken (BRANCHES) and the smallest
relative margin of any comparison that decides a branch: |pt1 - threshold| / tice for temperatures, |dq0| / wqsat and |dq| / qsi for the
saturation deficits, |a - b| / max(|a|, |b|) for mixing ratios against thresholds (a comparison of an exact zero with zero cannot flip under
rounding and counts as infinitely safe).  `exp` / `log` can be replaced (the tolerance measurement nudges their results by an ulp)."""
import numpy as np

from pace_amd import constants as pc

NTAB = 2621
# name -> bit.  "x" is a branch taken; the other arm of a conditional is "the bit is clear" (ARMS below lists what coverage asks for)
BRANCHES = ("s2", "s3", "s4_qs", "s4_qg", "s5_ql", "s5_qr", "s6", "s7_cond", "s7_evap", "s8_cond", "s8_evap", "s9", "s10", "s11", "s12", "s13", "s14_tsub", "s14_range",
            "s14_pidep", "s14_dep", "s14_subl", "s16", "s17")
BIT = {n: 1 << i for i, n in enumerate(BRANCHES)}


def arms(mask, last_step):
    """{arm: number of cells} for every arm of every conditional of the 17 steps (steps 1 and 15 have none); step 8 exists only with last_step."""
    has = lambda n: (mask & BIT[n]) != 0  # noqa: E731
    out = {}
    for n in ("s2", "s3", "s6", "s9", "s10", "s11", "s12", "s13", "s16", "s17"):
        out[n] = int(has(n).sum())
        out["not " + n] = int((~has(n)).sum())
    for a, b in (("s4_qs", "s4_qg"), ("s5_ql", "s5_qr")):
        out[a], out[b], out[f"neither {a} nor {b}"] = int(has(a).sum()), int(has(b).sum()), int((~has(a) & ~has(b)).sum())
    out["s7_cond"], out["s7_evap"] = int(has("s7_cond").sum()), int(has("s7_evap").sum())
    if last_step:
        out["s8_cond"], out["s8_evap"] = int(has("s8_cond").sum()), int(has("s8_evap").sum())
    out["s14_tsub"], out["s14_range"] = int(has("s14_tsub").sum()), int(has("s14_range").sum())
    out["s14_warm"] = int((~has("s14_tsub") & ~has("s14_range")).sum())
    out["s14_dep"], out["s14_subl"] = int(has("s14_dep").sum()), int(has("s14_subl").sum())
    out["s14_pidep"], out["s14_no_pidep"] = int(has("s14_pidep").sum()), int((has("s14_range") & ~has("s14_pidep")).sum())
    return out


def constants(npd, mdt, params=None, cst=None, cv_vap=pc.CV_VAP, c_liq=pc.C_LIQ, c_ice=pc.C_ICE, hlv=pc.HLV, hlf=pc.HLF, t_ice=pc.T_ICE):
    """The constants of a call, formed in double and cast once."""
    p = dict(pc.SAT_ADJ_DEFAULTS)
    p.update(params or {})
    cst = cst or pc.get_constants()
    sdt = 0.5 * mdt
    d0_vap, dc_ice = cv_vap - c_liq, c_liq - c_ice
    k = dict(cv_air=cst.CP_AIR - cst.RDGAS, cv_vap=cv_vap, c_liq=c_liq, c_ice=c_ice, d0_vap=d0_vap, lv00=hlv - d0_vap * t_ice, dc_ice=dc_ice, li00=hlf - dc_ice * t_ice,
             zvir=cst.RVGAS / cst.RDGAS - 1.0, rvgas=cst.RVGAS, grav=cst.GRAV, rdgas=cst.RDGAS, rrg=-cst.RDGAS / cst.GRAV, tice=t_ice, tice0=t_ice - 0.01, t_wfr=t_ice - 40.0,
             lat2=(hlv + hlf) ** 2, sdt=sdt, dt_bigg=mdt)
    for n in ("i2s", "r2g", "l2r", "smlt"):
        k["fac_" + n] = 1.0 - np.exp(-mdt / p["tau_" + n])
    for n in ("v2l", "imlt"):
        k["fac_" + n] = 1.0 - np.exp(-sdt / p["tau_" + n])
    k["fac_l2v"] = min(p["sat_adj0"], 1.0 - np.exp(-sdt / p["tau_l2v"]))
    for n in ("ql_gen", "qi_gen", "qi_lim", "ql_mlt", "qs_mlt", "ql0_max", "qi0_max", "sat_adj0", "t_sub"):
        k[n] = p[n]
    return {n: npd(v) for n, v in k.items()}


def closed_form_tables(cst=None, cv_vap=pc.CV_VAP, c_liq=pc.C_LIQ, c_ice=pc.C_ICE, hlv=pc.HLV, hlf=pc.HLF, t_ice=pc.T_ICE):
    """(tablew, table2) of FV3's qs_init in numpy double, table2 before its two entries are smoothed."""
    cst = cst or pc.get_constants()
    rvgas = cst.RVGAS
    t = (t_ice - 160.0) + 0.1 * np.arange(NTAB)
    dc_vap = (cv_vap + rvgas) - c_liq
    lv0 = hlv - dc_vap * t_ice
    dc_ice = c_liq - c_ice
    li00 = hlf - dc_ice * t_ice
    form = lambda d, l: 611.21 * np.exp((d * np.log(t / t_ice) + l * (t - t_ice) / (t * t_ice)) / rvgas)  # noqa: E731
    tw = form(dc_vap, lv0)
    t2 = np.where(np.arange(NTAB) < 1600, form(dc_vap + dc_ice, lv0 + li00), tw)
    return tw, t2


def _mn(a, b):
    return np.where(a < b, a, b)


def _mx(a, b):
    return np.where(a > b, a, b)


def qs2(tab, des, t, den, k):
    """wqs2 / iqs2: (saturation mixing ratio, its derivative in t)"""
    npd = t.dtype.type
    ap1 = _mn(npd(NTAB), npd(10) * _mx(t - (k["tice"] - npd(160)), npd(0)) + npd(1))
    it = np.maximum(ap1.astype(np.int64), 1)
    es = tab[it - 1] + (ap1 - it.astype(npd)) * des[it - 1]
    rtd = k["rvgas"] * t * den
    q = es / rtd
    it = np.clip((ap1 - npd(0.5)).astype(np.int64), 1, NTAB - 1)
    d0, d1 = des[it - 1], des[it]
    return q, npd(10) * (d0 + (ap1 - it.astype(npd)) * (d1 - d0)) / rtd


def sat_adj(tv, qv, ql, qr, qi, qs, qg, dp, delz, tables, k, last_step, exp=np.exp, log=np.log):
    """Arrays of one shape and dtype; tables: (4, NTAB) of that dtype; k: constants().  Returns ({tv, qv .. qg, q_con, cappa, pkz, pt1}, mask, margin)."""
    npd = tv.dtype.type
    assert all(a.dtype == tv.dtype for a in (qv, ql, qr, qi, qs, qg, dp, delz, tables)) and all(type(v) is npd for v in k.values())
    tv, qv, ql, qr, qi, qs, qg = (a.copy() for a in (tv, qv, ql, qr, qi, qs, qg))
    zero, one = npd(0), npd(1)
    mask = np.zeros(tv.shape, dtype=np.int64)
    margin = np.full(tv.shape, np.inf)
    every = np.ones(tv.shape, dtype=bool)

    def note(active, m):
        margin[...] = np.where(active, np.minimum(margin, m), margin)

    def rel(a, b):  # mixing ratios: |a - b| / max(|a|, |b|), an exact tie of zeros is safe
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
        s = np.maximum(np.abs(a), np.abs(b))
        return np.where(s == 0, np.inf, np.abs(a - b) / np.where(s == 0, 1.0, s))

    def temp(a, b):
        return np.abs(np.asarray(a, dtype=np.float64) - np.float64(b)) / np.float64(k["tice"])

    def take(name, cond):
        mask[...] |= np.where(cond, BIT[name], 0)

    with np.errstate(all="ignore"):
        # ---- 1
        q_liq = ql + qr
        q_sol = (qi + qs) + qg
        qpz = q_liq + q_sol
        pt1 = tv / ((one + k["zvir"] * qv) * (one - qpz))
        qpz = qpz + qv
        den = dp / (-k["grav"] * delz)
        mc_air = (one - qpz) * k["cv_air"]
        st = dict(cvm=None, lhl=None, lhi=None, lcp2=None, icp2=None)

        def cvm_now():
            return ((mc_air + qv * k["cv_vap"]) + q_liq * k["c_liq"]) + q_sol * k["c_ice"]

        def lat(cond):
            lhl = k["lv00"] + k["d0_vap"] * pt1
            lhi = k["li00"] + k["dc_ice"] * pt1
            for n, v in (("lhl", lhl), ("lhi", lhi), ("lcp2", lhl / st["cvm"]), ("icp2", lhi / st["cvm"])):
                st[n] = v if st[n] is None else np.where(cond, v, st[n])

        def heat(cond, s, L):
            nonlocal pt1
            st["cvm"] = np.where(cond, cvm_now(), st["cvm"])
            pt1 = np.where(cond, pt1 + s * L / st["cvm"], pt1)

        st["cvm"] = cvm_now()
        lat(every)
        # ---- 2
        c = qi < zero
        note(every, rel(qi, zero))
        take("s2", c)
        qs = np.where(c, qs + qi, qs)
        qi = np.where(c, zero, qi)
        # ---- 3
        c1 = qi > npd(1.0e-8)
        note(every, rel(qi, npd(1.0e-8)))
        note(c1, temp(pt1, k["tice"]))
        c = c1 & (pt1 > k["tice"])
        take("s3", c)
        sink = _mn(qi, k["fac_imlt"] * (pt1 - k["tice"]) / st["icp2"])
        tmp = _mn(sink, _mx(k["ql_mlt"] - ql, zero))
        qi = np.where(c, qi - sink, qi)
        ql, qr = np.where(c, ql + tmp, ql), np.where(c, qr + (sink - tmp), qr)
        q_liq, q_sol = np.where(c, q_liq + sink, q_liq), np.where(c, q_sol - sink, q_sol)
        heat(c, -sink, st["lhi"])
        lat(c)
        # ---- 4
        ca = qs < zero
        note(every, rel(qs, zero))
        cb = ~ca & (qg < zero)
        note(~ca, rel(qg, zero))
        take("s4_qs", ca)
        take("s4_qg", cb)
        tmp = _mn(-qg, _mx(zero, qs))
        qg, qs = np.where(ca, qg + qs, np.where(cb, qg + tmp, qg)), np.where(ca, zero, np.where(cb, qs - tmp, qs))
        # ---- 5
        ca = ql < zero
        note(every, rel(ql, zero))
        cb = ~ca & (qr < zero)
        note(~ca, rel(qr, zero))
        take("s5_ql", ca)
        take("s5_qr", cb)
        ta, tb = _mn(-ql, _mx(zero, qr)), _mn(-qr, _mx(zero, ql))
        ql, qr = np.where(ca, ql + ta, np.where(cb, ql - tb, ql)), np.where(ca, qr - ta, np.where(cb, qr + tb, qr))

        def freeze(name, dtmp, threshold):
            nonlocal ql, qi, q_liq, q_sol
            c1 = ql > zero
            note(every, rel(ql, zero))
            note(c1, temp(pt1, threshold))
            c = c1 & (dtmp > zero)
            take(name, c)
            sink = _mn(_mn(ql, ql * dtmp * npd(0.125)), dtmp / st["icp2"])
            ql, qi = np.where(c, ql - sink, ql), np.where(c, qi + sink, qi)
            q_liq, q_sol = np.where(c, q_liq - sink, q_liq), np.where(c, q_sol + sink, q_sol)
            heat(c, sink, st["lhi"])
            lat(c)

        # ---- 6
        t48 = k["tice"] - npd(48)
        freeze("s6", t48 - pt1, t48)
        # ---- 7 / 8
        for step in ((7, 8) if last_step else (7,)):
            wqsat, dq2dt = qs2(tables[0], tables[2], pt1, den, k)
            dq0 = (qv - wqsat) / (one + st["lcp2"] * dq2dt)
            c = dq0 > zero
            note(every, np.abs(dq0.astype(np.float64)) / wqsat.astype(np.float64))
            take(f"s{step}_cond", c)
            take(f"s{step}_evap", ~c)
            cond = dq0 if step == 8 else _mn(k["sat_adj0"] * dq0, _mx(k["ql_gen"] - ql, k["fac_v2l"] * dq0))
            factor = -_mn(one, k["fac_l2v"] * npd(10) * (one - qv / wqsat))
            src = np.where(c, cond, -_mn(ql, factor * dq0))
            qv, ql, q_liq = qv - src, ql + src, q_liq + src
            heat(every, src, st["lhl"])
            lat(every)
        # ---- 9
        freeze("s9", k["t_wfr"] - pt1, k["t_wfr"])
        # ---- 10
        tc = k["tice0"] - pt1
        c1 = ql > zero
        note(every, rel(ql, zero))
        note(c1, temp(pt1, k["tice0"]))
        c = c1 & (tc > zero)
        take("s10", c)
        sink = npd(3.3333e-10) * k["dt_bigg"] * (exp(npd(0.66) * tc) - one) * den * ql * ql
        sink = _mn(_mn(ql, tc / st["icp2"]), sink)
        ql, qi = np.where(c, ql - sink, ql), np.where(c, qi + sink, qi)
        q_liq, q_sol = np.where(c, q_liq - sink, q_liq), np.where(c, q_sol + sink, q_sol)
        heat(c, sink, st["lhi"])
        lat(c)
        # ---- 11
        t11 = k["tice"] - npd(0.1)
        dtmp = t11 - pt1
        c1 = qr > npd(1.0e-7)
        note(every, rel(qr, npd(1.0e-7)))
        note(c1, temp(pt1, t11))
        c = c1 & (dtmp > zero)
        take("s11", c)
        x = dtmp * npd(0.025)
        tmp = _mn(one, x * x) * qr
        sink = _mn(tmp, k["fac_r2g"] * dtmp / st["icp2"])
        qr, qg = np.where(c, qr - sink, qr), np.where(c, qg + sink, qg)
        q_liq, q_sol = np.where(c, q_liq - sink, q_liq), np.where(c, q_sol + sink, q_sol)
        heat(c, sink, st["lhi"])
        lat(c)
        # ---- 12
        t12 = k["tice"] + npd(0.1)
        dtmp = pt1 - t12
        c1 = qs > npd(1.0e-7)
        note(every, rel(qs, npd(1.0e-7)))
        note(c1, temp(pt1, t12))
        c = c1 & (dtmp > zero)
        take("s12", c)
        x = dtmp * npd(0.1)
        tmp = _mn(one, x * x) * qs
        sink = _mn(tmp, k["fac_smlt"] * dtmp / st["icp2"])
        tmp = _mn(sink, _mx(k["qs_mlt"] - ql, zero))
        qs = np.where(c, qs - sink, qs)
        ql, qr = np.where(c, ql + tmp, ql), np.where(c, qr + (sink - tmp), qr)
        q_liq, q_sol = np.where(c, q_liq + sink, q_liq), np.where(c, q_sol - sink, q_sol)
        heat(c, -sink, st["lhi"])
        # ---- 13
        c = ql > k["ql0_max"]
        note(every, rel(ql, k["ql0_max"]))
        take("s13", c)
        sink = k["fac_l2r"] * (ql - k["ql0_max"])
        qr, ql = np.where(c, qr + sink, qr), np.where(c, ql - sink, ql)
        lat(every)
        tcp2 = st["lcp2"] + st["icp2"]
        # ---- 14
        ca = pt1 < k["t_sub"]
        note(every, temp(pt1, k["t_sub"]))
        cb = ~ca & (pt1 < k["tice0"])
        note(~ca, temp(pt1, k["tice0"]))
        take("s14_tsub", ca)
        take("s14_range", cb)
        qsi, dqsdt = qs2(tables[1], tables[3], pt1, den, k)
        dq = qv - qsi
        sink = k["sat_adj0"] * dq / (one + tcp2 * dqsdt)
        cp = qi > npd(1.0e-8)
        note(cb, rel(qi, npd(1.0e-8)))
        take("s14_pidep", cb & cp)
        pidep = k["sdt"] * dq * npd(349138.78) * exp(npd(0.875) * log(qi * den)) / (qsi * den * k["lat2"] / (npd(0.0243) * k["rvgas"] * pt1 * pt1) + npd(4.42478e4))
        pidep = np.where(cp, pidep, zero)
        cd = dq > zero
        note(cb, np.abs(dq.astype(np.float64)) / qsi.astype(np.float64))
        take("s14_dep", cb & cd)
        take("s14_subl", cb & ~cd)
        tmp = k["tice"] - pt1
        qi_crt = k["qi_gen"] * _mn(k["qi_lim"], npd(0.1) * tmp) / den
        dep = _mn(_mn(sink, _mx(qi_crt - qi, pidep)), tmp / tcp2)
        pidep2 = pidep * _mn(one, _mx(pt1 - k["t_sub"], zero) * npd(0.2))
        sub = _mx(_mx(pidep2, sink), -qi)
        src = np.where(ca, _mx(qv - npd(1.0e-6), zero), np.where(cb, np.where(cd, dep, sub), zero))
        qv, qi, q_sol = qv - src, qi + src, q_sol + src
        heat(every, src, st["lhl"] + st["lhi"])
        # ---- 15
        q_con = q_liq + q_sol
        tv = pt1 * (one + k["zvir"] * qv) * (one - q_con)
        # ---- 16
        c = qg < zero
        note(every, rel(qg, zero))
        take("s16", c)
        tmp = _mn(-qg, _mx(zero, qi))
        qg, qi = np.where(c, qg + tmp, qg), np.where(c, qi - tmp, qi)
        # ---- 17
        qim = k["qi0_max"] / den
        c = qi > qim
        note(every, rel(qi, qim))
        take("s17", c)
        sink = k["fac_i2s"] * (qi - qim)
        qi, qs = np.where(c, qi - sink, qi), np.where(c, qs + sink, qs)
        # ---- what the entry stores beside the species and tv: moist_cv of the final species, pkz with that cappa
        m_liq = ql + qr
        m_sol = (qi + qs) + qg
        m_con = m_liq + m_sol
        cvm = (((one - (qv + m_con)) * k["cv_air"] + qv * k["cv_vap"]) + m_liq * k["c_liq"]) + m_sol * k["c_ice"]
        cappa = k["rdgas"] / (k["rdgas"] + cvm / (one + k["zvir"] * qv))
        pkz = exp(cappa * log(k["rrg"] * dp / delz * tv))
    out = dict(tv=tv, qv=qv, ql=ql, qr=qr, qi=qi, qs=qs, qg=qg, q_con=m_con, cappa=cappa, pkz=pkz, pt1=pt1, cvm_last=st["cvm"], q_sol=q_sol, q_liq=q_liq)
    assert all(v.dtype == tv.dtype for v in out.values()), {n: v.dtype for n, v in out.items()}
    return out, mask, margin
