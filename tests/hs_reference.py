"""numpy restatement of the Held-Suarez (1994) forcing, from the paper (Held & Suarez, Bull. Amer. Meteor. Soc. 75, 1825-1830, section 2),
with the tendencies in the implicit form the kernel uses (-k / (1 + dt k); dt = 0 is the paper's explicit form).  Arrays are the compute
cells only: ua, va, T, delp [nx, ny, nz], lat [nx, ny]; float64 throughout.  The operation order follows the kernel's where it matters for
rounding (the downward pressure scan), so that a parity test sees the device log / exp / sin / cos and little else."""
import numpy as np

SECONDS_PER_DAY = 86400.0
DEFAULTS = dict(sigma_b=0.7, k_f=1.0 / SECONDS_PER_DAY, k_a=1.0 / (40.0 * SECONDS_PER_DAY), k_s=1.0 / (4.0 * SECONDS_PER_DAY), delta_t_y=60.0, delta_theta_z=10.0,
                p0=1.0e5, kappa=2.0 / 7.0, t_min=200.0)


def pressures(delp, ptop):
    """(p, ps): layer pressures 0.5 (pe_k + pe_k+1) of the downward scan pe_0 = ptop, pe_k+1 = pe_k + delp_k, and ps = pe_nz."""
    top = np.full(delp.shape[:2] + (1,), float(ptop))
    pe = np.cumsum(np.concatenate([top, delp], axis=2), axis=2)
    return 0.5 * (pe[..., :-1] + pe[..., 1:]), pe[..., -1]


def terms(delp, lat, ptop, **cfg):
    """dict of sigma, s, k_v, k_T, T_eq [nx, ny, nz] and ln(p / p0)."""
    c = {**DEFAULTS, **cfg}
    p, ps = pressures(np.asarray(delp, dtype=np.float64), ptop)
    sl, cl = np.sin(lat)[..., None], np.cos(lat)[..., None]
    s2, c2 = sl * sl, cl * cl
    c4 = c2 * c2
    sigma = p / ps[..., None]
    s = np.maximum(0.0, (sigma - c["sigma_b"]) / (1.0 - c["sigma_b"]))
    k_v = c["k_f"] * s
    k_t = c["k_a"] + ((c["k_s"] - c["k_a"]) * s) * c4
    lr = np.log(p / c["p0"])
    bracket = (315.0 - c["delta_t_y"] * s2) - (c["delta_theta_z"] * lr) * c2
    pk = np.exp(c["kappa"] * lr)
    t_eq = np.maximum(c["t_min"], bracket * pk)
    return dict(p=p, ps=ps, sigma=sigma, s=s, k_v=k_v, k_t=k_t, lr=lr, bracket=bracket, pk=pk, t_eq=t_eq, s2=s2, c2=c2, c4=c4, cfg=c)


def held_suarez(ua, va, t, delp, lat, ptop, dt, **cfg):
    """(u_dt, v_dt, t_dt, terms)."""
    tm = terms(delp, lat, ptop, **cfg)
    fv = tm["k_v"] / (1.0 + dt * tm["k_v"])
    ft = tm["k_t"] / (1.0 + dt * tm["k_t"])
    return -fv * ua, -fv * va, -ft * (t - tm["t_eq"]), tm


def error_bound(ua, va, t, tm, dt, eps, nz):
    """Per-cell bounds on |kernel - this restatement| for a kernel that evaluates the same formulas in arithmetic of unit round-off
    ``eps`` with log / exp / sin / cos good to 1 ulp each (tests/test_fast_math.py pins the device log / exp to that; the reference's own
    libm calls are given the same), first-order in eps.  Derivation, with x' the kernel's value of x and d(x) = |x' - x|:

    * the scan adds nz terms and the layer mean one more: d(p) / p, d(ps) / ps <= (nz + 1) eps, so d(sigma) <= (2 nz + 3) eps sigma;
    * s = (sigma - sigma_b) / (1 - sigma_b): d(s) <= (d(sigma) + eps sigma + eps) / (1 - sigma_b) + 2 eps s  (no relative bound: it cancels);
    * L = ln(p / p0): d(L) <= (nz + 2) eps + 2 eps |L|  (argument error, two log implementations);
    * E = exp(kappa L): d(E) / E <= kappa d(L) + eps |kappa L| + 2 eps;
    * sin^2, cos^2 carry 2 (1 + 1) + 1 = 5 eps, cos^4 11 eps (two implementations, squares);
    * B = (315 - dTy s2) - (dthz L) c2: d(B) <= dTy s2 6 eps + dthz c2 (d(L) + 7 eps |L|) + 3 eps (315 + dTy s2 + dthz |L| c2);
    * T_eq = B E (or the floor, which is exact): d(T_eq) <= E d(B) + |B| E (d(E) / E + eps);
    * k_v = k_f s: d(k_v) <= k_f d(s) + eps k_v;  k_T = k_a + (dk s) c4: d(k_T) <= dk (d(s) c4 + s c4 13 eps) + eps k_T;
    * f = k / (1 + dt k) has |df/dk| <= 1: d(f) <= d(k) + 3 eps f;
    * u_dt = -f_v ua: d <= |ua| d(f_v) + eps |u_dt|;  t_dt = -f_T (T - T_eq): d <= |T - T_eq| d(f_T) + f_T (d(T_eq) + eps |T - T_eq|) + eps |t_dt|."""
    c = tm["cfg"]
    one_sb = 1.0 - c["sigma_b"]
    d_sigma = (2 * nz + 3) * eps * tm["sigma"]
    d_s = (d_sigma + eps * tm["sigma"] + eps) / one_sb + 2 * eps * tm["s"]
    al = np.abs(tm["lr"])
    d_l = (nz + 2) * eps + 2 * eps * al
    d_e_rel = c["kappa"] * d_l + eps * c["kappa"] * al + 2 * eps
    d_b = c["delta_t_y"] * tm["s2"] * 6 * eps + c["delta_theta_z"] * tm["c2"] * (d_l + 7 * eps * al) + 3 * eps * (315.0 + c["delta_t_y"] * tm["s2"] + c["delta_theta_z"] * al * tm["c2"])
    d_teq = tm["pk"] * d_b + np.abs(tm["bracket"]) * tm["pk"] * (d_e_rel + eps)
    d_kv = c["k_f"] * d_s + eps * tm["k_v"]
    dk = abs(c["k_s"] - c["k_a"])
    d_kt = dk * (d_s * tm["c4"] + tm["s"] * tm["c4"] * 13 * eps) + eps * tm["k_t"]
    fv = tm["k_v"] / (1.0 + dt * tm["k_v"])
    ft = tm["k_t"] / (1.0 + dt * tm["k_t"])
    d_fv, d_ft = d_kv + 3 * eps * fv, d_kt + 3 * eps * ft
    dev = np.abs(t - tm["t_eq"])
    b_u = np.abs(ua) * d_fv + eps * fv * np.abs(ua)
    b_v = np.abs(va) * d_fv + eps * fv * np.abs(va)
    b_t = dev * d_ft + ft * (d_teq + eps * dev) + eps * ft * dev
    return b_u, b_v, b_t
