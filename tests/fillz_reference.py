"""numpy restatement of FV3's ``fillz`` (fv_fill.F90, default form; pyFV3 ``fillz.py``), written from the specification in
include/fv3_mi355x.h, not from the kernel: vectorised over the columns, sequential in k, in the dtype it is given.  Every product,
quotient and sum is one numpy operation (one rounding); min(a, b) is ``a < b ? a : b`` and the comparisons are plain IEEE, so -0.0
and NaN take no branch.

``fillz(q, dp)`` takes ``q``, ``dp`` of shape (n_columns, km) and returns ``(q_filled, branches)``; ``branches`` maps the names in
``BRANCHES`` to boolean arrays over the columns (a column is in a class if ANY of its levels took that path)."""
import numpy as np

BRANCHES = ("top", "above_only", "below_only", "both", "bottom_fix", "bottom_left_alone", "zfix", "nonlocal")


def _min(a, b):
    return np.where(a < b, a, b)


def fillz(q, dp):
    q = np.array(q, copy=True)
    dp = np.asarray(dp)
    assert q.ndim == 2 and q.shape == dp.shape and q.dtype == dp.dtype and q.shape[1] >= 2
    T = q.dtype.type
    ncol, km = q.shape
    zero = T(0)
    br = {n: np.zeros(ncol, dtype=bool) for n in BRANCHES}
    with np.errstate(all="ignore"):
        # 1: top layer (does not set zfix)
        m = q[:, 0] < zero
        q[:, 1] = np.where(m, q[:, 1] + (q[:, 0] * dp[:, 0]) / dp[:, 1], q[:, 1])
        q[:, 0] = np.where(m, zero, q[:, 0])
        br["top"] = m
        # 2: interior, in increasing k
        zfix = np.zeros(ncol, dtype=bool)
        for k in range(1, km - 1):
            neg = q[:, k] < zero
            zfix |= neg
            up = neg & (q[:, k - 1] > zero)
            dq = _min(q[:, k - 1] * dp[:, k - 1], -q[:, k] * dp[:, k])
            q[:, k - 1] = np.where(up, q[:, k - 1] - dq / dp[:, k - 1], q[:, k - 1])
            q[:, k] = np.where(up, q[:, k] + dq / dp[:, k], q[:, k])
            dn = neg & (q[:, k] < zero) & (q[:, k + 1] > zero)  # q[k] is the value after the step above
            dq = _min(q[:, k + 1] * dp[:, k + 1], -q[:, k] * dp[:, k])
            q[:, k + 1] = np.where(dn, q[:, k + 1] - dq / dp[:, k + 1], q[:, k + 1])
            q[:, k] = np.where(dn, q[:, k] + dq / dp[:, k], q[:, k])
            br["above_only"] |= up & ~dn
            br["below_only"] |= dn & ~up
            br["both"] |= up & dn
        # 3: bottom layer
        k = km - 1
        neg = q[:, k] < zero
        fix = neg & (q[:, k - 1] > zero)
        zfix |= fix
        dup = _min(-q[:, k] * dp[:, k], q[:, k - 1] * dp[:, k - 1])
        q[:, k - 1] = np.where(fix, q[:, k - 1] - dup / dp[:, k - 1], q[:, k - 1])
        q[:, k] = np.where(fix, q[:, k] + dup / dp[:, k], q[:, k])
        br["bottom_fix"] = fix
        br["bottom_left_alone"] = neg & ~fix
        br["zfix"] = zfix
        # 4: non-local fix
        dm = q * dp  # (level 0 is not used)
        sum0 = np.zeros(ncol, dtype=q.dtype)
        sum1 = np.zeros(ncol, dtype=q.dtype)
        for k in range(1, km):
            sum0 = sum0 + dm[:, k]
            sum1 = sum1 + np.where(dm[:, k] > zero, dm[:, k], zero)
        nl = zfix & (sum0 > zero)
        fac = sum0 / sum1
        for k in range(1, km):
            v = (fac * dm[:, k]) / dp[:, k]
            v = np.where(v < zero, zero, v)
            q[:, k] = np.where(nl, v, q[:, k])
        br["nonlocal"] = nl
    assert q.dtype == dp.dtype
    return q, br
