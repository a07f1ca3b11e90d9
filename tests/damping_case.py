"""Input builders, exact solutions and checkers of tests/test_analytic_damping.py: the corner divergence of c_sw and the damping operators of d_sw held
against closed-form solutions, continuing tests/analytic_case.py (pins 1 - 9) under its ground rule: inputs and expected values come from the corner
positions, the cell centres, the sphere radius and closed-form functions of position.  No metric array a kernel reads (dx, dxc, rarea_c, divg_u, del6_*,
sin_sg*, cosa_*, f0, fC) enters an expected value; edge lengths are arc() of the corners.  The stated exception: the scalars da_min and da_min_c enter the
expected coefficients as configuration, like the Courant number of pin 2, and are held once to the smallest spherical-excess area of the cells, respectively
the dual cells, computed from corner and centre positions (area_minima).

On the sphere of radius a a harmonic of degree l, P_l(p . b), is an eigenfunction of the Laplacian with eigenvalue -l (l + 1) / a^2 =: -lam, and every del-n
chain of d_sw is a power of that Laplacian.  The fields:

  Potential   chi = a c P_l(mu), mu = p . b:  V = grad chi = c P_l'(mu) (b - mu p),  div V = -lam chi = -l (l + 1) c P_l(mu) / a,  curl V = 0
  Stream      psi = a c P_l(mu):              V = p x grad psi = c P_l'(mu) (p x b), curl V = -lam psi,                           div V = 0
              (l = 1, c = -U0, b = AXIS is analytic_case.Flow, the solid-body rotation)
  scalars     d0 (1 + eps P_l(mu))

  pin 10  c_sw, divgd     == minus the divergence of V_rot + V_div, +l (l + 1) chi / a^2 (FV3's divg_d is minus the divergence), by divergence_classes (DivergenceCase)
  pin 11  c_sw, dt2 != 0  delpc, ptc, omga == delp, pt, w at the departure points of the half step; (uc, vc)(dt2) - (uc, vc)(0) == dt2 x the projection
                          of -(zeta + f) k x V - grad K on the cross-face directions of pin 3, by face_classes                    (CswCase)
  pin 12  d_sw            u dx (damping on) - u dx (DSW_OFF) == F(A) - F(B) over the face from corner A to corner B,
                          F = [da_min_c d2 + dd8 lam^n] D, D = divg_d = -div V (every pass of FV3's chain is minus the Laplacian, so no (-1)^n is left),
                          dd8 = (da_min_c d4_bg)^(n + 1), stretched_grid: da_min d4_bg^(n + 1);
                          with dddmp: F += da_min_c dddmp dt sqrt(D^2 + zeta^2) D, zeta = 2 omega (p . axis)                (DivDampCase)
  pin 14  damping heat    heat_source of d_sw at rest with one-pass damping == the kinetic energy taken (heat_errors); del2_cubed on a harmonic (Del2Case);
                          apply_diffusive_heating pointwise, pkz from the gas law (heating_case)
  pin 13  d_sw at rest    uc = vc = 0: one call multiplies the harmonic part of delp, pt, q_con by 1 - (damp da_min lam)^(n + 1), that of w by
                          1 - (damp da_min_c lam)^(n + 1), and changes a rotational wind by -(damp_vt da_min_c lam)^(nord_v + 1) V  (RestCase)

d_sw returns u dx and v dy (the winds times the edge length; dyn_core divides afterwards), so the increments of pins 12 and 13 are compared per unit
length: divided by arc(A, B) a.

FV3's del-n operator is the Laplacian only where the grid lines cross at right angles and the cells are square (tests/test_analytic_damping.py, DESIGN.md
section 2, restatement 13): the closed forms of pins 12 (nord >= 1) and 13 are compared on the interior faces / cells within CENTRE_CELLS cells of the tile's centre
("centre"), every other class is held to the oracle's record.

FV3 takes da_min in fv_tp_2d's deln_flux (delp, pt, q_con) and da_min_c in d_sw's own del6_vt_flux calls (w and the vorticity); the expected factors follow
that.  The per-level (order, coefficient) pairs of the default configuration are written out by hand in SPONGE_TABLE, not read from any table the oracle or
the library forms.
"""
import numpy as np
from numpy.polynomial import legendre

import analytic_case as ac
from analytic_case import NH, CheckFailed, Geometry, _grow, _tangent, _unit, arc, levels, require  # noqa: F401

POLE = _unit(np.array([-0.55, 0.35, 0.76]))  # oblique to every tile, 77 degrees from AXIS
DAMP_NZ = 5
EPS_SCALAR = 0.05


class Harmonic:
    """P_l(p . b) and its derivative with respect to mu = p . b"""

    def __init__(self, l, b=POLE):
        self.l, self.b = int(l), _unit(np.asarray(b, dtype=np.float64))
        self.coef = np.zeros(self.l + 1)
        self.coef[self.l] = 1.0
        self.dcoef = legendre.legder(self.coef)

    def mu(self, p):
        return np.sum(p * self.b, -1)

    def P(self, p):
        return legendre.legval(self.mu(p), self.coef)

    def dP(self, p):
        return legendre.legval(self.mu(p), self.dcoef)

    def lam(self, a):
        return self.l * (self.l + 1) / a**2


class Potential:
    """V = grad chi, chi = a c P_l(p . b)"""

    def __init__(self, a, c, l, b=POLE):
        self.a, self.c, self.h = float(a), float(c), Harmonic(l, b)

    def wind(self, p):
        return self.c * self.h.dP(p)[..., None] * (self.h.b - self.h.mu(p)[..., None] * p)

    def div(self, p):
        return -self.h.l * (self.h.l + 1) * self.c * self.h.P(p) / self.a

    def curl(self, p):
        return np.zeros(p.shape[:-1])


class Stream:
    """V = p x grad psi, psi = a c P_l(p . b)"""

    def __init__(self, a, c, l, b=POLE):
        self.a, self.c, self.h = float(a), float(c), Harmonic(l, b)

    def wind(self, p):
        return self.c * self.h.dP(p)[..., None] * np.cross(p, np.broadcast_to(self.h.b, p.shape))

    def div(self, p):
        return np.zeros(p.shape[:-1])

    def curl(self, p):
        return -self.h.l * (self.h.l + 1) * self.c * self.h.P(p) / self.a


def rotation(a):
    """analytic_case.Flow as a Stream: (the Stream, the Flow)"""
    fl = ac.Flow(a)
    return Stream(a, -fl.u0, 1, fl.axis), fl


class Winds:
    """a sum of Potential / Stream parts, sampled on the staggered grids from positions alone"""

    def __init__(self, *parts):
        self.parts = parts

    def wind(self, p):
        return sum(x.wind(p) for x in self.parts)

    def div(self, p):
        return sum(x.div(p) for x in self.parts)

    def curl(self, p):
        return sum(x.curl(p) for x in self.parts)

    def d_grid(self, G):
        return np.sum(self.wind(G.my) * G.tx, -1), np.sum(self.wind(G.mx) * G.ty, -1)

    def c_grid(self, G):
        return np.sum(self.wind(G.mx) * G.e1(), -1), np.sum(self.wind(G.my) * G.e2(), -1)

    def a_grid(self, G):
        """(ua, va): the contravariant components at the cell centres, V = ua ex + va ey with ex, ey the unit vectors from the west to the east and
        from the south to the north face mid-point"""
        shape = G.P.shape[:2]
        ex = _tangent(_grow(G.mx[1:] - G.mx[:-1], shape), G.C)
        ey = _tangent(_grow(G.my[:, 1:] - G.my[:, :-1], shape), G.C)
        V = self.wind(G.C)
        vx, vy, cs = np.sum(V * ex, -1), np.sum(V * ey, -1), np.sum(ex * ey, -1)
        with np.errstate(divide="ignore", invalid="ignore"):  # (the storage padding of _grow has no direction)
            return (vx - cs * vy) / (1.0 - cs**2), (vy - cs * vx) / (1.0 - cs**2)


def edge_lengths(G, a):
    """(length of the u faces, corner i -> i + 1; of the v faces, corner j -> j + 1), storage shape, from corner positions"""
    P = G.P
    return a * _grow(arc(P[:-1, :], P[1:, :]), P.shape[:2]), a * _grow(arc(P[:, :-1], P[:, 1:]), P.shape[:2])


def cell_classes(G, width=3):
    """masks over the compute cells: "corner" within ``width`` cells of two tile edges, "edge" of one, "interior" of none (the del-n chains of order 2
    reach three cells)"""
    g = G.g
    near_x, near_y = np.zeros((g.nx, g.ny), bool), np.zeros((g.nx, g.ny), bool)
    if g.west_edge:
        near_x[:width] = True
    if g.east_edge:
        near_x[-width:] = True
    if g.south_edge:
        near_y[:, :width] = True
    if g.north_edge:
        near_y[:, -width:] = True
    return {"interior": ~(near_x | near_y), "edge": near_x ^ near_y, "corner": near_x & near_y}


CENTRE_CELLS = 2.05  # the "centre" class reaches two cells from the tile's centre at every resolution (0.13 rad at C24)


def tile_centre(G):
    """the centre of the tile the rank lies on: the cube-face centre nearest to the rank's middle corner (through the Schmidt transform on a stretched grid)"""
    from pace_amd.grid import tile_point

    c = np.array([tile_point(t, np.array(0.5), np.array(0.5), 1) for t in range(6)])
    if G.g.stretch is not None:
        c = G.g.stretch(c)
    mid = G.P[NH + G.nx // 2, NH + G.ny // 2]
    return c[np.argmin(arc(c, np.broadcast_to(mid, c.shape)))]


def near_centre(G, p):
    """mask of the positions p [..., 3] within CENTRE_CELLS cell widths of the tile's centre, where the grid lines cross at right angles and the cells are
    square, so that FV3's damping operator (module docstring) is the Laplacian; its deviation grows as the square of the distance from the centre, so a
    radius counted in cells makes the class converge.  The cell width is that of the rank's corner nearest to the centre"""
    c = tile_centre(G)
    P = G.P[G.corners]
    i, j = np.unravel_index(np.argmin(arc(P, np.broadcast_to(c, P.shape))), P.shape[:2])
    i = min(i, P.shape[0] - 2)
    return arc(p, np.broadcast_to(c, p.shape)) < CENTRE_CELLS * arc(P[i, j], P[i + 1, j])


FACE_KEYS = ac.CLASS_KEYS  # {0: "class0", 1: "class1", SECOND: "second_line", INTERIOR: "class2"}


def _worst(err, key, d):
    if d.size:
        err[key] = max(err.get(key, 0.0), float(np.abs(d).max()))


def _excess(p0, p1, p2):
    """spherical excess of a triangle of unit vectors"""
    return 2.0 * np.arctan2(np.abs(np.sum(p0 * np.cross(p1, p2), -1)), 1.0 + np.sum(p0 * p1, -1) + np.sum(p1 * p2, -1) + np.sum(p2 * p0, -1))


def _quad(p0, p1, p2, p3):
    return _excess(p0, p1, p2) + _excess(p0, p2, p3)


def area_minima(grids, a):
    """(smallest cell area, smallest dual-cell area) over the compute domains of ``grids``, from corner and centre positions by spherical excess: a
    dual cell is the quadrilateral of the four centres round a corner; on a tile edge twice its half on this tile (edge mid-points and two centres),
    at a cube corner three times the kite corner - edge mid-point - centre - edge mid-point"""
    amin = cmin = np.inf
    for g in grids:
        G = Geometry(g)
        P, C, nx, ny = G.P, G.C, g.nx, g.ny
        I, J = np.meshgrid(np.arange(NH, NH + nx), np.arange(NH, NH + ny), indexing="ij")
        amin = min(amin, float(_quad(P[I, J], P[I + 1, J], P[I + 1, J + 1], P[I, J + 1]).min()))
        I, J = np.meshgrid(np.arange(NH, NH + nx + 1), np.arange(NH, NH + ny + 1), indexing="ij")
        dual = _quad(C[I - 1, J - 1], C[I, J - 1], C[I, J], C[I - 1, J])
        on_w, on_e = g.west_edge & (I == NH), g.east_edge & (I == NH + nx)
        on_s, on_n = g.south_edge & (J == NH), g.north_edge & (J == NH + ny)
        mid = lambda p, q: _unit(p + q)  # noqa: E731
        for on, ci in ((on_w, I), (on_e, I - 1)):
            half = 2.0 * _quad(mid(P[I, J - 1], P[I, J]), C[ci, J - 1], C[ci, J], mid(P[I, J], P[I, J + 1]))
            dual = np.where(on, half, dual)
        for on, cj in ((on_s, J), (on_n, J - 1)):
            half = 2.0 * _quad(mid(P[I - 1, J], P[I, J]), C[I - 1, cj], C[I, cj], mid(P[I, J], P[I + 1, J]))
            dual = np.where(on, half, dual)
        for onx, ci, di in ((on_w, I, 1), (on_e, I - 1, -1)):
            for ony, cj, dj in ((on_s, J, 1), (on_n, J - 1, -1)):
                kite = 3.0 * _quad(P[I, J], mid(P[I, J], P[I + di, J]), C[ci, cj], mid(P[I, J], P[I, J + dj]))
                dual = np.where(onx & ony, kite, dual)
        cmin = min(cmin, float(dual.min()))
    return amin * a * a, cmin * a * a


# ---------------------------------------------------------------------------------------------------------------------------
# pin 10: the corner divergence of c_sw
# ---------------------------------------------------------------------------------------------------------------------------
DIV_L = (3, 1)


def divergence_classes(G):
    """corner_classes with the corners three lines from a tile edge ("third_line") taken out of "interior": there d2a2c_vect goes over from two-point to
    four-point averages of the winds that divergence_corner's cosine terms read, and the error is first order (measured: 2.2e-3 at C24, 1.3e-3 at C48,
    against 1.6e-3 and 4.0e-4 on the lines either side).  Every compute corner is in exactly one class"""
    g, cls = G.g, ac.corner_classes(G)
    third = np.zeros_like(cls["interior"])
    for flag, idx in ((g.west_edge, (3,)), (g.east_edge, (-4,)), (g.south_edge, (slice(None), 3)), (g.north_edge, (slice(None), -4))):
        if flag:
            third[idx] = True
    third &= cls["interior"]
    return {"interior": cls["interior"] & ~third, "third_line": third, "edge": cls["edge"], "corner": cls["corner"]}


def div_amplitude(l, u0):
    """c of the potential flow: |V| of the order of U0 (max |P_3'(mu)| sin(theta) = 2.07)"""
    return 0.5 * u0 if l == 3 else u0


class DivergenceCase:
    """per rank: D-grid winds u, v [i, j, nz] of the rotation (Flow) plus, unless ``rotation_only``, the potential flow of degree l"""

    def __init__(self, grids, a, l=3, rotation_only=False, nz=ac.DYN_NZ):
        rot, self.flow = rotation(a)
        self.pot = Potential(a, div_amplitude(l, self.flow.u0), l)
        self.winds = Winds(rot) if rotation_only else Winds(rot, self.pot)
        self.a, self.nz, self.grids = float(a), nz, grids
        self.G = [Geometry(g) for g in grids]
        self.ins = []
        for G in self.G:
            u, v = self.winds.d_grid(G)
            self.ins.append({"u": levels(u, nz), "v": levels(v, nz)})
        self.top_div = self.pot.h.l * (self.pot.h.l + 1) * self.pot.c / self.a  # max |D| of the potential flow
        self.top_wind = 3.0 * self.flow.u0

    def errors(self, divgds, scale=None, sign=1.0):
        """max |divgd + div V| / scale per class of corners (default scale: the largest exact divergence); sign = -1: against +div V (the control)"""
        scale = self.top_div if scale is None else scale
        err = {"interior": 0.0, "third_line": 0.0, "edge": 0.0, "corner": 0.0}
        for G, got in zip(self.G, divgds):
            d = np.asarray(got, dtype=np.float64)[G.corners][..., : self.nz] + sign * self.winds.div(G.P[G.corners])[..., None]
            require(np.all(np.isfinite(d)), "non-finite divergence")
            cls = divergence_classes(G)
            require(np.all(sum(m.astype(int) for m in cls.values()) == 1), "a corner in no class or in two")
            for k, m in cls.items():
                _worst(err, k, d[m])
        return {k: v / scale for k, v in err.items()}


def oracle_c_sw(doms, ins, dt2=0.0, nord=1):
    """the oracle's c_sw on copies: per rank a dict of its outputs"""
    from fv3_oracle import c_sw as o_csw

    outs = []
    for D, x in zip(doms, ins):
        z = lambda: np.zeros_like(x["u"])  # noqa: E731
        w = {k: (x[k].copy() if k in x else (np.ones_like(x["u"]) if k in ("delp", "pt") else z())) for k in ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "ut", "vt", "divgd", "omga")}
        w["delpc"], w["ptc"] = o_csw.c_sw(D, *[w[k] for k in ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "ut", "vt", "divgd", "omga")], dt2, nord=nord)
        outs.append(w)
    return outs


# ---------------------------------------------------------------------------------------------------------------------------
# pin 12: the divergence damping of d_sw, on against off
# ---------------------------------------------------------------------------------------------------------------------------
DIVDAMP_RUNS = {  # name: what is switched on over DSW_OFF
    "nord0": dict(nord=0, d2_bg=0.05),
    "nord1": dict(nord=1, d4_bg=0.15),
    "nord2": dict(nord=2, d4_bg=0.15),
    "nord3": dict(nord=3, d4_bg=0.15),
    "smag": dict(nord=2, d4_bg=0.15, dddmp=0.5),
    "nord0_l1": dict(nord=0, d2_bg=0.05),  # the potential flow of degree 1 (DIVDAMP_L)
}
DIVDAMP_L = {"nord0_l1": 1}  # the degree of the potential flow where it is not 3


def damp_config(run, **kw):
    return dict(ac.DSW_OFF, **DIVDAMP_RUNS[run], **kw)


class DivDampCase(ac.DswCase):
    """DswCase on V_rot + V_div (or the rotation alone): u, v, uc, vc, ua, va analytic, divgd the exact divergence at the corners on every corner of the
    storage (what c_sw's divergence_corner would hand on, less its truncation error; nord = 0 forms its own from u, v, ua, va), scalars as DswCase"""

    def __init__(self, n, grids, a, omega_earth, l=3, rotation_only=False, nz=ac.DYN_NZ):
        super().__init__(n, grids, a, omega_earth, nz=nz)
        rot, _ = rotation(a)
        self.pot = Potential(a, div_amplitude(l, self.flow.u0), l)
        self.winds = Winds(rot) if rotation_only else Winds(rot, self.pot)
        self.lam = self.pot.h.lam(self.flow.a)
        for G, x in zip(self.G, self.ins):
            (u, v), (uc, vc), (ua, va) = self.winds.d_grid(G), self.winds.c_grid(G), self.winds.a_grid(G)
            x.update({"u": levels(u, nz), "v": levels(v, nz), "uc": levels(uc, nz), "vc": levels(vc, nz), "ua": levels(ua, nz), "va": levels(va, nz), "divgd": levels(-self.winds.div(G.P), nz)})

    def damping_field(self, p, g, kw, spoil=None):
        """F(p), closed form.  spoil: "exponent" (n for n + 1), "da_min" (for da_min_c), "sign" ((-1)^n dropped)"""
        n, d2, d4, dddmp = kw["nord"], kw["d2_bg"], kw["d4_bg"], kw["dddmp"]
        D = -self.winds.div(p)  # FV3's divg_d
        dac = g.da_min if spoil == "da_min" else g.da_min_c
        power = n if spoil == "exponent" else n + 1
        dd8 = g.da_min * d4**power if kw.get("stretched_grid") else (dac * d4) ** power
        coef = dac * d2
        if n > 0:
            coef = coef + dd8 * ((-self.lam if spoil == "sign" else self.lam) ** n)  # every pass of FV3's chain is -Laplacian
        if dddmp > 0.0:
            vort = abs(self.dt) * (np.sqrt(D**2 + self.winds.curl(p) ** 2) if n > 0 else np.abs(D))
            require(float((dddmp * vort).max()) < 0.2 and float((dddmp * vort).min()) > d2, "the Smagorinsky coefficient has left its free branch")
            coef = dac * dddmp * vort + (coef - dac * d2)
        return coef * D

    def increments(self, on, off, kw, spoil=None):
        """per rank ((classes, got, want) of the u faces, of the v faces): the wind increment per unit length, (u dx (on) - u dx (off)) / L against
        (F(A) - F(B)) / L; with the largest |want| and the largest eps |u dx| / L (the round-off of the difference)"""
        out, top, noise = [], 0.0, 0.0
        eps = float(np.finfo(np.float64).eps)
        for g, G, a, b in zip(self.grids, self.G, on, off):
            Lu, Lv = edge_lengths(G, self.flow.a)
            F = self.damping_field(G.P, g, kw, spoil)
            cu, cv = ac.face_classes(G)
            pair = []
            for name, F0, F1, L, S, mid in (("u", F[:-1, :], F[1:, :], Lu, G.Y, G.my), ("v", F[:, :-1], F[:, 1:], Lv, G.X, G.mx)):
                A, B = (np.asarray(x[name], dtype=np.float64)[:, :, : self.nz][S] for x in (a, b))
                got = (A - B) / L[S][..., None]
                want = (_grow(F0 - F1, F.shape)[S] / L[S])[..., None]
                require(np.all(np.isfinite(got)), "non-finite wind")
                top, noise = max(top, float(np.abs(want).max())), max(noise, eps * float(np.abs(B / L[S][..., None]).max()))
                pair.append((cu if name == "u" else cv, got, want, near_centre(G, mid[S])))
            out.append(tuple(pair))
        return out, top, noise

    def errors(self, on, off, kw, spoil=None, scale=None):
        """max |increment - exact| / max |exact| (or ``scale``) per class of faces, and over the interior faces near the tile's centre ("centre"); "signal": max |exact| over the round-off of the on/off difference; "top": max |exact|;
        "largest": the largest increment got on the "centre" faces, in the unit of top (the chains of order 2 and 3 carry the tile-edge error far into
        class 2+; at the centre the figure says how much was damped)"""
        res, top, noise = self.increments(on, off, kw, spoil)
        err, largest = dict.fromkeys(list(FACE_KEYS.values()) + ["centre"], 0.0), 0.0
        for pair in res:
            for cls, got, want, centre in pair:
                _worst(err, "centre", (got - want)[centre & (cls == ac.INTERIOR)])
                seen = np.zeros(cls.shape, int)
                for c, key in FACE_KEYS.items():
                    _worst(err, key, (got - want)[cls == c])
                    seen += cls == c
                require(np.all(seen == 1), "a face in no class or in two")
                largest = max(largest, float(np.abs(got[centre & (cls == ac.INTERIOR)]).max(initial=0.0)))
        scale = top if scale is None else scale
        out = {k: v / scale for k, v in err.items()}
        out.update({"signal": top / noise, "top": top, "noise": noise, "largest": largest / scale})
        return out


def oracle_d_sw_pair(doms, cfg_on, cfg_off, dc):
    return ac.oracle_d_sw(doms, cfg_on, dc), ac.oracle_d_sw(doms, cfg_off, dc)


# ---------------------------------------------------------------------------------------------------------------------------
# pin 13: the del-n chains of d_sw on a state at rest
# ---------------------------------------------------------------------------------------------------------------------------
# The default configuration (n_sponge 48, d2_bg_k1 0.2, d2_bg_k2 0.1, d2_bg 0, nord 3, vtdm4 0.06, do_vort_damp) on five levels, by hand from FV3's
# d_sw namelist logic: level 0 and 1 are "lowest" sponge levels (order 0 for the divergence, w and the vorticity, their coefficients from d2_bg_k1 /
# d2_bg_k2: w takes d2, the vorticity and with it delp / pt half of it), level 2 the third (order 0 for w with 0.2 d2_bg_k2; the vorticity keeps order 2),
# levels 3 and 4 regular (min(2, nord) = 2, vtdm4).  q_con (nord_t, damp_t) is never touched by the sponge.  Each entry: (order, coefficient).
SPONGE_TABLE = {
    "delp": [(0, 0.10), (0, 0.05), (2, 0.06), (2, 0.06), (2, 0.06)],
    "pt": [(0, 0.10), (0, 0.05), (2, 0.06), (2, 0.06), (2, 0.06)],
    "q_con": [(2, 0.06), (2, 0.06), (2, 0.06), (2, 0.06), (2, 0.06)],
    "w": [(0, 0.20), (0, 0.10), (0, 0.02), (2, 0.06), (2, 0.06)],
    "vort": [(0, 0.10), (0, 0.05), (2, 0.06), (2, 0.06), (2, 0.06)],
}
NORD1_TABLE = {  # the same sponge over nord = 1 (the fp32 case): the regular levels are of order min(2, nord) = 1
    "delp": [(0, 0.10), (0, 0.05), (1, 0.06), (1, 0.06), (1, 0.06)],
    "pt": [(0, 0.10), (0, 0.05), (1, 0.06), (1, 0.06), (1, 0.06)],
    "q_con": [(1, 0.06)] * 5,
    "w": [(0, 0.20), (0, 0.10), (0, 0.02), (1, 0.06), (1, 0.06)],
    "vort": [(0, 0.10), (0, 0.05), (1, 0.06), (1, 0.06), (1, 0.06)],
}
ONE_PASS = ("delp.0", "delp.1", "pt.0", "pt.1", "w.0", "w.1", "w.2", "vort.0", "vort.1")  # the (field, level) pairs of order 0 under the default sponge
NO_SPONGE_TABLE = {k: [(2, 0.06)] * DAMP_NZ for k in SPONGE_TABLE}  # n_sponge = -1
AREA_OF = {"delp": "da_min", "pt": "da_min", "q_con": "da_min", "w": "da_min_c", "vort": "da_min_c"}
REST_BASE = {"delp": 1000.0, "pt": 300.0, "q_con": 0.025, "w": 2.5}
REST_CONFIG = dict(d_con=0.0)  # everything else the default; pin 13 looks at the fields, not at the heat
REST_DT = 300.0


def damping_factor(name, k, g, lam, table=SPONGE_TABLE, spoil=None):
    """(damp area lam)^(n + 1) of field ``name`` on level k: one call takes this share of the harmonic away.  spoil: "exponent" (n for n + 1), "shift"
    (the table one level down), "half" (the mass-weighted flux of pt / q_con without its 1/2: twice the share)"""
    n, damp = table[name][min(k + 1, DAMP_NZ - 1) if spoil == "shift" else k]
    share = (damp * getattr(g, AREA_OF[name]) * lam) ** (n if spoil == "exponent" else n + 1)
    return 2.0 * share if (spoil == "half" and name in ("pt", "q_con")) else share


class RestCase:
    """d_sw with uc = vc = 0 (no transport: fxadv returns zero Courant numbers and area fluxes), per rank the inputs of one call, kind "mass": delp
    harmonic, everything else uniform and u = v = 0; kind "fields": delp uniform, pt, q_con, w harmonic (degree l, amplitudes EPS_SCALAR and a different
    sign per level so that a level taken for another shows), u, v the D-grid winds of a stream function of degree l, ua, va its contravariant components,
    divgd = 0 (its exact divergence)"""

    def __init__(self, grids, a, kind, l=3, nz=DAMP_NZ):
        self.grids, self.a, self.kind, self.nz = grids, float(a), kind, nz
        self.h = Harmonic(l)
        self.lam = self.h.lam(self.a)
        self.stream = Stream(a, 0.5 * ac.Flow(a).u0, l)
        self.winds = Winds(self.stream)
        self.G = [Geometry(g) for g in grids]
        self.amp = np.array([EPS_SCALAR * (1.0 + 0.2 * k) * (-1.0) ** k for k in range(nz)])
        self.ins = []
        for G in self.G:
            shape = G.P.shape[:2]
            x = {k: np.zeros(shape + (nz,)) for k in ("u", "v", "uc", "vc", "ua", "va", "divgd", "mfxd", "mfyd", "cxd", "cyd")}
            for k, base in REST_BASE.items():
                x[k] = np.full(shape + (nz,), base)
            if kind == "mass":
                x["delp"] = self.scalar("delp", G.C)
            else:
                for k in ("pt", "q_con", "w"):
                    x[k] = self.scalar(k, G.C)
                (u, v), (ua, va) = self.winds.d_grid(G), self.winds.a_grid(G)
                x.update({"u": levels(u, nz), "v": levels(v, nz), "ua": levels(ua, nz), "va": levels(va, nz)})
            self.ins.append(x)
        self.dt = REST_DT

    def scalar(self, name, p, share=None):
        """base (1 + amp_k (1 - share_k) P_l): the input (share None) or the exact answer"""
        keep = 1.0 if share is None else 1.0 - np.asarray(share)
        return REST_BASE[name] * (1.0 + self.amp * keep * self.h.P(p)[..., None])

    def names(self):
        return ("delp",) if self.kind == "mass" else ("pt", "q_con", "w", "vort")

    def errors(self, outs, table=SPONGE_TABLE, spoil=None):
        """{"field.level.class": max |change - exact change| / max |exact change|} over the cells (scalars: cell_classes and "centre") or the faces (the
        wind increment per unit length, "vort": face_classes and "centre"), "field.level.size": the largest change got on the interior class over the largest exact change (how much was damped, whatever the pattern),
        "field.level.top": the largest exact change over the size of the field itself (what a rounding of the field is measured against in fp32),
        plus "field.level.l2": the area-weighted l2 norm of the scalar's harmonic part
        after the call over that before, which damping keeps below 1 (area weights this norm and nothing else)"""
        err, norms = {}, {}
        for g, G, x, o in zip(self.grids, self.G, self.ins, outs):
            cls = cell_classes(G)
            require(np.all(sum(m.astype(int) for m in cls.values()) == 1), "a cell in no class or in two")
            for name in self.names():
                share = np.array([damping_factor(name, k, g, self.lam, table, spoil) for k in range(self.nz)])
                if name != "vort":
                    got = np.asarray(o[name], dtype=np.float64)[G.cells][..., : self.nz] - x[name][G.cells]
                    want = self.scalar(name, G.C[G.cells], share) - x[name][G.cells]
                    require(np.all(np.isfinite(got)), f"{name}: non-finite")
                    top = np.abs(want).max((0, 1))
                    centre = near_centre(G, G.C[G.cells])
                    for k in range(self.nz):
                        for c, m in cls.items():
                            _worst(err, f"{name}.{k}.{c}", (got - want)[..., k][m] / top[k])
                        _worst(err, f"{name}.{k}.centre", (got - want)[..., k][centre & cls["interior"]] / top[k])
                        _worst(err, f"{name}.{k}.size", got[..., k][cls["interior"]] / top[k])
                        err[f"{name}.{k}.top"] = max(err.get(f"{name}.{k}.top", 0.0), float(top[k]) / REST_BASE[name])
                        w, before = g.area[G.cells], x[name][G.cells][..., k] - REST_BASE[name]
                        norms[(name, k)] = norms.get((name, k), np.zeros(2)) + np.array([(w * (before + got[..., k]) ** 2).sum(), (w * before**2).sum()])
                    continue
                Lu, Lv = edge_lengths(G, self.a)
                cu, cv = ac.face_classes(G)
                tops = []
                for comp, L, S, want0, mid in (("u", Lu, G.Y, x["u"], G.my), ("v", Lv, G.X, x["v"], G.mx)):
                    got = np.asarray(o[comp], dtype=np.float64)[..., : self.nz][S] / L[S][..., None] - x[comp][S]
                    want = -share * want0[S]
                    require(np.all(np.isfinite(got)), f"{comp}: non-finite")
                    tops.append((comp, got, want, near_centre(G, mid[S])))
                top = np.maximum(*[np.abs(w).max((0, 1)) for _, _, w, _ in tops])
                for (comp, got, want, centre), fc in zip(tops, (cu, cv)):
                    for k in range(self.nz):
                        for c, key in FACE_KEYS.items():
                            _worst(err, f"vort.{k}.{key}", (got - want)[..., k][fc == c] / top[k])
                        _worst(err, f"vort.{k}.centre", (got - want)[..., k][centre & (fc == ac.INTERIOR)] / top[k])
                        _worst(err, f"vort.{k}.size", got[..., k][fc == ac.INTERIOR] / top[k])
                        err[f"vort.{k}.top"] = max(err.get(f"vort.{k}.top", 0.0), float(top[k]) / float(np.abs(x["u"][G.Y]).max()))
        for (name, k), (after, before) in norms.items():
            err[f"{name}.{k}.l2"] = float(np.sqrt(after / before))
        return err


def rest_config(n, layout, **kw):
    return ac.dyn_config(n, layout, DAMP_NZ, **{**{k: v for k, v in _DEFAULTS.items()}, **REST_CONFIG, **kw})


# the damping entries of the default configuration, restated here so that DSW_OFF (which dyn_config starts from) is undone explicitly
_DEFAULTS = dict(nord=3, d2_bg=0.0, d2_bg_k1=0.2, d2_bg_k2=0.1, d4_bg=0.15, dddmp=0.5, d_con=1.0, vtdm4=0.06, ke_bg=0.0, do_vort_damp=True, n_sponge=48)


def oracle_rest(doms, cfg, rc):
    from fv3_oracle import d_sw as o_dsw

    col = o_dsw.get_column_namelist(cfg, rc.nz)
    outs = []
    for D, x in zip(doms, rc.ins):
        w = {k: (x[k].copy() if k in x else np.zeros_like(x["u"])) for k in ac.D_SW_ORDER}
        w["zh"] = None
        o_dsw.d_sw(D, cfg, col, *[w[k] for k in ac.D_SW_ORDER], rc.dt)
        outs.append(w)
    return outs


# ---------------------------------------------------------------------------------------------------------------------------
# the record: the numpy oracle's figures on the same inputs (``python tests/analytic_case.py --record damping``)
# ---------------------------------------------------------------------------------------------------------------------------
# which runs of pin 12 go on which shape: nord 3 at C24 only -- at C48 its closed-form signal is 9e2 x the round-off of the on/off difference, below the
# 1e4 the pins ask for (C24: 2.4e5)
DIVDAMP_SHAPES = {"c24": ("nord0", "nord1", "nord2", "nord3", "smag", "nord0_l1"), "c48": ("nord0", "nord1", "nord2", "smag"), "c48_2x2": ("nord0", "nord2", "smag"), "c65": ("nord0", "nord2", "smag")}
HELD12 = tuple(FACE_KEYS.values()) + ("centre",)


def measure_divergence(shape):
    n, layout, ranks = ac.SHAPES[shape]
    part, grids, doms, c = ac.make(n, layout, ranks, ac.DYN_NZ)
    out = {}
    for key, kw in (("l3", dict(l=3)), ("l1", dict(l=1)), ("rotation", dict(rotation_only=True))):
        dc = DivergenceCase(grids, c.RADIUS, **kw)
        out[key] = dc.errors([o["divgd"] for o in oracle_c_sw(doms, dc.ins)])
    return out


def measure_divdamp(shape, run, rotation_only=False):
    n, layout, ranks = ac.SHAPES[shape]
    part, grids, doms, c = ac.make(n, layout, ranks, ac.DYN_NZ)
    dc = DivDampCase(n, grids, c.RADIUS, c.OMEGA, l=DIVDAMP_L.get(run, 3), rotation_only=rotation_only)
    on, off = oracle_d_sw_pair(doms, ac.dyn_config(n, layout, **DIVDAMP_RUNS[run]), ac.dyn_config(n, layout), dc)
    return dc.errors(on, off, damp_config(run), scale=rotation_scale(n, grids, c, run) if rotation_only else None)


STRETCHED_RUN, STRETCHED_N = "nord1", 12


def stretched_grids():
    """the six ranks of tests/stretched_case.py's C12 grid (stretch 3) on DYN_NZ levels, with the oracle's domains"""
    import stretched_case as sc
    from fv3_oracle.util import Dom
    from pace_amd.constants import get_constants

    c = get_constants()
    part, grids = sc.grids((1, 1), nz=ac.DYN_NZ, n=STRETCHED_N)
    return list(grids), [Dom(g, c) for g in grids], c


def stretched_config(g):
    """STRETCHED_RUN with the flag and a d4_bg of 0.15 da_min_c / sqrt(da_min) (about 1e4).  FV3's stretched form da_min d4_bg^(nord + 1) is not a power of an
    area: with d4_bg = 0.15 it is 1e10 times smaller than the congruent one and its increment lies below the round-off of the on/off difference (signal
    0.28).  The closed form is linear in dd8, so the form of the coefficient is tested at the d4_bg that makes it as large as the congruent form with 0.15"""
    kw = damp_config(STRETCHED_RUN, stretched_grid=True)
    kw["d4_bg"] = 0.15 * g.da_min_c / np.sqrt(g.da_min)
    return kw


def measure_stretched():
    """pin 12 with stretched_grid: the closed form has dd8 = da_min d4_bg^(n + 1); the oracle knows the congruent form only and is given the d4_bg with which
    that equals the stretched one (stretched_case.equivalent_d4_bg, as tests/test_stretched_parity.py does)"""
    import stretched_case as sc

    grids, doms, c = stretched_grids()
    n, kw = STRETCHED_N, stretched_config(grids[0])
    dc = DivDampCase(n, grids, c.RADIUS, c.OMEGA)
    d4 = sc.equivalent_d4_bg(grids[0], kw["d4_bg"], kw["nord"])
    on, off = oracle_d_sw_pair(doms, ac.dyn_config(n, (1, 1), nord=kw["nord"], d4_bg=d4), ac.dyn_config(n, (1, 1)), dc)
    return dc.errors(on, off, kw)


def rotation_scale(n, grids, c, run):
    """the largest exact increment of the same run on V_rot + V_div: the unit in which the rotation's (zero) increment is quoted"""
    dc = DivDampCase(n, grids, c.RADIUS, c.OMEGA)
    zero = [{k: np.zeros_like(x[k]) for k in ("u", "v")} for x in dc.ins]
    return dc.increments(zero, zero, damp_config(run))[1]


def measure_rest(shape, kind, **kw):
    n, layout, ranks = ac.SHAPES[shape]
    part, grids, doms, c = ac.make(n, layout, ranks, DAMP_NZ)
    rc = RestCase(grids, c.RADIUS, kind)
    return rc.errors(oracle_rest(doms, rest_config(n, layout, **kw), rc), table_for(kw))


def table_for(kw):
    return NO_SPONGE_TABLE if kw.get("n_sponge", 48) < 0 else NORD1_TABLE if kw.get("nord", 3) == 1 else SPONGE_TABLE


# ---------------------------------------------------------------------------------------------------------------------------
# pin 14: the damping heat, del2_cubed and apply_diffusive_heating
# ---------------------------------------------------------------------------------------------------------------------------
HEAT_SHARE = 0.2  # the share one call takes off the wind and off w in the heat case: large, so that the 1/2 |dV|^2 term is a tenth of the heat
DEL2_CD = 0.2  # cd = 0.2 da_min, the value dyn_core hands to del2_cubed


def heat_config(g, lam):
    """every damping of d_sw one pass (nord 0, hence nord_v = nord_w = 0) and the same on every level (n_sponge -1), d_con on, no divergence damping:
    vtdm4 is set so that the wind and w lose HEAT_SHARE of their harmonic in one call"""
    return dict(_DEFAULTS, nord=0, n_sponge=-1, d_con=1.0, dddmp=0.0, d2_bg=0.0, vtdm4=HEAT_SHARE / (g.da_min_c * lam))


HEAT_W0, HEAT_WA = 2.0, 40.0


HEAT_POLE = Harmonic(3, ac.Z_AXIS)


def heat_case(grids, a):
    """RestCase "fields" with w = HEAT_W0 + HEAT_WA (-1)^k P_3(p_z): a harmonic part as large as the wind and larger than its mean, about the z axis, so that
    it is +-1 at the centres of the two polar tiles: there, on "centre", the heat of w is half of the total and its dw^2 / 2 term a twentieth"""
    rc = RestCase(grids, a, "fields")
    sign = np.array([(-1.0) ** k for k in range(rc.nz)])
    for G, x in zip(rc.G, rc.ins):
        x["w"] = HEAT_W0 + HEAT_WA * sign * HEAT_POLE.P(G.C)[..., None]
    return rc


def heat_errors(rc, outs, spoil=None):
    """heat_source of d_sw on heat_case under heat_config against delp [(s - s^2 / 2) |V|^2 + s w' (w - s w' / 2)], s = HEAT_SHARE, w' the harmonic
    part of w, V the wind at the cell centre: the kinetic energy -(V . dV + |dV|^2 / 2) - dw (w + dw / 2) that dV = -s V, dw = -s w' take away.  spoil
    "half": without the |dV|^2 / 2 term, "half_w": without dw^2 / 2.  max |got - exact| / max |exact| per class of cells and on "centre", and "size" as RestCase.errors"""
    s, err, top, res = HEAT_SHARE, {}, 0.0, []
    for g, G, x, o in zip(rc.grids, rc.G, rc.ins, outs):
        V2 = np.sum(rc.winds.wind(G.C[G.cells]) ** 2, -1)[..., None]
        w = x["w"][G.cells]
        wp = w - HEAT_W0
        want = x["delp"][G.cells] * ((s if spoil == "half" else s - 0.5 * s * s) * V2 + s * wp * (w if spoil == "half_w" else w - 0.5 * s * wp))
        got = np.asarray(o["heat_source"], dtype=np.float64)[G.cells][..., : rc.nz]
        require(np.all(np.isfinite(got)), "non-finite heat")
        top = max(top, float(np.abs(want).max()))
        res.append((cell_classes(G), near_centre(G, G.C[G.cells]), got, want))
    for cls, centre, got, want in res:
        for c, m in cls.items():
            _worst(err, c, (got - want)[m] / top)
        _worst(err, "centre", (got - want)[centre & cls["interior"]] / top)
        _worst(err, "size", got[cls["interior"]] / top)
    return err


SPONGE_HEAT_LEVELS = (0, 1, 2)  # d_con is off there and w is damped in one pass


def sponge_heat_config():
    """the default configuration (n_sponge 48, nord 3, d_con = 1, ke_bg = 0) on five levels"""
    return dict(_DEFAULTS, d_con=1.0, ke_bg=0.0)


def sponge_heat_errors(rc, outs, spoil=None):
    """heat_source of d_sw on heat_case under the default sponge.  On levels 0 - 2 the column's d_con is 0, so the wind heat is off although the wind is
    damped, and what is left is the heat of w alone, s_k w' (w - s_k w' / 2) with s_k = (damp_w da_min_c lam) of SPONGE_TABLE -- NOT weighted by delp: FV3's
    d_sw multiplies by delp inside the block that d_con > 1e-5 guards, and adds the level's heat to heat_source under the global d_con.  Per level k of
    those: "k.centre", "k.interior", "k.edge", "k.corner" (max |got - exact| / max |exact|) and "k.size"; levels 3 - 4 (order 2, wind heat on: no closed
    form) "k.level", the largest |heat| of the interior over level 0's largest exact heat, recorded.  spoil "wind_on": the wind heat delp (s - s^2 / 2) |V|^2
    (s the vorticity's share) left on at the sponge levels; "delp": the heat of w weighted by delp"""
    err, res, nz = {}, [], rc.nz
    top = np.zeros(nz)
    for g, G, x, o in zip(rc.grids, rc.G, rc.ins, outs):
        w = x["w"][G.cells]
        wp = w - HEAT_W0
        sw = np.array([damping_factor("w", k, g, rc.lam) for k in range(nz)])
        want = sw * wp * (w - 0.5 * sw * wp)
        if spoil == "delp":
            want = want * x["delp"][G.cells]
        if spoil == "wind_on":
            sv = np.array([damping_factor("vort", k, g, rc.lam) for k in range(nz)])
            want = want + x["delp"][G.cells] * (sv - 0.5 * sv * sv) * np.sum(rc.winds.wind(G.C[G.cells]) ** 2, -1)[..., None]
        got = np.asarray(o["heat_source"], dtype=np.float64)[G.cells][..., :nz]
        require(np.all(np.isfinite(got)), "non-finite heat")
        top = np.maximum(top, np.abs(want).max((0, 1)))
        res.append((cell_classes(G), near_centre(G, G.C[G.cells]), got, want))
    for cls, centre, got, want in res:
        for k in range(nz):
            if k in SPONGE_HEAT_LEVELS:
                for c, m in cls.items():
                    _worst(err, f"{k}.{c}", (got - want)[..., k][m] / top[k])
                _worst(err, f"{k}.centre", (got - want)[..., k][centre & cls["interior"]] / top[k])
                _worst(err, f"{k}.size", got[..., k][cls["interior"]] / top[k])
            else:
                _worst(err, f"{k}.level", got[..., k][cls["interior"]] / top[0])
    return err


def measure_sponge_heat(shape):
    n, layout, ranks = ac.SHAPES[shape]
    part, grids, doms, c = ac.make(n, layout, ranks, DAMP_NZ)
    rc = heat_case(grids, c.RADIUS)
    return sponge_heat_errors(rc, oracle_rest(doms, ac.dyn_config(n, layout, DAMP_NZ, **sponge_heat_config()), rc))


def measure_heat(shape):
    n, layout, ranks = ac.SHAPES[shape]
    part, grids, doms, c = ac.make(n, layout, ranks, DAMP_NZ)
    rc = heat_case(grids, c.RADIUS)
    cfg = ac.dyn_config(n, layout, DAMP_NZ, **heat_config(grids[0], rc.lam))
    return heat_errors(rc, oracle_rest(doms, cfg, rc))


class Del2Case:
    """del2_cubed on q = 1 + amp_k P_3 (five levels, amp as RestCase): every pass multiplies the harmonic part by 1 - cd lam, cd = DEL2_CD da_min"""

    def __init__(self, grids, a, nz=DAMP_NZ):
        self.rc = RestCase(grids, a, "mass", nz=nz)
        self.grids, self.G, self.nz = grids, self.rc.G, nz
        self.cd = DEL2_CD * grids[0].da_min
        self.ins = [1.0 + self.rc.amp * self.rc.h.P(G.C)[..., None] for G in self.G]

    def errors(self, outs, nmax, spoil=None):
        """max |change - exact change| / max |exact change| per class of cells, on "centre", and "size"; spoil "passes": one pass too few"""
        keep = (1.0 - self.cd * self.rc.lam) ** (min(3, nmax) - (1 if spoil == "passes" else 0))
        err, res, top = {}, [], 0.0
        for G, x, o in zip(self.G, self.ins, outs):
            got = np.asarray(o, dtype=np.float64)[G.cells][..., : self.nz] - x[G.cells]
            want = (keep - 1.0) * (x[G.cells] - 1.0)
            require(np.all(np.isfinite(got)), "non-finite field")
            top = max(top, float(np.abs(want).max()))
            res.append((cell_classes(G), near_centre(G, G.C[G.cells]), got, want))
        for cls, centre, got, want in res:
            for c, m in cls.items():
                _worst(err, c, (got - want)[m] / top)
            _worst(err, "centre", (got - want)[centre & cls["interior"]] / top)
            _worst(err, "size", got[cls["interior"]] / top)
        return err


def measure_del2(shape):
    from fv3_oracle import nh as o_nh

    n, layout, ranks = ac.SHAPES[shape]
    part, grids, doms, c = ac.make(n, layout, ranks, DAMP_NZ)
    d2 = Del2Case(grids, c.RADIUS)
    out = {}
    for nmax in (1, 2, 3):
        qs = [x.copy() for x in d2.ins]
        for D, q in zip(doms, qs):
            o_nh.del2_cubed(D, q, d2.cd, nmax)
        out[f"nmax{nmax}"] = d2.errors(qs, nmax)
    return out


HEATING_FACTOR = 2.0e-3  # delt_time_factor: the limit is 0.1, 0.5, 1, 1, .. times this, by level


def heating_case(G, c, nz=DAMP_NZ):
    """apply_diffusive_heating is pointwise: (inputs [i, j, nz] as smooth functions of position, the exact pt).  dT = heat / (cv delp) runs from -3 to 3 times
    the limit, so every level has limited and free points of both signs; pkz = (rdg delp pt / delz)^(cappa / (1 - cappa)) from the gas law"""
    p = G.C
    f = [1.0 + 0.3 * ac._wave(p, ac.K_PT, 0.4 * k) / 1.5 for k in range(nz)]
    x = {"delp": np.stack([1000.0 * (1.0 + k) * f[k] for k in range(nz)], -1), "pt": ac.scalar_field("pt", p, nz),
         "cappa": np.stack([c.KAPPA * (1.0 - 0.05 * ac._wave(p, ac.K_QC, 0.2 * k) / 1.5) for k in range(nz)], -1)}
    x["delz"] = -x["delp"] / c.GRAV * c.RDGAS * x["pt"] / np.stack([3.0e4 * (1.0 + k) for k in range(nz)], -1)  # (a layer near 3e4 (1 + k) Pa)
    lim = HEATING_FACTOR * np.array([0.1, 0.5] + [1.0] * (nz - 2))
    x["heat_source"] = 3.0 * lim * c.CV_AIR * x["delp"] * np.stack([ac._wave(p, ac.K_W, 0.9 * k) / 1.5 for k in range(nz)], -1)
    dT = x["heat_source"] / (c.CV_AIR * x["delp"])
    pkz = (c.RDG * x["delp"] / x["delz"] * x["pt"]) ** (x["cappa"] / (1.0 - x["cappa"]))
    dpt = np.sign(dT) * np.minimum(lim, np.abs(dT)) / pkz
    return x, x["pt"] + dpt, dpt


def heating_error(G, x, want, dpt, got, nz=DAMP_NZ):
    """max |pt - exact| over the bound 4 eps |pt| + 32 eps |dpt| -- one rounding of the sum, a few of the quotient, exp and log -- in eps of got's type"""
    got = np.asarray(got)
    eps = float(np.finfo(got.dtype).eps)
    bound = 4.0 * eps * np.abs(want[G.cells]) + 32.0 * eps * np.abs(dpt[G.cells])
    d = np.abs(got.astype(np.float64)[G.cells][..., :nz] - want[G.cells])
    require(np.all(np.isfinite(d)), "non-finite pt")
    return float((d / bound).max())


def measure_damping(shapes=None):
    """the oracle's figures of pins 10 - 14: {pin: {shape: ...}}"""
    out = {"pin10": {}, "pin11": {}, "pin12": {}, "pin12_rotation": {}, "pin13": {}, "pin14_heat": {}, "pin14_sponge_heat": {}, "pin14_del2": {}}
    for shape in shapes or ac.SHAPES:
        out["pin10"][shape] = measure_divergence(shape)
        out["pin11"][shape] = measure_c_sw(shape)
        out["pin12"][shape] = {run: measure_divdamp(shape, run) for run in DIVDAMP_SHAPES[shape]}
        out["pin13"][shape] = {kind: measure_rest(shape, kind) for kind in ("mass", "fields")}
        out["pin14_heat"][shape], out["pin14_del2"][shape] = measure_heat(shape), measure_del2(shape)
        out["pin14_sponge_heat"][shape] = measure_sponge_heat(shape)
        if shape == "c24":
            out["pin12_stretched"] = {"c12_stretched": {STRETCHED_RUN: measure_stretched()}}
            out["pin12_rotation"][shape] = {run: measure_divdamp(shape, run, rotation_only=True) for run in ("nord0", "nord2")}
            out["pin13"][shape]["fields_no_sponge"] = measure_rest(shape, "fields", n_sponge=-1)
            out["pin13"][shape]["fields_nord1"] = measure_rest(shape, "fields", nord=1)
            out["pin13"][shape]["mass_nord1"] = measure_rest(shape, "mass", nord=1)
        print(shape, out["pin10"][shape])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# pin 11: the half step of c_sw on the rotation
# ---------------------------------------------------------------------------------------------------------------------------
CSW_SCALARS = {"delpc": "delp", "ptc": "pt", "omga": "w"}


class CswCase(ac.DswCase):
    """c_sw at dt2 = dt / 2 (dt the Courant number of dyn_dt) on solid-body rotation: u, v analytic, delp, pt, w the smooth fields of DswCase.  delpc, ptc and
    omga are the fields at the departure points of the half step; (uc, vc)(dt2) - (uc, vc)(0) is dt2 x the projection of -(zeta + f) k x V - grad K (DswCase.tendency)
    on the cross-face directions of pin 3 (Geometry.e1 / e2)"""

    def __init__(self, n, grids, a, omega_earth, nz=ac.DYN_NZ):
        super().__init__(n, grids, a, omega_earth, nz=nz)
        self.dt2 = 0.5 * self.dt
        self.ins = [{k: x[k] for k in ("delp", "pt", "u", "v", "w")} for x in self.ins]

    def errors(self, half, zero, way=1.0):
        """half / zero: the outputs of c_sw at dt2 and at 0.  {"delpc", "ptc", "omga": max |got - exact| / SCALAR_SCALE over the cells (way = -1: against the
        fields turned the wrong way); "class0" .. "class2": max |wind change / dt2 - exact tendency| / max |exact tendency| per class of faces (face_classes: uc
        lives on the faces of v, vc on those of u)}"""
        fl, nz = self.flow, self.nz
        err, top = dict.fromkeys(list(CSW_SCALARS) + list(FACE_KEYS.values()), 0.0), 0.0
        res = []
        for G, a, b in zip(self.G, half, zero):
            back = fl.rotate_back(G.C[G.cells], way * self.dt2)
            for out, name in CSW_SCALARS.items():
                got = np.asarray(a[out], dtype=np.float64)[G.cells][..., :nz]
                require(np.all(np.isfinite(got)), f"{out}: non-finite")
                _worst(err, out, (got - ac.scalar_field(name, back, nz)) / ac.SCALAR_SCALE[name])
            cu, cv = ac.face_classes(G)
            for name, S, m, e, cls in (("uc", G.X, G.mx, G.e1(), cv), ("vc", G.Y, G.my, G.e2(), cu)):
                got = (np.asarray(a[name], dtype=np.float64) - np.asarray(b[name], dtype=np.float64))[S][..., :nz] / self.dt2
                want = np.sum(self.tendency(m[S]) * e[S], -1)[..., None]
                require(np.all(np.isfinite(got)), f"{name}: non-finite")
                top = max(top, float(np.abs(want).max()))
                res.append((cls, got - want))
        for cls, d in res:
            seen = np.zeros(cls.shape, int)
            for c, key in FACE_KEYS.items():
                _worst(err, key, d[cls == c] / top)
                seen += cls == c
            require(np.all(seen == 1), "a face in no class or in two")
        return err


def measure_c_sw(shape):
    n, layout, ranks = ac.SHAPES[shape]
    part, grids, doms, c = ac.make(n, layout, ranks, ac.DYN_NZ)
    cc = CswCase(n, grids, c.RADIUS, c.OMEGA)
    return {"dt2": cc.dt2, **cc.errors(oracle_c_sw(doms, cc.ins, cc.dt2), oracle_c_sw(doms, cc.ins, 0.0))}


def _flat(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from _flat(v, f"{prefix}{k} ")
        else:
            yield prefix + k, v


def stale_entries(rec):
    """the C24 entries of pins 10 - 13 re-measured with the oracle: those further than 1 % from ``rec`` (round-off figures, below 1e-12, are not compared)"""
    bad = []
    for pin, d in measure_damping(("c24",)).items():
        for shape in d:
            want = dict(_flat(rec[pin][shape]))
            for k, v in _flat(d[shape]):
                if max(abs(v), abs(want[k])) >= 1e-12 and abs(v - want[k]) > 0.01 * abs(want[k]):
                    bad.append(f"{pin} {shape} {k}: {v} now, {want[k]} recorded")
    return bad
