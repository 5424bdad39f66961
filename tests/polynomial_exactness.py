"""The classical patch test, stated for this project: what a conforming Q_p space on an octree must reproduce exactly, with
references that cost O(n) and come from mathematics alone.  Not a test module and not a conftest; numpy only, nothing from oracle/.

Three identities (u, v, w in Q_p, u_h the nodal values at DoFs.node_positions()):

  1. rows    u harmonic:  vmult(u)[i] - rhs_dirichlet(g = u)[i] = 0  on every free row i whose node lies on no natural face, on
             any octree with hanging nodes (Q_p is conforming there, so C u_free + g^ is u itself).  With a mass term the row is
             sigma (C^T M u_h)[i], which vmult_mass(u) and rhs_dirichlet(u, True) - rhs_dirichlet(u, False) supply.  On a natural
             face the row is the flux load of a d_n u (rhs_boundary_flux, where that is constant on the face).
  2. Gram    v_h^T A w_h = sum_cells a_c int_c grad v . grad w + sigma int v w + sum_f beta_f int_f v w, and likewise
             v^T rhs_boundary_flux(q) = sum_f q_f int_f v,  v^T rhs(0) = int v,  v^T vmult_mass(w) = int v w.  The right-hand sides
             are sums of products of 1D polynomial integrals over dyadic intervals: no shape function, no quadrature, no
             constraint matrix.
  3. transfers   prolongate_and_add(0, interp_coarse u) = interp_fine u on the fine free DoFs for u in Q_{p_coarse}.

The 1D integrals: every factor is a numpy.polynomial series; on an interval [x0, x1] both factors are expanded about the midpoint
(derivatives of the series, no change of basis), multiplied as numpy Polynomials in t = x - midpoint and integrated with
Polynomial.integ over [-h/2, h/2], on pieces no longer than 1/4.  The odd powers drop out, the even ones decay, and the integral
carries a few ulp of int |v w|.

RHO turns the project's norm-wise operator tolerance into a row-wise one:
    |r_i| <= TOL sum_j |A_ij| |u_j| <= TOL RHO d_i max|u|,   RHO >= max_i sum_j |A_ij| / A_ii over the free rows.
For the Laplacian under six Dirichlet faces the ratio is 2.08, 3.66, 5.53, 7.54, 8.20, 9.68, 11.06 at p = 1 ... 7, which would
give 12.  Rows on natural faces exceed that at p = 7: 12.22 under M1, 12.09 under M2, 12.29 under M0 with sigma = 7.5, 12.20 with a
convective face.  So RHO is 13, the ceiling of what is measured over every problem variant; tests/test_polynomial_exactness_host.py
recomputes the ratio for all of them and asserts it.

Out of scope: the time stepper.  vmult_mass drops the source on Dirichlet nodes (include/mgamd.h) and only constant fluxes exist,
so no polynomial-in-space solution with curved content is exact there; local smoothing (the edge matrices obey other
identities) and simulated ranks are left to their own tests."""
import math

import numpy as np
from numpy.polynomial import Legendre, Polynomial

RHO = 13


# ------------------------------------------------------------------ polynomials in three variables
class Poly3:
    """c[i, j, k] x^i y^j z^k with an accurate evaluation of its own (fn) where one exists"""

    def __init__(self, c, fn=None):
        self.c, self.fn = np.asarray(c, dtype=float), fn

    def __call__(self, x, y, z):
        if self.fn is not None:
            return self.fn(np.asarray(x, dtype=float), np.asarray(y, dtype=float), np.asarray(z, dtype=float))
        return np.polynomial.polynomial.polyval3d(x, y, z, self.c)

    def deriv(self, axis, m=1):
        return Poly3(np.polynomial.polynomial.polyder(self.c, m, axis=axis) if self.c.shape[axis] > m else np.zeros((1, 1, 1)))

    def laplacian(self):
        out = np.zeros(self.c.shape)
        for axis in range(3):
            d = self.deriv(axis, 2).c
            out[tuple(slice(0, s) for s in d.shape)] += d
        return Poly3(out)

    def on_face(self, f):
        """the coefficients [., .] in the two remaining variables on face f = 2 axis + side of the cube"""
        axis, x = f >> 1, (1.0 if f & 1 else -1.0)
        return np.tensordot(self.c, x ** np.arange(self.c.shape[axis]), axes=([axis], [0]))


def _re_power(p):
    """coefficients [a, b] of Re((s + i t)^p) = sum over even k of C(p, k) (-1)^(k / 2) s^(p - k) t^k"""
    c = np.zeros((p + 1, p + 1))
    for k in range(0, p + 1, 2):
        c[p - k, k] = math.comb(p, k) * (-1) ** (k // 2)
    return c


def harmonic(p, x_independent=False):
    """u = Re((x+iy)^p) z + Re((y+iz)^p) x + Re((z+ix)^p) y + 0.3 xyz + 0.1: every term harmonic, degree exactly p in each variable
    (p >= 1).  x_independent: Re((y+iz)^p) + 0.1, for coefficients layered in x."""
    assert p >= 1
    n, r = p + 1, _re_power(p)
    c = np.zeros((n, n, n))
    c[0, 0, 0] = 0.1
    if x_independent:
        c[0, :, :] += r
        return Poly3(c, lambda x, y, z: ((y + 1j * z) ** p).real + 0.1)
    c[:, :, 1] += r  # Re((x+iy)^p) z
    c[1, :, :] += r  # Re((y+iz)^p) x
    c[:, 1, :] += r.T  # Re((z+ix)^p) y: z is the first variable of the pair
    c[1, 1, 1] += 0.3
    return Poly3(c, lambda x, y, z: ((x + 1j * y) ** p).real * z + ((y + 1j * z) ** p).real * x + ((z + 1j * x) ** p).real * y
                 + 0.3 * x * y * z + 0.1)


def linear_in_y():
    """u = y + 0.1: harmonic, in Q_p for every p >= 1, with the constant normal derivative -1, +1 on the faces y = -1, +1 and 0 on the
    others, so that under a constant coefficient every natural face takes part in identity 1 through rhs_boundary_flux"""
    c = np.zeros((2, 2, 2))
    c[0, 0, 0], c[0, 1, 0] = 0.1, 1.0
    return Poly3(c, lambda x, y, z: y + 0.1 + 0.0 * x)


def row_function(p, kind):
    """the harmonic polynomial of identity 1 by kind: "full", "x_independent" (coefficients layered in x), "linear_y" (flux loads)"""
    return linear_in_y() if kind == "linear_y" else harmonic(p, kind == "x_independent")


def constant_normal_flux(u, f):
    """d_n u on face f if it is constant there, else None (n the outward normal)"""
    d = u.deriv(f >> 1).on_face(f)
    rest = d.copy()
    rest[0, 0] = 0.0
    if np.any(rest != 0.0):
        return None
    return float(d[0, 0]) * (1.0 if f & 1 else -1.0)


# ------------------------------------------------------------------ tensor bases of Q_p
class Basis:
    """functions f[0][a](x) f[1][b](y) f[2][c](z) for the rows (a, b, c) of idx; f[d]: the 1D series of axis d"""

    def __init__(self, f, idx):
        self.f, self.idx = tuple(list(fd) for fd in f), np.asarray(idx, dtype=np.int64).reshape(-1, 3)

    def __len__(self):
        return len(self.idx)

    def subset(self, rows):
        return Basis(self.f, self.idx[np.asarray(rows)])

    def __call__(self, x, y, z):
        """values [function, point]"""
        v = [np.array([s(np.asarray(t, dtype=float)) for s in fd]) for fd, t in zip(self.f, (x, y, z))]
        return v[0][self.idx[:, 0]] * v[1][self.idx[:, 1]] * v[2][self.idx[:, 2]]

    def coefficients(self):
        """[function, i, j, k] in powers of x, y, z"""
        n = max(s.degree() for fd in self.f for s in fd) + 1
        mono = [np.array([np.pad(s.convert(kind=Polynomial).coef, (0, n))[:n] for s in fd]) for fd in self.f]
        return np.einsum("ni,nj,nk->nijk", mono[0][self.idx[:, 0]], mono[1][self.idx[:, 1]], mono[2][self.idx[:, 2]])

    def max_abs(self):
        """an upper bound of max |v| on the cube per function: the product of the 1D maxima on a fine grid plus the end points"""
        t = np.linspace(-1.0, 1.0, 2001)
        m = [np.array([np.abs(s(t)).max() for s in fd]) for fd in self.f]
        return m[0][self.idx[:, 0]] * m[1][self.idx[:, 1]] * m[2][self.idx[:, 2]]


class Factored:
    """factor(x) base(x) as a 1D function: evaluated as the product, so a zero of the factor is an exact zero; differentiated and
    integrated through the product series"""

    def __init__(self, factor, base):
        self.factor, self.base, self.series = factor, base, factor * base

    def __call__(self, x):
        return self.factor(x) * self.base(x)

    def deriv(self, m=1):
        return self.series.deriv(m) if m else self

    def degree(self):
        return self.series.degree()

    def convert(self, kind):
        return self.series.convert(kind=kind)


def legendre_basis(p, vanishing=0):
    """all (p+1)^3 products of 1D Legendre polynomials of degree <= p.  vanishing: 6-bit mask of faces f = 2 axis + side on which
    every function is zero, by a factor (1 + x) for side 0 and (1 - x) for side 1 whose degree is taken from the budget of p"""
    f = []
    for axis in range(3):
        factor, budget = Legendre([1.0]), p
        if (vanishing >> (2 * axis)) & 1:
            factor, budget = factor * Legendre([1.0, 1.0]), budget - 1
        if (vanishing >> (2 * axis + 1)) & 1:
            factor, budget = factor * Legendre([1.0, -1.0]), budget - 1
        assert budget >= 0, "degree too low to vanish on both faces of an axis"
        f.append([Factored(factor, Legendre.basis(k)) for k in range(budget + 1)])
    idx = [(a, b, c) for c in range(len(f[2])) for b in range(len(f[1])) for a in range(len(f[0]))]
    return Basis(f, idx)


def chosen(basis, n, seed):
    """all functions if there are at most n, else a seeded subset of n that always holds the top-degree product and the three
    functions of top degree in one variable alone"""
    if len(basis) <= n:
        return basis
    top = [len(fd) - 1 for fd in basis.f]
    must = [tuple(top), (top[0], 0, 0), (0, top[1], 0), (0, 0, top[2])]
    rows = [i for i, t in enumerate(map(tuple, basis.idx)) if t in must]
    rest = [i for i in range(len(basis)) if i not in rows]
    rows += list(np.random.default_rng(seed).choice(rest, n - len(rows), replace=False))
    return basis.subset(sorted(rows))


def bases(p, mask):
    """(V, W) of a Gram matrix under the mask of Dirichlet faces: W all (p+1)^3 Legendre products for p <= 3, else a seeded 64 of
    them with the top-degree product and the three pure degree-p functions; V the same or, under a mask, the functions that vanish
    on its faces.  None where the degree leaves no such function (both faces of an axis need p >= 2)."""
    W = chosen(legendre_basis(p), 64, p)
    if mask == 0:
        return W, W
    if any(((mask >> (2 * ax)) & 3) == 3 for ax in range(3)) and p < 2:
        return None
    return chosen(legendre_basis(p, mask), 64, p), W


# ------------------------------------------------------------------ exact 1D integrals over dyadic intervals
def _taylor(series, m, n):
    """[function, k]: coefficient of t^k of s(m + t), from the derivatives of the series"""
    return np.array([[s.deriv(k)(m) / math.factorial(k) if k <= s.degree() else 0.0 for k in range(n)] for s in series])


def interval_integrals(fv, fw, x0, x1):
    """(M, K): M[a, b] = int fv[a] fw[b], K[a, b] = int fv[a]' fw[b]' over [x0, x1].  An interval longer than 1/4 is halved until its
    pieces are not: about the midpoint of a long interval the powers of t carry the large, alternating coefficients of the
    monomial form (int P_6^2 over [-1, 1] loses three digits that way), on a short one they decay and nothing cancels"""
    if x1 - x0 > 0.25:
        left, right = interval_integrals(fv, fw, x0, 0.5 * (x0 + x1)), interval_integrals(fv, fw, 0.5 * (x0 + x1), x1)
        return left[0] + right[0], left[1] + right[1]
    m, h = 0.5 * (x0 + x1), 0.5 * (x1 - x0)
    n = max(s.degree() for s in list(fv) + list(fw)) + 1
    tv, tw = _taylor(fv, m, n), _taylor(fw, m, n)
    k = np.arange(1, n)
    dv, dw = np.pad(tv[:, 1:] * k, ((0, 0), (0, 1))), np.pad(tw[:, 1:] * k, ((0, 0), (0, 1)))

    def integrate(a, b):
        out = np.zeros((len(a), len(b)))
        for i in range(len(a)):
            for j in range(len(b)):
                F = (Polynomial(a[i]) * Polynomial(b[j])).integ()
                out[i, j] = F(h) - F(-h)
        return out

    return integrate(tv, tw), integrate(dv, dw)


class _Axis:
    """the integrals of one axis per distinct interval (level, index)"""

    def __init__(self, fv, fw):
        self.fv, self.fw, self.done = fv, fw, {}

    def __call__(self, level, index):
        key = (int(level), int(index))
        if key not in self.done:
            h = 2.0 / (1 << key[0])
            self.done[key] = interval_integrals(self.fv, self.fw, -1.0 + h * key[1], -1.0 + h * (key[1] + 1))
        return self.done[key]


def _end_values(series, side):
    return np.array([s(1.0 if side else -1.0) for s in series])


def gram(cells, a_of_cell, sigma, beta, basis_v, basis_w):
    """G[v, w] = sum_cells a_c int_c grad v . grad w + sigma int v w + sum_f beta[f] int_f v w over the leaves
    cells = (level, i, j, k[, ...]) (Triangulation.cells()), a_of_cell one value per leaf (Triangulation.coefficient()) or None"""
    lev, ijk = np.asarray(cells[0], dtype=np.int64), [np.asarray(c, dtype=np.int64) for c in cells[1:4]]
    a = np.ones(len(lev)) if a_of_cell is None else np.asarray(a_of_cell, dtype=float)
    beta = np.zeros(6) if beta is None else np.asarray(beta, dtype=float)
    axes = [_Axis(basis_v.f[d], basis_w.f[d]) for d in range(3)]
    iv, iw = basis_v.idx, basis_w.idx
    ends = [[np.outer(_end_values(basis_v.f[d], s), _end_values(basis_w.f[d], s))[np.ix_(iv[:, d], iw[:, d])] for s in (0, 1)]
            for d in range(3)]
    G = np.zeros((len(basis_v), len(basis_w)))
    for c in range(len(lev)):
        M, K = zip(*[tuple(t[np.ix_(iv[:, d], iw[:, d])] for t in axes[d](lev[c], ijk[d][c])) for d in range(3)])
        G += a[c] * (K[0] * M[1] * M[2] + M[0] * K[1] * M[2] + M[0] * M[1] * K[2])
        if sigma != 0.0:
            G += sigma * M[0] * M[1] * M[2]
        for d in range(3):
            for s in (0, 1):
                if beta[2 * d + s] != 0.0 and ijk[d][c] == (((1 << lev[c]) - 1) if s else 0):
                    G += beta[2 * d + s] * ends[d][s] * M[(d + 1) % 3] * M[(d + 2) % 3]
    return G


_ONE = Basis(([Legendre([1.0])],) * 3, [(0, 0, 0)])
_ROOT = (np.zeros(1, np.int64),) * 4


def mass_gram(basis_v, basis_w, cells=_ROOT):
    """int v w over the cube (summed over the given leaves)"""
    lev, ijk = np.asarray(cells[0], dtype=np.int64), [np.asarray(c, dtype=np.int64) for c in cells[1:4]]
    axes = [_Axis(basis_v.f[d], basis_w.f[d]) for d in range(3)]
    G = np.zeros((len(basis_v), len(basis_w)))
    for c in range(len(lev)):
        M = [axes[d](lev[c], ijk[d][c])[0][np.ix_(basis_v.idx[:, d], basis_w.idx[:, d])] for d in range(3)]
        G += M[0] * M[1] * M[2]
    return G


def integrals(basis, cells=_ROOT):
    """int v over the cube per function"""
    return mass_gram(basis, _ONE, cells)[:, 0]


def face_integrals(basis, q, cells=_ROOT):
    """sum_f q[f] int_{face f} v per function"""
    return gram(cells, np.zeros(len(np.asarray(cells[0]))), 0.0, q, basis, _ONE)[:, 0]


# ------------------------------------------------------------------ a coefficient in layers normal to x
LAYER_PLANES, LAYER_VALUES = (-0.5, 0.0), (1.0, 5.0, 0.2)


def layer_planes(cells):
    """those of LAYER_PLANES that are faces of every leaf: across such a plane only a d_x u has to be continuous, which the
    x-independent harmonic gives.  A mesh that keeps level-1 cells (quadrant 2) has x = 0 alone and so two of the three layers."""
    lev, i = np.asarray(cells[0], dtype=np.int64), np.asarray(cells[1], dtype=np.int64)
    h = 2.0 / (1 << lev)
    x0, x1 = -1.0 + h * i, -1.0 + h * (i + 1)
    return [pl for pl in LAYER_PLANES if not np.any((x0 < pl) & (pl < x1))]


# ------------------------------------------------------------------ rows
def face_dofs(cells, cell_dofs, p, faces):
    """the DoFs that the cells list on the faces of the 6-bit mask `faces`: found from cells() (which cells lie on the face) and
    cell_dofs() ((p+1)^3 entries per cell, x fastest; entries >= 2^32 - 1 are skipped)"""
    lev, ijk = np.asarray(cells[0], dtype=np.int64), [np.asarray(c, dtype=np.int64) for c in cells[1:4]]
    n1 = p + 1
    local = np.arange(n1 ** 3).reshape(n1, n1, n1)  # [c, b, a]: x fastest
    out = []
    for f in range(6):
        if not (faces >> f) & 1:
            continue
        d, side = f >> 1, f & 1
        on = ijk[d] == (((1 << lev) - 1) if side else 0)
        sel = np.take(local, p if side else 0, axis=2 - d).ravel()
        out.append(np.asarray(cell_dofs)[on][:, sel].ravel())
    out = np.unique(np.concatenate(out)) if out else np.zeros(0, np.int64)
    return out[out != 0xFFFFFFFF].astype(np.int64)


def natural_face_plan(u, cells, a_of_cell, dirichlet_faces, robin=(0.0,) * 6):
    """(q, skipped) for identity 1 under a mask: q[f] = a d_n u on the natural faces where that is one constant (the rows there are
    checked with rhs_boundary_flux(q)); skipped: the mask of the natural faces where it is not, and of the convective faces, whose
    rows are left out"""
    lev = np.asarray(cells[0], dtype=np.int64)
    a = np.ones(len(lev)) if a_of_cell is None else np.asarray(a_of_cell, dtype=float)
    q, skipped = np.zeros(6), 0
    for f in range(6):
        if (dirichlet_faces >> f) & 1:
            continue
        flux = constant_normal_flux(u, f)
        on = np.asarray(cells[1 + (f >> 1)], dtype=np.int64) == (((1 << lev) - 1) if f & 1 else 0)
        if flux is None or len(set(a[on])) != 1 or robin[f] != 0.0:
            skipped |= 1 << f
        else:
            q[f] = a[on][0] * flux
    return q, skipped


def checked_rows(free, pos, cells, cell_dofs, p, skipped):
    """the free rows identity 1 is asked of: all but those ON the skipped faces (the basis function of a node off a face vanishes
    on it, hanging nodes included: the parents of a hanging node on a face lie on that face).  Found from cells() and cell_dofs(),
    held against the support points; at most the rows on natural faces are left out, so at least the interior rows remain."""
    free = np.asarray(free, dtype=bool)
    on = np.zeros(len(free), dtype=bool)
    on[face_dofs(cells, cell_dofs, p, skipped)] = True
    by_position = np.zeros(len(free), dtype=bool)
    for f in range(6):
        if (skipped >> f) & 1:
            by_position |= pos[:, f >> 1] == (1.0 if f & 1 else -1.0)
    assert np.array_equal(on & free, by_position & free)
    rows = free & ~on
    interior = free & np.all(np.abs(pos) < 1.0, axis=1)
    assert rows.sum() >= interior.sum() > 0
    return rows, int((rows & ~interior).sum())


def row_residual(au, lift, rows, *loads):
    """(A u - lift - loads)[rows]: zero for a harmonic u in Q_p"""
    r = np.asarray(au, dtype=float) - np.asarray(lift, dtype=float)
    for b in loads:
        r = r - np.asarray(b, dtype=float)
    return r[rows]


def row_figure(r, d, u):
    """max_i |r_i| / (d_i max|u|), d the diagonal on the rows of r"""
    return float(np.max(np.abs(r) / (np.asarray(d) * np.abs(u).max()))) if len(r) else 0.0


def gram_bound(V, d, w_max, tol):
    """per (v, w): tol RHO max|w| sum_i |v_i| d_i, the sum of the row bounds; V[function, row], d on the same rows"""
    return tol * RHO * np.outer(np.abs(V) @ np.asarray(d), np.asarray(w_max))
