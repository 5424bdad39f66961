"""ORACLE (test side only, not a test module) of the error norms of Operator.integrate_difference: an independent statement of

    L2      sqrt( sum_q w_q h^3 (u_h - w)^2 )                     H1 seminorm  sqrt( sum_q w_q h^3 |grad u_h - grad w|^2 )
    energy  sqrt( sum_q w_q h^3 ( a |grad u_h - grad w|^2 + sigma (u_h - w)^2 ) )            Linfty  max_q |u_h - w|

per leaf, over the tensor rule QGauss(n_q)^3.  numpy and oracle/mgoracle.py only, nothing from the product: the rule comes from
numpy.polynomial.legendre.leggauss, the nodal values are Level.Ch @ x on cell_dofs (so the hanging entries of x are never used), the
shape functions come from mgoracle.lagrange_eval, and value and gradient at all points of a leaf are ONE full tensor contraction
(no staged sweeps, no sum factorisation).  The spaces are those of error_estimator_oracle.nodal_space (cached), vectors in the numbering of
the product's tables are brought to them with error_estimator_oracle.to_oracle.

Below the oracle: the closed forms its tests and the device tests share.  For tensor polynomials v, w (polynomial_exactness.Poly3)
int_K (v - w)^2 and int_K |grad (v - w)|^2 are sums of products of exact 1D integrals (polynomial_exactness.interval_integrals).

Layouts are those of include/mgamd.h: points [cell, qz, qy, qx, 3], values [cell, qz, qy, qx], gradients [cell, component, qz, qy, qx]."""
import numpy as np
from numpy.polynomial import Polynomial
from numpy.polynomial.legendre import leggauss

import mgoracle as mg
import polynomial_exactness as pe

L2, H1, ENERGY, LINFTY = 0, 1, 2, 3


def rule(n_q):
    """QGauss(n_q) on [0, 1]: points ascending, weights summing to 1"""
    x, w = leggauss(n_q)
    return 0.5 * (x + 1.0), 0.5 * w


def cell_h(cells):
    return np.array([2.0 / (1 << c[0]) for c in cells])


def quadrature_points(cells, n_q):
    """the physical points [cell, qz, qy, qx, 3]: corner + h x_q per coordinate"""
    xq, _ = rule(n_q)
    out = np.zeros((len(cells), n_q, n_q, n_q, 3))
    for ci, (l, i, j, k) in enumerate(cells):
        h = 2.0 / (1 << l)
        out[ci, :, :, :, 0] = (-1.0 + h * i + h * xq)[None, None, :]
        out[ci, :, :, :, 1] = (-1.0 + h * j + h * xq)[None, :, None]
        out[ci, :, :, :, 2] = (-1.0 + h * k + h * xq)[:, None, None]
    return out


def evaluate(space, x, n_q):
    """(u_h [cell, qz, qy, qx], grad u_h [cell, component, qz, qy, qx]) of the vector x (the space's numbering) at the points"""
    n1, nc = space.p + 1, len(space.cells)
    xq, _ = rule(n_q)
    V, D = mg.lagrange_eval(space.fe.nodes, xq)  # [q, a]
    nodal = space.Ch @ np.asarray(x, dtype=float)
    loc = nodal[space.cell_dofs].reshape(nc, n1, n1, n1)  # [cell, c (z), b (y), a (x)]
    h = cell_h(space.cells)[:, None, None, None]
    u = np.einsum("ncba,zc,yb,xa->nzyx", loc, V, V, V, optimize=False)
    g = np.stack([np.einsum("ncba,zc,yb,xa->nzyx", loc, V, V, D, optimize=False) / h,
                  np.einsum("ncba,zc,yb,xa->nzyx", loc, V, D, V, optimize=False) / h,
                  np.einsum("ncba,zc,yb,xa->nzyx", loc, D, V, V, optimize=False) / h], axis=1)
    return u, g


def norms_of(cells, n_q, e, ge, a=None, sigma=0.0):
    """the four per-leaf norms {L2, H1, ENERGY, LINFTY: [cell]} of a difference given at the points: e [cell, qz, qy, qx] and
    ge [cell, component, qz, qy, qx] (None: the L2 and Linfty norms only); a: one coefficient per leaf (None: 1)"""
    _, wq = rule(n_q)
    w3 = wq[:, None, None] * wq[None, :, None] * wq[None, None, :]
    h3 = cell_h(cells) ** 3
    a = np.ones(len(cells)) if a is None else np.asarray(a, dtype=float)
    out = {L2: np.sqrt(h3 * np.sum(w3 * e * e, axis=(1, 2, 3))), LINFTY: np.abs(e).reshape(len(cells), -1).max(axis=1)}
    if ge is not None:
        g2 = h3 * np.sum(w3[None, None] * ge * ge, axis=(1, 2, 3, 4))
        out[H1] = np.sqrt(g2)
        out[ENERGY] = np.sqrt(a * g2 + sigma * out[L2] ** 2)
    return out


def norms(space, x, n_q, w=None, grad_w=None, a=None, sigma=0.0):
    """the four per-leaf norms of u_h - w for the vector x (the space's numbering); w, grad_w: arrays at the points in the layouts above
    or functions of (x, y, z) (grad_w returning the three components); None: zero"""
    u, g = evaluate(space, x, n_q)
    X = np.moveaxis(quadrature_points(space.cells, n_q), -1, 0)
    if callable(w):
        w = w(*X)
    if callable(grad_w):
        grad_w = np.stack([np.broadcast_to(c, X[0].shape) for c in grad_w(*X)], axis=1)
    return norms_of(space.cells, n_q, u - (0.0 if w is None else w), g - (0.0 if grad_w is None else grad_w), a, sigma)


def global_error(per_cell, norm):
    return float(np.max(per_cell)) if norm == LINFTY else float(np.sqrt(np.sum(np.square(per_cell))))


def gaussian_gradient(x, y, z, width=0.1, centre=(-0.5, -0.5, -0.5)):
    """the gradient of mgoracle.gaussian_solution in closed form"""
    g = mg.gaussian_solution(x, y, z, width, centre)
    return tuple(-2.0 * (t - c) / width ** 2 * g for t, c in zip((x, y, z), centre))


# ------------------------------------------------------------------ closed forms for tensor polynomials (no shape function, no quadrature)
def polynomial(degree, seed):
    """a seeded Poly3 of degree `degree` per variable with tame coefficients and every top-degree term present"""
    c = np.random.default_rng(seed).uniform(0.25, 1.0, (degree + 1,) * 3) * np.random.default_rng(seed + 1).choice([-1.0, 1.0], (degree + 1,) * 3)
    i, j, k = np.meshgrid(*[np.arange(degree + 1)] * 3, indexing="ij")
    return pe.Poly3(c / (1.0 + i + j + k))


def difference(v, w):
    n = max(v.c.shape[0], w.c.shape[0])
    pad = lambda c: np.pad(c, [(0, n - s) for s in c.shape])
    return pe.Poly3(pad(v.c) - pad(w.c))


class ClosedForms:
    """int_K d^2 and int_K |grad d|^2 per leaf for Poly3s of at most `degree` per variable, the 1D integrals once per interval"""

    def __init__(self, degree):
        mono = [Polynomial.basis(i) for i in range(degree + 1)]
        self.n, self.axis = degree + 1, pe._Axis(mono, mono)

    def squares(self, cells, d):
        c = np.pad(d.c, [(0, self.n - s) for s in d.c.shape])
        l2, h1 = np.zeros(len(cells)), np.zeros(len(cells))
        for t, (l, i, j, k) in enumerate(cells):
            (Mx, Kx), (My, Ky), (Mz, Kz) = self.axis(l, i), self.axis(l, j), self.axis(l, k)
            form = lambda X, Y, Z: np.einsum("ijk,lmn,il,jm,kn->", c, c, X, Y, Z, optimize=True)
            l2[t] = form(Mx, My, Mz)
            h1[t] = form(Kx, My, Mz) + form(Mx, Ky, Mz) + form(Mx, My, Kz)
        return l2, h1

    def norms(self, cells, d, a=None, sigma=0.0):
        l2, h1 = self.squares(cells, d)
        a = np.ones(len(cells)) if a is None else np.asarray(a)
        return {L2: np.sqrt(l2), H1: np.sqrt(h1), ENERGY: np.sqrt(a * h1 + sigma * l2)}


def gradient_of(w):
    return lambda x, y, z: tuple(w.deriv(axis)(x, y, z) for axis in range(3))
