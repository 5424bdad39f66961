"""ORACLE (test side only, not a test module) of the cell evaluate and integrate (DoFs.evaluate / DoFs.integrate on the host,
Operator.evaluate / Operator.integrate on the device): an independent statement of

    evaluate   u_h(x_q) [cell, qz, qy, qx]  and  grad u_h(x_q) [cell, component, qz, qy, qx]
    integrate  b_i = sum_K sum_q w_q h_K^3 ( v_q phi_i(x_q) + V_q . grad phi_i(x_q) )   through Ch^T, constrained rows 0

over the tensor rule QGauss(n_q)^3 per leaf.  numpy and oracle/mgoracle.py only, nothing from the product: the rule comes from
numpy.polynomial.legendre.leggauss, the Lagrange basis and its derivative are tabulated directly at the points
(mgoracle.lagrange_eval), value, gradient and load of a leaf are ONE tensor contraction each, written as the definition (one einsum
over all seven indices; no staged sweeps and no sum factorisation of its own: with optimize=True numpy may order the contraction, which
test_cell_values_host.py holds against optimize=False, the plain seven-fold loop), the nodal values are Level.Ch @ x on cell_dofs (so
the hanging entries of x are never used) and the load goes through Level.Ch.T.  No coefficient and no sigma anywhere.

integrate(..., absolute=True) is the size of the inputs of a row: the same sums with |data|, |phi_i|, |grad phi_i| and |Ch|, the bound
B_i of the device and host tests (a bound on what is added, not on a sum that may cancel).

Layouts are those of include/mgamd.h: points [cell, qz, qy, qx, 3], values [cell, qz, qy, qx], gradients [cell, component, qz, qy, qx]."""
import numpy as np
from numpy.polynomial.legendre import leggauss

import mgoracle as mg


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


def tabulate(cells, n_q, f, grad_f=None):
    """f (and the three components of grad_f) at the points, in the layouts above"""
    X = np.moveaxis(quadrature_points(cells, n_q), -1, 0)
    v = np.ascontiguousarray(np.broadcast_to(f(*X), X[0].shape))
    if grad_f is None:
        return v
    return v, np.ascontiguousarray(np.stack([np.broadcast_to(c, X[0].shape) for c in grad_f(*X)], axis=1))


def shape(space, n_q):
    """(V, D)[q, a] = phi_a(x_q), phi_a'(x_q) on the reference interval"""
    return mg.lagrange_eval(space.fe.nodes, rule(n_q)[0])


def evaluate(space, x, n_q, optimize=True):
    """(u_h [cell, qz, qy, qx], grad u_h [cell, component, qz, qy, qx]) of the vector x (the space's numbering) at the points"""
    n1, nc = space.p + 1, len(space.cells)
    V, D = shape(space, n_q)
    nodal = space.Ch @ np.asarray(x, dtype=float)
    loc = nodal[space.cell_dofs].reshape(nc, n1, n1, n1)  # [cell, c (z), b (y), a (x)]
    h = cell_h(space.cells)[:, None, None, None]
    u = np.einsum("ncba,zc,yb,xa->nzyx", loc, V, V, V, optimize=optimize)
    g = np.stack([np.einsum("ncba,zc,yb,xa->nzyx", loc, V, V, D, optimize=optimize) / h,
                  np.einsum("ncba,zc,yb,xa->nzyx", loc, V, D, V, optimize=optimize) / h,
                  np.einsum("ncba,zc,yb,xa->nzyx", loc, D, V, V, optimize=optimize) / h], axis=1)
    return u, g


def integrate(space, values, gradients, n_q, absolute=False, keep_dirichlet=False, optimize=True):
    """the load vector (the space's numbering) of values [cell, qz, qy, qx] and/or gradients [cell, component, qz, qy, qx] (either may
    be None); absolute: the sizes of the addends instead (see above); keep_dirichlet: the rows of Dirichlet DoFs are left standing
    (the load of a space without Dirichlet faces: then v^T b = int f v_h for every conforming v_h)"""
    nc = len(space.cells)
    V, D = shape(space, n_q)
    _, wq = rule(n_q)
    Ch = space.Ch
    if absolute:
        V, D, Ch = np.abs(V), np.abs(D), abs(Ch)
    h = cell_h(space.cells)[:, None, None, None]
    W = h ** 3 * (wq[:, None, None] * wq[None, :, None] * wq[None, None, :])[None]
    take = (lambda a: np.abs(np.asarray(a, dtype=float))) if absolute else (lambda a: np.asarray(a, dtype=float))
    loc = np.zeros((nc,) + (space.p + 1,) * 3)  # [cell, c (z), b (y), a (x)]
    if values is not None:
        loc += np.einsum("nzyx,zc,yb,xa->ncba", take(values) * W, V, V, V, optimize=optimize)
    if gradients is not None:
        G = take(gradients)
        loc += np.einsum("nzyx,zc,yb,xa->ncba", G[:, 0] * W / h, V, V, D, optimize=optimize)
        loc += np.einsum("nzyx,zc,yb,xa->ncba", G[:, 1] * W / h, V, D, V, optimize=optimize)
        loc += np.einsum("nzyx,zc,yb,xa->ncba", G[:, 2] * W / h, D, V, V, optimize=optimize)
    F = np.zeros(space.n)
    np.add.at(F, space.cell_dofs, loc.reshape(nc, -1))
    b = Ch.T @ F
    b[space.hanging if keep_dirichlet else space.hanging | space.dirichlet] = 0.0
    return b


# ------------------------------------------------------------------ closed forms for tensor polynomials (no shape function, no quadrature)
# Below the oracle, as in error_norm_oracle.py: what its own tests and the device tests share.  For tensor polynomials f, v
# (polynomial_exactness.Poly3, monomial coefficients) int_K f v is a sum of products of exact 1D integrals of monomials over the
# leaf's intervals (polynomial_exactness.interval_integrals).
def polynomial(degrees, seed):
    """a seeded Poly3 of the given degree per variable (one int or three) with tame coefficients and every top-degree term present"""
    import polynomial_exactness as pe

    d = (degrees,) * 3 if np.isscalar(degrees) else tuple(degrees)
    shape_ = tuple(t + 1 for t in d)
    c = np.random.default_rng(seed).uniform(0.25, 1.0, shape_) * np.random.default_rng(seed + 1).choice([-1.0, 1.0], shape_)
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape_], indexing="ij")
    return pe.Poly3(c / (1.0 + i + j + k))


class Products:
    """sum over the leaves of int_K f v for Poly3s of at most `degree` per variable, the 1D integrals once per interval"""

    def __init__(self, degree):
        import polynomial_exactness as pe
        from numpy.polynomial import Polynomial

        mono = [Polynomial.basis(i) for i in range(degree + 1)]
        self.n, self.axis = degree + 1, pe._Axis(mono, mono)

    def integral(self, cells, f, v):
        cf = np.pad(f.c, [(0, self.n - s) for s in f.c.shape])
        cv = np.pad(v.c, [(0, self.n - s) for s in v.c.shape])
        total = 0.0
        for (l, i, j, k) in cells:
            Mx, My, Mz = self.axis(l, i)[0], self.axis(l, j)[0], self.axis(l, k)[0]
            total += np.einsum("ijk,lmn,il,jm,kn->", cf, cv, Mx, My, Mz, optimize=True)
        return float(total)

    def source(self, cells, f, v):
        """int f v"""
        return self.integral(cells, f, v)

    def divergence_form(self, cells, F, v):
        """int F . grad v, F three Poly3s"""
        return sum(self.integral(cells, F[axis], v.deriv(axis)) for axis in range(3))


def addends(space):
    """per DoF of the space, how many leaves add into its row: the leaves that gather it, directly or through a hanging node"""
    pattern = (abs(space.Ch) > 0).astype(np.int64).tocsr()
    count = np.zeros(space.n, np.int64)
    for ci in range(len(space.cells)):
        rows = np.unique(space.cell_dofs[ci])
        count[np.unique(pattern[rows].indices)] += 1
    return count


def rows_of_leaf(space, ci):
    """the DoFs (boolean, the space's numbering) leaf ci adds into, through hanging nodes included; constrained rows are not among them"""
    pattern = (abs(space.Ch) > 0).tocsr()
    on = np.zeros(space.n, bool)
    on[np.unique(pattern[np.unique(space.cell_dofs[ci])].indices)] = True
    return on & ~(space.hanging | space.dirichlet)
