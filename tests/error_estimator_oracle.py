"""ORACLE (test side only, not a test module) of the jump error indicator: an independent statement of the definition

    eta_K^2 = (h_K / 24) sum_{F in dK} int_F r_F^2 dS

r_F = a_K d_d u|_K - a_N d_d u|_N on an interior face of axis d (same-level neighbour; one level coarser neighbour evaluated on K's
face; four finer neighbours as the sum over the four quarter faces), r_F = q_f - beta_f u - a_K d_n u on a boundary face f that is not
Dirichlet when q is given, nothing otherwise.

The route differs from the product's on purpose: the nodal values are Level.Ch @ x on cell_dofs, BOTH sides' fluxes are evaluated
with mgoracle.lagrange_eval at the PHYSICAL Gauss points (QGauss(p + 1) per direction, exact for the squared jump of degree 2p) of each
(sub-)face, and the neighbours come from mgoracle._find_leaf.  No mass matrix and no I0 / I1 appears.  Coefficient, mask and beta come
from a physics_oracle.Problem.

nodal_space(leaves, p) is mgoracle.Level without its matrices (the indicator needs the constraint search only), cached; vectors in the
numbering of the product's tables are brought to it with to_oracle(space, keys, x)."""
import numpy as np

import mgoracle as mg
import physics_oracle as po


class NodalSpace(mg.Level):
    """cells, cell_dofs, keys, hanging and Ch of mgoracle.Level; the assembly is skipped"""

    def _assemble(self):
        pass


_spaces = {}


def nodal_space(leaves, p):
    tag = (frozenset(leaves), p)
    if tag not in _spaces:
        _spaces[tag] = NodalSpace(leaves, p)
    return _spaces[tag]


def to_oracle(space, keys, x):
    """the vector x, numbered like `keys` (the product's DoF keys), in the numbering of the space"""
    ext = {tuple(int(v) for v in k): i for i, k in enumerate(keys)}
    assert len(ext) == space.n
    return np.asarray(x, dtype=float)[np.array([ext[tuple(int(v) for v in k)] for k in space.keys], dtype=np.int64)]


_basis = {}


def basis(nodes, xi):
    """lagrange_eval at the reference points xi, remembered: the points of a mesh come from a handful of reference positions"""
    tag = (len(nodes), tuple(np.round(np.atleast_1d(xi), 13)))
    if tag not in _basis:
        _basis[tag] = mg.lagrange_eval(nodes, np.atleast_1d(xi))
    return _basis[tag]


def cell_values(space, nodal, ci, d, xd, e, xe, g, xg):
    """u and d_d u of cell ci at the physical points {x_d = xd} x {x_e in xe} x {x_g in xg}: arrays [len(xe), len(xg)]"""
    l, i, j, k = space.cells[ci]
    h, n1 = 2.0 / (1 << l), space.p + 1
    x0 = (-1.0 + h * i, -1.0 + h * j, -1.0 + h * k)
    U = nodal[space.cell_dofs[ci]].reshape(n1, n1, n1).transpose(2, 1, 0)  # [x, y, z]
    U = np.moveaxis(U, (d, e, g), (0, 1, 2))
    Vd, Dd = basis(space.fe.nodes, (xd - x0[d]) / h)
    Ve, Vg = basis(space.fe.nodes, (xe - x0[e]) / h)[0], basis(space.fe.nodes, (xg - x0[g]) / h)[0]
    # (the normal direction first, then the two tangential ones as matrix products)
    return Ve @ np.tensordot(Vd[0], U, 1) @ Vg.T, Ve @ np.tensordot(Dd[0] / h, U, 1) @ Vg.T


def indicator_squared(space, problem, x, q=None):
    """eta_K^2 per cell of the space (Morton order, the product's) for the vector x in the space's numbering"""
    nodal = space.Ch @ np.asarray(x, dtype=float)
    a = np.ones(len(space.cells)) if problem.coefficient is None else np.array([problem.coefficient[tuple(c)] for c in space.cells])
    index = {c: t for t, c in enumerate(space.cells)}
    xq, wq = space.fe.xq, space.fe.wq
    W = wq[:, None] * wq[None, :]
    eta2 = np.zeros(len(space.cells))
    for ci, (l, i, j, k) in enumerate(space.cells):
        h, ijk = 2.0 / (1 << l), (i, j, k)
        x0 = [-1.0 + h * v for v in ijk]
        total = 0.0
        for f in range(6):
            d, side = f >> 1, f & 1
            e, g = (d + 1) % 3, (d + 2) % 3
            xd = x0[d] + side * h
            n = list(ijk)
            n[d] += 1 if side else -1
            if not 0 <= n[d] < (1 << l):  # a face of the cube
                if q is None or (problem.dirichlet_faces >> f) & 1:
                    continue
                u, du = cell_values(space, nodal, ci, d, xd, e, x0[e] + h * xq, g, x0[g] + h * xq)
                r = q[f] - problem.robin[f] * u - (1.0 if side else -1.0) * a[ci] * du
                total += h * h * np.sum(W * r * r)
                continue
            nb = mg._find_leaf(space.leaves, l, *n)
            if nb is not None:  # the same level or one level coarser: K's whole face
                assert nb[0] >= l - 1
                sub = [(nb, x0[e], x0[g], h)]
            else:  # four finer neighbours: the quarters of K's face
                sub = []
                for c2 in (0, 1):
                    for c1 in (0, 1):
                        m = [0, 0, 0]
                        m[d], m[e], m[g] = 2 * n[d] + (0 if side else 1), 2 * ijk[e] + c1, 2 * ijk[g] + c2
                        fine = mg._find_leaf(space.leaves, l + 1, *m)
                        assert fine is not None and fine[0] == l + 1
                        sub.append((fine, x0[e] + 0.5 * h * c1, x0[g] + 0.5 * h * c2, 0.5 * h))
            for nb, oe, og, hf in sub:
                xe, xg = oe + hf * xq, og + hf * xq
                r = a[ci] * cell_values(space, nodal, ci, d, xd, e, xe, g, xg)[1] - a[index[nb]] * cell_values(space, nodal, index[nb], d, xd, e, xe, g, xg)[1]
                total += hf * hf * np.sum(W * r * r)
        eta2[ci] = h / 24.0 * total
    return eta2


def on(problem, cells):
    """the problem with a named or callable coefficient evaluated on the cells"""
    c = problem.coefficient
    if isinstance(c, str):
        c = po.FIELDS[c]
    if callable(c):
        import dataclasses

        return dataclasses.replace(problem, coefficient=po.field_on(cells, c))
    return problem
