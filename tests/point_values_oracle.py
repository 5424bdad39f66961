"""ORACLE (test side only, not a test module) of point evaluation and point sources (DoFs.locate_points / point_evaluate /
point_integrate on the host, Operator.point_set on the device): an independent statement of

    locate     the leaf of a point of [-1, 1]^3 and its reference coordinate
    evaluate   u_h(x_k) [n]  and  grad u_h(x_k) [3, n]
    integrate  b_i = sum_k ( w_k phi_i(x_k) + W_k . grad phi_i(x_k) )   through Ch^T, constrained rows 0: no quadrature weight, no h^3

numpy and oracle/mgoracle.py only, nothing from the product.  Location is a brute-force box test over space.cells with the integer
rule of include/mgamd.h restated: per coordinate s = (x + 1) 2^14 (one addition in double, an exact scale), c = min(2^15 - 1, floor(s)),
found iff every s lies in [0, 2^15] (NaN is not); the leaf (l, i, j, k) with edge e = 2^(15 - l) holds the point iff i e <= c_x < (i + 1) e
and likewise in y and z -- no Morton key and no search; the reference coordinate is (s - i e) / e.  So a point on an interior face, edge
or vertex belongs to the leaf on its upper side and a point on a face = +1 to the last leaf.  The basis comes from
mgoracle.lagrange_eval(space.fe.nodes, xi), the nodal values are space.Ch @ x on space.cell_dofs (the hanging entries of x are never
used), the load goes through space.Ch.T.  Points that are not found get 0 and add nothing.

absolute=True gives the sizes instead: evaluate the per-point bounds sum_i |phi_i| |u_i| and sum_i |d_c phi_i| |u_i| (|u_i| the
conforming nodal values of the leaf), integrate the per-row bound B_i (|data|, |phi_i|, |grad phi_i|, |Ch|): bounds on what is added,
not on a sum that may cancel, as cell_values_oracle.py does.

absolute="reference" gives THIS ORACLE'S OWN ERROR in the same layout, to be added to a tolerance at full weight.  At the Gauss points
of cell_values_oracle.py no basis function and no derivative vanishes; at caller points they do (phi_a at another node, phi_a' of the
middle node at the centre of a leaf of even degree), and there the tabulated number is not small relative to itself: it is the
residue of the representation error of the nodes (mgoracle's middle node of p = 6 is 0.5 - 1.1e-16, the product's is 0.5) and of the
cancelling sum behind phi_a'.  The model: every difference xi - x_b of the two defining formulas
    phi_a = prod_{b != a} (xi - x_b) / den_a,      phi_a' = sum_{c != a} prod_{b != a, c} (xi - x_b) / den_a
carries an absolute error of 2^-50, four units in the last place of a node in [0.5, 1]: against 40-digit roots of P_p' mgoracle's nodes
are off by up to 1.7 units (p = 6) and their sums x_i + x_{p-i} - 1 reach 4 units (p = 7), the product's own symmetrised nodes by up to
one, and xi itself is exact.  To first order phi_a moves by 2^-50 sum_c prod |xi - x_b| / |den_a| and phi_a' by 2^-50 sum_e sum_c
prod_{b != a, c, e} |xi - x_b| / |den_a|; the latter also covers the rounding of the cancelling sum behind phi_a' (every
|xi - x_b| <= 1).  The sizes are formed once with |phi| and once with |phi| + that error, and the difference is returned.  It is used in ONE place, row_ratio below, for the rows of a load
against THIS oracle.  Every evaluate (whose per-point bounds never vanish at a found point: sum_a |phi_a| >= 1) is held to the plain
bound tol B.  For a load the plain bound is not attainable against this oracle: a row that a point reaches only through small
basis values (1e-4 ... 1e-5 of the largest row's size) still sees the oracle's node error at full size, and the raw ratio err_i / B_i
reaches 2.8e-11 on quadrant 3 at p = 6 for the HOST restatement, whose nodes are right (its middle node is 0.5).  The device tests
therefore also hold the device load against the host restatement, both on the product's nodes, under the plain bound on every row
above noise level (B_i > 1e-12 max_j B_j).

Layouts are those of include/mgamd.h: points [n, 3], cells [n] (-1: not found), reference points [n, 3], values [n], gradients [3, n]."""
import numpy as np

import mgoracle as mg

LMAX = 15


def locate(cells, points):
    """(cell [n] int32, xi [n, 3]) by the box test; cells: the leaves (level, i, j, k) in the order of the space"""
    pts = np.asarray(points, dtype=float).reshape(-1, 3)
    s = (pts + 1.0) * float(1 << (LMAX - 1))
    with np.errstate(invalid="ignore"):
        found = ((s >= 0.0) & (s <= float(1 << LMAX))).all(axis=1)
    c = np.minimum((1 << LMAX) - 1, np.floor(np.where(found[:, None], s, 0.0))).astype(np.int64)
    arr = np.array([tuple(t) for t in cells], dtype=np.int64).reshape(-1, 4)
    e = (1 << (LMAX - arr[:, 0]))
    lo = arr[:, 1:] * e[:, None]
    cell, xi = np.full(len(pts), -1, np.int32), np.zeros((len(pts), 3))
    for k in np.flatnonzero(found):
        inside = ((lo <= c[k]) & (c[k] < lo + e[:, None])).all(axis=1)
        (hit,) = np.flatnonzero(inside)  # exactly one leaf: the leaves tile the cube
        cell[k] = hit
        xi[k] = (s[k] - lo[hit].astype(float)) / float(e[hit])
    return cell, xi


_rows = {}  # (degree, xi) -> (phi_a(xi), phi_a'(xi)): mgoracle.lagrange_eval loops over its points in Python, so every xi is tabulated once


def _bases(space, xi):
    """(V, D)[d][k, a] = phi_a, phi_a' at xi[k, d]"""
    new = sorted({float(t) for t in xi.ravel() if (space.p, float(t)) not in _rows})
    if new:
        V, D = mg.lagrange_eval(space.fe.nodes, np.array(new))
        for t, v, d in zip(new, V, D):
            _rows[(space.p, t)] = (v, d)
    V = [np.array([_rows[(space.p, float(t))][0] for t in xi[:, d]]) for d in range(3)]
    D = [np.array([_rows[(space.p, float(t))][1] for t in xi[:, d]]) for d in range(3)]
    return V, D


def _basis_error(nodes, xi):
    """(eV, eD)[k, a]: the first-order change of phi_a(xi_k) and phi_a'(xi_k) when every difference xi - x_b moves by 2^-50"""
    nodes, xi = np.asarray(nodes, dtype=float), np.asarray(xi, dtype=float)
    n, f = len(nodes), np.abs(xi[:, None] - np.asarray(nodes)[None, :])
    eV, eD = np.zeros((len(xi), n)), np.zeros((len(xi), n))
    for a in range(n):
        den = abs(np.prod([nodes[a] - nodes[b] for b in range(n) if b != a]))
        for c in range(n):
            if c == a:
                continue
            eV[:, a] += np.prod(f[:, [b for b in range(n) if b not in (a, c)]], axis=1) / den
            for e in range(n):
                if e not in (a, c):
                    eD[:, a] += np.prod(f[:, [b for b in range(n) if b not in (a, c, e)]], axis=1) / den
    return 2.0 ** -50 * eV, 2.0 ** -50 * eD


def _sizes(space, xi, inflated):
    """|V|, |D| of _bases, with this oracle's own error added where `inflated`"""
    V, D = _bases(space, xi)
    V, D = [np.abs(v) for v in V], [np.abs(d) for d in D]
    if inflated:
        for d in range(3):
            eV, eD = _basis_error(space.fe.nodes, xi[:, d])
            V[d], D[d] = V[d] + eV, D[d] + eD
    return V, D


def cell_h(space, cell):
    return np.array([2.0 / (1 << space.cells[c][0]) for c in cell])


def evaluate(space, x, points, absolute=False):
    """(u_h [n], grad u_h [3, n]) of the vector x (the space's numbering) at the points; absolute: the per-point bounds instead;
    absolute="reference": this oracle's own error (see above)"""
    if absolute == "reference":
        plain, wide = evaluate(space, x, points, True), evaluate(space, x, points, "inflated")
        return wide[0] - plain[0], wide[1] - plain[1]
    cell, xi = locate(space.cells, points)
    n1 = space.p + 1
    nodal = space.Ch @ np.asarray(x, dtype=float)
    u, g = np.zeros(len(cell)), np.zeros((3, len(cell)))
    on = np.flatnonzero(cell >= 0)
    if len(on) == 0:
        return u, g
    V, D = _bases(space, xi[on])
    loc = nodal[space.cell_dofs[cell[on]]].reshape(len(on), n1, n1, n1)  # [point, c (z), b (y), a (x)]
    if absolute:
        (V, D), loc = _sizes(space, xi[on], absolute == "inflated"), np.abs(loc)
    h = cell_h(space, cell[on])
    u[on] = np.einsum("kcba,kc,kb,ka->k", loc, V[2], V[1], V[0])
    g[0, on] = np.einsum("kcba,kc,kb,ka->k", loc, V[2], V[1], D[0]) / h
    g[1, on] = np.einsum("kcba,kc,kb,ka->k", loc, V[2], D[1], V[0]) / h
    g[2, on] = np.einsum("kcba,kc,kb,ka->k", loc, D[2], V[1], V[0]) / h
    return u, g


def integrate(space, points, values=None, gradients=None, absolute=False, keep_dirichlet=False):
    """the load vector (the space's numbering) of values [n] and/or gradients [3, n] (either may be None) at the points; absolute:
    the sizes of the addends instead; absolute="reference": this oracle's own error (see above); keep_dirichlet: the rows of Dirichlet
    DoFs are left standing"""
    if absolute == "reference":
        return (integrate(space, points, values, gradients, "inflated", keep_dirichlet) -
                integrate(space, points, values, gradients, True, keep_dirichlet))
    cell, xi = locate(space.cells, points)
    n1 = space.p + 1
    on = np.flatnonzero(cell >= 0)
    Ch = abs(space.Ch) if absolute else space.Ch
    take = (lambda a: np.abs(np.asarray(a, dtype=float))) if absolute else (lambda a: np.asarray(a, dtype=float))
    F = np.zeros(space.n)
    if len(on):
        V, D = _bases(space, xi[on])
        if absolute:
            V, D = _sizes(space, xi[on], absolute == "inflated")
        h = cell_h(space, cell[on])
        loc = np.zeros((len(on), n1, n1, n1))
        if values is not None:
            loc += np.einsum("k,kc,kb,ka->kcba", take(values).reshape(-1)[on], V[2], V[1], V[0])
        if gradients is not None:
            G = take(gradients).reshape(3, -1)[:, on] / h
            loc += np.einsum("k,kc,kb,ka->kcba", G[0], V[2], V[1], D[0])
            loc += np.einsum("k,kc,kb,ka->kcba", G[1], V[2], D[1], V[0])
            loc += np.einsum("k,kc,kb,ka->kcba", G[2], D[2], V[1], V[0])
        np.add.at(F, space.cell_dofs[cell[on]], loc.reshape(len(on), -1))
    b = Ch.T @ F
    b[space.hanging if keep_dirichlet else space.hanging | space.dirichlet] = 0.0
    return b


# ------------------------------------------------------------------ the checks the host and the device tests share
NOISE = 1e-12  # a row of a load with B_i <= NOISE max_j B_j is a noise row (see the module docstring)


def ratio(err, size):
    """max err / size over the entries with size > 0; the others must be exactly 0: the plain bound"""
    on = size > 0
    assert (err[~on] == 0.0).all()
    return (err[on] / size[on]).max() if on.any() else 0.0


def row_ratio(err, size, own, tol, against_oracle=True):
    """the rows of a load.  Against this oracle every row is held to tol B_i + the oracle's own error; returned are the RAW ratio
    max err_i / B_i over the rows above noise level, whatever it is, and how many rows needed the allowance (err_i > tol B_i).  Against
    another statement on the product's own nodes (against_oracle=False) the rows above noise level are held to the plain tol B_i, and
    only the noise rows, whose B_i is itself a residue of this oracle, get the allowance."""
    noise = size <= NOISE * size.max()
    allowed = noise | against_oracle
    assert (err[allowed] <= tol * size[allowed] + own[allowed]).all()
    assert (err[~allowed] <= tol * size[~allowed]).all()
    return ratio(err[~noise], size[~noise]), int((err > tol * size).sum())


# ------------------------------------------------------------------ point sets the host and the device tests share
def leaf_box(cell):
    """(lower corner [3], edge h) of the leaf (level, i, j, k) in [-1, 1]^3"""
    h = 2.0 / (1 << cell[0])
    return -1.0 + h * np.array(cell[1:], dtype=float), h


def uniform(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))


def inside_leaf(cells, ci, n, seed):
    """n seeded points strictly inside leaf ci"""
    lo, h = leaf_box(cells[ci])
    return lo + h * np.random.default_rng(seed).uniform(0.01, 0.99, (n, 3))


def centres_and_corners(cells):
    """the centre and the eight corners of every leaf: ties on faces, edges and vertices, and the +1 faces"""
    out = []
    for c in cells:
        lo, h = leaf_box(c)
        out.append(lo + 0.5 * h)
        for v in range(8):
            out.append(lo + h * np.array([v & 1, (v >> 1) & 1, (v >> 2) & 1], dtype=float))
    return np.array(out)


def outside():
    """five points outside the cube (one by 2^-40: the rule has no tolerance beyond the rounding of x + 1) and one NaN"""
    return np.array([[1.5, 0.0, 0.0], [0.0, -1.0000001, 0.0], [0.3, 0.2, 1.0 + 2.0 ** -40], [-3.0, -3.0, -3.0], [0.0, np.inf, 0.0],
                     [0.1, np.nan, 0.2]])


_device_sets = {}


def device_sets(cells):
    """the sets of the device tests on a mesh: 1000 uniform points, 700 in one leaf, centres and corners, sets of 1, 0 and 257 points,
    duplicates, and `everything`: their concatenation with the duplicates and the points outside mixed in; `inside`: which points of
    `everything` lie in the cube"""
    tag = tuple(tuple(c) for c in cells)
    if tag not in _device_sets:
        sets = dict(uniform=uniform(1000, 1), one_leaf=inside_leaf(cells, (2 * len(cells)) // 3, 700, 2), corners=centres_and_corners(cells))
        sets["one"], sets["none"], sets["wave_and_one"] = sets["uniform"][:1], np.zeros((0, 3)), sets["uniform"][:257]
        sets["duplicates"] = np.concatenate([sets["uniform"][:20]] * 3 + [sets["corners"][:9]] * 2)
        inside = np.concatenate([sets[k] for k in ("uniform", "one_leaf", "corners", "duplicates")])
        sets["everything"] = np.concatenate([inside[:500], outside()[:3], inside[500:], outside()[3:]])
        mask = np.ones(len(sets["everything"]), bool)
        mask[500:503] = False
        mask[-3:] = False
        sets["inside"] = mask
        _device_sets[tag] = sets
    return _device_sets[tag]
