"""Test-side oracle of the operator with a piecewise-constant diffusion coefficient, A = K_a + sigma M (weak form of
-div(a grad u) + sigma u, a constant on every leaf): pure numpy/scipy on top of tests/helmholtz_oracle.py and the PUBLIC pieces of
oracle/mgoracle.py, neither of which is edited.  Not a test module.

level_class(oracle, sigma, coeff) subclasses helmholtz_oracle.level_class: after the parent's _assemble it replaces K0raw by
sum over cells of a_c h_c Kc on cell_dofs and re-shifts (Kraw = K0raw + sigma Mraw, A, inv_diag).  rhs_function's lifting goes
through Kraw and follows; rhs_constant, the constraints and the transfers do not depend on a.  coeff maps a cell (level, i, j, k)
to its value and must cover the level's cells.

Coarse coefficients are restated here, independently of the product: restrict_field(finest, cells) gives every cell of a coarser
mesh the volume-weighted arithmetic mean of the FINEST field over the leaves it covers, found from (level, i, j, k) alone: a
finest leaf (lf, i, j, k) lies in the coarse cell (l, i >> (lf - l), ...) and weighs 8^-(lf - l) of it.  The sums use math.fsum.

level and build_hierarchy build on a named geometry; level_on and build_hierarchy_on take a caller's set of leaves, and (meshes,
degrees) from helmholtz_oracle.level_plan_on.  with_coefficient(level, coeff, sigma) gives an existing level another coefficient
without repeating the constraint search, as reshift does for sigma.

f32_emulation and time_stepping_oracle take these levels unchanged.

The coefficient fields of the tests are functions of a cell (level, i, j, k): FIELDS.
"""
import copy
import math

import numpy as np
import scipy.sparse as sp

import helmholtz_oracle as ho


# ------------------------------------------------------------------ the fields
def _centre(cell):
    l, i, j, k = cell
    h = 2.0 / (1 << l)
    return (-1.0 + h * (i + 0.5), -1.0 + h * (j + 0.5), -1.0 + h * (k + 0.5))


def uniform(cell):
    """a = 3.5 everywhere: the slot structure is unchanged, every kernel family runs as without a coefficient but with a != 1"""
    return 3.5


def octants(cell):
    """a = 1 + 0.75 (octant index of the cell centre): the jumps lie on the planes through 0"""
    x, y, z = _centre(cell)
    return 1.0 + 0.75 * ((x > 0) + 2 * (y > 0) + 4 * (z > 0))


def inclusion(cell):
    """a = 1000 in [-0.5, 0]^3, 1 elsewhere: high contrast"""
    return 1000.0 if all(-0.5 < c < 0.0 for c in _centre(cell)) else 1.0


def per_cell(cell):
    """a = 0.5 + (hash of (level, i, j, k) mod 97) / 16.  The hash is linear with steps 31, 17, 13 (none a multiple of 97) in i, j,
    k, so no two face neighbours of one level agree and every brick is split."""
    l, i, j, k = cell
    return 0.5 + ((3 * l + 31 * i + 17 * j + 13 * k) % 97) / 16.0


def per_family(cell):
    """a = 0.5 + (hash of (level, i >> 1, j >> 1, k >> 1) mod 97) / 16: the eight siblings of a family share one value, so 2^3 bricks
    survive; face-neighbouring families of one level never agree (steps 31, 17, 13, none a multiple of 97), so no 4^3 brick forms
    and slots that sit side by side carry different values.  The mean over a whole family is exact: one coarsening step
    reproduces the value."""
    l, i, j, k = cell
    return 0.5 + ((5 * l + 31 * (i >> 1) + 17 * (j >> 1) + 13 * (k >> 1)) % 97) / 16.0


def per_block4(cell):
    """the same on aligned 4^3 blocks: bricks of B = 4 survive, each with a value of its own"""
    l, i, j, k = cell
    return 0.5 + ((5 * l + 31 * (i >> 2) + 17 * (j >> 2) + 13 * (k >> 2)) % 97) / 16.0


def octants_xyz(x, y, z):
    """octants as a function of the leaf centres (arrays), the form Hierarchy(coefficient=...) takes"""
    return 1.0 + 0.75 * ((x > 0) + 2 * (y > 0) + 4 * (z > 0))


def inclusion_xyz(x, y, z):
    inside = (x > -0.5) & (x < 0.0) & (y > -0.5) & (y < 0.0) & (z > -0.5) & (z < 0.0)
    return np.where(inside, 1000.0, 1.0)


XYZ = dict(uniform=lambda x, y, z: np.full(np.shape(x), 3.5), octants=octants_xyz, inclusion=inclusion_xyz)
FIELDS = dict(uniform=uniform, octants=octants, inclusion=inclusion, per_cell=per_cell, per_family=per_family, per_block4=per_block4)


def field_on(cells, f):
    """{cell: f(cell)} for an iterable of (level, i, j, k)"""
    return {tuple(int(v) for v in c): float(f(tuple(int(v) for v in c))) for c in cells}


def product_cells(tria):
    """the product's leaves as (level, i, j, k) tuples, in its order"""
    lev, i, j, k, _ = tria.cells()
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(lev, i, j, k)]


def product_values(tria, coeff):
    """the values of {cell: a} in the order of the product's cells"""
    return np.array([coeff[c] for c in product_cells(tria)])


# ------------------------------------------------------------------ coarse coefficients
def restrict_field(finest, cells):
    """{cell: volume-weighted mean of the finest field over the cell} for the cells of a coarser (or the same) mesh"""
    cells = set(tuple(c) for c in cells)
    parts = {c: [] for c in cells}
    for (l, i, j, k), a in finest.items():
        for up in range(l + 1):
            anc = (l - up, i >> up, j >> up, k >> up)
            if anc in cells:
                parts[anc].append(a * 0.125 ** up)
                break
        else:
            raise ValueError(f"finest leaf {(l, i, j, k)} is not covered by the coarse mesh")
    out = {}
    for c, terms in parts.items():
        if not terms:
            raise ValueError(f"cell {c} covers no finest leaf (it is finer than the finest mesh there)")
        out[c] = math.fsum(terms)
    return out


def harmonic_restrict_field(finest, cells):
    """the volume-weighted HARMONIC mean instead (what a caller may overwrite a coarse mesh with)"""
    inv = restrict_field({c: 1.0 / a for c, a in finest.items()}, cells)
    return {c: 1.0 / v for c, v in inv.items()}


# ------------------------------------------------------------------ levels
def stiffness(lv, coeff):
    """sum over the cells of lv of a_c h_c Kc on cell_dofs, a_c = coeff[cell]: the raw stiffness matrix of -div(a grad u)"""
    fe, nloc = lv.fe, (lv.p + 1) ** 3
    Kc = np.kron(np.kron(fe.M, fe.M), fe.K) + np.kron(np.kron(fe.M, fe.K), fe.M) + np.kron(np.kron(fe.K, fe.M), fe.M)
    rows = np.repeat(lv.cell_dofs, nloc, axis=1).ravel()
    cols = np.tile(lv.cell_dofs, (1, nloc)).ravel()
    ah = np.array([coeff[tuple(c)] * 2.0 / (1 << c[0]) for c in lv.cells])
    return sp.coo_matrix(((ah[:, None] * Kc.ravel()[None, :]).ravel(), (rows, cols)), shape=(lv.n, lv.n)).tocsr()


def level_class(oracle, sigma, coeff):
    base = ho.level_class(oracle, sigma)

    class CoefficientLevel(base):
        coefficient = coeff

        def _assemble(self):
            super()._assemble()
            self.cell_coefficient = np.array([self.coefficient[tuple(c)] for c in self.cells])
            self.K0raw = stiffness(self, self.coefficient)
            ho._shift(self, self.mass_coefficient)

    return CoefficientLevel


def with_coefficient(lv, coeff, sigma=None):
    """the level lv (a HelmholtzLevel, with or without a coefficient) for the coefficient {cell: a} and sigma (default: lv's): a
    shallow copy whose stiffness matrix, A and inv_diag are formed anew; the constraint search is not repeated and lv is left
    unchanged.  What level_class(oracle, sigma, coeff) builds on the same mesh, degree and numbering."""
    out = copy.copy(lv)
    out.__dict__.pop("_rounded", None)
    out.coefficient = coeff
    out.cell_coefficient = np.array([coeff[tuple(c)] for c in lv.cells])
    out.K0raw = stiffness(out, coeff)
    ho._shift(out, lv.mass_coefficient if sigma is None else sigma)
    return out


def level(oracle, sigma, field, dofs, geometry, n_ref, degree):
    """one level numbered like the product's `dofs`, field: a function of the cell"""
    return level_on(oracle, sigma, field, dofs, oracle.create_mesh(geometry, n_ref), degree)


def level_on(oracle, sigma, field, dofs, mesh, degree):
    """the same on a caller's set of leaves (level, i, j, k); field: a function of the cell or {cell: a} covering the mesh"""
    coeff = field_on(mesh, field) if callable(field) else field
    return level_class(oracle, sigma, coeff)(mesh, degree, numbering_keys=dofs.keys())


def build_hierarchy(oracle, sigma, field, geometry, n_ref_global, degree, mg_type="HMG-global", numbering_keys=None, restrict=restrict_field):
    """levels (coarse -> fine) and transfers; the finest field is `field` on the finest mesh, every other mesh gets restrict(...)"""
    meshes, degs = ho.level_plan(oracle, geometry, n_ref_global, degree, mg_type)
    return build_hierarchy_on(oracle, sigma, field, meshes, degs, numbering_keys, restrict)


def build_hierarchy_on(oracle, sigma, field, meshes, degs, numbering_keys=None, restrict=restrict_field):
    """the same on given (meshes, degrees), coarse -> fine (helmholtz_oracle.level_plan_on for a caller's leaves)"""
    finest = field_on(meshes[-1], field)
    levels = []
    for l, (m, p) in enumerate(zip(meshes, degs)):
        coeff = finest if m is meshes[-1] or m == meshes[-1] else restrict(finest, m)
        levels.append(level_class(oracle, sigma, coeff)(m, p, numbering_keys[l] if numbering_keys is not None else None))
    P = [None] + [oracle.build_transfer(levels[l], levels[l - 1]) for l in range(1, len(levels))]
    return levels, P


reshift = ho.reshift
reshift_hierarchy = ho.reshift_hierarchy
