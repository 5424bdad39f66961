"""
ORACLE (test infrastructure, NOT product code) -- the operator  -div(a grad u) + sigma u  on the cube [-1, 1]^3 with per-face
boundary conditions, stated once: pure numpy/scipy on the public pieces of mgoracle.py, which is not edited.

A Problem says WHAT is solved: sigma, a piecewise-constant coefficient {cell: a}, a 6-bit mask of Dirichlet faces and six Robin
coefficients beta_f >= 0 (a grad u . n + beta_f (u - u_ext) = 0 on face f).  Faces are numbered f = 2 axis + side (0: x = -1,
1: x = +1, ... 5: z = +1); bit f of the mask set means face f is Dirichlet, clear means natural or, with beta_f > 0, convective.

A Space holds what depends on (mesh, degree) alone and costs: cells, cell_dofs, keys, the hanging-node search of mgoracle.Level
(hanging, Ch) and the raw matrices that no Problem changes (Mraw, the raw unit load, the unit-coefficient stiffness).
Space.renumbered(keys) is the same space in another order of its DoF keys, without repeating the search.

Level(space, problem) forms the level:

    dirichlet by face, constrained = dirichlet | hanging, C = Ch diag(not dirichlet)
    K0raw = sum_c a_c h_c Kc,  Braw = sum_f beta_f h^2 M (x) M over the boundary cell faces (empty without convective faces)
    Kraw = K0raw + sigma Mraw + Braw,  A = C^T Kraw C + diag(constrained),  inv_diag with mgoracle's 1e-10 guard
    rhs_constant = C^T raw_load, constrained rows 0

Another sigma, mask, coefficient or beta is Level(space, dataclasses.replace(problem, ...)): nothing is applied in an order.  A
level carries the attribute and method names of mgoracle.Level, so f32_emulation, amg_oracle and the time-stepping oracles of
tests/ take it unchanged; rhs_function, distribute and node_positions ARE mgoracle.Level's.

The transfers of a mask derive from those of mask 0 (natural_transfers, mask_transfers).  The functions of a level (flux_load,
lift, distribute_values, face_values, ...) and the coefficient fields of the tests follow.

Pinned by tests/test_physics_oracle.py: against vectors recorded from the layered modules this one replaced
(tests/golden/physics_oracle_quadrant2.npz), bit for bit against mgoracle.Level for the default problem, and by the host tests of
every term (test_helmholtz_host, test_coefficient_host, test_boundary_host, test_robin_host, test_dirichlet_data_host).
"""
from __future__ import annotations

import copy
import dataclasses
import math

import numpy as np
import scipy.sparse as sp

import mgoracle as mg

ALL = 0x3F
M1 = 0b000001  # only x = -1 is Dirichlet
M2 = 0b101010  # the three "+" faces are Dirichlet
M0 = 0         # no Dirichlet face (with sigma > 0)
# (mask, beta): R1 = only x = +1 is Dirichlet, beta = 2.5 on x = -1 (on quadrant the refined corner touches it: a convective face
# with hanging nodes) and 0.75 on y = +1 (none);  R2 = no Dirichlet face, sigma = 0, beta = 1.5 on y = -1 and 4 on z = +1: regular
# only because of the convective faces
R1 = (0b000010, (2.5, 0.0, 0.0, 0.75, 0.0, 0.0))
R2 = (0, (0.0, 0.0, 1.5, 0.0, 0.0, 4.0))


@dataclasses.dataclass(frozen=True, eq=False)
class Problem:
    sigma: float = 0.0
    coefficient: dict | None = None  # {cell (level, i, j, k): a}, covering the level's cells; None: a == 1
    dirichlet_faces: int = ALL
    robin: tuple = (0.0,) * 6

    def __post_init__(self):
        object.__setattr__(self, "sigma", float(self.sigma))
        object.__setattr__(self, "dirichlet_faces", int(self.dirichlet_faces))
        object.__setattr__(self, "robin", tuple(float(b) for b in self.robin))
        assert len(self.robin) == 6 and all(b >= 0.0 for b in self.robin)
        assert not any(b > 0.0 and (self.dirichlet_faces >> f) & 1 for f, b in enumerate(self.robin))


def _cell_sum(cell_dofs, n, scale, local):
    """sum over cells of scale_c * local on cell_dofs, sparse"""
    nloc = cell_dofs.shape[1]
    rows = np.repeat(cell_dofs, nloc, axis=1).ravel()
    cols = np.tile(cell_dofs, (1, nloc)).ravel()
    return sp.coo_matrix(((scale[:, None] * local.ravel()[None, :]).ravel(), (rows, cols)), shape=(n, n)).tocsr()


class Space:
    """Q_p on an octree mesh: what mgoracle.Level finds (one constraint search) and the raw pieces no Problem changes"""

    def __init__(self, leaves, p, numbering_keys=None):
        base = mg.Level(leaves, p, numbering_keys)
        for name in ("p", "fe", "leaves", "cells", "cell_dofs", "keys", "key_to_dof", "n", "hanging", "Ch"):
            setattr(self, name, getattr(base, name))
        fe = self.fe
        self.h = np.array([2.0 / (1 << c[0]) for c in self.cells])
        self.K1raw = base.Kraw  # a == 1
        self.Mraw = _cell_sum(self.cell_dofs, self.n, self.h ** 3, np.kron(np.kron(fe.M, fe.M), fe.M))
        self.raw_load = np.zeros(self.n)  # f == 1 before any constraint
        np.add.at(self.raw_load, self.cell_dofs.ravel(), ((self.h ** 3)[:, None] * np.kron(np.kron(fe.m, fe.m), fe.m)[None, :]).ravel())

    def renumbered(self, keys):
        """(the space with its DoFs in the order of `keys`, Q): what Space(leaves, p, numbering_keys=keys) builds; Q is the
        permutation matrix, new vector = Q @ old vector"""
        ext = {tuple(int(v) for v in k): i for i, k in enumerate(keys)}
        assert len(ext) == self.n, (len(ext), self.n)
        perm = np.array([ext[tuple(int(v) for v in k)] for k in self.keys], dtype=np.int64)  # old -> new
        inv = np.argsort(perm)
        Q = sp.csr_matrix((np.ones(self.n), (perm, np.arange(self.n))), shape=(self.n, self.n))
        out = copy.copy(self)
        out.cell_dofs = perm[self.cell_dofs]
        out.keys = [self.keys[o] for o in inv]
        out.key_to_dof = {k: i for i, k in enumerate(out.keys)}
        out.hanging, out.raw_load = self.hanging[inv], self.raw_load[inv]
        for name in ("Ch", "K1raw", "Mraw"):
            setattr(out, name, (Q @ getattr(self, name) @ Q.T).tocsr())
        return out, Q


def dirichlet_by_face(keys, p, mask):
    """bool per DoF: the key lies on a face whose bit is set in mask"""
    top = p << mg.LMAX
    out = np.zeros(len(keys), dtype=bool)
    for d, key in enumerate(keys):
        out[d] = any((key[t] == 0 and (mask >> (2 * t)) & 1) or (key[t] == top and (mask >> (2 * t + 1)) & 1) for t in range(3))
    return out


def boundary_faces(space, weight):
    """(face f, h of the cell, the (p+1)^2 DoFs of the cell on that face) for every boundary cell face with weight[f] != 0: the one
    walk of face_matrix and flux_load.  The DoFs are ordered a_e (p+1) + a_g, e and g the axes after the face's own; cell_dofs: x
    fastest."""
    p, n1 = space.p, space.p + 1
    stride = (1, n1, n1 * n1)
    for ci, (l, i, j, k) in enumerate(space.cells):
        ijk, last = (i, j, k), (1 << l) - 1
        for f in range(6):
            d, side = f >> 1, f & 1
            if weight[f] == 0.0 or ijk[d] != (last if side else 0):
                continue
            e, g = (d + 1) % 3, (d + 2) % 3
            local = side * p * stride[d] + stride[e] * np.arange(n1)[:, None] + stride[g] * np.arange(n1)[None, :]
            yield f, 2.0 / (1 << l), space.cell_dofs[ci, local.ravel()]


def face_matrix(space, beta):
    """B = sum_f beta[f] int_{face f} phi_i phi_j over ALL DoFs of the cells (before any constraint): per boundary cell face
    beta h^2 M (x) M on the face nodes"""
    MM = np.kron(space.fe.M, space.fe.M)  # [(ae, ag), (be, bg)]
    rows, cols, vals = [], [], []
    for f, h, dofs in boundary_faces(space, beta):
        rows.append(np.repeat(dofs, len(dofs)))
        cols.append(np.tile(dofs, len(dofs)))
        vals.append(beta[f] * h * h * MM.ravel())
    if not rows:
        return sp.csr_matrix((space.n, space.n))
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(space.n, space.n)).tocsr()


class Level:
    """one level of a Problem on a Space; the names are mgoracle.Level's and those the layers on it added"""

    rhs_function = mg.Level.rhs_function
    distribute = mg.Level.distribute
    node_positions = mg.Level.node_positions

    def __init__(self, space, problem=Problem()):
        for name in ("p", "fe", "leaves", "cells", "cell_dofs", "keys", "key_to_dof", "n", "hanging", "Ch", "Mraw"):
            setattr(self, name, getattr(space, name))
        self.space, self.problem = space, problem
        self.mass_coefficient, self.dirichlet_faces, self.robin = problem.sigma, problem.dirichlet_faces, problem.robin
        self.dirichlet = dirichlet_by_face(self.keys, self.p, problem.dirichlet_faces)
        self.constrained = self.dirichlet | self.hanging
        self.C = (self.Ch @ sp.diags((~self.dirichlet).astype(float))).tocsr()
        self.coefficient = problem.coefficient
        if problem.coefficient is None:
            self.cell_coefficient = np.ones(len(self.cells))
            self.K0raw = space.K1raw
        else:
            self.cell_coefficient = np.array([problem.coefficient[tuple(c)] for c in self.cells])
            fe = self.fe
            Kc = np.kron(np.kron(fe.M, fe.M), fe.K) + np.kron(np.kron(fe.M, fe.K), fe.M) + np.kron(np.kron(fe.K, fe.M), fe.M)
            self.K0raw = _cell_sum(self.cell_dofs, self.n, self.cell_coefficient * space.h, Kc)
        self.Braw = face_matrix(space, problem.robin)
        self.Kraw = (self.K0raw + problem.sigma * self.Mraw + self.Braw).tocsr()
        A = (self.C.T @ self.Kraw @ self.C).tocsr()
        self.A = (A + sp.diags(self.constrained.astype(float))).tocsr()
        d = self.A.diagonal().copy()
        self.inv_diag = np.where(np.abs(d) > 1e-10, 1.0 / d, 1.0)
        self.rhs_constant = self.C.T @ space.raw_load
        self.rhs_constant[self.constrained] = 0.0

    def vmult(self, x):
        return self.A @ x


def changed(lv, **fields):
    """the level lv with fields of its problem replaced, e.g. changed(lv, sigma=7.5)"""
    return Level(lv.space, dataclasses.replace(lv.problem, **fields))


# ------------------------------------------------------------------ hierarchies and transfers
def level_plan(geometry, n_ref_global, degree, mg_type):
    """(meshes, degrees) coarse -> fine, as mgoracle.build_hierarchy chooses them"""
    return level_plan_on(mg.create_mesh(geometry, n_ref_global), degree, mg_type)


def level_plan_on(fine, degree, mg_type):
    """the same for a caller's set of leaves (level, i, j, k) as the finest mesh"""
    pseq = [degree]
    while pseq[-1] > 1:
        pseq.append(max(pseq[-1] // 2, 1))
    pseq = pseq[::-1]
    if mg_type == "HMG-global":
        meshes = mg.coarsening_sequence(fine)
        return meshes, [degree] * len(meshes)
    if mg_type == "PMG":
        return [fine] * len(pseq), pseq
    if mg_type == "HPMG":
        hm = mg.coarsening_sequence(fine)
        return hm + [fine] * (len(pseq) - 1), [pseq[0]] * len(hm) + pseq[1:]
    raise ValueError(mg_type)


def natural_transfer(fine, coarse):
    """the transfer between two spaces under mask 0 (no Dirichlet DoF: constrained means hanging, C is Ch)"""
    def natural(s):
        out = copy.copy(s)
        out.constrained, out.C = s.hanging, s.Ch
        return out
    return mg.build_transfer(natural(fine), natural(coarse))


def natural_transfers(spaces):
    return [None] + [natural_transfer(spaces[l], spaces[l - 1]) for l in range(1, len(spaces))]


def mask_transfers(P0, levels):
    """the transfers of the levels from those of mask 0, without walking the cells again.  build_transfer returns
    diag(w) Praw C_c with w = 0 on constrained fine rows and 1 / touch elsewhere, and C_c = Ch_c diag(not dirichlet_c).  Under mask
    0 constrained means hanging, so  P0 = diag(w0) Praw Ch_c;  a mask adds the Dirichlet DoFs to both sets:
    P = diag(not dirichlet_f) P0 diag(not dirichlet_c), products with 0 and 1 only.  test_boundary_host.py holds it against
    build_transfer on the levels."""
    return [None] + [(sp.diags((~levels[l].dirichlet).astype(float)) @ P0[l] @ sp.diags((~levels[l - 1].dirichlet).astype(float))).tocsr()
                     for l in range(1, len(levels))]


def level_coefficients(finest, meshes, restrict=None):
    """{cell: a} per mesh: `finest` on the finest mesh, restrict(finest, mesh) (default restrict_field) on every other; None
    without a coefficient"""
    if finest is None:
        return [None] * len(meshes)
    restrict = restrict or restrict_field
    return [finest if m is meshes[-1] or m == meshes[-1] else restrict(finest, m) for m in meshes]


def hierarchy(spaces, P0, problem, restrict=None):
    """(levels, P) of the problem on spaces coarse -> fine with their mask-0 transfers P0; problem.coefficient is the field on
    the finest mesh"""
    coeffs = level_coefficients(problem.coefficient, [s.leaves for s in spaces], restrict)
    levels = [Level(s, dataclasses.replace(problem, coefficient=c)) for s, c in zip(spaces, coeffs)]
    return levels, mask_transfers(P0, levels)


def build_hierarchy_on(problem, meshes, degs, numbering_keys=None, restrict=None):
    """(levels, P) on given (meshes, degrees), coarse -> fine, built directly (one constraint search per level)"""
    spaces = [Space(m, p, numbering_keys[l] if numbering_keys is not None else None) for l, (m, p) in enumerate(zip(meshes, degs))]
    return hierarchy(spaces, natural_transfers(spaces), problem, restrict)


def build_hierarchy(problem, geometry, n_ref_global, degree, mg_type="HMG-global", numbering_keys=None, restrict=None):
    """the same on a named geometry; problem.coefficient may be a function of the cell (evaluated on the finest mesh)"""
    meshes, degs = level_plan(geometry, n_ref_global, degree, mg_type)
    if callable(problem.coefficient):
        problem = dataclasses.replace(problem, coefficient=field_on(meshes[-1], problem.coefficient))
    return build_hierarchy_on(problem, meshes, degs, numbering_keys, restrict)


# ------------------------------------------------------------------ functions of a level
def gaussian_load(sigma):
    """f of the manufactured Gaussian solution: -Laplace u_g + sigma u_g"""
    return lambda x, y, z: mg.gaussian_rhs(x, y, z) + sigma * mg.gaussian_solution(x, y, z)


def flux_load(lv, q):
    """b_i = sum_f q[f] int_{face f} phi_i through the hanging-node constraints, constrained rows 0: per boundary cell face
    q h^2 m (x) m on the face nodes, written independently of the product"""
    mm = np.kron(lv.fe.m, lv.fe.m)
    F = np.zeros(lv.n)
    for f, h, dofs in boundary_faces(lv, q):
        np.add.at(F, dofs, q[f] * h * h * mm)
    b = lv.C.T @ F
    b[lv.constrained] = 0.0
    return b


def dirichlet_dofs(lv):
    return lv.dirichlet & ~lv.hanging


def data(lv, g):
    """g^: g on the Dirichlet DoFs, 0 elsewhere"""
    return np.where(dirichlet_dofs(lv), g, 0.0)


def stiffness_raw(lv):
    """the raw stiffness matrix of the level: with its coefficient and the surface term of its convective faces"""
    return (lv.K0raw + lv.Braw).tocsr()


def lift(lv, g, include_mass=True):
    """-[Ch^T (K + s sigma Mraw) Ch g^] on free rows, 0 on constrained rows: mgoracle.Level.rhs_function's lifting with g a vector
    of which only the entries at Dirichlet DoFs count"""
    K = stiffness_raw(lv)
    if include_mass:
        K = K + lv.mass_coefficient * lv.Mraw
    b = -(lv.Ch.T @ (K @ (lv.Ch @ data(lv, g))))
    b[lv.constrained] = 0.0
    return b


def distribute_values(lv, x, g):
    """Dirichlet DoFs from g, hanging DoFs from their parents, free DoFs kept"""
    x = np.array(x, dtype=float)
    bd = dirichlet_dofs(lv)
    x[bd] = g[bd]
    x[lv.hanging] = 0.0
    return lv.Ch @ x


def n_cells_with_dirichlet_dof(lv):
    """number of cells that gather at least one Dirichlet DoF, hanging nodes resolved to their parents through Ch"""
    touches = (abs(lv.Ch) @ dirichlet_dofs(lv).astype(float)) > 0  # per node: a Dirichlet DoF has weight in its value
    return int(np.sum(np.any(touches[lv.cell_dofs], axis=1)))


def face_values(lv, v):
    """v[f] on the Dirichlet DoFs of face f, the lowest-numbered Dirichlet face of a DoF on several; 0 elsewhere"""
    top, mask, g = lv.p << mg.LMAX, lv.dirichlet_faces, np.zeros(lv.n)
    for d in np.flatnonzero(dirichlet_dofs(lv)):
        key = lv.keys[d]
        for f in range(6):
            if (mask >> f) & 1 and key[f >> 1] == (top if f & 1 else 0):
                g[d] = v[f]
                break
    return g


# ------------------------------------------------------------------ the coefficient fields of the tests
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
    """octants as a function of the leaf centres (arrays), the form the product's Hierarchy(coefficient=...) takes"""
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


def restrict_field(finest, cells):
    """{cell: volume-weighted arithmetic mean of the FINEST field over the cell} for the cells of a coarser (or the same) mesh,
    restated independently of the product and found from (level, i, j, k) alone: a finest leaf (lf, i, j, k) lies in the coarse
    cell (l, i >> (lf - l), ...) and weighs 8^-(lf - l) of it.  The sums use math.fsum."""
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
