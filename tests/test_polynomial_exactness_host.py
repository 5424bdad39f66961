"""Polynomial exactness on the CPU (tests/polynomial_exactness.py): the helper against closed forms, then the numpy oracle and the
product's host tables against the helper, at p = 1 ... 7 (quadrant 3 for p <= 4, quadrant 2 for p >= 5).

The bound is 1e-13 on every figure; the measured figures are printed and lie near 1e-15.  Figures:
  rows     max_i |r_i| / (d_i max|u|) over the free rows that are checked
  Gram     max |v^T A w - exact| / (RHO max|w| sum_i |v_i| d_i)
  vectors  max |v^T b - exact| / sum_i |v_i| |b_i|
  transfer max |P u_c - u_f| / max|u| on the fine free DoFs

Where a Dirichlet mask leaves too little room for the face-vanishing test functions (ALL needs a factor (1 - x^2) per axis, so
p >= 2) the Gram case is left out at that degree; the rows are checked at every degree.  Rows are not asked of `per_cell` (the
harmonic polynomial is no solution under a coefficient that jumps across every face) and `convective` (the rows on a convective
face carry beta u); both have their Gram matrices.

Every problem variant runs at every degree for both sources.  The host tables have no mass product, so under sigma the mass term
of the rows is what sigma adds to DoFs.matrix() (a second assembly at sigma = 0) with the two liftings; algebraically that row
then holds DoFs.matrix() at sigma = 0 and rhs_dirichlet(include_mass=False) of the same tables to zero, while sigma M itself is
pinned by the Gram matrices.

Cost: the file takes about two minutes of CPU, of which the host tables at p = 6 and 7 take 11 s and 32 s (DoFs.matrix() assembles
for about 2 s at p = 7, thirteen times) and the oracle at p = 7 takes 14 s."""
import dataclasses
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import physics_oracle as po
import polynomial_exactness as pe
import support as su
from physics_oracle import ALL, M0, M1, M2, Problem

BOUND = 1e-13
SIGMA = 7.5
DEGREES = [1, 2, 3, 4, 5, 6, 7]
LAYER_VALUES, layer_planes = pe.LAYER_VALUES, pe.layer_planes


def mesh_of(p):
    return ("quadrant", 3 if p <= 4 else 2)


def layered(cells):
    """the coefficient of the leaves (level, i, j, k) in x-layers, as a function of the cell"""
    planes = layer_planes(cells)
    return lambda cell: float(su.layers(-1.0 + 2.0 / (1 << cell[0]) * (cell[1] + 0.5), planes, LAYER_VALUES))


# name: (problem, the harmonic is independent of x, rows are checked, the Gram matrix is checked)
PROBLEMS = dict(
    default=(Problem(), "full", True, True),
    sigma=(Problem(SIGMA), "full", True, True),
    uniform=(Problem(coefficient="uniform"), "full", True, True),
    layers=(Problem(coefficient="layers"), "x_independent", True, True),
    layers_M1=(Problem(coefficient="layers", dirichlet_faces=M1), "x_independent", True, True),
    per_cell=(Problem(coefficient="per_cell"), "full", False, True),
    M1=(Problem(dirichlet_faces=M1), "full", True, True),
    M2=(Problem(dirichlet_faces=M2), "full", True, True),
    M0_sigma=(Problem(SIGMA, dirichlet_faces=M0), "full", True, True),
    convective=(Problem(SIGMA, dirichlet_faces=M1, robin=(0.0, 2.5, 0.0, 0.0, 0.0, 0.0)), "full", False, True),
    # u = y + 0.1: a d_n u is the constant -3.5, +3.5 on y = -1, +1 and 0 on the other natural faces: every free row is checked,
    # those on the five natural faces with rhs_boundary_flux
    flux_M1=(Problem(coefficient="uniform", dirichlet_faces=M1), "linear_y", True, False),
)


def resolved(problem, geo, L):
    if problem.coefficient == "layers":
        return dataclasses.replace(problem, coefficient=layered(np.array(sorted(su.mesh(geo, L))).T))
    return problem


class Tables:
    """what the checks need of one level, from the numpy oracle (lv) or from the product's host tables (d, t)"""

    def __init__(self, p, problem, lv=None, d=None, t=None, with_mass=True):
        self.p, self.problem = p, problem
        if lv is not None:
            self.n, self.A, self.free, self.pos = lv.n, lv.A.tocsr(), ~lv.constrained, _positions(lv)
            self.cells, self.a, self.cell_dofs = np.array(lv.cells).T, lv.cell_coefficient, lv.cell_dofs
            self.lift, self.lifts = (lambda g, include_mass=True: po.lift(lv, g, include_mass)), _oracle_lifts(lv)
            self.flux = lambda q: po.flux_load(lv, q)
            self.rhs_constant = lv.rhs_constant
            self.mass = lambda x: lv.C.T @ (lv.Mraw @ (lv.C @ x))
        else:
            self.n, self.pos = d.n_dofs, d.node_positions()
            self.A = _csr(d)
            self.free = np.arange(self.n) < d.info.n_interior + d.info.n_tail
            self.cells, self.a, self.cell_dofs = t.cells(), t.coefficient(), d.cell_dofs()
            self.lift, self.flux, self.rhs_constant, self.mass = d.rhs_dirichlet, d.rhs_boundary_flux, d.rhs_constant(), None
            self.lifts = lambda G: np.stack([d.rhs_dirichlet(g, True) for g in G.T], axis=1)
            if problem.sigma != 0.0 and with_mass:
                # the host tables have no mass product of their own: C^T M C is what sigma adds to the assembled matrix
                d.set_mass_coefficient(0.0)
                M = ((self.A - _csr(d)) / problem.sigma).tocsr()
                d.set_mass_coefficient(problem.sigma)
                self.mass = lambda x: np.where(self.free, M @ x, 0.0)
        self.diag = self.A.diagonal()
        self.ratio = float(((abs(self.A) @ np.ones(self.n))[self.free] / self.diag[self.free]).max())


def _csr(d):
    ptr, col, val = d.matrix()
    return sp.csr_matrix((val, col.astype(np.int64), ptr.astype(np.int64)), shape=(d.n_dofs, d.n_dofs))


def _oracle_lifts(lv):
    """physics_oracle.lift (with the mass term) for the columns of a matrix at once: its formula with the sum of the raw matrices
    formed once instead of per column; held against lift itself on the first column"""
    def lifts(G):
        K = (po.stiffness_raw(lv) + lv.mass_coefficient * lv.Mraw).tocsr()
        B = -(lv.Ch.T @ (K @ (lv.Ch @ np.where(po.dirichlet_dofs(lv)[:, None], G, 0.0))))
        B[lv.constrained] = 0.0
        ref = po.lift(lv, G[:, 0], True)
        assert np.abs(B[:, 0] - ref).max() <= 1e-14 * max(np.abs(ref).max(), 1e-300)
        return B
    return lifts


_pos = {}


def _positions(lv):
    key = id(lv.space)
    if key not in _pos:
        _pos[key] = (lv.space, lv.node_positions())
    return _pos[key][1]


@functools.lru_cache(maxsize=2)
def oracle_tables(p, name):
    geo, L = mesh_of(p)
    problem = resolved(PROBLEMS[name][0], geo, L)
    return Tables(p, problem, lv=su.oracle_level(None, geo, L, p, problem))


@functools.lru_cache(maxsize=None)
def oracle_ratio(p, name):
    """max_i sum_j |A_ij| / A_ii over the free rows of the oracle's level: one number per case, kept for the session"""
    return oracle_tables(p, name).ratio


def product_tables(mgamd, p, name):
    geo, L = mesh_of(p)
    problem = resolved(PROBLEMS[name][0], geo, L)
    t = su.tria(mgamd, geo, L, problem)
    d = mgamd.DoFs(t, p, 0)
    d.set_mass_coefficient(problem.sigma)
    return Tables(p, problem, d=d, t=t, with_mass=PROBLEMS[name][2])


# ------------------------------------------------------------------ the checks, shared by both sources
def rows_figure(T, u_poly):
    """identity 1.  Natural faces: where a d_n u is constant on the face its flux load is added, else the rows ON the face are left
    out (a basis function of a node off the face vanishes on it); convective faces are left to the Gram matrix"""
    problem, u = T.problem, u_poly(*T.pos.T)
    uf = np.where(T.free, u, 0.0)
    r = T.A @ uf - T.lift(u, True)
    if problem.sigma != 0.0:
        r -= problem.sigma * T.mass(uf) - (T.lift(u, True) - T.lift(u, False))
    q, skipped = pe.natural_face_plan(u_poly, T.cells, T.a, problem.dirichlet_faces, problem.robin)
    if np.any(q != 0.0):
        r -= T.flux(q)
    rows, n_boundary = pe.checked_rows(T.free, T.pos, T.cells, T.cell_dofs, T.p, skipped)
    return pe.row_figure(r[rows], T.diag[rows], u), int(rows.sum()), n_boundary


def gram_figure(T):
    problem = T.problem
    VW = pe.bases(T.p, problem.dirichlet_faces)
    if VW is None:
        return None
    V, W = VW
    fr = T.free
    Vh, Wh = V(*T.pos.T), W(*T.pos.T)
    Y = T.A @ np.where(fr[:, None], Wh.T, 0.0)
    if problem.dirichlet_faces:
        Y = Y - T.lifts(Wh.T)
    G = Vh[:, fr] @ Y[fr]
    exact = pe.gram(T.cells, T.a, problem.sigma, problem.robin, V, W)
    bound = pe.gram_bound(Vh[:, fr], T.diag[fr], W.max_abs(), 1.0)
    return float((np.abs(G - exact) / bound).max())


def vector_figures(T):
    """v^T rhs_constant = int v and v^T rhs_boundary_flux(q) = sum_f q_f int_f v, v vanishing on the Dirichlet faces"""
    problem = T.problem
    VW = pe.bases(T.p, problem.dirichlet_faces)
    if VW is None:
        return None
    V, fr = VW[0], T.free
    Vh = V(*T.pos.T)[:, fr]
    out = [np.max(np.abs(Vh @ T.rhs_constant[fr] - pe.integrals(V)) / (np.abs(Vh) @ np.abs(T.rhs_constant[fr])))]
    q = np.array([0.0 if (problem.dirichlet_faces >> f) & 1 else 1.0 + 0.5 * f for f in range(6)])
    if np.any(q != 0.0):
        b = T.flux(q)
        out.append(np.max(np.abs(Vh @ b[fr] - pe.face_integrals(V, q)) / (np.abs(Vh) @ np.abs(b[fr]))))
    return [float(e) for e in out]


def check(T, name, p, source):
    _, kind, rows, gram = PROBLEMS[name]
    if rows:
        e, n_rows, n_boundary = rows_figure(T, pe.row_function(p, kind))
        print(f"{source} {name} p={p}: row figure {e:.2e} over {n_rows} rows ({n_boundary} of them on natural faces)")
        assert e <= BOUND and (kind != "linear_y" or n_boundary > 0)
    if gram:
        e = gram_figure(T)
        print(f"{source} {name} p={p}: Gram figure {'left out' if e is None else format(e, '.2e')}")
        assert e is None or e <= BOUND
    v = vector_figures(T)
    print(f"{source} {name} p={p}: vector figures {v}")
    assert v is None or max(v) <= BOUND


# ------------------------------------------------------------------ the helper against itself
def monomials(p):
    f = [[np.polynomial.Polynomial.basis(k) for k in range(p + 1)]] * 3
    return pe.Basis(f, [(a, b, c) for c in range(p + 1) for b in range(p + 1) for a in range(p + 1)])


def closed_form(p, sigma, beta):
    """the Gram matrix of the monomials on [-1, 1]^3: int x^a x^b = 2 / (a + b + 1) for a + b even, int (x^a)' (x^b)' = 2 a b /
    (a + b - 1) for a + b even and a, b >= 1; on the face x = s the trace of x^a x^b is s^(a + b)"""
    k = np.arange(p + 1)
    s = k[:, None] + k[None, :]
    M = np.where(s % 2 == 0, 2.0 / (s + 1), 0.0)
    K = np.where((s % 2 == 0) & (k[:, None] >= 1) & (k[None, :] >= 1), 2.0 * k[:, None] * k[None, :] / np.maximum(s - 1, 1), 0.0)
    E = [(-1.0) ** s, np.ones_like(M)]
    kron = lambda Z, Y, X: np.kron(np.kron(Z, Y), X)  # x fastest
    G = kron(M, M, K) + kron(M, K, M) + kron(K, M, M) + sigma * kron(M, M, M)
    for side in (0, 1):
        G = G + beta[0 + side] * kron(M, M, E[side]) + beta[2 + side] * kron(M, E[side], M) + beta[4 + side] * kron(E[side], M, M)
    return G


def cells_of(leaves):
    return np.array(sorted(leaves)).T


@pytest.mark.parametrize("p", [1, 2, 4, 7])
def test_helper_one_cell_against_closed_forms(p):
    B, beta = monomials(p), (0.5, 0.0, 1.5, 0.0, 0.0, 4.0)
    G = pe.gram(cells_of({(0, 0, 0, 0)}), None, SIGMA, beta, B, B)
    ref = closed_form(p, SIGMA, beta)
    e = np.abs(G - ref).max() / np.abs(ref).max()
    print(f"one cell p={p}: Gram against closed forms {e:.2e}")
    assert e <= 1e-14
    top = len(B) - 1  # x^p y^p z^p with itself, the issue's figure
    assert pe.gram(cells_of({(0, 0, 0, 0)}), None, 0.0, None, B.subset([top]), B.subset([top]))[0, 0] == pytest.approx(
        3 * (2 * p * p / (2 * p - 1)) * (2 / (2 * p + 1)) ** 2, rel=1e-14)
    assert np.abs(pe.integrals(B) - ref_integrals(p)).max() <= 1e-15
    q = np.array([1.0, 0.0, 0.0, -2.0, 0.5, 0.0])
    fi = closed_form(p, 0.0, q)[:, 0] - closed_form(p, 0.0, np.zeros(6))[:, 0]
    assert np.abs(pe.face_integrals(B, q) - fi).max() <= 1e-14 * np.abs(fi).max()


def ref_integrals(p):
    k = np.arange(p + 1)
    m = np.where(k % 2 == 0, 2.0 / (k + 1), 0.0)
    return np.kron(np.kron(m, m), m)


@pytest.mark.parametrize("p", [2, 5, 7])
def test_helper_is_additive_over_cells(oracle, p):
    """one cell, its 8 children and the 15 cells of quadrant 2 give the same matrices; the Legendre basis and its face-vanishing form"""
    beta = (0.5, 0.0, 1.5, 0.0, 0.0, 4.0)
    V, W = pe.chosen(pe.legendre_basis(p, M2), 40, 3), pe.chosen(pe.legendre_basis(p), 40, 4)
    one = pe.gram(cells_of({(0, 0, 0, 0)}), None, SIGMA, beta, V, W)
    for leaves in (oracle.refine_global({(0, 0, 0, 0)}, 1), oracle.create_mesh("quadrant", 2)):
        assert len(leaves) in (8, 15)
        G = pe.gram(cells_of(leaves), None, SIGMA, beta, V, W)
        e = np.abs(G - one).max() / np.abs(one).max()
        print(f"p={p}: {len(leaves)} cells against one {e:.2e}")
        assert e <= 1e-14
        # sums of up to 15 terms of size <= 8 max|v|, each good to a few ulp
        assert np.abs(pe.integrals(V, cells_of(leaves)) - pe.integrals(V)).max() <= 1e-14 * 8.0 * V.max_abs().max()
    x = np.random.default_rng(1).uniform(-1.0, 1.0, (3, 20))
    assert np.abs(np.polynomial.polynomial.polyval3d(*x, np.moveaxis(V.coefficients(), 0, -1)) - V(*x)).max() <= 1e-13
    face = np.abs(V(np.ones(20), x[1], x[2])).max(), np.abs(V(x[0], np.ones(20), x[2])).max(), np.abs(V(x[0], x[1], np.ones(20))).max()
    assert max(face) == 0.0  # M2: the three "+" faces


@pytest.mark.parametrize("p", [3, 6, 7])
def test_helper_legendre_orthogonality(p):
    """int P_a P_b = 2 / (2a + 1) delta_ab per variable, on the whole cube and summed over the cells of quadrant 2: a few ulp of
    int |v w| <= 8 (the monomial form about x = 0 would lose three digits at degree 6)"""
    B = pe.chosen(pe.legendre_basis(p), 64, p)
    ref = np.diag(np.prod(2.0 / (2.0 * B.idx + 1.0), axis=1))
    for cells in (cells_of({(0, 0, 0, 0)}), cells_of(su.mesh("quadrant", 2))):
        e = np.abs(pe.mass_gram(B, B, cells) - ref).max()
        print(f"p={p}, {len(cells[0])} cells: Legendre mass matrix against the closed form {e:.2e}")
        assert e <= 8 * 4 * np.finfo(float).eps


@pytest.mark.parametrize("p", DEGREES)
def test_harmonic_is_harmonic(p):
    for x_independent in (False, True):
        u = pe.harmonic(p, x_independent)
        assert u.c.shape == (p + 1,) * 3 and np.all(u.laplacian().c == 0.0)
        for axis in range(3):  # the full form has degree exactly p in each variable
            assert x_independent or np.any(np.take(u.c, p, axis=axis) != 0.0)
        x = np.random.default_rng(p).uniform(-1.0, 1.0, (3, 50))
        assert np.abs(u(*x) - np.polynomial.polynomial.polyval3d(*x, u.c)).max() <= 1e-13
    assert np.all(pe.harmonic(p, True).c[1:] == 0.0)
    assert pe.constant_normal_flux(pe.harmonic(p, True), 1) == 0.0 and pe.constant_normal_flux(pe.harmonic(p), 1) is None


# ------------------------------------------------------------------ the numpy oracle
@pytest.mark.parametrize("p", DEGREES)
def test_oracle_holds_rows_and_gram(p):
    for name in PROBLEMS:
        check(oracle_tables(p, name), name, p, "oracle")
        oracle_ratio(p, name)  # from the level just built; test_rho_is_a_ceiling reads it


@pytest.mark.parametrize("p", DEGREES)
def test_default_problem_is_mgoracle_level(oracle, p):
    """mgoracle.Level itself (the default problem: six Dirichlet faces) from its own pieces Ch, Kraw: the rows of the harmonic
    polynomial, and the Gram matrix with V vanishing on the boundary (p >= 2)"""
    lv = oracle.Level(su.mesh(*mesh_of(p)), p)
    pos, free, d = lv.node_positions(), ~lv.constrained, lv.A.diagonal()
    u = pe.harmonic(p)(*pos.T)
    e = pe.row_figure((lv.Ch.T @ (lv.Kraw @ u))[free], d[free], u)
    print(f"mgoracle.Level p={p}: row figure {e:.2e}")
    assert e <= BOUND
    VW = pe.bases(p, ALL)
    if VW is None:
        print(f"mgoracle.Level p={p}: Gram figure left out")
        return
    V, W = VW
    Vh, Wh = V(*pos.T)[:, free], W(*pos.T)
    Y = lv.Ch.T @ (lv.Kraw @ (lv.Ch @ np.where(lv.hanging[:, None], 0.0, Wh.T)))  # A w_free - lift(w): w with its boundary values
    cells = np.array(lv.cells).T
    eg = (np.abs(Vh @ Y[free] - pe.gram(cells, None, 0.0, None, V, W)) / pe.gram_bound(Vh, d[free], W.max_abs(), 1.0)).max()
    print(f"mgoracle.Level p={p}: Gram figure {eg:.2e}")
    assert eg <= BOUND


# ------------------------------------------------------------------ the product's host tables
@pytest.mark.parametrize("p", DEGREES)
def test_host_tables_hold_rows_and_gram(mgamd, p):
    """every variant at every degree.  With sigma the mass term of the rows is what sigma adds to DoFs.matrix() (a second
    assembly at sigma = 0) together with the two liftings.  DoFs.matrix() dominates the cost: about 2 s per assembly at p = 7."""
    for name in PROBLEMS:
        check(product_tables(mgamd, p, name), name, p, "host tables")


def test_layer_planes_are_faces_of_every_leaf(mgamd):
    assert layer_planes(mgamd.Triangulation("quadrant", 3).cells()) == [-0.5, 0.0]
    assert layer_planes(mgamd.Triangulation("quadrant", 2).cells()) == [0.0]
    T = product_tables(mgamd, 2, "layers")
    assert sorted(set(T.a)) == sorted(LAYER_VALUES)


# ------------------------------------------------------------------ transfers
@pytest.mark.parametrize("p", DEGREES)
def test_transfers_reproduce_polynomials(p):
    """identity 3 through the oracle's natural transfers (mask 0: every polynomial, no boundary condition in the way), on every
    level pair of the HMG-global, PMG and HPMG plans"""
    geo, L = mesh_of(p)
    for mg_type in ("HMG-global", "PMG", "HPMG"):
        meshes, degs = po.level_plan_on(su.mesh(geo, L), p, mg_type)
        P = su.natural_transfers(meshes, degs)
        worst = 0.0
        for l in range(1, len(meshes)):
            f, c = su.oracle_level_on(None, meshes[l], degs[l], Problem(SIGMA, dirichlet_faces=M0)), su.oracle_level_on(
                None, meshes[l - 1], degs[l - 1], Problem(SIGMA, dirichlet_faces=M0))
            pf, pc = _positions(f), _positions(c)
            top = pe.legendre_basis(degs[l - 1]).subset([-1])
            for fn in (pe.harmonic(degs[l - 1]), lambda x, y, z: top(x, y, z)[0]):
                uf, uc = fn(*pf.T), fn(*pc.T)
                e = np.abs(P[l] @ np.where(c.constrained, 0.0, uc) - uf)[~f.constrained].max() / np.abs(uf).max()
                worst = max(worst, e)
        print(f"{geo} {L} p={p} {mg_type}: {len(meshes) - 1} transfers, worst {worst:.2e}")
        assert worst <= BOUND


# ------------------------------------------------------------------ RHO
def test_rho_is_a_ceiling():
    """max_i sum_j |A_ij| / A_ii over the free rows, for every problem above and every degree"""
    worst = {}
    for p in DEGREES:
        for name in PROBLEMS:
            worst[name, p] = oracle_ratio(p, name)
        print(f"p={p}: " + ", ".join(f"{name} {worst[name, p]:.2f}" for name in PROBLEMS))
    assert max(worst.values()) <= pe.RHO
    assert [round(worst["default", p], 2) for p in DEGREES] == [2.08, 3.66, 5.53, 7.54, 8.20, 9.68, 11.06]
    assert max(worst.values()) > pe.RHO - 1  # RHO is the ceiling of what is measured, not a guess far above it
