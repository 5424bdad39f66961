"""Polynomial exactness on the device (tests/polynomial_exactness.py): operator, liftings, loads, mass operator, transfers and the
solve against mathematics.  No test of this file builds an oracle level; from physics_oracle only the mask constants, the Problem
record and the coefficient fields are taken.

Figures and bounds (TOL_OP, TOL_F32, TOL_CHEB are tests/support.py's, RHO the helper's; nothing new is introduced):
  rows     e = max_i |r_i| / (d_i max|u|) <= RHO TOL, d_i = 1 / compute_inverse_diagonal on the free rows, TOL = TOL_OP on FP64 levels
           and TOL_F32 on FP32 levels
  Gram     |v_h^T (A w_h) - exact| <= TOL RHO max|w| sum_i |v_i| d_i, the sum of the row bounds
  vectors  |v^T b - exact| <= TOL sum_i |v_i| |b_i| for rhs_boundary_flux, rhs(0) and vmult_mass
  transfer max |P u_c - u_f| <= TOL max|u| on the fine free DoFs; |(R v)^T w - v^T (P w)| <= TOL sum_i |v_i| |(P w)_i|
  solve    nodal error <= 1e-8 max|u| after solve_cg at reltol 1e-12 (test_linear_function_is_reproduced's bound and reasoning)
Every figure is printed, Gram and vector figures as the largest ratio to their bound.

Sources carry 1e30 in their constrained entries (never read), destinations are NaN-prefilled (support.apply_nan).

Where a degree leaves no test function that vanishes on the Dirichlet faces (ALL at p = 1) the Gram case is left out; the rows are
checked at every degree.  The layered coefficient uses those of the planes x = -0.5, 0 that are faces of every leaf.

Out of scope: the time stepper (vmult_mass drops the source on Dirichlet nodes and only constant fluxes exist, so no exact
polynomial solution with curved content is available), local smoothing and simulated ranks.

Measured on an MI355X (worst case per number type over every case of a test):
  rows       FP64 2.8e-16 ... 6.4e-16 at p = 1 ... 7 (bound 1.3e-12), FP32 1.1e-7 ... 1.9e-7 (bound 2.6e-5); at 17 M DoFs 7.4e-16 / 3.0e-7
             the flux case (u = y + 0.1, every row of the five natural faces checked through rhs_boundary_flux) 1.7e-16 ... 5.7e-16 and
             7.4e-8 ... 1.7e-7
  control    one entry off by 1 + 1e-6: 8.0e-7, 6e5 times the FP64 bound; by 1 + 1e-2 in FP32: 4.5e-3, 173 times the bound
  Gram       error / bound <= 4.2e-4 in FP64 and <= 2.0e-3 in FP32;  loads and mass operator <= 4.2e-2 and <= 9.6e-2
  transfers  prolongation 1.9e-15 / 2.1e-7, adjoint error / bound 1.2e-3 / 3.1e-2
  solve      nodal error 3.3e-14 ... 3.4e-13 after 10 or 11 CG iterations
Every test takes at most 2.6 s but the two of section 6, whose wall times, dominated by host table construction, are 5.8 s
(hypercube 6, p = 4: FP64, the Chebyshev step and FP32) and 9.7 s (quadrant 9, p = 1)."""
import time

import numpy as np
import pytest

import polynomial_exactness as pe
import support as su
from physics_oracle import ALL, M0, M1, M2, Problem
from polynomial_exactness import RHO
from support import TOL_CHEB, TOL_F32, TOL_OP

pytestmark = pytest.mark.gpu

SIGMA = 7.5
OP_CASES = su.OP_CASES + [("quadrant", 2, 3, 0), ("quadrant", 2, 6, 0)]
case_id = lambda c: "-".join(map(str, c))  # noqa: E731


def test_every_degree_occurs():
    assert sorted(set(c[2] for c in OP_CASES)) == [1, 2, 3, 4, 5, 6, 7]


def type_name(mgamd, number_type):
    return "FP64" if number_type == mgamd.F64 else "FP32"


def tol_of(mgamd, number_type):
    return TOL_OP if number_type == mgamd.F64 else TOL_F32


def mesh(mgamd, geo, L, problem, layers=False):
    """the product's mesh with the problem's mask, Robin coefficients and coefficient; layers: the coefficient in x-layers"""
    t = su.tria(mgamd, geo, L, problem)
    if layers:
        planes = pe.layer_planes(t.cells())
        assert planes
        t.set_coefficient_function(lambda x, y, z: su.layers(x, planes, pe.LAYER_VALUES))
        assert len(set(t.coefficient())) == len(planes) + 1
    return t


class Level:
    """one level operator with what the checks read off its tables"""

    def __init__(self, mgamd, ctx, t, p, max_brick, sigma, number_type, with_cell_dofs=True):
        self.mgamd, self.ctx, self.t, self.p, self.sigma, self.number_type = mgamd, ctx, t, p, sigma, number_type
        self.d = mgamd.DoFs(t, p, max_brick)
        self.d.set_mass_coefficient(sigma)
        self.op = mgamd.Operator(ctx, self.d, number_type)
        self.n, self.pos = self.d.n_dofs, self.d.node_positions()
        self.free = np.arange(self.n) < self.d.info.n_interior + self.d.info.n_tail
        self.cells, self.a = t.cells(), t.coefficient()
        self.cell_dofs = self.d.cell_dofs() if with_cell_dofs else None
        dinv = self.op.initialize_dof_vector()
        self.op.compute_inverse_diagonal(dinv)
        self.diag = 1.0 / dinv.to_host()
        self.tol = tol_of(mgamd, number_type)
        self._src = self._dst = None

    def rounded(self, x):
        return x if self.number_type == self.mgamd.F64 else x.astype(np.float32).astype(np.float64)

    def apply(self, fn, x):
        """fn(dst, src) into a NaN-prefilled destination: support.apply_nan on FP64 levels, the same on vectors of the level's
        number type otherwise"""
        if self.number_type == self.mgamd.F64:
            return su.apply_nan(self.mgamd, self.ctx, fn, x)
        x = self.rounded(x)
        src, dst = su.vec(self.op, x), su.vec(self.op, np.full(self.n, np.nan))
        fn(dst, src)
        assert np.array_equal(src.to_host(), x)
        out = dst.to_host()
        assert np.isfinite(out).all()
        return out

    def apply_columns(self, fn, X):
        """the same for the columns of X, on one pair of vectors"""
        if self._src is None:
            self._src, self._dst = self.op.initialize_dof_vector(), self.op.initialize_dof_vector()
        nan, out = np.full(self.n, np.nan), np.zeros(X.shape)
        for k in range(X.shape[1]):
            self._src.from_host(X[:, k])
            self._dst.from_host(nan)
            fn(self._dst, self._src)
            out[:, k] = self._dst.to_host()
        assert np.isfinite(out).all()
        return out

    def lift(self, g, include_mass=True):
        b = su.vec(self.op, np.full(self.n, np.nan))
        self.op.rhs_dirichlet(b, su.vec(self.op, g), include_mass)
        return b.to_host()

    def flux(self, q):
        b = su.vec(self.op, np.full(self.n, np.nan))
        self.op.rhs_boundary_flux(b, q)
        return b.to_host()

    def source(self, x):
        """x on the free entries, 1e30 on the constrained ones, which no kernel reads"""
        return np.where(self.free if np.ndim(x) == 1 else self.free[:, None], x, 1e30)


def rows_figure(lv, problem, u_poly, perturb=0.0, passes=1):
    """identity 1 on the device: (figure, rows checked, of them on natural faces).  perturb: one free entry of u, the largest, is
    multiplied by 1 + perturb (the negative control)"""
    u = u_poly(*lv.pos.T)
    src = lv.source(u)
    if perturb:
        j = np.flatnonzero(lv.free)[np.argmax(np.abs(u[lv.free]))]
        src[j] *= 1.0 + perturb
    lift = lv.lift(u, True)
    q, skipped = pe.natural_face_plan(u_poly, lv.cells, lv.a, problem.dirichlet_faces, problem.robin)
    rows, n_boundary = pe.checked_rows(lv.free, lv.pos, lv.cells, lv.cell_dofs, lv.p, skipped)
    loads = [lv.flux(q)] if np.any(q != 0.0) else []
    if problem.sigma != 0.0:
        loads.append(problem.sigma * lv.apply(lv.op.vmult_mass, src) - (lift - lv.lift(u, False)))
    worst = 0.0
    for _ in range(passes):
        r = pe.row_residual(lv.apply(lv.op.vmult, src), lift, rows, *loads)
        worst = max(worst, pe.row_figure(r, lv.diag[rows], u))
    return worst, int(rows.sum()), n_boundary


# ------------------------------------------------------------------ 1. the row-wise patch test on every kernel family
# (name, mask, sigma, coefficient field, kind of polynomial: polynomial_exactness.row_function).  With the two harmonics of degree
# p, a d_n u is constant on a natural face only where it is zero (the x faces under the x-independent one), so no load enters
# there; "flux" is the case in which rhs_boundary_flux enters identity 1: u = y + 0.1 under a = 3.5 and M1 has q = -3.5, +3.5 on
# y = -1, +1 and 0 on the other natural faces, and every free row is checked, those on the five natural faces included.
ROW_VARIANTS = [("plain", ALL, 0.0, None, "full"), ("plain", M1, 0.0, None, "full"), ("plain", M2, 0.0, None, "full"),
                ("sigma", ALL, SIGMA, None, "full"), ("sigma", M1, SIGMA, None, "full"), ("uniform", ALL, 0.0, "uniform", "full"),
                ("layers", ALL, 0.0, None, "x_independent"), ("layers", M1, 0.0, None, "x_independent"),
                ("flux", M1, 0.0, "uniform", "linear_y"), ("flux sigma", M1, SIGMA, "uniform", "linear_y")]


@pytest.mark.parametrize("case", OP_CASES, ids=case_id)
def test_rows_on_every_kernel_family(mgamd, ctx, case):
    geo, L, p, max_brick = case
    for name, mask, sigma, field, kind in ROW_VARIANTS:
        problem = Problem(sigma, field, mask)
        t = mesh(mgamd, geo, L, problem, kind == "x_independent")
        for number_type in (mgamd.F64, mgamd.F32):
            lv = Level(mgamd, ctx, t, p, max_brick, sigma, number_type)
            e, n_rows, n_boundary = rows_figure(lv, problem, pe.row_function(p, kind))
            print(f"{case_id(case)} {name} mask={mask:#04x} {type_name(mgamd, number_type)}: row figure {e:.2e} over {n_rows} rows "
                  f"({n_boundary} on natural faces), groups {lv.d.groups()}, bound {RHO * lv.tol:.1e}")
            assert e <= RHO * lv.tol
            if kind == "linear_y":  # nothing is left out: the flux load carries the rows of all five natural faces
                assert n_rows == int(lv.free.sum()) and n_boundary > 0


# ------------------------------------------------------------------ 2. the negative control
@pytest.mark.parametrize("case,f32,perturb", [(("quadrant", 3, 4, 0), False, 1e-6), (("quadrant", 3, 2, 0), True, 1e-2)],
                         ids=["FP64", "FP32"])
def test_negative_control(mgamd, ctx, case, f32, perturb):
    """the same check with ONE free entry of u off by a factor 1 + perturb exceeds the bound a hundredfold: the inputs are
    legitimate, the check can fail"""
    geo, L, p, max_brick = case
    problem = Problem()
    lv = Level(mgamd, ctx, mesh(mgamd, geo, L, problem), p, max_brick, 0.0, mgamd.F32 if f32 else mgamd.F64)
    clean = rows_figure(lv, problem, pe.harmonic(p))[0]
    off = rows_figure(lv, problem, pe.harmonic(p), perturb)[0]
    print(f"{case_id(case)} {type_name(mgamd, lv.number_type)}: clean {clean:.2e}, one entry off by 1 + {perturb:g}: {off:.2e} = "
          f"{off / (RHO * lv.tol):.1f} times the bound {RHO * lv.tol:.1e}")
    assert clean <= RHO * lv.tol and off >= 100.0 * RHO * lv.tol


# ------------------------------------------------------------------ 3. Gram matrices and loads
GRAM_CASES = [("quadrant", 3, 1), ("quadrant", 3, 2), ("quadrant", 3, 3), ("quadrant", 3, 4), ("quadrant", 2, 5), ("quadrant", 2, 6),
              ("quadrant", 2, 7), ("hypercube", 2, 4)]
# no convective face shares an edge with a Dirichlet face
GRAM_PROBLEMS = [("M0", Problem(0.0, None, M0)), ("M0 sigma", Problem(SIGMA, None, M0)), ("octants", Problem(SIGMA, "octants", M0)),
                 ("per_cell M1", Problem(0.0, "per_cell", M1)), ("beta on one face", Problem(0.0, None, M0, (0.0, 0.0, 0.0, 0.75, 0.0, 0.0))),
                 ("beta on two faces", Problem(0.0, None, M0, (0.0, 0.0, 1.5, 0.0, 0.0, 4.0))),
                 ("beta opposite M1", Problem(SIGMA, None, M1, (0.0, 2.5, 0.0, 0.0, 0.0, 0.0))), ("M1", Problem(0.0, None, M1)),
                 ("ALL", Problem(0.0, None, ALL))]


bases = pe.bases


@pytest.mark.parametrize("case", GRAM_CASES, ids=case_id)
def test_gram_matrices(mgamd, ctx, case):
    """one vmult per w, then V^T A W in numpy against sums of products of 1D integrals; under a mask V vanishes on the Dirichlet
    faces and A w_free - rhs_dirichlet(w) stands for A w, which pins the lifting and the face kernel to integrals"""
    geo, L, p = case
    for name, problem in GRAM_PROBLEMS:
        VW = bases(p, problem.dirichlet_faces)
        if VW is None:
            print(f"{case_id(case)} {name}: no function of Q_{p} vanishes on the Dirichlet faces, left out")
            continue
        V, W = VW
        t = mesh(mgamd, geo, L, problem)
        exact = pe.gram(t.cells(), t.coefficient(), problem.sigma, problem.robin, V, W)
        for number_type in [mgamd.F64] + [mgamd.F32] * (p in (2, 4, 7)):
            lv = Level(mgamd, ctx, t, p, 0, problem.sigma, number_type, with_cell_dofs=False)
            Vh, Wh = V(*lv.pos.T)[:, lv.free], lv.rounded(W(*lv.pos.T).T)
            Y = lv.apply_columns(lv.op.vmult, lv.source(Wh))
            if problem.dirichlet_faces:
                Y -= np.stack([lv.lift(w, True) for w in Wh.T], axis=1)
            G = Vh @ Y[lv.free]
            ratio = (np.abs(G - exact) / pe.gram_bound(Vh, lv.diag[lv.free], W.max_abs(), lv.tol)).max()
            print(f"{case_id(case)} {name} {type_name(mgamd, number_type)}: {len(V)} x {len(W)} Gram entries, largest "
                  f"|entry| {np.abs(exact).max():.3e}, worst error / bound {ratio:.2e}")
            assert ratio <= 1.0


@pytest.mark.parametrize("case", GRAM_CASES, ids=case_id)
def test_loads_and_mass_operator(mgamd, ctx, case):
    """v^T vmult_mass(w) = int v w, v^T rhs_boundary_flux(q) = sum_f q_f int_f v (the device entry) and v^T rhs(0) = int v, with v (and
    for the mass operator w) vanishing on the Dirichlet faces"""
    geo, L, p = case
    for mask in (M0, M1):
        problem = Problem(SIGMA, None, mask)
        V = bases(p, mask)[0]
        t = mesh(mgamd, geo, L, problem)
        q = np.array([0.0 if (mask >> f) & 1 else 1.0 + 0.5 * f for f in range(6)])
        for number_type in [mgamd.F64] + [mgamd.F32] * (p in (2, 4, 7)):
            lv = Level(mgamd, ctx, t, p, 0, SIGMA, number_type, with_cell_dofs=False)
            Vh = V(*lv.pos.T)
            Y = lv.apply_columns(lv.op.vmult_mass, lv.source(lv.rounded(Vh.T)))
            assert np.all(Y[~lv.free] == 0.0)
            Vf, Yf = Vh[:, lv.free], Y[lv.free]
            e_mass = (np.abs(Vf @ Yf - pe.mass_gram(V, V)) / (lv.tol * (np.abs(Vf) @ np.abs(Yf)))).max()
            b = lv.flux(q)[lv.free]
            e_flux = (np.abs(Vf @ b - pe.face_integrals(V, q)) / (lv.tol * (np.abs(Vf) @ np.abs(b)))).max()
            c = su.vec(lv.op, np.full(lv.n, np.nan))
            lv.op.rhs(c, 0)
            c = c.to_host()[lv.free]
            e_rhs = (np.abs(Vf @ c - pe.integrals(V)) / (lv.tol * (np.abs(Vf) @ np.abs(c)))).max()
            print(f"{case_id(case)} mask={mask:#04x} {type_name(mgamd, number_type)}: error / bound of vmult_mass {e_mass:.2e}, "
                  f"rhs_boundary_flux {e_flux:.2e}, rhs(0) {e_rhs:.2e}")
            assert e_mass <= 1.0 and e_flux <= 1.0 and e_rhs <= 1.0


# ------------------------------------------------------------------ 4. transfers
TRANSFER_CASES = [(geo, L, p, mg_type) for geo, L, p in (("quadrant", 3, 4), ("quadrant", 2, 7), ("circle", 4, 2))
                  for mg_type in ("HMG-global", "PMG", "HPMG")]


def free_of(d):
    return np.arange(d.n_dofs) < d.info.n_interior + d.info.n_tail


@pytest.mark.parametrize("case", TRANSFER_CASES, ids=case_id)
def test_transfers_reproduce_polynomials(mgamd, ctx, case):
    """identity 3 on every level pair under both slot policies and both number types.  Without a Dirichlet face (mask 0, sigma > 0)
    every element of Q_{p_coarse} is reproduced: the harmonic one and the top-degree Legendre product; under ALL the functions that
    vanish on the boundary are (p_coarse >= 2).  Then R is the transpose of P, both sides from the device."""
    rng = np.random.default_rng(5)
    for problem, tag in ((Problem(SIGMA, None, M0), "mask 0"), (Problem(), "ALL")):
        for max_brick in (0, -1):
            for number_type in (mgamd.F64, mgamd.F32):
                h = su.hierarchy(mgamd, ctx, case, problem, max_brick=max_brick, number_type=number_type)
                tol, worst_p, worst_r, n_fn, n_pairs = tol_of(mgamd, number_type), 0.0, 0.0, 0, 0
                for l in range(1, len(h.operators)):
                    dc, df, opc, opf = h.dofs[l - 1], h.dofs[l], h.operators[l - 1], h.operators[l]
                    pc, pf, fc, ff = dc.node_positions(), df.node_positions(), free_of(dc), free_of(df)
                    if problem.dirichlet_faces == M0:
                        top = pe.legendre_basis(dc.degree).subset([-1])
                        fns = [pe.harmonic(dc.degree), lambda x, y, z: top(x, y, z)[0]]
                    elif dc.degree >= 2:
                        zero = pe.legendre_basis(dc.degree, ALL).subset([-1])
                        fns = [lambda x, y, z: zero(x, y, z)[0]]
                    else:
                        fns = []  # no element of Q_1 but 0 vanishes on the whole boundary: this pair has nothing to reproduce
                    n_pairs += bool(fns)
                    for fn in fns:
                        uc, uf = fn(*pc.T), fn(*pf.T)
                        vf, vc = su.vec(opf, np.zeros(df.n_dofs)), su.vec(opc, np.where(fc, uc, 1e30))
                        h.transfers[l].prolongate_and_add(vf, vc)
                        Pw = vf.to_host()
                        assert np.isfinite(Pw).all()
                        worst_p = max(worst_p, np.abs(Pw - uf)[ff].max() / np.abs(uf).max())
                        v = rng.standard_normal(df.n_dofs).astype(np.float32).astype(np.float64)
                        vd = su.vec(opc, np.zeros(dc.n_dofs))
                        h.transfers[l].restrict_and_add(vd, su.vec(opf, v))
                        w = np.where(fc, uc, 0.0)
                        worst_r = max(worst_r, abs(vd.to_host() @ w - v @ Pw) / (tol * (np.abs(v) @ np.abs(Pw))))
                        n_fn += 1
                expected = sum(problem.dirichlet_faces == M0 or d.degree >= 2 for d in h.dofs[:-1])
                print(f"{case_id(case)} {tag} max_brick={max_brick} {type_name(mgamd, number_type)}: {n_pairs} of {len(h.operators) - 1} "
                      f"level pairs checked with {n_fn} functions, prolongation {worst_p:.2e} (bound {tol:.1e}), adjoint error / bound "
                      f"{worst_r:.2e}")
                # every pair under mask 0; under ALL every pair whose coarse degree is at least 2 (circle 4 at p = 2 has none in its
                # PMG and HPMG plans, whose coarse degrees are all 1: they are held under mask 0 alone)
                assert n_pairs == expected and n_fn >= n_pairs
                assert expected > 0 or (tag == "ALL" and case[2] == 2 and case[3] != "HMG-global")
                assert worst_p <= tol and worst_r <= 1.0


# ------------------------------------------------------------------ 5. the solve
@pytest.mark.parametrize("case", [("quadrant", 4, 3, "HMG-global"), ("quadrant", 3, 5, "HMG-global"), ("annulus", 5, 2, "HMG-global"),
                                  ("quadrant", 3, 4, "HPMG")], ids=case_id)
def test_harmonic_polynomial_is_the_solution(mgamd, ctx, case):
    """g = harmonic(p) on all six faces, f = 0: the discrete solution is the polynomial at every node, hanging ones included"""
    p = case[2]
    h = su.hierarchy(mgamd, ctx, case, Problem(), max_brick=0)
    op, d = h.fine_operator, h.dofs[-1]
    exact = pe.harmonic(p)(*d.node_positions().T)
    g, b, u = su.vec(op, exact), op.initialize_dof_vector(), op.initialize_dof_vector()
    op.rhs_dirichlet(b, g)
    it, _ = mgamd.solve_cg(op, h.mg, u, b, 1e-12)
    op.distribute_values(u, g)
    err = np.abs(u.to_host() - exact).max() / np.abs(exact).max()
    print(f"{case_id(case)}: n_dofs {d.n_dofs}, n_hanging {d.info.n_hanging}, CG iterations {it}, relative nodal error {err:.2e}")
    assert d.info.n_hanging > 0 and err <= 1e-8


# ------------------------------------------------------------------ 6. sizes the oracle cannot reach
# Without MGAMD_PERSISTENT_GRID the persistent 17-point brick kernels launch resident_workgroups = 512 workgroups (two per compute
# unit); a mesh draws tickets only with more bricks than that.  The smallest that do:
#   hypercube 6, p = 4   4 096 bricks of 4^3 cells, 17.0 M DoFs
#   quadrant 9, p = 1    3 375 plain and 721 constrained bricks of 16^3 cells in the two halves of the pair kernel, 17.1 M DoFs
#                        (quadrant 8 has 343 and 169)
LARGE = [("hypercube", 6, 4), ("quadrant", 9, 1)]
RESIDENT_WORKGROUPS = 512


@pytest.mark.parametrize("case", LARGE, ids=case_id)
def test_rows_where_the_uncapped_kernels_draw_tickets(mgamd, ctx, case, monkeypatch):
    """the row-wise patch test on vmult, twice (the second pass meets the counters the first one left), FP64 and at p = 4 FP32; at
    p = 4 one Chebyshev step from x = u with b = the lifting leaves u where it is, the residual being zero.
    Wall times on an MI355X machine, host tables included: 5.8 s (hypercube 6, p = 4) and 9.7 s (quadrant 9, p = 1, below the 30 s
    at which it would have been dropped)."""
    monkeypatch.delenv("MGAMD_PERSISTENT_GRID", raising=False)
    geo, L, p = case
    start = time.time()
    problem = Problem()
    t = mesh(mgamd, geo, L, problem)
    for number_type in [mgamd.F64] + [mgamd.F32] * (p == 4):
        lv = Level(mgamd, ctx, t, p, 0, 0.0, number_type)
        bricks = [n for B, n in lv.d.groups() if B * p + 1 == 17 and n > 0]
        assert bricks and min(bricks) > RESIDENT_WORKGROUPS  # resident_workgroups: two per CU, so every workgroup draws tickets
        assert len(bricks) == (2 if p == 1 else 1)  # p = 1: the plain and the constrained half of the pair kernel
        e, n_rows, _ = rows_figure(lv, problem, pe.harmonic(p), passes=2)
        print(f"{case_id(case)} {type_name(mgamd, number_type)}: {lv.n} DoFs, bricks {bricks}, row figure {e:.2e} over {n_rows} rows "
              f"in two passes, bound {RHO * lv.tol:.1e}, {time.time() - start:.1f} s so far")
        assert e <= RHO * lv.tol
        if p == 4 and number_type == mgamd.F64:
            u = pe.harmonic(p)(*lv.pos.T)
            ch = mgamd.PreconditionChebyshev(lv.op, 3, 20.0, 20)
            x, b = su.vec(lv.op, np.where(lv.free, u, 0.0)), su.vec(lv.op, lv.lift(u, True))
            ch.step(x, b)
            es = np.abs(x.to_host() - u)[lv.free].max() / np.abs(u).max()
            print(f"{case_id(case)}: Chebyshev step from the solution moves it by {es:.2e}, bound {RHO * TOL_CHEB:.1e}")
            assert es <= RHO * TOL_CHEB
    print(f"{case_id(case)}: wall time {time.time() - start:.1f} s")
