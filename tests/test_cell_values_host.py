"""Cell evaluate and integrate on the host: the numpy oracle (tests/cell_values_oracle.py) against mathematics, the host functions
DoFs.evaluate / DoFs.integrate (LevelTables::evaluate_values / integrate_values) against the oracle, the tie to the load that exists
(DoFs.rhs_function(1)) and the host-side refusals.  The device kernels are held against the same oracle and the same closed forms by
test_gpu_cell_values.py.

Closed forms (polynomial_exactness.interval_integrals through cell_values_oracle.Products): for a tensor polynomial f and a conforming
v in Q_p with nodal values v_h,
    v_h^T integrate(values = f)    = sum_K int_K f v            f of degree <= 2 n_q - 1 - p per variable,
    v_h^T integrate(gradients = F) = sum_K int_K F . grad v     F_c of degree <= 2 n_q - p in x_c and <= 2 n_q - 1 - p in the other two:
the rule QGauss(n_q) is exact to degree 2 n_q - 1 per variable, v has degree p and d_c v degree p - 1 in x_c and p in the other two
variables, so 2 n_q - p per variable is exact in x_c only (in x_e the integrand F_c d_c v would reach 2 n_q); the F used here has the
largest degrees at which the identity holds.  The sums run over ALL rows that are not hanging (the identity needs the rows of the
boundary nodes): the oracle keeps them (keep_dirichlet), the product runs on a mesh without Dirichlet faces.

Tolerances (from the arithmetic, not from what the code gives):
  * a load, against the oracle or a closed form: 1e-12 B_i, B_i the oracle's load of |data| against |phi_i|, |grad phi_i| through |Ch|:
    the project's per-kernel FP64 bound (README) on the sizes of what is added, not on a sum that may cancel; for v^T b the bound is
    1e-12 sum_i |v_i| B_i;
  * evaluate: 1e-12 max|u| on the leaf for the values and 1e-12 |G|_inf max|u| / h_K for the gradients (|G|_inf the largest row sum of
    the tabulated derivative matrix): (p+1)^3 products per point, each with a few roundings.
The largest measured ratio is printed by every test (DESIGN.md records them)."""
import ctypes as C

import numpy as np
import pytest

import cell_values_oracle as co
import error_estimator_oracle as eo
import mgoracle
import physics_oracle as po
import random_mesh_physics as rm
from physics_oracle import Problem
from support import mesh, tria_of

DEGREES = (1, 2, 3, 4, 5, 6, 7)
TOL = 1e-12


def leaves_of(oracle, name):
    named = dict(quadrant2=("quadrant", 2), quadrant3=("quadrant", 3), hypercube0=("hypercube", 0), hypercube1=("hypercube", 1))
    return mesh(*named[name]) if name in named else rm.leaves_of(oracle, name)


def product(mgamd, oracle, name, p, problem=Problem()):
    """the product's tables on the named leaves, the oracle's space and the permutation x_oracle = x_product[perm]"""
    leaves = leaves_of(oracle, name)
    t = tria_of(mgamd, leaves, problem)
    d = mgamd.DoFs(t, p)
    s = eo.nodal_space(leaves, p)
    assert po.product_cells(t) == [tuple(c) for c in s.cells]
    return t, d, s, eo.to_oracle(s, d.keys(), np.arange(d.n_dofs)).astype(np.int64)


def exact_data(p, n_q, seed):
    """(f, F): the polynomials of the largest degrees at which the two identities hold (see above)"""
    top = 2 * n_q - 1 - p
    F = [co.polynomial([top + (1 if axis == c else 0) for axis in range(3)], seed + 10 * (c + 1)) for c in range(3)]
    return co.polynomial(top, seed), F


def gradient_bound(space, n_q):
    return np.abs(co.shape(space, n_q)[1]).sum(axis=1).max()


def sine(x, y, z):
    return np.sin(2.0 * x + 0.5) * np.cos(1.5 * y) + 0.3 * z * z * x


def sine_gradient(x, y, z):
    return (2.0 * np.cos(2.0 * x + 0.5) * np.cos(1.5 * y) + 0.3 * z * z, -1.5 * np.sin(2.0 * x + 0.5) * np.sin(1.5 * y), 0.6 * z * x)


@pytest.mark.parametrize("p", DEGREES)
def test_oracle_against_closed_forms(p):
    """the oracle against mathematics on quadrant 2 (hanging faces and edges), all three n_q"""
    s = eo.nodal_space(mesh("quadrant", 2), p)
    pos = mgoracle.Level.node_positions(s)
    v = co.polynomial(p, 10 + p)
    x = np.where(s.hanging, 0.0, v(*pos.T))  # (the hanging rows of a load are 0)
    forms = co.Products(p + 6)
    worst = worst_e = 0.0
    for n_q in (p + 1, p + 2, p + 3):
        f, F = exact_data(p, n_q, 20 + p)
        fq = co.tabulate(s.cells, n_q, f)
        Fq = np.stack([co.tabulate(s.cells, n_q, c) for c in F], axis=1)
        for values, gradients, ref in ((fq, None, forms.source(s.cells, f, v)), (None, Fq, forms.divergence_form(s.cells, F, v)),
                                       (fq, Fq, forms.source(s.cells, f, v) + forms.divergence_form(s.cells, F, v))):
            got = x @ co.integrate(s, values, gradients, n_q, keep_dirichlet=True)
            size = np.abs(x) @ co.integrate(s, values, gradients, n_q, absolute=True, keep_dirichlet=True)
            worst = max(worst, abs(got - ref) / size)
        # evaluate of a polynomial of Q_p is the polynomial at the points (NaN in the hanging entries: never used)
        u, g = co.evaluate(s, np.where(s.hanging, np.nan, v(*pos.T)), n_q)
        ref_u, ref_g = co.tabulate(s.cells, n_q, v, lambda *X: tuple(v.deriv(axis)(*X) for axis in range(3)))
        top = np.abs(ref_u).reshape(len(s.cells), -1).max(axis=1)
        worst_e = max(worst_e, (np.abs(u - ref_u).reshape(len(s.cells), -1).max(axis=1) / top).max(),
                      (np.abs(g - ref_g).reshape(len(s.cells), -1).max(axis=1) / (gradient_bound(s, n_q) * top / co.cell_h(s.cells))).max())
    print(f"p={p}: max |v^T b - closed form| / sum |v_i| B_i = {worst:.2e}, evaluate against the polynomial {worst_e:.2e}")
    assert worst <= TOL and worst_e <= TOL


@pytest.mark.parametrize("p", [1, 2, 3])
def test_oracle_contraction_order(p):
    """the oracle's einsums with numpy's own ordering (optimize=True, what the tests use) against the plain loop over all indices"""
    s = eo.nodal_space(mesh("quadrant", 2), p)
    rng = np.random.default_rng(p)
    for n_q in (p + 1, p + 3):
        x = rng.standard_normal(s.n)
        values, gradients = rng.standard_normal((len(s.cells),) + (n_q,) * 3), rng.standard_normal((len(s.cells), 3) + (n_q,) * 3)
        size = co.integrate(s, values, gradients, n_q, absolute=True, optimize=False)
        assert (np.abs(co.integrate(s, values, gradients, n_q) - co.integrate(s, values, gradients, n_q, optimize=False)) <= 1e-14 * size).all()
        for fast, plain in zip(co.evaluate(s, x, n_q), co.evaluate(s, x, n_q, optimize=False)):
            assert np.abs(fast - plain).max() <= 1e-13 * np.abs(plain).max()


@pytest.mark.parametrize("name,degrees", [("quadrant2", DEGREES), ("quadrant3", (1, 2, 4, 7)), ("S", (1, 3, 5, 7))])
def test_host_functions_against_oracle(mgamd, oracle, name, degrees):
    """DoFs.evaluate and DoFs.integrate against the oracle: a seeded vector with NaN in the hanging entries; seeded data and a function
    that is no polynomial; values only, gradients only, both; all three n_q"""
    worst_b = worst_e = 0.0
    for p in degrees:
        t, d, s, perm = product(mgamd, oracle, name, p)
        rng = np.random.default_rng(30 + p)
        x = rng.standard_normal(d.n_dofs)
        if d.info.n_hanging:
            x[d.n_dofs - d.info.n_hanging:] = np.nan
        for n_q in (p + 1, p + 2, p + 3):
            assert np.array_equal(d.quadrature_points(n_q), d.quadrature_points(n_q))
            u, g = d.evaluate(x, n_q, True, True)
            ref_u, ref_g = co.evaluate(s, np.nan_to_num(x)[perm], n_q)
            assert np.array_equal(u, d.evaluate(x, n_q)) and np.array_equal(g, d.evaluate(x, n_q, False, True))
            nodal = np.abs((s.Ch @ np.nan_to_num(x)[perm])[s.cell_dofs]).max(axis=1)
            worst_e = max(worst_e, (np.abs(u - ref_u).reshape(len(s.cells), -1).max(axis=1) / nodal).max(),
                          (np.abs(g - ref_g).reshape(len(s.cells), -1).max(axis=1) / (gradient_bound(s, n_q) * nodal / co.cell_h(s.cells))).max())
            shape = (len(s.cells), n_q, n_q, n_q)
            for values, gradients in ((rng.standard_normal(shape), rng.standard_normal((shape[0], 3) + shape[1:])),
                                      co.tabulate(s.cells, n_q, sine, sine_gradient)):
                for v_, g_ in ((values, None), (None, gradients), (values, gradients)):
                    b = d.integrate(v_, g_, n_q)
                    assert (b[d.n_dofs - d.info.n_hanging - d.info.n_dirichlet:] == 0.0).all()
                    ref, size = co.integrate(s, v_, g_, n_q), co.integrate(s, v_, g_, n_q, absolute=True)
                    free = size > 0
                    assert (b[perm][~free] == 0.0).all()
                    worst_b = max(worst_b, (np.abs(b[perm] - ref)[free] / size[free]).max())
        data = rng.standard_normal((len(s.cells),) + (p + 2,) * 3)
        assert np.array_equal(d.integrate(data, None, 0), d.integrate(data, None, p + 2))  # 0 stands for p + 2
    print(f"{name}: integrate max |b_i - oracle| / B_i = {worst_b:.2e}, evaluate max error / bound = {worst_e:.2e}")
    assert worst_b <= TOL and worst_e <= TOL


@pytest.mark.parametrize("name", ["quadrant2", "quadrant3", "S"])
@pytest.mark.parametrize("sigma", [0.0, 3.0])
def test_reproduces_the_builtin_gaussian_load(mgamd, oracle, name, sigma):
    """the tie to the path that exists: integrate(values = f at the p + 1 points) + rhs_dirichlet(g) is DoFs.rhs_function(1), with
    f = -Laplace u_g + sigma u_g and g = u_g of the Gaussian restated by the oracle (mgoracle.gaussian_rhs, gaussian_solution) -- rhs_dirichlet
    returns the NEGATIVE lifting, so the two are added.  The bound is on the sizes of both parts."""
    worst = 0.0
    for p in (1, 2, 4, 7):
        t, d, s, perm = product(mgamd, oracle, name, p)
        d.set_mass_coefficient(sigma)
        f = co.tabulate(s.cells, p + 1, lambda x, y, z: mgoracle.gaussian_rhs(x, y, z) + sigma * mgoracle.gaussian_solution(x, y, z))
        g = mgoracle.gaussian_solution(*d.node_positions().T)
        load, lift, ref = d.integrate(f, None, p + 1), d.rhs_dirichlet(g), d.rhs_function(1)
        size = co.integrate(s, f, None, p + 1, absolute=True)
        bound = TOL * (size + np.abs(lift[perm]))
        on = bound > 0
        assert np.array_equal((load + lift)[perm][~on], ref[perm][~on])
        worst = max(worst, (np.abs(load + lift - ref)[perm][on] / bound[on]).max())
    print(f"{name} sigma={sigma}: max |integrate + lifting - rhs_function(1)| / (1e-12 (B_i + |lifting_i|)) = {worst:.2e}")
    assert worst <= 1.0


def test_host_refusals(mgamd):
    plain = mgamd.Triangulation("quadrant", 3)
    d = mgamd.DoFs(plain, 2)
    E = mgamd.MgamdError
    values, gradients, u = np.zeros((120, 4, 4, 4)), np.zeros((120, 3, 4, 4, 4)), np.zeros(d.n_dofs)
    for n_q in (-1, 1, 2, 6, 11, 1000):
        with pytest.raises(E, match=rf"integrate: n_q = {n_q} refused"):
            d.integrate(values, None, n_q)
        with pytest.raises(E, match=rf"evaluate: n_q = {n_q} refused"):
            d.evaluate(u, n_q)
    with pytest.raises(E, match="integrate: neither values nor gradients"):
        d.integrate()
    with pytest.raises(E, match="evaluate: neither values nor gradients"):
        d.evaluate(u, 0, False, False)
    with pytest.raises(ValueError, match="integrate: 1 values"):
        d.integrate(np.zeros(1))
    with pytest.raises(ValueError, match="evaluate"):
        d.evaluate(np.zeros(d.n_dofs + 1))
    lib = C.CDLL(mgamd._LIB_PATH)
    lib.mgamd_last_error.restype = C.c_char_p
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mgamd_dofs_integrate(d._h, ptr(values), None, 0, None) == 3 and b"integrate: out is null" in lib.mgamd_last_error()
    assert lib.mgamd_dofs_evaluate(d._h, None, 0, ptr(values), None) == 3 and b"evaluate: u is null" in lib.mgamd_last_error()
    assert lib.mgamd_dofs_integrate(None, ptr(values), None, 0, ptr(u)) == 3 and b"null argument" in lib.mgamd_last_error()
    ls = mgamd.DoFs(plain.level_mesh(2), 2, local_smoothing_level=True)
    with pytest.raises(E, match="integrate: refused on the level of a local-smoothing hierarchy"):
        ls.integrate(np.zeros((ls.info.n_cells, 4, 4, 4)))
    with pytest.raises(E, match="evaluate: refused on the level of a local-smoothing hierarchy"):
        ls.evaluate(np.zeros(ls.n_dofs))
    trias = mgamd.create_geometric_coarsening_sequence(plain)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    sharded = mgamd.DoFs(trias[-1], 2, 0, partition=part, level=len(trias) - 1, rank=0)
    with pytest.raises(E, match="integrate: not implemented: sharded"):
        sharded.integrate(np.zeros((sharded.info.n_cells, 4, 4, 4)))
    with pytest.raises(E, match="evaluate: not implemented: sharded"):
        sharded.evaluate(np.zeros(sharded.n_dofs))
