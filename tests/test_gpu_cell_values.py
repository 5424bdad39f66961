"""Cell evaluate and integrate on the device (Operator.evaluate: cell_evaluate_kernel, Operator.integrate: cell_integrate_kernel) against
tests/cell_values_oracle.py, against closed forms, against the kernels that exist (vmult_mass, vmult), in a solve, in the time stepper
and in the example; the lazily built shared gather table and the refusals.

Meshes, those of test_gpu_error_norm.py for the same reasons: hypercube 0 (one leaf: a partial group at every degree), hypercube 1
(8 leaves: less than one group at p = 1 and 2), quadrant 3 (120 leaves, hanging faces and edges, several groups) and the random octree S
(50 leaves, levels 1-3).  cell_evaluate_kernel packs 32, 9, 4, 2, 1, 1, 1 leaves per workgroup pass at p = 1 ... 7, cell_integrate_kernel
16, 9, 4, 2, 1, 1, 1 (its four buffers of (p+3)^3 doubles per leaf leave room for 16 leaves at p = 1), and both give two groups to a
workgroup (test_partial_groups).  Degrees 1 ... 7, both number types, per_family coefficient and sigma = 3 where they enter.

Tolerances (from the arithmetic, not from what the kernels give):
  * evaluate, FP64: values <= 1e-12 max|u| on the leaf (the largest nodal value the leaf gathers), gradients <= 1e-12 |G|_inf max|u| / h_K
    (|G|_inf the largest row sum of the tabulated 1D derivative matrix): (p+1)^3 products per point, each with a few roundings;
  * evaluate, FP32: the kernel converts at the load, computes in double and converts at the store, so its result is BIT-identical to
    the FP64 operator's on the double vector that holds the same float values, rounded to float;
  * integrate: |b_i - oracle_i| <= tol B_i, B_i the oracle's load of |data| against |phi_i|, |grad phi_i| through |Ch| (a bound on the sizes
    of what is added, not on a sum that may cancel); tol = 1e-12 in FP64 and 2e-6 in FP32, the project's per-kernel bounds (README): the
    arithmetic is double up to the scatter and the float atomics add at most a few ulp (6e-8) per addend.  For v^T b the bound is
    tol sum_i |v_i| B_i;
  * the solve: per leaf |u_h - u*|_L2(K) <= 1e-10 |u*|_L2(cube), the project's bound on a CG iterate (TOL_SOL) with the global norm of
    u* as the size: the CG's reltol bounds the global residual, not a leaf's; the discrete solution is u* itself;
  * the example against the oracle's own solve: 1e-9 relative, on two CG iterates at reltol 1e-12.
The largest measured ratios are printed by every test (DESIGN.md records them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import cell_values_oracle as co
import error_estimator_oracle as eo
import error_norm_oracle as no
import physics_oracle as po
import random_mesh_physics as rm
import time_stepping_oracle as ts
from conftest import ROOT, rel_err
from physics_oracle import Problem
from support import TOL_SOL, layers, mesh, oracle_level_on, run_ranks, space, tria_of

pytestmark = pytest.mark.gpu

TOL, TOL_F32 = 1e-12, 2e-6
DEGREES = (1, 2, 3, 4, 5, 6, 7)
MESHES = ("hypercube0", "hypercube1", "quadrant3", "S")
SIGMA = 3.0
PHYSICS = Problem(coefficient="per_family", sigma=SIGMA)
NATURAL = Problem(coefficient="per_family", sigma=SIGMA, dirichlet_faces=0)  # every row of a non-hanging node is a free row


def leaves_of(oracle, name):
    named = dict(hypercube0=("hypercube", 0), hypercube1=("hypercube", 1), quadrant3=("quadrant", 3))
    return mesh(*named[name]) if name in named else rm.leaves_of(oracle, name)


_built = {}


def build(mgamd, ctx, oracle, name, p, number_type=8, problem=PHYSICS):
    """the product's mesh, tables (mass coefficient set before the operator is built) and operator on the named leaves, the oracle's
    space, the coefficient per leaf, and the permutation that brings a vector of the product's numbering to the space's"""
    tag = (name, p, number_type, id(problem))
    if tag not in _built:
        leaves = leaves_of(oracle, name)
        t = tria_of(mgamd, leaves, problem)
        d = mgamd.DoFs(t, p)
        d.set_mass_coefficient(problem.sigma)
        op = mgamd.Operator(ctx, d, number_type)
        s = eo.nodal_space(leaves, p)
        assert po.product_cells(t) == [tuple(c) for c in s.cells]
        a = po.product_values(t, eo.on(problem, s.cells).coefficient)
        perm = eo.to_oracle(s, d.keys(), np.arange(d.n_dofs)).astype(np.int64)
        _built[tag] = (t, d, op, s, a, perm)
    return _built[tag]


def vec(op, x):
    return op.initialize_dof_vector().from_host(x)


def rounded(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def sine(x, y, z):
    return np.sin(2.0 * x + 0.5) * np.cos(1.5 * y) + 0.3 * z * z * x


def sine_gradient(x, y, z):
    return (2.0 * np.cos(2.0 * x + 0.5) * np.cos(1.5 * y) + 0.3 * z * z, -1.5 * np.sin(2.0 * x + 0.5) * np.sin(1.5 * y), 0.6 * z * x)


def shaped(v, s, n_q, components=None):
    shape = (len(s.cells),) + (() if components is None else (components,)) + (n_q,) * 3
    return v.to_host().reshape(shape)


def integrate(op, d, values, gradients, n_q, prefill=np.nan):
    """Operator.integrate into a vector pre-filled with NaN; nothing may be NaN afterwards and the constrained tail is exactly 0"""
    b = vec(op, np.full(d.n_dofs, prefill))
    op.integrate(b, values, gradients, n_q)
    out = b.to_host()
    assert np.isfinite(out).all()
    assert (out[d.n_dofs - d.info.n_hanging - d.info.n_dirichlet:] == 0.0).all()
    return out


def test_partial_groups(oracle):
    """test_gpu_error_norm.py's test_partial_groups for the leaves per pass of the two kernels: for every degree at least one mesh leaves
    the last group of leaves partial; where a group is one leaf (p >= 5) at least one mesh has an odd number of groups, so that the last
    workgroup (two groups each) runs a partial trip of the grid stride"""
    counts = [len(leaves_of(oracle, name)) for name in MESHES]
    assert counts == [1, 8, 120, 50]
    for p in DEGREES:
        for per_group in (max(1, 256 // (p + 1) ** 3), 16 if p == 1 else max(1, 256 // (p + 1) ** 3)):
            assert any(n % per_group for n in counts) if per_group > 1 else any(n % 2 for n in counts)
            assert any(n > 2 * per_group for n in counts)  # more than one workgroup
    assert 8 < 32 and 8 < 16 and 8 < 9  # hypercube 1: less than one group at p = 1 and 2, in either kernel


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("p", DEGREES)
def test_evaluate_against_oracle(mgamd, ctx, oracle, name, p):
    """case 1: a seeded vector (NaN in the hanging entries) and a polynomial of Q_p, all three n_q, values and gradients separately and
    together; FP32 bit-identical to FP64 on the rounded input, rounded; two calls give the same bits"""
    t, d, op, s, a, perm = build(mgamd, ctx, oracle, name, p)
    op32 = build(mgamd, ctx, oracle, name, p, mgamd.F32)[2]
    v = co.polynomial(p, 10 + p)
    random = np.random.default_rng(30 + p).standard_normal(d.n_dofs)
    h = co.cell_h(s.cells)
    worst = 0.0
    for x in (random, v(*d.node_positions().T)):
        nan = x.copy()
        nan[d.n_dofs - d.info.n_hanging:] = np.nan
        nodal = np.abs((s.Ch @ np.where(s.hanging, 0.0, x[perm]))[s.cell_dofs]).max(axis=1)
        for n_q in (p + 1, p + 2, p + 3):
            both = op.evaluate(vec(op, nan), n_q, True, True)
            u, g = shaped(both[0], s, n_q), shaped(both[1], s, n_q, 3)
            assert np.isfinite(u).all() and np.isfinite(g).all()
            # separately, a second call, the hanging entries readable: the same bits
            assert np.array_equal(op.evaluate(vec(op, x), n_q).to_host(), both[0].to_host())
            assert np.array_equal(op.evaluate(vec(op, x), n_q, False, True).to_host(), both[1].to_host())
            again = op.evaluate(vec(op, nan), n_q, True, True)
            assert np.array_equal(again[0].to_host(), both[0].to_host()) and np.array_equal(again[1].to_host(), both[1].to_host())
            ref_u, ref_g = co.evaluate(s, np.where(s.hanging, 0.0, x[perm]), n_q)
            worst = max(worst, (np.abs(u - ref_u).reshape(len(s.cells), -1).max(axis=1) / nodal).max(),
                        (np.abs(g - ref_g).reshape(len(s.cells), -1).max(axis=1) / (np.abs(co.shape(s, n_q)[1]).sum(axis=1).max() * nodal / h)).max())
            if x is not random:  # the polynomial itself at the points
                pts = co.tabulate(s.cells, n_q, v, no.gradient_of(v))
                top = np.abs(pts[0]).reshape(len(s.cells), -1).max(axis=1)
                assert (np.abs(u - pts[0]).reshape(len(s.cells), -1).max(axis=1) <= TOL * top).all()
            # FP32: conversion at the load and at the store, FP64 between
            u64, g64 = op.evaluate(vec(op, rounded(nan)), n_q, True, True)
            u32, g32 = op32.evaluate(vec(op32, nan), n_q, True, True)
            assert np.array_equal(u32.to_host(), rounded(u64.to_host())) and np.array_equal(g32.to_host(), rounded(g64.to_host()))
    print(f"{name} p={p}: {len(s.cells)} leaves, evaluate max error / (1e-12 bound's size) = {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("p", DEGREES)
def test_integrate_against_oracle(mgamd, ctx, oracle, name, p):
    """case 2: seeded data and tabulated data of a function that is no polynomial; values only, gradients only, both; b pre-filled with
    NaN; FP32 against the oracle on the rounded data; on one leaf two FP64 calls give the same bits (one addend per row)"""
    t, d, op, s, a, perm = build(mgamd, ctx, oracle, name, p)
    op32 = build(mgamd, ctx, oracle, name, p, mgamd.F32)[2]
    rng = np.random.default_rng(40 + p)
    worst = worst32 = 0.0
    for n_q in (p + 1, p + 2, p + 3):
        shape = (len(s.cells), n_q, n_q, n_q)
        for values, gradients in ((rng.standard_normal(shape), rng.standard_normal((shape[0], 3) + shape[1:])),
                                  co.tabulate(s.cells, n_q, sine, sine_gradient)):
            values, gradients = rounded(values), rounded(gradients)  # (the same numbers in both number types)
            for v_, g_ in ((values, None), (None, gradients), (values, gradients)):
                ref, size = co.integrate(s, v_, g_, n_q), co.integrate(s, v_, g_, n_q, absolute=True)
                on = size > 0
                for o, tol in ((op, TOL), (op32, TOL_F32)):
                    b = integrate(o, d, v_, g_, n_q)
                    assert (b[perm][~on] == 0.0).all()
                    ratio = (np.abs(b[perm] - ref)[on] / size[on]).max() if on.any() else 0.0  # (one leaf at p = 1 has no free row)
                    worst, worst32 = (max(worst, ratio), worst32) if o is op else (worst, max(worst32, ratio))
                if name == "hypercube0":
                    assert np.array_equal(integrate(op, d, v_, g_, n_q), integrate(op, d, v_, g_, n_q, prefill=0.0))
    print(f"{name} p={p}: integrate max |b_i - oracle| / B_i = {worst:.2e} (FP64), {worst32:.2e} (FP32)")
    assert worst <= TOL and worst32 <= TOL_F32


@pytest.mark.parametrize("p", DEGREES)
def test_closed_forms(mgamd, ctx, oracle, p):
    """case 3: the v^T b identities of test_cell_values_host.py on the device, on the octree S without Dirichlet faces (every row of a
    non-hanging node is free): v_h^T integrate(f) = sum_K int_K f v for f of degree 2 n_q - 1 - p per variable, and
    v_h^T integrate(gradients = F) = sum_K int_K F . grad v for F_c of degree 2 n_q - p in x_c and 2 n_q - 1 - p in the other two"""
    t, d, op, s, a, perm = build(mgamd, ctx, oracle, "S", p, problem=NATURAL)
    assert d.info.n_dirichlet == 0
    v = co.polynomial(p, 10 + p)
    x = v(*d.node_positions().T)
    x[d.n_dofs - d.info.n_hanging:] = 0.0
    forms = co.Products(p + 6)
    worst = 0.0
    for n_q in (p + 1, p + 2, p + 3):
        top = 2 * n_q - 1 - p
        f = co.polynomial(top, 20 + p)
        F = [co.polynomial([top + (1 if axis == c else 0) for axis in range(3)], 20 + p + 10 * (c + 1)) for c in range(3)]
        fq = co.tabulate(s.cells, n_q, f)
        Fq = np.stack([co.tabulate(s.cells, n_q, c) for c in F], axis=1)
        for values, gradients, ref in ((fq, None, forms.source(s.cells, f, v)), (None, Fq, forms.divergence_form(s.cells, F, v)),
                                       (fq, Fq, forms.source(s.cells, f, v) + forms.divergence_form(s.cells, F, v))):
            size = np.abs(x[perm]) @ co.integrate(s, values, gradients, n_q, absolute=True, keep_dirichlet=True)
            worst = max(worst, abs(x @ integrate(op, d, values, gradients, n_q) - ref) / size)
    print(f"p={p}: max |v^T b - closed form| / sum |v_i| B_i = {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("p", DEGREES)
def test_identities_against_existing_kernels(mgamd, ctx, oracle, p):
    """case 4: integrate(values = evaluate(u)) is vmult_mass(u) and integrate(values = sigma u_q, gradients = a_K grad u_q) is vmult(u) on
    the free rows, for u zero on the Dirichlet entries, every n_q (the integrands have degree 2p <= 2 n_q - 1), both number types; the
    bound is case 2's, B_i from the sizes of the data"""
    worst = {}
    for number_type, tol in ((mgamd.F64, TOL), (mgamd.F32, TOL_F32)):
        t, d, op, s, a, perm = build(mgamd, ctx, oracle, "quadrant3", p, number_type)
        x = rounded(np.random.default_rng(50 + p).standard_normal(d.n_dofs))
        x[d.n_dofs - d.info.n_hanging - d.info.n_dirichlet:] = 0.0
        free = slice(0, d.n_dofs - d.info.n_hanging - d.info.n_dirichlet)
        mass, stiff = vec(op, np.full(d.n_dofs, np.nan)), vec(op, np.full(d.n_dofs, np.nan))
        op.vmult_mass(mass, vec(op, x))
        op.vmult(stiff, vec(op, x))
        for n_q in (p + 1, p + 2, p + 3):
            u, g = op.evaluate(vec(op, x), n_q, True, True)
            uq, gq = shaped(u, s, n_q), shaped(g, s, n_q, 3)
            size = co.integrate(s, uq, None, n_q, absolute=True)[np.argsort(perm)]
            ratio = (np.abs(integrate(op, d, u, None, n_q) - mass.to_host())[free] / size[free]).max()
            data = (SIGMA * uq, a[:, None, None, None, None] * gq)
            size = co.integrate(s, *data, n_q, absolute=True)[np.argsort(perm)]
            ratio = max(ratio, (np.abs(integrate(op, d, *data, n_q) - stiff.to_host())[free] / size[free]).max())
            worst[number_type] = max(worst.get(number_type, 0.0), ratio / tol)
    print(f"p={p}: integrate(evaluate(u)) against vmult_mass and vmult, max difference / (tol B_i) = {worst[8]:.2e} (FP64), {worst[4]:.2e} (FP32)")
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("p", DEGREES)
def test_negative_control(mgamd, ctx, oracle, p):
    """case 5: another data at the points of ONE leaf with a hanging face changes exactly the rows that leaf gathers, through hanging
    nodes included; every other row keeps its bits where it has one addend and stays within the bound elsewhere"""
    t, d, op, s, a, perm = build(mgamd, ctx, oracle, "quadrant3", p)
    n_q, rng = p + 2, np.random.default_rng(60 + p)
    values = rng.standard_normal((len(s.cells),) + (n_q,) * 3)
    gradients = rng.standard_normal((len(s.cells), 3) + (n_q,) * 3)
    # the leaf with the most rows it reaches through hanging nodes only
    direct = lambda ci: np.isin(np.arange(s.n), s.cell_dofs[ci])
    ci = max(range(len(s.cells)), key=lambda c: int((co.rows_of_leaf(s, c) & ~direct(c)).sum()))
    rows = co.rows_of_leaf(s, ci)
    assert 0 < (rows & ~direct(ci)).sum() and rows.sum() < (~(s.hanging | s.dirichlet)).sum()
    moved_v, moved_g = values.copy(), gradients.copy()
    moved_v[ci] += 1.0 + rng.random(values[ci].shape)
    moved_g[ci] += 1.0 + rng.random(gradients[ci].shape)
    before, after = integrate(op, d, values, gradients, n_q)[perm], integrate(op, d, moved_v, moved_g, n_q)[perm]
    ref, size = co.integrate(s, moved_v, moved_g, n_q), co.integrate(s, moved_v, moved_g, n_q, absolute=True)
    single = co.addends(s) == 1
    free = ~(s.hanging | s.dirichlet)
    assert (after[rows] != before[rows]).all()
    assert np.array_equal(after[free & ~rows & single], before[free & ~rows & single])
    assert (free & ~rows & single).any() or p == 1  # (at p = 1 every DoF is a vertex that several leaves share)
    shared = free & ~rows & ~single
    assert (np.abs(after - before)[shared] <= 2.0 * TOL * size[shared]).all()
    worst = (np.abs(after - ref)[free] / size[free]).max()
    print(f"p={p}: leaf {ci} adds into {rows.sum()} rows ({(rows & ~direct(ci)).sum()} through hanging nodes only); {int((free & ~rows & single).sum())} "
          f"other rows with one addend keep their bits; max |b_i - oracle| / B_i = {worst:.2e}")
    assert worst <= TOL


def polynomial_problem(mgamd, ctx, oracle, name, p):
    t = tria_of(mgamd, leaves_of(oracle, name), PHYSICS)
    return mgamd.Hierarchy(ctx, t, None, p, "HMG-global", coarse_solver="amg", mass_coefficient=SIGMA), t


@pytest.mark.parametrize("name", ["quadrant3", "S"])
@pytest.mark.parametrize("p", [1, 2, 4, 7])
def test_solve(mgamd, ctx, oracle, name, p):
    """case 6: u* in Q_p, per_family a, sigma = 3, Dirichlet data u* at node_positions, the load in divergence form (gradients = a_K grad
    u*, values = sigma u*) at n_q = p + 1 (the integrands have degree 2p): the discrete solution is u* itself"""
    h, t = polynomial_problem(mgamd, ctx, oracle, name, p)
    op, d = h.fine_operator, h.dofs[-1]
    u_star = co.polynomial(p, 70 + p)
    grad = no.gradient_of(u_star)
    a = t.coefficient()[:, None, None, None]
    g = vec(op, u_star(*d.node_positions().T))
    b, lift, x = op.initialize_dof_vector(), op.initialize_dof_vector(), op.initialize_dof_vector()
    op.integrate(b, lambda *X: SIGMA * u_star(*X), lambda *X: tuple(a * c for c in grad(*X)), p + 1)
    op.rhs_dirichlet(lift, g)
    b.from_host(b.to_host() + lift.to_host())
    it, res = mgamd.solve_cg(op, h.mg, x, b, 1e-12)
    op.distribute_values(x, g)
    cells = po.product_cells(t)
    size = np.sqrt(np.sum(no.ClosedForms(p).norms(cells, u_star)[no.L2] ** 2))
    err = op.integrate_difference(x, (u_star, grad), mgamd.NORM_L2)
    print(f"{name} p={p}: {it} CG iterations, max per-leaf L2 error / |u*|_L2 = {err.max() / size:.2e}")
    assert err.max() <= TOL_SOL * size


def test_time_stepper_load(mgamd, ctx, oracle):
    """case 6, the time stepper: one theta step whose source enters as a LOAD from Operator.integrate of a callable,
    l = theta l(t + dt) + (1 - theta) l(t) through the stepper's `load` argument (its f_old / f_new are nodal values that it multiplies
    by the mass matrix; a quadrature load goes where the boundary loads go), against tests/time_stepping_oracle.py's step restated with
    the oracle's load: r = M sigma u + l - A u"""
    theta, dt, p = 0.5, 0.05, 2
    sigma = mgamd.TimeStepper.mass_coefficient(theta, dt)
    leaves = mesh("quadrant", 3)
    h = mgamd.Hierarchy(ctx, tria_of(mgamd, leaves), None, p, "HMG-global", coarse_solver="amg", mass_coefficient=sigma)
    op, d = h.fine_operator, h.dofs[-1]
    lv = oracle_level_on(d, leaves, p, Problem(sigma=sigma))
    source = lambda time: (lambda x, y, z: (1.0 + time) * sine(x, y, z))
    u0 = np.where(lv.constrained, 0.0, np.sin(0.37 * np.arange(lv.n)) + 0.25)
    load = np.zeros(lv.n)
    dev = op.initialize_dof_vector()
    total = vec(op, np.zeros(d.n_dofs))
    for time, weight in ((0.0, 1.0 - theta), (dt, theta)):
        load += weight * co.integrate(lv, co.tabulate(lv.cells, p + 2, source(time)), None, p + 2)  # (lv: the product's numbering)
        op.integrate(dev, source(time))
        total.from_host(total.to_host() + weight * dev.to_host())
    u = vec(op, u0)
    mgamd.TimeStepper(op, h.mg, theta, dt).step(u, load=total, reltol=1e-12)
    r = ts.mass_matrix(lv) @ (sigma * u0) + load - lv.A @ u0
    r[lv.constrained] = 0.0
    ref = u0 + ts.exact_solver(lv)(r / theta)[0]
    ref[lv.constrained] = 0.0
    err = rel_err(u.to_host(), ref)
    print(f"one theta step with an integrated load: iterate against the oracle {err:.2e}, |load| {np.abs(load).max():.2e}")
    assert err <= TOL_SOL and np.abs(ref - u0).max() > 1e-3


def test_lazy_allocation_and_the_shared_table(mgamd, ctx):
    """case 7: a fresh operator holds nothing; evaluate and integrate build the shared gather table only, neither the indicator's
    neighbour table nor the norms' arrays; the norms and the indicator afterwards use the same copy"""
    t = mgamd.Triangulation("quadrant", 3)
    d = mgamd.DoFs(t, 3)
    op, other = mgamd.Operator(ctx, d), mgamd.Operator(ctx, d)
    assert op._cell_values_info() == (0, 0.0, 0.0) and op._error_norm_info() == (0, 0.0, False) and op._estimator_info() == (0, 0.0, 0.0)
    x = vec(op, np.random.default_rng(80).standard_normal(d.n_dofs))
    n, gather = 4, 120 * (4 * 4 ** 3 + 18)
    values = op.evaluate(x)
    nbytes, evaluate_ms, integrate_ms = op._cell_values_info()
    assert nbytes == gather and evaluate_ms > 0 and integrate_ms == 0.0
    op.integrate(op.initialize_dof_vector(), values)
    assert op._cell_values_info()[0] == gather and op._cell_values_info()[2] > 0
    assert op._error_norm_info() == (0, 0.0, False) and op._estimator_info()[0] == 0
    other.integrate(other.initialize_dof_vector(), values)  # integrate first
    assert other._cell_values_info()[0] == gather and other._cell_values_info()[1] == 0.0 and other._error_norm_info() == (0, 0.0, False)
    # the norms and the indicator on top: ONE copy of the table
    norm = op.integrate_difference(x, 0, no.L2)
    assert op._error_norm_info()[0] == gather + 120 * 32 and not op._error_norm_info()[2]
    eta = op.estimate_error(x)
    assert op._estimator_info()[0] == 120 * (4 * n ** 3 + 48 * n ** 2 + 128) and op._cell_values_info()[0] == gather
    fresh = mgamd.Operator(ctx, d)
    assert np.array_equal(fresh.integrate_difference(vec(fresh, x.to_host()), 0, no.L2), norm)
    assert np.array_equal(fresh.estimate_error(vec(fresh, x.to_host())), eta)
    assert fresh._cell_values_info() == (0, 0.0, 0.0)
    assert np.array_equal(fresh.evaluate(vec(fresh, x.to_host())).to_host(), values.to_host())


def test_refusals(mgamd, ctx):
    """case 8: every device-side refusal, by name; a refused call builds nothing"""
    plain = mgamd.Triangulation("quadrant", 3)
    d = mgamd.DoFs(plain, 2)
    op = mgamd.Operator(ctx, d)
    u, b, n_points = op.initialize_dof_vector(), op.initialize_dof_vector(), 120 * 4 ** 3
    values, gradients = mgamd.Vector(ctx, n_points), mgamd.Vector(ctx, 3 * n_points)
    E = mgamd.MgamdError
    lib = C.CDLL(mgamd._LIB_PATH)
    lib.mgamd_last_error.restype = C.c_char_p
    refused = lambda status, text: status == 3 and text in lib.mgamd_last_error()
    # integrate
    with pytest.raises(E, match="integrate: vector size mismatch"):
        op.integrate(mgamd.Vector(ctx, d.n_dofs + 1), values)
    with pytest.raises(E, match="number type"):
        op.integrate(mgamd.Vector(ctx, d.n_dofs, mgamd.F32), values)
    with pytest.raises(E, match="integrate: values size mismatch"):
        op.integrate(b, mgamd.Vector(ctx, n_points + 1))
    with pytest.raises(E, match="integrate: values size mismatch"):
        op.integrate(b, values, None, 5)  # (the data of n_q = 4 at n_q = 5)
    with pytest.raises(E, match="number type"):
        op.integrate(b, mgamd.Vector(ctx, n_points, mgamd.F32))
    with pytest.raises(E, match="integrate: gradients size mismatch"):
        op.integrate(b, values, mgamd.Vector(ctx, n_points))
    with pytest.raises(E, match="number type"):
        op.integrate(b, None, mgamd.Vector(ctx, 3 * n_points, mgamd.F32))
    with pytest.raises(E, match="integrate: neither values nor gradients"):
        op.integrate(b)
    with pytest.raises(E, match="integrate: b is null"):
        op.integrate(None, values)
    with pytest.raises(E, match="integrate: b aliases values"):
        op.integrate(b, b)
    with pytest.raises(E, match="integrate: b aliases gradients"):
        op.integrate(b, values, b)
    for n_q in (-1, 1, 2, 6, 11):
        with pytest.raises(E, match=rf"integrate: n_q = {n_q} refused"):
            op.integrate(b, values, None, n_q)
        with pytest.raises(E, match=rf"evaluate: n_q = {n_q} refused"):
            op.evaluate(u, n_q)
    with pytest.raises(E, match=r"quadrature_points: n_q = 6 refused"):
        op.integrate(b, sine, None, 6)  # (a callable is tabulated first)
    # evaluate
    with pytest.raises(E, match="evaluate: vector size mismatch"):
        op.evaluate(mgamd.Vector(ctx, d.n_dofs + 1))
    with pytest.raises(E, match="number type"):
        op.evaluate(mgamd.Vector(ctx, d.n_dofs, mgamd.F32))
    with pytest.raises(E, match="evaluate: neither values nor gradients"):
        op.evaluate(u, 0, False, False)
    with pytest.raises(E, match="evaluate: u is null"):
        op.evaluate(None)
    assert refused(lib.mgamd_level_op_evaluate(op._h, u._h, 0, gradients._h, None), b"evaluate: values size mismatch")
    assert refused(lib.mgamd_level_op_evaluate(op._h, u._h, 0, None, values._h), b"evaluate: gradients size mismatch")
    assert refused(lib.mgamd_level_op_evaluate(op._h, u._h, 0, mgamd.Vector(ctx, n_points, mgamd.F32)._h, None), b"number type")
    assert op._cell_values_info() == (0, 0.0, 0.0) and op._estimator_info()[0] == 0  # a refused call builds nothing
    # the operator of a local-smoothing level is refused; the active-mesh operator of such a hierarchy works
    ls = mgamd.Operator(ctx, mgamd.DoFs(plain.level_mesh(2), 2, local_smoothing_level=True))
    with pytest.raises(E, match="evaluate: refused on the level of a local-smoothing hierarchy"):
        ls.evaluate(ls.initialize_dof_vector())
    with pytest.raises(E, match="integrate: refused on the level of a local-smoothing hierarchy"):
        ls.integrate(ls.initialize_dof_vector(), mgamd.Vector(ctx, 64 * 4 ** 3))
    h = mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-local")
    active = h.fine_operator
    load = active.initialize_dof_vector()
    active.integrate(load, active.evaluate(active.initialize_dof_vector()))
    assert (load.to_host() == 0.0).all()

    # a distributed operator, two simulated ranks
    trias = mgamd.create_geometric_coarsening_sequence(plain)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    group = mgamd.SimGroup(2)

    def rank(r):
        sharded = mgamd.DoFs(trias[-1], 2, 0, partition=part, level=len(trias) - 1, rank=r)
        dist = mgamd.Operator(ctx, sharded, mgamd.F64, comm=group.comm(r))
        with pytest.raises(E, match="evaluate: not implemented: sharded"):
            dist.evaluate(dist.initialize_dof_vector())
        with pytest.raises(E, match="integrate: not implemented: sharded"):
            dist.integrate(dist.initialize_dof_vector(), mgamd.Vector(ctx, 8))
        return dist._cell_values_info()

    assert run_ranks(2, rank) == [(0, 0.0, 0.0)] * 2


def manufactured_loop(mgamd, ctx, degree, refinements):
    """the Python restatement of examples/manufactured_solution.cpp: per mesh (cells, DoFs, L2 error, H1 error, tables, solution)"""
    sigma, n_q, out = 1.0, degree + 2, []
    for r in range(refinements):
        t = mgamd.Triangulation("hypercube", 2 + r)
        t.set_coefficient(layers(t.cell_centres()[:, 0], (-0.5, 0.0), (1.0, 5.0, 0.2)))
        h = mgamd.Hierarchy(ctx, t, None, degree, "HMG-global", coarse_solver="amg", mass_coefficient=sigma)
        op, d = h.fine_operator, h.dofs[-1]
        a = t.coefficient()[:, None, None, None]
        g = vec(op, sine(*d.node_positions().T))
        b, lift, x = op.initialize_dof_vector(), op.initialize_dof_vector(), op.initialize_dof_vector()
        op.integrate(b, lambda *X: sigma * sine(*X), lambda *X: tuple(a * c for c in sine_gradient(*X)), n_q)
        op.rhs_dirichlet(lift, g)
        b.from_host(b.to_host() + lift.to_host())
        it, _ = mgamd.solve_cg(op, h.mg, x, b, 1e-12)
        op.distribute_values(x, g)
        l2 = mgamd.compute_global_error(op.integrate_difference(x, sine, mgamd.NORM_L2, n_q), mgamd.NORM_L2)
        h1 = mgamd.compute_global_error(op.integrate_difference(x, (None, sine_gradient), mgamd.NORM_H1_SEMINORM, n_q), mgamd.NORM_H1_SEMINORM)
        out.append(dict(cells=t.n_cells, dofs=d.n_dofs, iterations=it, l2=l2, h1=h1, tria=t, keys=d.keys()))
    return out


def test_example(mgamd, ctx):
    """case 9: bin/manufactured_solution 2 3 against the Python loop to the printed digits, and on the two smallest meshes against the
    oracle's errors of the oracle's own solve (its load, its lifting, a sparse LU).  A record: no convergence rate is asserted."""
    r = subprocess.run([os.path.join(ROOT, "bin", "manufactured_solution"), "2", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    lines = [l.split() for l in r.stdout.strip().split("\n")]
    assert len(lines) == 3
    loop = manufactured_loop(mgamd, ctx, 2, 3)
    for l, dev in zip(lines, loop):
        assert l[0:12:2] == ["refinement", "cells", "dofs", "cg_iterations", "l2_error", "h1_error"]
        rec = dict(zip(l[0::2], l[1::2]))
        assert int(rec["cells"]) == dev["cells"] and int(rec["dofs"]) == dev["dofs"]
        assert abs(float(rec["l2_error"]) / dev["l2"] - 1.0) <= 1e-5 and abs(float(rec["h1_error"]) / dev["h1"] - 1.0) <= 1e-5  # (six printed digits)
    for dev in loop[:2]:
        cells = po.product_cells(dev["tria"])
        problem = Problem(sigma=1.0, coefficient=dict(zip(cells, dev["tria"].coefficient())))
        s = lv = po.Level(space(set(cells), 2), problem)  # (the oracle's own numbering)
        assert [tuple(c) for c in s.cells] == cells
        a = dev["tria"].coefficient()[:, None, None, None, None]
        values, gradients = co.tabulate(s.cells, 4, sine, sine_gradient)
        g = sine(*lv.node_positions().T)
        b = co.integrate(s, values, a * gradients, 4) + po.lift(lv, g)
        x = po.distribute_values(lv, spla.spsolve(lv.A.tocsc(), b), g)
        ref = no.norms(s, x, 4, sine, sine_gradient)
        for norm, key in ((no.L2, "l2"), (no.H1, "h1")):
            err = abs(dev[key] / no.global_error(ref[norm], norm) - 1.0)
            print(f"{dev['cells']} cells: {key} error {dev[key]:.6e}, relative to the oracle's own solve {err:.2e}")
            assert err <= 1e-9
