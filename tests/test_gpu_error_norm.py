"""The error norms on the device (Operator.integrate_difference: difference_norm_kernel) against closed forms and against
tests/error_norm_oracle.py, the built-in Gaussian, the numbers of the adaptive loop, the lazily built shared gather table and the
refusals.

Meshes, the smallest that reach each way the kernel can go wrong: hypercube 0 (one leaf: a partial group at every degree), hypercube 1
(8 leaves: less than one group at p = 1 and 2), quadrant 3 (120 leaves, hanging faces and edges, several groups) and the random octree S
(50 leaves, levels 1-3).  The kernel packs 32, 9, 4, 2, 1, 1, 1 leaves per workgroup pass at p = 1 ... 7 and gives two groups to a
workgroup (test_partial_groups).

Tolerances (from the arithmetic, not from what the kernel gives):
  * FP64 against a closed form or the oracle: |norm_K - ref_K| <= 1e-12 (|u_h|_K + |w|_K) in the respective norm: up to 1000 FP64
    additions per leaf plus the sweeps; a norm is Lipschitz in the point values, so the bound is on the inputs' sizes, not on a
    difference that may cancel;
  * Linfty: 1e-13 of the oracle's maximum on the leaf;
  * w = v in Q_p: every leaf <= 1e-13 |v|_K;
  * FP32: the kernel converts at the load and computes in double, so its result is BIT-identical to the FP64 operator's on the double
    vector (and data) that hold the same float values.
The largest measured ratios are printed by every test (DESIGN.md records them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import error_estimator_oracle as eo
import error_norm_oracle as no
import mgoracle
import physics_oracle as po
import random_mesh_physics as rm
from conftest import ROOT
from physics_oracle import Problem
from support import mesh, run_ranks, tria_of

pytestmark = pytest.mark.gpu

TOL, TOL_LINF, TOL_ZERO = 1e-12, 1e-13, 1e-13
DEGREES = (1, 2, 3, 4, 5, 6, 7)
MESHES = ("hypercube0", "hypercube1", "quadrant3", "S")
GRADIENT_NORMS = (no.H1, no.ENERGY)
SIGMA = 3.0
PHYSICS = Problem(coefficient="per_family", sigma=SIGMA)


def leaves_of(oracle, name):
    named = dict(hypercube0=("hypercube", 0), hypercube1=("hypercube", 1), hypercube2=("hypercube", 2), quadrant3=("quadrant", 3))
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
        a = None if problem.coefficient is None else po.product_values(t, eo.on(problem, s.cells).coefficient)
        perm = eo.to_oracle(s, d.keys(), np.arange(d.n_dofs)).astype(np.int64)
        _built[tag] = (t, d, op, s, a, perm)
    return _built[tag]


def vec(op, x):
    return op.initialize_dof_vector().from_host(x)


def rounded(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def tabulated(d, n_q, w, grad_w):
    """(values, gradients) of the functions at the product's own points, in the layouts of mgamd.h"""
    X = np.moveaxis(d.quadrature_points(n_q), -1, 0)
    return np.ascontiguousarray(w(*X)), np.ascontiguousarray(np.stack([np.broadcast_to(c, X[0].shape) for c in grad_w(*X)], axis=1))


def all_norms(op, u, exact, n_q=0):
    return {norm: op.integrate_difference(u, exact, norm, n_q) for norm in (no.L2, no.H1, no.ENERGY, no.LINFTY)}


def test_partial_groups(oracle):
    """for every degree at least one mesh leaves the last group of leaves partial; where a group is one leaf (p >= 5) at least one mesh
    has an odd number of groups, so that the last workgroup (two groups each) runs a partial trip of the grid stride"""
    counts = [len(leaves_of(oracle, name)) for name in MESHES]
    assert counts == [1, 8, 120, 50]
    for p in DEGREES:
        per_group = max(1, 256 // (p + 1) ** 3)
        assert any(n % per_group for n in counts) if per_group > 1 else any(n % 2 for n in counts)
    assert 8 < 32 and 8 < 9  # hypercube 1: less than one group at p = 1 and 2


def sine(x, y, z):
    return np.sin(2.0 * x + 0.5) * np.cos(1.5 * y) + 0.3 * z * z * x


def sine_gradient(x, y, z):
    return (2.0 * np.cos(2.0 * x + 0.5) * np.cos(1.5 * y) + 0.3 * z * z, -1.5 * np.sin(2.0 * x + 0.5) * np.sin(1.5 * y), 0.6 * z * x)


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("p", DEGREES)
def test_polynomial_closed_form(mgamd, ctx, oracle, name, p):
    """case 1: u_h the nodal interpolant of v in Q_p, w of degree p + 1 per variable tabulated at the points with its gradient, per_family
    coefficient and sigma = 3: L2, H1 and energy per leaf against the closed forms (the squared integrands have degree 2p + 2 <= 2 n_q - 1
    at n_q = p + 2; at n_q = p + 1 the rule is exact for w = 0, degree 2p).  FP32: bit-identical to FP64 on the rounded inputs."""
    t, d, op, s, a, perm = build(mgamd, ctx, oracle, name, p)
    v, w = no.polynomial(p, 10 + p), no.polynomial(p + 1, 20 + p)
    x = v(*d.node_positions().T)
    forms = no.ClosedForms(p + 1)
    size_v, size_w = forms.norms(s.cells, v, a, SIGMA), forms.norms(s.cells, w, a, SIGMA)
    worst = 0.0
    for n_q in ((p + 2, p + 1, p + 3) if p in (1, 4, 7) else (p + 2,)):
        exact_rule = n_q >= p + 2
        ref = forms.norms(s.cells, no.difference(v, w) if exact_rule else v, a, SIGMA)
        data = tabulated(d, n_q, w, no.gradient_of(w)) if exact_rule else 0
        for norm in (no.L2, no.H1, no.ENERGY):
            got = op.integrate_difference(vec(op, x), data, norm, n_q)
            assert got.shape == (len(s.cells),) and np.isfinite(got).all()
            worst = max(worst, (np.abs(got - ref[norm]) / (size_v[norm] + (size_w[norm] if exact_rule else 0.0))).max())
    print(f"{name} p={p}: {len(s.cells)} leaves, max |norm - closed form| / (|v|_K + |w|_K) = {worst:.2e}")
    assert worst <= TOL
    op32 = build(mgamd, ctx, oracle, name, p, mgamd.F32)[2]
    data = tuple(rounded(c) for c in tabulated(d, p + 2, w, no.gradient_of(w)))
    for norm in (no.L2, no.H1, no.ENERGY, no.LINFTY):
        assert np.array_equal(op32.integrate_difference(vec(op32, x), data, norm), op.integrate_difference(vec(op, rounded(x)), data, norm))


@pytest.mark.parametrize("name", ["quadrant3", "S"])
@pytest.mark.parametrize("p", DEGREES)
def test_against_oracle(mgamd, ctx, oracle, name, p):
    """case 2: a seeded vector (free and Dirichlet entries arbitrary, NaN in the hanging ones), all four norms, the built-in Gaussian and
    caller data from a function that is no polynomial"""
    t, d, op, s, a, perm = build(mgamd, ctx, oracle, name, p)
    x = np.random.default_rng(30 + p).standard_normal(d.n_dofs)
    x[d.n_dofs - d.info.n_hanging:] = np.nan
    assert d.info.n_hanging > 0
    n_q, u, xo = p + 2, vec(op, x), np.nan_to_num(x)[perm]
    own = no.norms(s, xo, n_q, None, None, a, SIGMA)
    X = np.moveaxis(no.quadrature_points(s.cells, n_q), -1, 0)
    worst, worst_linf = 0.0, 0.0
    for tag, exact, w, gw in (("Gaussian", 1, mgoracle.gaussian_solution, no.gaussian_gradient), ("sine", (sine, sine_gradient), sine, sine_gradient)):
        ref = no.norms(s, xo, n_q, w, gw, a, SIGMA)
        size_w = no.norms_of(s.cells, n_q, w(*X), np.stack(gw(*X), axis=1), a, SIGMA)
        got = all_norms(op, u, exact, n_q)
        for norm in (no.L2, no.H1, no.ENERGY):
            worst = max(worst, (np.abs(got[norm] - ref[norm]) / (own[norm] + size_w[norm])).max())
        worst_linf = max(worst_linf, (np.abs(got[no.LINFTY] - ref[no.LINFTY]) / ref[no.LINFTY]).max())
    print(f"{name} p={p}: max |norm - oracle| / (|u_h|_K + |w|_K) = {worst:.2e}, Linfty relative {worst_linf:.2e}")
    assert worst <= TOL and worst_linf <= TOL_LINF


@pytest.mark.parametrize("p", DEGREES)
def test_zero_and_negative_control(mgamd, ctx, oracle, p):
    """case 3: w = v in Q_p leaves nothing; one free DoF moved by delta changes exactly the leaves that gather it (directly or through a
    hanging node), by the oracle's value, and leaves all others bit-identical"""
    t, d, op, s, a, perm = build(mgamd, ctx, oracle, "quadrant3", p)
    v = no.polynomial(p, 40 + p)
    x = v(*d.node_positions().T)
    n_q = p + 2
    data = tabulated(d, n_q, v, no.gradient_of(v))
    size_v = no.ClosedForms(p).norms(s.cells, v, a, SIGMA)
    before = all_norms(op, vec(op, x), data, n_q)
    for norm in (no.L2, no.H1, no.ENERGY):
        assert (before[norm] <= TOL_ZERO * size_v[norm]).all(), (norm, (before[norm] / size_v[norm]).max())
    # a free DoF that hanging nodes depend on (a column of Ch with entries in hanging rows), so that some leaves gather it through
    # the constraints only: of the first 32 such DoFs the one with the most leaves of that kind
    Ch = s.Ch.tocsc()
    free = ~(s.hanging | s.dirichlet)
    parents = [j for j in np.flatnonzero(free) if s.hanging[Ch.indices[Ch.indptr[j]:Ch.indptr[j + 1]]].any()][:32]

    def leaves(j):
        e = np.zeros(s.n)
        e[j] = 1.0
        return np.abs((s.Ch @ e)[s.cell_dofs]).max(axis=1) > 0, (s.cell_dofs == j).any(axis=1)

    j = max(parents, key=lambda c: int(leaves(c)[0].sum() - leaves(c)[1].sum()))
    gathers, direct = leaves(j)
    assert 0 < direct.sum() < gathers.sum() < len(s.cells)
    delta = 0.125
    moved = x.copy()
    moved[perm[j]] += delta  # (x_oracle = x_product[perm])
    after = all_norms(op, vec(op, moved), data, n_q)
    ref = no.norms(s, moved[perm], n_q, v, no.gradient_of(v), a, SIGMA)
    own = no.norms(s, moved[perm], n_q, None, None, a, SIGMA)
    pts = np.moveaxis(no.quadrature_points(s.cells, n_q), -1, 0)
    size_v[no.LINFTY] = np.abs(v(*pts)).reshape(len(s.cells), -1).max(axis=1)
    worst = 0.0
    for norm in (no.L2, no.H1, no.ENERGY, no.LINFTY):
        assert np.array_equal(after[norm][~gathers], before[norm][~gathers])
        assert (after[norm][gathers] != before[norm][gathers]).all()
        tol = TOL_LINF if norm == no.LINFTY else TOL
        worst = max(worst, (np.abs(after[norm] - ref[norm]) / (tol * (own[norm] + size_v[norm])))[gathers].max())
    print(f"p={p}: {gathers.sum()} leaves gather the moved DoF ({direct.sum()} directly); max |norm - oracle| / bound = {worst:.2e}")
    assert worst <= 1.0


@pytest.mark.parametrize("p", [1, 3, 4, 7])
def test_hanging_entries_unread_and_bit_identity(mgamd, ctx, oracle, p):
    """case 4"""
    t, d, op, s, a, perm = build(mgamd, ctx, oracle, "quadrant3", p)
    x = np.random.default_rng(50 + p).standard_normal(d.n_dofs)
    nan = x.copy()
    nan[d.n_dofs - d.info.n_hanging:] = np.nan
    assert d.info.n_hanging > 0
    for exact in (1, (sine, sine_gradient)):
        first, second, unread = all_norms(op, vec(op, x), exact), all_norms(op, vec(op, x), exact), all_norms(op, vec(op, nan), exact)
        for norm in first:
            assert np.isfinite(first[norm]).all() and np.array_equal(first[norm], second[norm]) and np.array_equal(first[norm], unread[norm])


@pytest.mark.parametrize("p", DEGREES)
def test_fp32_bit_identical_to_fp64_on_the_same_values(mgamd, ctx, oracle, p):
    """case 5: conversion at the load, FP64 after"""
    t, d, op, s, a, perm = build(mgamd, ctx, oracle, "quadrant3", p)
    op32 = build(mgamd, ctx, oracle, "quadrant3", p, mgamd.F32)[2]
    x = rounded(np.random.default_rng(60 + p).standard_normal(d.n_dofs))
    for n_q in (p + 1, p + 2, p + 3):
        data = tuple(rounded(c) for c in tabulated(d, n_q, sine, sine_gradient))
        for exact in (0, 1, data):
            a32, a64 = all_norms(op32, vec(op32, x), exact, n_q), all_norms(op, vec(op, x), exact, n_q)
            assert all(np.array_equal(a32[norm], a64[norm]) and a64[norm].max() > 0 for norm in a64)


@pytest.mark.parametrize("p", [2, 5])
def test_builtin_gaussian(mgamd, ctx, oracle, p):
    """case 6: kind 1 against caller data tabulated from mgoracle.gaussian_solution and its analytic gradient; kind 0 against zeros"""
    t, d, op, s, a, perm = build(mgamd, ctx, oracle, "quadrant3", p)
    x = np.random.default_rng(70 + p).standard_normal(d.n_dofs)
    u = vec(op, x)
    worst = 0.0
    for n_q in (p + 1, p + 2, p + 3):
        data = tabulated(d, n_q, mgoracle.gaussian_solution, no.gaussian_gradient)
        for norm in (no.L2, no.H1):
            built_in, ref = op.integrate_difference(u, 1, norm, n_q), op.integrate_difference(u, data, norm, n_q)
            worst = max(worst, (np.abs(built_in - ref) / ref).max())
        zeros = (np.zeros_like(data[0]), np.zeros_like(data[1]))
        for norm in (no.L2, no.H1, no.ENERGY, no.LINFTY):
            assert np.array_equal(op.integrate_difference(u, 0, norm, n_q), op.integrate_difference(u, zeros, norm, n_q))
    print(f"p={p}: built-in Gaussian against tabulated data, max relative difference per leaf {worst:.2e}")
    assert worst <= TOL


@pytest.fixture(scope="module")
def loop(mgamd, ctx):
    """the adaptive loop of test_gpu_error_estimator.py on the device: p = 2 from hypercube 2, theta = 0.5, CG to 1e-10, four solves,
    with the error norms of every cycle (kind 1, n_q = p + 2)"""
    t, out = mgamd.Triangulation("hypercube", 2), []
    for cycle in range(4):
        h = mgamd.Hierarchy(ctx, t, degree=2, mg_type="HMG-global")
        op, d = h.fine_operator, h.dofs[-1]
        b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
        op.rhs(b, 1)
        mgamd.solve_cg(op, h.mg, x, b, 1e-10)
        op.distribute(x, 1)
        eta = op.estimate_error(x)
        norms = {norm: mgamd.compute_global_error(op.integrate_difference(x, 1, norm, 4), norm) for norm in (no.L2, no.H1, no.ENERGY, no.LINFTY)}
        out.append(dict(cells=po.product_cells(t), keys=d.keys(), x=x.to_host(), eta=eta, norms=norms))
        t = t.refine(mgamd.mark_maximum(eta, 0.5))
    return out


def test_solve(mgamd, loop):
    """case 7: the global L2 and H1 errors of the first two cycles against the oracle on the same device solution"""
    for cycle, dev in enumerate(loop[:2]):
        s = eo.nodal_space(set(dev["cells"]), 2)
        assert [tuple(c) for c in s.cells] == dev["cells"]
        ref = no.norms(s, eo.to_oracle(s, dev["keys"], dev["x"]), 4, mgoracle.gaussian_solution, no.gaussian_gradient)
        for norm in (no.L2, no.H1):
            err = abs(dev["norms"][norm] / no.global_error(ref[norm], norm) - 1.0)
            print(f"cycle {cycle}: {len(s.cells)} cells, norm {norm}: device {dev['norms'][norm]:.6e}, relative to the oracle {err:.2e}")
            assert err <= 1e-10
    # a = 1 and sigma = 0: the energy norm is the H1 seminorm
    assert all(abs(dev["norms"][no.ENERGY] / dev["norms"][no.H1] - 1.0) <= 1e-14 for dev in loop)
    for cycle, dev in enumerate(loop):
        n = dev["norms"]
        print(f"cycle {cycle}: {len(dev['cells'])} cells, L2 {n[no.L2]:.6e} H1 {n[no.H1]:.6e} Linfty {n[no.LINFTY]:.6e} "
              f"effectivity {np.sqrt(np.sum(dev['eta'] ** 2)) / n[no.ENERGY]:.6e}")


def test_example_prints_the_error_norms(loop):
    """the new keys of bin/adaptive_gaussian 2 4 against the Python values, to the printed digits (a record, no rate is asserted)"""
    r = subprocess.run([os.path.join(ROOT, "bin", "adaptive_gaussian"), "2", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l.split() for l in r.stdout.strip().split("\n")]
    assert len(lines) == 4
    for l, dev in zip(lines, loop):
        assert l[0::2] == ["cycle", "cells", "dofs", "cg_iterations", "sum_eta2", "max_nodal_error", "l2_error", "h1_error", "effectivity"]
        rec = dict(zip(l[0::2], l[1::2]))
        assert int(rec["cells"]) == len(dev["cells"])
        effectivity = np.sqrt(np.sum(dev["eta"] ** 2)) / dev["norms"][no.ENERGY]
        assert abs(float(rec["l2_error"]) / dev["norms"][no.L2] - 1.0) <= 1e-5  # (six printed digits)
        assert abs(float(rec["h1_error"]) / dev["norms"][no.H1] - 1.0) <= 1e-5
        assert abs(float(rec["effectivity"]) / effectivity - 1.0) <= 1e-5


def test_lazy_allocation_and_the_shared_table(mgamd, ctx):
    """case 8: nothing before the first call; a norm-only operator never builds the neighbour table; the indicator afterwards equals the
    indicator of a fresh operator bit for bit, and the other way round"""
    t = mgamd.Triangulation("quadrant", 3)
    t.set_dirichlet_faces(0b011110)
    d = mgamd.DoFs(t, 3)
    first, fresh = mgamd.Operator(ctx, d), mgamd.Operator(ctx, d)
    assert first._error_norm_info() == (0, 0.0, False) and first._estimator_info() == (0, 0.0, 0.0)
    x = np.random.default_rng(80).standard_normal(d.n_dofs)
    q = np.array([0.6, 0.0, 0.0, 0.0, 0.0, -1.25])
    norm_first = first.integrate_difference(vec(first, x), 1, no.ENERGY)
    nbytes, kernel_ms, neighbours = first._error_norm_info()
    n = 4
    assert nbytes == 120 * (4 * n ** 3 + 18 + 32) and kernel_ms > 0 and not neighbours
    assert first._estimator_info()[0] == 0  # the indicator's tables and scratch are not there
    eta_fresh = fresh.estimate_error(vec(fresh, x), q)
    assert fresh._error_norm_info() == (0, 0.0, True)
    eta_after = first.estimate_error(vec(first, x), q)
    assert np.array_equal(eta_after, eta_fresh) and eta_fresh.max() > 0
    assert first._estimator_info()[0] == fresh._estimator_info()[0] == 120 * (4 * n ** 3 + 48 * n ** 2 + 128)  # ONE copy of idx
    assert first._error_norm_info()[2]
    assert np.array_equal(fresh.integrate_difference(vec(fresh, x), 1, no.ENERGY), norm_first)
    assert np.array_equal(first.integrate_difference(vec(first, x), 1, no.ENERGY), norm_first)
    assert fresh._error_norm_info()[0] == nbytes


def test_sigma_is_the_operators_own(mgamd, ctx, oracle):
    """the energy norm takes the mass coefficient the operator was BUILT with, whatever the tables are given later"""
    t, d, op, s, a, perm = build(mgamd, ctx, oracle, "hypercube1", 2)
    u = vec(op, np.random.default_rng(81).standard_normal(d.n_dofs))
    before = op.integrate_difference(u, 0, no.ENERGY)
    d.set_mass_coefficient(5.0)
    try:
        assert op.mass_coefficient() == SIGMA and np.array_equal(op.integrate_difference(u, 0, no.ENERGY), before)
        l2, h1 = op.integrate_difference(u, 0, no.L2), op.integrate_difference(u, 0, no.H1)
        assert (np.abs(before - np.sqrt(a * h1 ** 2 + SIGMA * l2 ** 2)) <= TOL * before).all()
    finally:
        d.set_mass_coefficient(SIGMA)


def test_refusals(mgamd, ctx):
    """case 9: every device-side refusal, by name; a refused call builds nothing"""
    plain = mgamd.Triangulation("quadrant", 3)
    d = mgamd.DoFs(plain, 2)
    op = mgamd.Operator(ctx, d)
    u, n_points = op.initialize_dof_vector(), 120 * 4 ** 3
    values, gradients = mgamd.Vector(ctx, n_points), mgamd.Vector(ctx, 3 * n_points)
    E = mgamd.MgamdError
    with pytest.raises(E, match="integrate_difference: vector size mismatch"):
        op.integrate_difference(mgamd.Vector(ctx, d.n_dofs + 1), 0, no.L2)
    with pytest.raises(E, match="number type"):
        op.integrate_difference(mgamd.Vector(ctx, d.n_dofs, mgamd.F32), 0, no.L2)
    with pytest.raises(E, match="integrate_difference: values size mismatch"):
        op.integrate_difference(u, mgamd.Vector(ctx, n_points + 1), no.L2)
    with pytest.raises(E, match="integrate_difference: values size mismatch"):
        op.integrate_difference(u, values, no.L2, 5)  # (the data of n_q = 4 at n_q = 5)
    with pytest.raises(E, match="number type"):
        op.integrate_difference(u, mgamd.Vector(ctx, n_points, mgamd.F32), no.L2)
    with pytest.raises(E, match="integrate_difference: gradients size mismatch"):
        op.integrate_difference(u, (values, mgamd.Vector(ctx, n_points)), no.H1)
    with pytest.raises(E, match="number type"):
        op.integrate_difference(u, (values, mgamd.Vector(ctx, 3 * n_points, mgamd.F32)), no.ENERGY)
    for norm in GRADIENT_NORMS:
        with pytest.raises(E, match="integrate_difference: a gradient norm without gradients"):
            op.integrate_difference(u, values, norm)
        with pytest.raises(E, match="integrate_difference: a gradient norm without gradients"):
            op.integrate_difference(u, sine, norm)
    with pytest.raises(E, match="integrate_difference: values is null"):
        op.integrate_difference(u, (None, gradients), no.ENERGY)
    for n_q in (-1, 1, 2, 6, 11):
        with pytest.raises(E, match=rf"integrate_difference: n_q = {n_q} refused"):
            op.integrate_difference(u, 0, no.L2, n_q)
    with pytest.raises(E, match=r"quadrature_points: n_q = 6 refused"):
        op.integrate_difference(u, sine, no.L2, 6)  # (a callable is tabulated first)
    for norm in (-1, 4):
        with pytest.raises(E, match=f"integrate_difference: unknown norm {norm}"):
            op.integrate_difference(u, 0, norm)
    for kind in (-1, 2):
        with pytest.raises(E, match=f"integrate_difference: unknown kind {kind}"):
            op.integrate_difference(u, kind, no.L2)
    lib = C.CDLL(mgamd._LIB_PATH)
    lib.mgamd_last_error.restype = C.c_char_p
    assert lib.mgamd_level_op_integrate_difference(op._h, u._h, 0, 0, 0, None) == 3 and b"out is null" in lib.mgamd_last_error()
    assert lib.mgamd_level_op_integrate_difference_values(op._h, u._h, values._h, None, 0, 0, None) == 3 and b"out is null" in lib.mgamd_last_error()
    assert op._error_norm_info() == (0, 0.0, False) and op._estimator_info()[0] == 0  # a refused call builds nothing
    assert np.isfinite(op.integrate_difference(u, (None, gradients), no.H1)).all()  # the H1 seminorm reads no values
    # the operator of a local-smoothing level is refused; the active-mesh operator of such a hierarchy works
    ls = mgamd.Operator(ctx, mgamd.DoFs(plain.level_mesh(2), 2, local_smoothing_level=True))
    with pytest.raises(E, match="integrate_difference: refused on the level of a local-smoothing hierarchy"):
        ls.integrate_difference(ls.initialize_dof_vector(), 0, no.L2)
    h = mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-local")
    active = h.fine_operator
    assert np.isfinite(active.integrate_difference(active.initialize_dof_vector(), 1, no.L2)).all()

    # a distributed operator, two simulated ranks
    trias = mgamd.create_geometric_coarsening_sequence(plain)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    group = mgamd.SimGroup(2)

    def rank(r):
        sharded = mgamd.DoFs(trias[-1], 2, 0, partition=part, level=len(trias) - 1, rank=r)
        dist = mgamd.Operator(ctx, sharded, mgamd.F64, comm=group.comm(r))
        with pytest.raises(E, match="integrate_difference: not implemented: sharded"):
            dist.integrate_difference(dist.initialize_dof_vector(), 0, no.L2)
        return dist._error_norm_info()

    assert run_ranks(2, rank) == [(0, 0.0, False)] * 2
