"""Point evaluation and point sources on the device (Operator.point_set: point_locate_kernel; PointSet.evaluate: point_evaluate_kernel;
PointSet.integrate: point_integrate_kernel) against tests/point_values_oracle.py, against closed forms, in the identities that tie the
two kernels together, and in the example; the lazily built tables, two sets on one operator and the refusals.  Every test goes through
entry points that exist only with the feature.

Meshes: hypercube 0 (one leaf: a partial group at every degree), hypercube 1 (8 leaves: less than one group at p = 1 and 2), quadrant 3
(120 leaves, hanging faces and edges, several groups) and the random octree S (50 leaves, levels 1-3).  Both kernels pack 32, 9, 4, 2, 1,
1, 1 OCCUPIED leaves per workgroup pass at p = 1 ... 7.

Point sets (point_values_oracle.py): 1000 seeded uniform points; 700 points inside one leaf (three strides of 256 threads in the evaluate
kernel, eleven batches of 64 points in the integrate kernel); the centre and all corners of every leaf (ties on faces, edges and
vertices, and the +1 faces); sets of 1, 0 and 257 points; duplicates; five points outside the cube and one NaN.  They are located as
ONE set per mesh (`everything`), so that leaves hold many and few points in the same launch, and the small ones separately
(test_point_values_host.py holds the sets against the kernels' constants).  Every
in-domain point must come back found: asserted, so that no test passes by dropping points.

Tolerances (from the arithmetic, not from what the kernels give):
  * location: cell and reference coordinate bit-equal to the oracle (one addition in double, then exact operations on both sides);
  * evaluate, FP64: per point 1e-12 sum_i |phi_i| |u_i| and 1e-12 sum_i |d_c phi_i| |u_i| (the oracle's absolute=True), the project's
    bound for cell_evaluate_kernel: (p+1)^3 products per point, each with a few roundings;
  * evaluate, FP32: the kernel converts at the load, computes in double (the reference coordinates are double for both number types) and
    converts at the store, so its result is BIT-identical to the FP64 operator's on the double vector that holds the same float values,
    rounded to float;
  * integrate: |b_i - oracle_i| <= tol B_i, B_i the oracle's load of |data| against |phi_i|, |grad phi_i| through |Ch|; tol = 1e-12 in
    FP64 and 2e-6 in FP32, the bounds of cell_integrate_kernel: the arithmetic is double up to the scatter and the float atomics add at
    most a few ulp (6e-8) per addend;
  * evaluate and the closed forms are held to these plain bounds.  integrate against the ORACLE is held to tol B_i plus the oracle's own
    error (point_values_oracle.py, absolute="reference": its nodes are off by up to 4 units in the last place, which rows with a small
    B_i see at full size); the RAW ratio over the rows above noise level (B_i > 1e-12 max_j B_j) is printed, with the number of rows that
    needed the allowance.  The FP64 device load is ALSO held to the host restatement DoFs.point_integrate (long double bases, the
    product's own nodes) under the plain 1e-12 B_i on every row above noise level; the noise rows, whose B_i is itself a residue of
    the oracle, get the allowance;
  * adjointness: both sides are sums of the same products, bound 1e-12 (sum_k |w_k| U_k + sum_ck |W_ck| G_ck + sum_i |u_i| B_i) with the
    per-point bounds U, G and the per-row bound B;
  * partition of unity: 1e-12 sum_i B_i;  a point at a node: 1e-13 |w|, the issue's figure (the node's position is rounded to double,
    so the other basis functions of the leaf are 1e-16-size, times their slopes).
The largest measured ratios are printed by every test (DESIGN.md records them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cell_values_oracle as co
import error_estimator_oracle as eo
import physics_oracle as po
import point_values_oracle as pv
import random_mesh_physics as rm
from conftest import ROOT
from physics_oracle import Problem
from support import mesh, run_ranks, tria_of

pytestmark = pytest.mark.gpu

TOL, TOL_F32 = 1e-12, 2e-6
DEGREES = (1, 2, 3, 4, 5, 6, 7)
MESHES = ("hypercube0", "hypercube1", "quadrant3", "S")
PLAIN = Problem()
NATURAL = Problem(dirichlet_faces=0)  # every row of a non-hanging node is a free row


def leaves_of(oracle, name):
    named = dict(hypercube0=("hypercube", 0), hypercube1=("hypercube", 1), quadrant3=("quadrant", 3))
    return mesh(*named[name]) if name in named else rm.leaves_of(oracle, name)


_built, _sets, _reference = {}, {}, {}


def build(mgamd, ctx, oracle, name, p, number_type=8, problem=PLAIN):
    """the product's mesh, tables and operator on the named leaves, the oracle's space and the permutation that brings a vector of
    the product's numbering to the space's"""
    tag = (name, p, number_type, id(problem))
    if tag not in _built:
        leaves = leaves_of(oracle, name)
        t = tria_of(mgamd, leaves, problem)
        d = mgamd.DoFs(t, p)
        op = mgamd.Operator(ctx, d, number_type)
        s = eo.nodal_space(leaves, p)
        assert po.product_cells(t) == [tuple(c) for c in s.cells]
        perm = eo.to_oracle(s, d.keys(), np.arange(d.n_dofs)).astype(np.int64)
        _built[tag] = (t, d, op, s, perm)
    return _built[tag]


points_of = pv.device_sets


def point_set(op, s, which="everything"):
    tag = (id(op), which)
    if tag not in _sets:
        _sets[tag] = op.point_set(points_of(s.cells)[which])
    return _sets[tag]


def reference(s, tag, fn):
    """an oracle result, computed once per (space, tag) and left unchanged"""
    key = (id(s), tag)
    if key not in _reference:
        _reference[key] = fn()
    return _reference[key]


def vec(op, x):
    return op.initialize_dof_vector().from_host(x)


def rounded(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def both(ps, u):
    v, g = ps.evaluate(u, True, True)
    return v.to_host(), g.to_host().reshape(3, ps.n)


def integrate(ps, op, d, values, gradients, prefill=np.nan):
    """PointSet.integrate into a vector pre-filled with NaN; nothing may be NaN afterwards and the constrained tail is exactly 0"""
    b = vec(op, np.full(d.n_dofs, prefill))
    ps.integrate(b, values, gradients)
    out = b.to_host()
    assert np.isfinite(out).all()
    assert (out[d.n_dofs - d.info.n_hanging - d.info.n_dirichlet:] == 0.0).all()
    return out


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("p", DEGREES)
def test_location_and_evaluate(mgamd, ctx, oracle, name, p):
    """location bit-equal to the oracle; a seeded vector with NaN in the hanging entries: FP64 against the oracle, two calls the same bits,
    values and gradients separately the same bits, exact zeros where a point is not found, FP32 bit-identical to FP64 on the rounded
    input, rounded; the sets of 1, 0 and 257 points"""
    t, d, op, s, perm = build(mgamd, ctx, oracle, name, p)
    op32 = build(mgamd, ctx, oracle, name, p, mgamd.F32)[2]
    sets = points_of(s.cells)
    x = np.random.default_rng(30 + p).standard_normal(d.n_dofs)
    nan = x.copy()
    nan[d.n_dofs - d.info.n_hanging:] = np.nan
    xo = np.where(s.hanging, 0.0, x[perm])
    worst = 0.0
    for which in ("everything", "one", "none", "wave_and_one"):
        pts, ps, ps32 = sets[which], point_set(op, s, which), point_set(op32, s, which)
        inside = sets["inside"] if which == "everything" else np.ones(len(pts), bool)
        ref_cell, ref_xi = reference(s, ("locate", which), lambda: pv.locate(s.cells, pts))
        for q in (ps, ps32):
            assert q.n == len(pts) and np.array_equal(q.found, inside) and q.all_points_found() == bool(inside.all())
            assert np.array_equal(q.cells, ref_cell) and np.array_equal(q.reference_points, ref_xi)
        u, g = both(ps, vec(op, nan))
        assert u.shape == (len(pts),) and g.shape == (3, len(pts))
        assert np.isfinite(u).all() and np.isfinite(g).all()
        assert (u[~inside] == 0.0).all() and (g[:, ~inside] == 0.0).all()
        # a second call, separately, the hanging entries readable: the same bits
        again = both(ps, vec(op, nan))
        assert np.array_equal(again[0], u) and np.array_equal(again[1], g)
        assert np.array_equal(ps.evaluate(vec(op, x)).to_host(), u)
        assert np.array_equal(ps.evaluate(vec(op, x), False, True).to_host().reshape(3, ps.n), g)
        ref_u, ref_g = reference(s, ("evaluate", which, p), lambda: pv.evaluate(s, xo, pts))
        bu, bg = reference(s, ("evaluate size", which, p), lambda: pv.evaluate(s, xo, pts, absolute=True))
        worst = max(worst, pv.ratio(np.abs(u - ref_u), bu), pv.ratio(np.abs(g - ref_g).ravel(), bg.ravel()))
        # FP32: conversion at the load and at the store, FP64 between
        u64, g64 = both(ps, vec(op, rounded(nan)))
        u32, g32 = both(ps32, vec(op32, nan))
        assert np.array_equal(u32, rounded(u64)) and np.array_equal(g32, rounded(g64))
    print(f"{name} p={p}: {len(s.cells)} leaves, evaluate max error / (1e-12 bound's size) = {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("p", DEGREES)
def test_closed_forms(mgamd, ctx, oracle, p):
    """u_h(x_k) = q(x_k) and grad u_h(x_k) = grad q(x_k) for q in Q_p on quadrant 3 (hanging faces and edges) at the uniform points and the
    points of one leaf, which are neither nodes nor Gauss points"""
    t, d, op, s, perm = build(mgamd, ctx, oracle, "quadrant3", p)
    sets = points_of(s.cells)
    ps = point_set(op, s)
    q = co.polynomial(p, 10 + p)
    x = q(*d.node_positions().T)
    x[d.n_dofs - d.info.n_hanging:] = np.nan
    u, g = both(ps, vec(op, x))
    pts, on = sets["everything"], np.arange(len(sets["everything"])) < 1703  # uniform, then the leaf's (three points outside among them)
    on &= sets["inside"]
    xo = np.where(s.hanging, 0.0, np.nan_to_num(x)[perm])
    bu, bg = reference(s, ("closed size", p), lambda: pv.evaluate(s, xo, pts, absolute=True))
    X = pts[on].T
    worst = max(pv.ratio(np.abs(u[on] - q(*X)), bu[on]), max(pv.ratio(np.abs(g[c, on] - q.deriv(c)(*X)), bg[c, on]) for c in range(3)))
    print(f"p={p}: max |u_h - q| and |grad u_h - grad q| / bound = {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("p", DEGREES)
def test_integrate_against_oracle(mgamd, ctx, oracle, name, p):
    """seeded weights (float-representable: the same numbers in both number types), values only, gradients only, both; b pre-filled
    with NaN; FP64 and FP32 against the oracle; points outside add nothing; on one leaf two FP64 calls give the same bits"""
    t, d, op, s, perm = build(mgamd, ctx, oracle, name, p)
    op32 = build(mgamd, ctx, oracle, name, p, mgamd.F32)[2]
    pts = points_of(s.cells)["everything"]
    ps, ps32 = point_set(op, s), point_set(op32, s)
    rng = np.random.default_rng(40 + p)
    w, W = rounded(rng.standard_normal(len(pts))), rounded(rng.standard_normal((3, len(pts))))
    worst = worst32 = worst_host = 0.0
    noise_rows = 0
    for k, (w_, W_) in enumerate(((w, None), (None, W), (w, W))):
        ref = reference(s, ("integrate", k, p), lambda: pv.integrate(s, pts, w_, W_))
        size = reference(s, ("integrate size", k, p), lambda: pv.integrate(s, pts, w_, W_, absolute=True))
        own = reference(s, ("integrate own", k, p), lambda: pv.integrate(s, pts, w_, W_, absolute="reference"))
        for o, q, tol in ((op, ps, TOL), (op32, ps32, TOL_F32)):
            b = integrate(q, o, d, w_, W_)
            r, n_noise = pv.row_ratio(np.abs(b[perm] - ref), size, own, tol)
            worst, worst32, noise_rows = (max(worst, r), worst32, noise_rows + n_noise) if o is op else (worst, max(worst32, r), noise_rows)
            if o is op:
                host = reference(s, ("integrate host", k, p), lambda: d.point_integrate(pts, w_, W_))
                worst_host = max(worst_host, pv.row_ratio(np.abs(b - host)[perm], size, own, TOL, against_oracle=False)[0])
        if name == "hypercube0":
            assert np.array_equal(integrate(ps, op, d, w_, W_), integrate(ps, op, d, w_, W_, prefill=0.0))
    empty = point_set(op, s, "none")
    assert (integrate(empty, op, d, np.zeros(0), None) == 0.0).all()
    print(f"{name} p={p}: integrate max |b_i - oracle| / B_i = {worst:.2e} (FP64), {worst32:.2e} (FP32) (raw, against the oracle; {noise_rows} FP64 rows above 1e-12 B_i), "
          f"{worst_host:.2e} against the host restatement")
    assert worst32 <= TOL_F32 and worst_host <= TOL  # (worst: the raw figure against the oracle, held in row_ratio with its own error)


@pytest.mark.parametrize("p", DEGREES)
def test_adjointness(mgamd, ctx, oracle, p):
    """sum_k w_k u_h(x_k) + W_k . grad u_h(x_k) = u^T b for u with zero Dirichlet and hanging entries, on quadrant 3"""
    t, d, op, s, perm = build(mgamd, ctx, oracle, "quadrant3", p)
    pts = points_of(s.cells)["everything"]
    ps = point_set(op, s)
    rng = np.random.default_rng(60 + p)
    x = rng.standard_normal(d.n_dofs)
    x[d.n_dofs - d.info.n_hanging - d.info.n_dirichlet:] = 0.0
    w, W = rng.standard_normal(len(pts)), rng.standard_normal((3, len(pts)))
    u, g = both(ps, vec(op, x))
    b = integrate(ps, op, d, w, W)
    bu, bg = pv.evaluate(s, x[perm], pts, absolute=True)
    size = np.abs(w) @ bu + (np.abs(W) * bg).sum() + np.abs(x[perm]) @ pv.integrate(s, pts, w, W, absolute=True)
    err = abs(w @ u + (W * g).sum() - x @ b) / size
    print(f"p={p}: |sum_k (w_k u_h + W_k . grad u_h) - u^T b| / size = {err:.2e}")
    assert err <= TOL


@pytest.mark.parametrize("p", DEGREES)
def test_partition_of_unity(mgamd, ctx, oracle, p):
    """without Dirichlet faces sum_i b_i = sum_k w_k over the found points (the rows of C sum to 1), on the octree S"""
    t, d, op, s, perm = build(mgamd, ctx, oracle, "S", p, problem=NATURAL)
    assert d.info.n_dirichlet == 0
    sets = points_of(s.cells)
    pts, ps = sets["everything"], point_set(op, s)
    w = np.random.default_rng(70 + p).standard_normal(len(pts))
    b = integrate(ps, op, d, w, None)
    size = pv.integrate(s, pts, w, None, absolute=True, keep_dirichlet=True).sum()
    err = abs(b.sum() - w[sets["inside"]].sum()) / size
    print(f"p={p}: |sum_i b_i - sum_k w_k| / sum_i B_i = {err:.2e}")
    assert err <= TOL


@pytest.mark.parametrize("p", DEGREES)
def test_point_at_a_node(mgamd, ctx, oracle, p):
    """one point at the position of a free (so non-hanging) node gives w e_i to 1e-13, on quadrant 3"""
    t, d, op, s, perm = build(mgamd, ctx, oracle, "quadrant3", p)
    n_free = d.n_dofs - d.info.n_hanging - d.info.n_dirichlet
    nodes = d.node_positions()
    worst = 0.0
    for i in (0, n_free // 3, n_free // 2, n_free - 1):
        ps = op.point_set(nodes[i])
        assert ps.all_points_found()
        b = integrate(ps, op, d, np.array([-2.5]), None)
        e = np.zeros(d.n_dofs)
        e[i] = -2.5
        worst = max(worst, np.abs(b - e).max() / 2.5)
    print(f"p={p}: a point at a node, max |b - w e_i| / |w| = {worst:.2e}")
    assert worst <= 1e-13


@pytest.mark.parametrize("p", DEGREES)
def test_negative_control(mgamd, ctx, oracle, p):
    """one point in one leaf of quadrant 3 that has hanging nodes touches only that leaf's rows, through its hanging nodes, and every
    other row keeps the bits the memset gave it"""
    t, d, op, s, perm = build(mgamd, ctx, oracle, "quadrant3", p)
    mask = t.cells()[4]
    ci = int(np.flatnonzero(mask >> 3)[len(np.flatnonzero(mask >> 3)) // 2])  # a leaf with a hanging face or edge
    ps = op.point_set(pv.inside_leaf(s.cells, ci, 1, 3))
    assert ps.cells[0] == ci
    rows = co.rows_of_leaf(s, ci)
    for w_, W_ in ((np.array([1.5]), None), (None, np.array([0.5, -1.0, 2.0])), (np.array([1.5]), np.array([0.5, -1.0, 2.0]))):
        b = integrate(ps, op, d, w_, W_)[perm]
        assert np.array_equal(b[~rows].view(np.uint64), np.zeros((~rows).sum(), np.uint64))  # +0.0, bit for bit
        free_of_leaf = np.unique(s.cell_dofs[ci])
        through_hanging = rows.copy()
        through_hanging[free_of_leaf] = False
        assert through_hanging.any() and (b[through_hanging] != 0.0).any()  # rows the leaf reaches only through its hanging nodes
        assert (b[rows] != 0.0).sum() >= rows.sum() // 2


def test_lazy_allocation_and_two_sets(mgamd, ctx, oracle):
    """a fresh operator holds nothing; the first point set uploads the keys and corners of the leaves (24 bytes per leaf) and nothing
    else; the first evaluate builds the shared gather table; the times read zero before the first use; two sets on one operator do
    not disturb each other, and one survives the other"""
    t = mgamd.Triangulation("quadrant", 3)
    d = mgamd.DoFs(t, 3)
    op, never = mgamd.Operator(ctx, d), mgamd.Operator(ctx, d)
    assert op._point_tables_bytes() == (0, 0) and op._cell_values_info() == (0, 0.0, 0.0)
    a, b_pts = pv.uniform(300, 5), pv.uniform(41, 6)
    first = op.point_set(a)
    assert op._point_tables_bytes() == (120 * 24, 0) and op._estimator_info()[0] == 0  # the keys and corners, not the gather table
    nbytes, build_ms, locate_ms, evaluate_ms, integrate_ms = first._info()
    occupied = len(np.unique(first.cells))
    assert nbytes == 300 * 28 + 300 * 8 + (2 * occupied + 1) * 4
    assert build_ms >= 0.0 and locate_ms > 0.0 and evaluate_ms == 0.0 and integrate_ms == 0.0
    x = vec(op, np.random.default_rng(80).standard_normal(d.n_dofs))
    ua = first.evaluate(x).to_host()
    assert op._point_tables_bytes() == (120 * 24, 120 * (4 * 4 ** 3 + 18))  # the shared gather table, built by the first evaluate
    assert op._estimator_info()[0] == 0 and op._error_norm_info() == (0, 0.0, False)  # neither the neighbour table nor the norms' arrays
    assert first._info()[3] > 0.0 and first._info()[4] == 0.0
    second = op.point_set(b_pts)
    assert op._point_tables_bytes()[0] == 120 * 24 and second._info()[3] == 0.0
    ub = second.evaluate(x).to_host()
    load = op.initialize_dof_vector()
    second.integrate(load, np.ones(41))
    assert second._info()[4] > 0.0 and first._info()[4] == 0.0
    assert np.array_equal(first.evaluate(x).to_host(), ua)
    del first
    assert np.array_equal(second.evaluate(x).to_host(), ub)
    fresh = mgamd.Operator(ctx, d).point_set(a)
    assert np.array_equal(fresh.evaluate(vec(fresh.op, x.to_host())).to_host(), ua)
    # an empty set builds and launches nothing on an operator that holds nothing else
    empty = never.point_set(np.zeros((0, 3)))
    assert empty.n == 0 and empty.all_points_found() and empty._info() == (0, 0.0, 0.0, 0.0, 0.0)
    assert empty.evaluate(never.initialize_dof_vector()).to_host().shape == (0,)
    assert never._point_tables_bytes() == (0, 0) and never._estimator_info()[0] == 0
    other = mgamd.Operator(ctx, d)
    assert other._point_tables_bytes() == (0, 0) and other._cell_values_info() == (0, 0.0, 0.0)  # never asked: nothing


def test_refusals(mgamd, ctx):
    """every device-side refusal, by name; a refused call builds nothing"""
    plain = mgamd.Triangulation("quadrant", 3)
    d = mgamd.DoFs(plain, 2)
    op, op2, op32 = mgamd.Operator(ctx, d), mgamd.Operator(ctx, d), mgamd.Operator(ctx, d, mgamd.F32)
    pts = pv.uniform(10, 9)
    ps = op.point_set(pts)
    u, b = op.initialize_dof_vector(), op.initialize_dof_vector()
    values, gradients = mgamd.Vector(ctx, 10), mgamd.Vector(ctx, 30)
    E = mgamd.MgamdError
    lib = C.CDLL(mgamd._LIB_PATH)
    lib.mgamd_last_error.restype = C.c_char_p
    refused = lambda status, text: status == 3 and text in lib.mgamd_last_error()
    # the set
    with pytest.raises(ValueError, match="point_set: points of shape"):
        op.point_set(np.zeros((5, 2)))
    handle = C.c_void_p()
    assert refused(lib.mgamd_level_op_point_set_create(op._h, C.c_uint64(10), None, C.byref(handle)), b"point_set: xyz is null")
    assert refused(lib.mgamd_level_op_point_set_create(None, C.c_uint64(10), pts.ctypes.data_as(C.c_void_p), C.byref(handle)), b"point_set: a null pointer")
    assert refused(lib.mgamd_level_op_point_set_create(op._h, C.c_uint64(10), pts.ctypes.data_as(C.c_void_p), None), b"point_set: a null pointer")
    assert refused(lib.mgamd_point_set_get(None, None, None, None, None), b"point_set: a null pointer")
    # evaluate
    with pytest.raises(E, match="point_evaluate: vector size mismatch"):
        ps.evaluate(mgamd.Vector(ctx, d.n_dofs + 1))
    with pytest.raises(E, match="number type"):
        ps.evaluate(mgamd.Vector(ctx, d.n_dofs, mgamd.F32))
    with pytest.raises(E, match="point_evaluate: neither values nor gradients"):
        ps.evaluate(u, False, False)
    with pytest.raises(E, match="point_evaluate: u is null"):
        ps.evaluate(None)
    other = b"point_evaluate: the point set belongs to another operator"
    assert refused(lib.mgamd_point_set_evaluate(ps._h, op2._h, u._h, values._h, None), other)
    assert refused(lib.mgamd_point_set_evaluate(ps._h, op32._h, op32.initialize_dof_vector()._h, mgamd.Vector(ctx, 10, mgamd.F32)._h, None), other)
    assert refused(lib.mgamd_point_set_evaluate(ps._h, op._h, u._h, gradients._h, None), b"point_evaluate: values size mismatch")
    assert refused(lib.mgamd_point_set_evaluate(ps._h, op._h, u._h, None, values._h), b"point_evaluate: gradients size mismatch")
    assert refused(lib.mgamd_point_set_evaluate(ps._h, op._h, u._h, mgamd.Vector(ctx, 10, mgamd.F32)._h, None), b"number type")
    assert refused(lib.mgamd_point_set_evaluate(ps._h, op._h, u._h, values._h, values._h), b"point_evaluate: gradients size mismatch")
    assert refused(lib.mgamd_point_set_evaluate(None, op._h, u._h, values._h, None), b"point_evaluate: a null pointer")
    assert refused(lib.mgamd_point_set_evaluate(ps._h, None, u._h, values._h, None), b"point_evaluate: a null pointer")
    # an output that is u or the other output: sizes that allow it (n_dofs points; a third of them for the gradient)
    many = op.point_set(pv.uniform(d.n_dofs, 10))
    assert refused(lib.mgamd_point_set_evaluate(many._h, op._h, u._h, u._h, None), b"point_evaluate: u, values and gradients must differ")
    if d.n_dofs % 3 == 0:
        third = op.point_set(pv.uniform(d.n_dofs // 3, 11))
        assert refused(lib.mgamd_point_set_evaluate(third._h, op._h, u._h, None, u._h), b"point_evaluate: u, values and gradients must differ")
    # integrate
    with pytest.raises(E, match="point_integrate: vector size mismatch"):
        ps.integrate(mgamd.Vector(ctx, d.n_dofs + 1), values)
    with pytest.raises(E, match="number type"):
        ps.integrate(mgamd.Vector(ctx, d.n_dofs, mgamd.F32), values)
    with pytest.raises(E, match="point_integrate: values size mismatch"):
        ps.integrate(b, mgamd.Vector(ctx, 11))
    with pytest.raises(E, match="number type"):
        ps.integrate(b, mgamd.Vector(ctx, 10, mgamd.F32))
    with pytest.raises(E, match="point_integrate: gradients size mismatch"):
        ps.integrate(b, values, mgamd.Vector(ctx, 10))
    with pytest.raises(E, match="number type"):
        ps.integrate(b, None, mgamd.Vector(ctx, 30, mgamd.F32))
    with pytest.raises(E, match="point_integrate: neither values nor gradients"):
        ps.integrate(b)
    with pytest.raises(E, match="point_integrate: b is null"):
        ps.integrate(None, values)
    with pytest.raises(E, match="point_integrate: b aliases values"):
        many.integrate(b, b)
    with pytest.raises(E, match="point_integrate: b aliases gradients"):
        many.integrate(b, mgamd.Vector(ctx, d.n_dofs), b)
    assert refused(lib.mgamd_point_set_integrate(ps._h, op2._h, values._h, None, b._h), b"point_integrate: the point set belongs to another operator")
    with pytest.raises(ValueError, match="point_integrate: 3 values"):
        ps.integrate(b, np.zeros(3))
    assert op._point_tables_bytes()[1] == 0 and op._estimator_info()[0] == 0  # a refused call builds nothing
    # the operator of a local-smoothing level is refused; the active-mesh operator of such a hierarchy works
    ls = mgamd.Operator(ctx, mgamd.DoFs(plain.level_mesh(2), 2, local_smoothing_level=True))
    with pytest.raises(E, match="point_set: refused on the level of a local-smoothing hierarchy"):
        ls.point_set(pts)
    assert ls._point_tables_bytes() == (0, 0)
    h = mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-local")
    active = h.fine_operator
    assert (active.point_set(pts).evaluate(active.initialize_dof_vector()).to_host() == 0.0).all()

    # a distributed operator, two simulated ranks
    trias = mgamd.create_geometric_coarsening_sequence(plain)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    group = mgamd.SimGroup(2)

    def rank(r):
        sharded = mgamd.DoFs(trias[-1], 2, 0, partition=part, level=len(trias) - 1, rank=r)
        dist = mgamd.Operator(ctx, sharded, mgamd.F64, comm=group.comm(r))
        with pytest.raises(E, match="point_set: not implemented: sharded"):
            dist.point_set(pts)
        return dist._point_tables_bytes()

    assert run_ranks(2, rank) == [(0, 0)] * 2


def point_source_loop(mgamd, ctx, degree, refinements):
    """the Python restatement of examples/point_source.cpp: per mesh (cells, DoFs, CG iterations, u_h at the probes, the exact values)"""
    source, probes = np.array([0.13, -0.21, 0.07]), np.array([[-0.5, 0.5, 0.25], [0.6, 0.6, -0.6], [0.7, -0.3, 0.4]])
    exact = lambda X: 1.0 / (4.0 * np.pi * np.linalg.norm(X - source, axis=-1))
    out = []
    for r in range(refinements):
        t = mgamd.Triangulation("hypercube", 2 + r)
        h = mgamd.Hierarchy(ctx, t, None, degree, "HMG-global", coarse_solver="amg")
        op, d = h.fine_operator, h.dofs[-1]
        g = vec(op, exact(d.node_positions()))
        b, lift, x = op.initialize_dof_vector(), op.initialize_dof_vector(), op.initialize_dof_vector()
        at_source = op.point_set(source)
        assert at_source.all_points_found()
        at_source.integrate(b, np.ones(1))
        op.rhs_dirichlet(lift, g)
        b.from_host(b.to_host() + lift.to_host())
        it, _ = mgamd.solve_cg(op, h.mg, x, b, 1e-12)
        op.distribute_values(x, g)
        at_probes = op.point_set(probes)
        assert at_probes.all_points_found()
        out.append(dict(cells=t.n_cells, dofs=d.n_dofs, iterations=it, u=at_probes.evaluate(x).to_host(), exact=exact(probes)))
    return out


def test_example(mgamd, ctx):
    """bin/point_source 2 2 runs, and its probes agree with the Python restatement of the same solve to the printed digits (two CG
    iterates at reltol 1e-12: 1e-5 relative on the six printed digits of u_h, and the printed error against |u_h - g| of the restatement
    to 1e-5 of u_h).  A record: no convergence rate is asserted."""
    r = subprocess.run([os.path.join(ROOT, "bin", "point_source"), "2", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    lines = [l.split() for l in r.stdout.strip().split("\n")]
    assert len(lines) == 2
    for l, dev in zip(lines, point_source_loop(mgamd, ctx, 2, 2)):
        assert l[0:8:2] == ["refinement", "cells", "dofs", "cg_iterations"]
        rec = dict(zip(l[0::2], l[1::2]))
        assert int(rec["cells"]) == dev["cells"] and int(rec["dofs"]) == dev["dofs"]
        for k in range(3):
            assert abs(float(rec[f"u_{k}"]) / dev["u"][k] - 1.0) <= 1e-5
            assert abs(float(rec[f"error_{k}"]) - abs(dev["u"][k] - dev["exact"][k])) <= 1e-5 * abs(dev["u"][k])
