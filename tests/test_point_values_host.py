"""Point evaluation and point sources on the host: the numpy oracle (tests/point_values_oracle.py) against mathematics, the host
functions DoFs.locate_points / point_evaluate / point_integrate (LevelTables::locate_points, point_evaluate, point_integrate) against
the oracle, and the host-side refusals.  The device kernels are held against the same oracle by test_gpu_point_values.py.

Closed form: for q in Q_p the level's function of the nodal values of q IS q, so u_h(x) = q(x) and grad u_h(x) = grad q(x) at ANY point
of any leaf, hanging nodes or not.

Tolerances (from the arithmetic, not from what the code gives), the project's per-kernel FP64 bound 1e-12 (README) on the sizes of what
is added, not on a sum that may cancel:
  * evaluate: per point 1e-12 sum_i |phi_i(x)| |u_i| for the value and 1e-12 sum_i |d_c phi_i(x)| |u_i| for each gradient component
    (u_i the conforming nodal values of the point's leaf; the oracle's absolute=True): (p+1)^3 products per point, each with a few
    roundings, and the 1D bases are products of at most p differences;
  * integrate: per row 1e-12 B_i, B_i the oracle's load of |data| against |phi_i|, |grad phi_i| through |Ch|.
evaluate is held to the plain bound.  For integrate the oracle's own error (point_values_oracle.py, absolute="reference": its nodes are
off by up to 4 units in the last place) is added to 1e-12 B_i, because rows with a small B_i see that node error at full size; the RAW
ratio max |b_i - oracle| / B_i over the rows above noise level (B_i > 1e-12 max_j B_j) is printed with the number of rows that needed
the allowance.
Location is compared bit for bit: one addition in double, then exact operations on both sides.
The largest measured ratio is printed by every test (DESIGN.md records them)."""
import ctypes as C

import numpy as np
import pytest

import cell_values_oracle as co
import error_estimator_oracle as eo
import mgoracle
import physics_oracle as po
import point_values_oracle as pv
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


def point_sets(cells, n_uniform=300):
    """every kind of set the device tests use, smaller: uniform points, many points in one leaf, centres and corners of every leaf (the
    ties and the +1 faces), duplicates, points outside the cube and a NaN; (all points, which of them lie in the cube)"""
    inside = np.concatenate([pv.uniform(n_uniform, 1), pv.inside_leaf(cells, len(cells) // 2, 70, 2), pv.centres_and_corners(cells)])
    inside = np.concatenate([inside, inside[:5], inside[:5]])
    return np.concatenate([inside, pv.outside()]), np.arange(len(inside) + 6) < len(inside)


@pytest.mark.parametrize("p", DEGREES)
def test_oracle_against_closed_forms(p):
    """the oracle against mathematics on quadrant 2 (hanging faces and edges): u_h = q and grad u_h = grad q for q in Q_p at uniform points,
    at the centres and corners of every leaf and at many points of one leaf; NaN in the hanging entries is never used"""
    s = eo.nodal_space(mesh("quadrant", 2), p)
    pos = mgoracle.Level.node_positions(s)
    q = co.polynomial(p, 10 + p)
    pts, inside = point_sets(s.cells, 200)
    cell, xi = pv.locate(s.cells, pts)
    assert np.array_equal(cell >= 0, inside) and (xi >= 0.0).all() and (xi <= 1.0).all()
    u, g = pv.evaluate(s, np.where(s.hanging, np.nan, q(*pos.T)), pts)
    bu, bg = pv.evaluate(s, np.where(s.hanging, 0.0, q(*pos.T)), pts, absolute=True)
    assert (u[~inside] == 0.0).all() and (g[:, ~inside] == 0.0).all()
    X = pts[inside].T
    worst = max(pv.ratio(np.abs(u[inside] - q(*X)), bu[inside]),
                max(pv.ratio(np.abs(g[c, inside] - q.deriv(c)(*X)), bg[c, inside]) for c in range(3)))
    print(f"p={p}: oracle against the polynomial, max error / bound = {worst:.2e}")
    assert worst <= TOL


def test_device_sets_reach_every_path(oracle):
    """the sets of test_gpu_point_values.py against the kernels' constants: a leaf with more points than three strides of 256 threads and
    than ten batches of 64; every leaf occupied by `everything`, so the occupied leaves fill more than one group and leave a partial last
    group at every degree on some mesh; leaves without points (the set of 257 uniform points leaves some of quadrant 3's leaves empty)"""
    for name in ("hypercube0", "hypercube1", "quadrant3", "S"):
        cells = eo.nodal_space(leaves_of(oracle, name), 1).cells
        sets = pv.device_sets(cells)
        cell, _ = pv.locate(cells, sets["everything"])
        assert np.array_equal(cell >= 0, sets["inside"]) and len(sets["everything"]) == 1000 + 700 + 9 * len(cells) + 78 + 6
        assert np.bincount(cell[cell >= 0]).max() > 700
        assert len(np.unique(cell[cell >= 0])) == len(cells)
        if name == "quadrant3":
            occupied = len(np.unique(pv.locate(cells, sets["wave_and_one"])[0]))
            assert 32 < occupied < 120
    counts = [1, 8, 120, 50]  # occupied leaves of `everything` per mesh
    for p in DEGREES:
        per_group = max(1, 256 // (p + 1) ** 3)
        assert any(n % per_group for n in counts) if per_group > 1 else True
        assert any(n > per_group for n in counts)  # more than one workgroup


def test_oracle_tie_rule():
    """the box test of the oracle on hypercube 1: the centre of the cube belongs to the last leaf (upper side in x, y and z), a point on
    x = +1 to the upper leaf in x with xi = 1, and the reference coordinates are exact"""
    cells = sorted(mesh("hypercube", 1))
    cell, xi = pv.locate(cells, [[0.0, 0.0, 0.0], [1.0, -0.5, -1.0], [-1.0, -1.0, -1.0], [0.0, -0.25, 0.5]])
    assert [tuple(cells[c]) for c in cell] == [(1, 1, 1, 1), (1, 1, 0, 0), (1, 0, 0, 0), (1, 1, 0, 1)]
    assert np.array_equal(xi, [[0.0, 0.0, 0.0], [1.0, 0.5, 0.0], [0.0, 0.0, 0.0], [0.0, 0.75, 0.5]])


@pytest.mark.parametrize("name", ["hypercube0", "hypercube1", "quadrant3", "S"])
def test_host_location_against_oracle(mgamd, oracle, name):
    """DoFs.locate_points against the oracle's box test, cell and reference coordinate bit for bit; every in-domain point is found"""
    t, d, s, perm = product(mgamd, oracle, name, 2)
    pts, inside = point_sets(s.cells)
    cell, xi = d.locate_points(pts)
    ref_cell, ref_xi = pv.locate(s.cells, pts)
    assert np.array_equal(cell >= 0, inside)
    assert np.array_equal(cell, ref_cell) and np.array_equal(xi, ref_xi)
    empty = d.locate_points(np.zeros((0, 3)))
    assert empty[0].shape == (0,) and empty[1].shape == (0, 3)


@pytest.mark.parametrize("name,degrees", [("quadrant2", DEGREES), ("quadrant3", (1, 2, 4, 7)), ("S", (1, 3, 5, 7))])
def test_host_functions_against_oracle(mgamd, oracle, name, degrees):
    """DoFs.point_evaluate and DoFs.point_integrate against the oracle: a seeded vector with NaN in the hanging entries; seeded weights,
    values only, gradients only, both; points outside the cube give exact zeros and add nothing"""
    worst_e = worst_b = 0.0
    noise_rows = 0
    for p in degrees:
        t, d, s, perm = product(mgamd, oracle, name, p)
        pts, inside = point_sets(s.cells, 100)
        rng = np.random.default_rng(30 + p)
        x = rng.standard_normal(d.n_dofs)
        if d.info.n_hanging:
            x[d.n_dofs - d.info.n_hanging:] = np.nan
        u, g = d.point_evaluate(pts, x, True, True)
        assert np.array_equal(u, d.point_evaluate(pts, x)) and np.array_equal(g, d.point_evaluate(pts, x, False, True))
        assert g.shape == (3, len(pts)) and (u[~inside] == 0.0).all() and (g[:, ~inside] == 0.0).all()
        ref_u, ref_g = pv.evaluate(s, np.nan_to_num(x)[perm], pts)
        bu, bg = pv.evaluate(s, np.nan_to_num(x)[perm], pts, absolute=True)
        worst_e = max(worst_e, pv.ratio(np.abs(u - ref_u), bu), pv.ratio(np.abs(g - ref_g).ravel(), bg.ravel()))
        w, W = rng.standard_normal(len(pts)), rng.standard_normal((3, len(pts)))
        for w_, W_ in ((w, None), (None, W), (w, W)):
            b = d.point_integrate(pts, w_, W_)
            assert (b[d.n_dofs - d.info.n_hanging - d.info.n_dirichlet:] == 0.0).all()
            ref, size = pv.integrate(s, pts, w_, W_), pv.integrate(s, pts, w_, W_, absolute=True)
            r, n_noise = pv.row_ratio(np.abs(b[perm] - ref), size, pv.integrate(s, pts, w_, W_, absolute="reference"), TOL)
            worst_b, noise_rows = max(worst_b, r), noise_rows + n_noise
        # the points outside add nothing: the same bits without them
        assert np.array_equal(d.point_integrate(pts[inside], w[inside], W[:, inside]), d.point_integrate(pts, w, W))
        assert (d.point_integrate(np.zeros((0, 3)), np.zeros(0)) == 0.0).all()
    print(f"{name}: point_evaluate max error / bound = {worst_e:.2e}, point_integrate max |b_i - oracle| / B_i = {worst_b:.2e} (raw; {noise_rows} rows above 1e-12 B_i)")
    assert worst_e <= TOL  # (worst_b: the raw figure, held row by row in row_ratio with the oracle's own error)


def test_host_refusals(mgamd):
    plain = mgamd.Triangulation("quadrant", 3)
    d = mgamd.DoFs(plain, 2)
    E = mgamd.MgamdError
    pts, u = np.zeros((4, 3)), np.zeros(d.n_dofs)
    with pytest.raises(E, match="point_integrate: neither values nor gradients"):
        d.point_integrate(pts)
    with pytest.raises(E, match="point_evaluate: neither values nor gradients"):
        d.point_evaluate(pts, u, False, False)
    with pytest.raises(ValueError, match="point_integrate: 1 values"):
        d.point_integrate(pts, np.zeros(1))
    with pytest.raises(ValueError, match="point_evaluate"):
        d.point_evaluate(pts, np.zeros(d.n_dofs + 1))
    with pytest.raises(ValueError, match="locate_points: points of shape"):
        d.locate_points(np.zeros((4, 2)))
    lib = C.CDLL(mgamd._LIB_PATH)
    lib.mgamd_last_error.restype = C.c_char_p
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    n, cell, ref, out = C.c_uint64(4), np.zeros(4, np.int32), np.zeros((4, 3)), np.zeros(4)
    assert lib.mgamd_dofs_locate_points(d._h, n, None, ptr(cell), ptr(ref)) == 3 and b"locate_points: a null pointer" in lib.mgamd_last_error()
    assert lib.mgamd_dofs_locate_points(d._h, n, ptr(pts), None, ptr(ref)) == 3 and b"locate_points: a null pointer" in lib.mgamd_last_error()
    assert lib.mgamd_dofs_locate_points(None, n, ptr(pts), ptr(cell), ptr(ref)) == 3 and b"null argument" in lib.mgamd_last_error()
    assert lib.mgamd_dofs_point_evaluate(d._h, n, ptr(pts), None, ptr(out), None) == 3 and b"point_evaluate: u is null" in lib.mgamd_last_error()
    assert lib.mgamd_dofs_point_evaluate(d._h, n, None, ptr(u), ptr(out), None) == 3 and b"point_evaluate: xyz is null" in lib.mgamd_last_error()
    assert lib.mgamd_dofs_point_integrate(d._h, n, ptr(pts), ptr(out), None, None) == 3 and b"point_integrate: out is null" in lib.mgamd_last_error()
    assert lib.mgamd_dofs_point_integrate(d._h, n, None, ptr(out), None, ptr(u)) == 3 and b"point_integrate: xyz is null" in lib.mgamd_last_error()
    ls = mgamd.DoFs(plain.level_mesh(2), 2, local_smoothing_level=True)
    for who, call in (("locate_points", lambda t: t.locate_points(pts)), ("point_evaluate", lambda t: t.point_evaluate(pts, np.zeros(t.n_dofs))),
                      ("point_integrate", lambda t: t.point_integrate(pts, np.zeros(4)))):
        with pytest.raises(E, match=f"{who}: refused on the level of a local-smoothing hierarchy"):
            call(ls)
    trias = mgamd.create_geometric_coarsening_sequence(plain)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    sharded = mgamd.DoFs(trias[-1], 2, 0, partition=part, level=len(trias) - 1, rank=0)
    for who, call in (("locate_points", lambda t: t.locate_points(pts)), ("point_evaluate", lambda t: t.point_evaluate(pts, np.zeros(t.n_dofs))),
                      ("point_integrate", lambda t: t.point_integrate(pts, np.zeros(4)))):
        with pytest.raises(E, match=f"{who}: not implemented: sharded"):
            call(sharded)
