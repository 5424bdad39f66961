"""The jump error indicator on the device (Operator.estimate_error: face_flux_kernel + flux_jump_kernel), the carry-over of a
solution onto the refined mesh, and the adaptive loop, against tests/error_estimator_oracle.py and closed forms.

Tolerances (they come from the arithmetic, not from what the kernels give):
  * |eta^2 - eta^2_ref| <= 1e-11 max eta^2_ref: FP64 rounding of a difference of two fluxes whose derivative entries are <~ p^2 / h,
    with headroom (operator applications are held to 1e-13 here);
  * where the reference is exactly 0: eta_K <= 1e-11 a_max max|grad u| h_K^(3/2);
  * FP32 operators are compared with the oracle on the float-rounded vector: the kernels convert at the load and compute in double.
    A closed form that is exactly 0 is, on the rounded vector, a reference of the size of the rounding (eta ~ 1e-7 h^(3/2)), and
    1e-11 of THAT is below the double rounding of either side.  eta is the (weighted) L2 norm of the jump r, so a perturbation
    delta of r moves it by at most the norm of delta: those cases assert |eta_K - eta_ref,K| <= 1e-11 a_max max|grad u| h_K^(3/2), the
    second rule applied to the difference, which is that rule itself where eta_ref = 0.
The largest measured ratios are printed by every test (DESIGN.md records them)."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import error_estimator_oracle as eo
import mgoracle
import physics_oracle as po
import random_mesh_physics as rm
from conftest import ROOT
from physics_oracle import Problem
from support import mesh, tria_of

pytestmark = pytest.mark.gpu

TOL = 1e-11
DEGREES = (1, 2, 3, 4, 5, 6, 7)


def build(mgamd, ctx, leaves, p, problem=Problem(), number_type=None):
    """the product's mesh, tables and operator of the problem on the leaves, and the oracle's space with the problem on its cells"""
    t = tria_of(mgamd, leaves, problem)
    d = mgamd.DoFs(t, p)
    op = mgamd.Operator(ctx, d, number_type or mgamd.F64)
    s = eo.nodal_space(leaves, p)
    assert po.product_cells(t) == [tuple(c) for c in s.cells]
    return t, d, op, s, eo.on(problem, s.cells)


def rounded(x, number_type):
    return x if number_type == 8 else x.astype(np.float32).astype(np.float64)


def estimate(op, x, q=None):
    return op.estimate_error(op.initialize_dof_vector().from_host(x), q)


def ratio(eta, ref2):
    return np.abs(eta ** 2 - ref2).max() / ref2.max()


def zero_ratio(eta, eta_ref, h, a_max, gmax):
    return (np.abs(eta - eta_ref) / (a_max * gmax * h ** 1.5)).max()


def cell_h(s):
    return np.array([2.0 / (1 << c[0]) for c in s.cells])


@pytest.mark.parametrize("number_type", [8, 4])
@pytest.mark.parametrize("p", DEGREES)
def test_closed_forms(mgamd, ctx, p, number_type):
    """u = x on quadrant 3 (120 cells): the coefficient jump across the hanging faces on x = 0, the natural, exact-flux and convective
    boundary residuals of test_error_estimator_host.py.  FP64 against the closed forms, FP32 against the oracle on the rounded vector."""
    leaves = mesh("quadrant", 3)
    f64 = number_type == 8
    worst, worst0 = 0.0, 0.0
    beta, u_ext = 2.5, -0.75
    r = beta * u_ext - beta - 1.0
    jump = Problem(coefficient=lambda c: 1.0 if po._centre(c)[0] < 0 else 3.0)
    natural = Problem(dirichlet_faces=0b111100)
    robin = Problem(dirichlet_faces=0b111101, robin=(0, beta, 0, 0, 0, 0))
    cases = [("jump", jump, None, 3.0), ("q=0", natural, np.zeros(6), 1.0), ("exact flux", natural, np.array([-1.0, 1, 0, 0, 0, 0]), 1.0),
             ("Robin exact", robin, np.array([0, beta * (1 + 1 / beta), 0, 0, 0, 0]), 1.0), ("Robin", robin, np.array([0, beta * u_ext, 0, 0, 0, 0]), 1.0)]
    built = {}
    for name, problem, q, a_max in cases:
        if id(problem) not in built:  # (the three q of `natural` and the two of `robin` share their tables and operator)
            built[id(problem)] = build(mgamd, ctx, leaves, p, problem, number_type)
        t, d, op, s, prob = built[id(problem)]
        h, x = cell_h(s), rounded(d.node_positions()[:, 0].copy(), number_type)
        eta = estimate(op, x, q)
        assert eta.shape == (120,) and np.isfinite(eta).all() and (eta >= 0).all()
        f0, f1 = (np.array([c[1] == (((1 << c[0]) - 1) if side else 0) for c in s.cells]) for side in (0, 1))
        touches = np.array([abs(po._centre(c)[0]) < 2.0 / (1 << c[0]) for c in s.cells])
        closed = dict(jump=np.where(touches, h ** 3 / 6, 0.0), **{"q=0": np.where(f0 | f1, h ** 3 / 24, 0.0), "exact flux": 0 * h, "Robin exact": 0 * h,
                                                                    "Robin": np.where(f1, h ** 3 / 24 * r * r, 0.0)})[name]
        ref2 = closed if f64 else eo.indicator_squared(s, prob, eo.to_oracle(s, d.keys(), x), q)
        if closed.max() > 0:
            worst = max(worst, ratio(eta, ref2))
        else:
            worst0 = max(worst0, zero_ratio(eta, np.sqrt(ref2), h, a_max, 1.0))
    print(f"closed forms p={p} {'FP64' if f64 else 'FP32'}: |eta^2 - ref| / max ref {worst:.2e}; zero references: eta / (a |grad u| h^1.5) {worst0:.2e}")
    assert worst <= TOL and worst0 <= TOL


MIXED = dict(coefficient="per_cell", dirichlet_faces=0b011110, robin=(1.75, 0, 0, 0, 0, 0))  # natural: x = -1 (convective) and z = +1
Q = np.array([0.6, 0.0, 0.0, 0.0, 0.0, -1.25])

ORACLE_CASES = ([("hypercube0", p) for p in DEGREES] + [("hypercube1", p) for p in DEGREES] + [("quadrant3", p) for p in DEGREES] +
                [("S", 5), ("S", 6), ("S", 7), ("M", 1), ("M", 2), ("M", 3), ("B", 1), ("B", 2), ("B", 3), ("R", 1), ("circle4", 2)])


def leaves_of(oracle, name):
    named = dict(hypercube0=("hypercube", 0), hypercube1=("hypercube", 1), quadrant3=("quadrant", 3), circle4=("circle", 4))
    return mesh(*named[name]) if name in named else rm.leaves_of(oracle, name)


def seeded_vector(d, seed):
    """random entries at free and Dirichlet DoFs; NaN at the hanging ones, which must never be read"""
    x = np.random.default_rng(seed).standard_normal(d.n_dofs)
    x[d.n_dofs - d.info.n_hanging:] = np.nan
    return x


@pytest.mark.parametrize("name,p", ORACLE_CASES)
def test_against_oracle(mgamd, oracle, ctx, name, p):
    """a seeded vector, the per_cell coefficient (the two sides of every face differ), natural faces, one convective face and q.
    The cell counts 1, 8, 50, 120, 344, 757 leave partial packs in both kernels at every degree (cells per workgroup pass 32, 9, 4, 2, 1,
    1, 1 and 64, 28, 16, 10, 7, 5, 4).  p = 4 with hanging faces runs on quadrant 3 here and on the PMG level below."""
    leaves = leaves_of(oracle, name)
    t, d, op, s, prob = build(mgamd, ctx, leaves, p, Problem(**MIXED))
    if name == "circle4":
        assert d.info.n_hanging > 0  # the smallest refinement of circle with hanging nodes
    x = seeded_vector(d, 11)
    eta = estimate(op, x, Q)
    assert np.isfinite(eta).all()
    ref2 = eo.indicator_squared(s, prob, eo.to_oracle(s, d.keys(), x), Q)
    print(f"{name} p={p}: {len(s.cells)} cells, |eta^2 - ref| / max ref {ratio(eta, ref2):.2e}")
    assert ratio(eta, ref2) <= TOL


@pytest.mark.parametrize("p", [2, 5])
def test_fp32_operator_against_oracle_on_rounded_vector(mgamd, oracle, ctx, p):
    leaves = leaves_of(oracle, "quadrant3" if p == 2 else "S")
    t, d, op, s, prob = build(mgamd, ctx, leaves, p, Problem(**MIXED), mgamd.F32)
    x = rounded(np.nan_to_num(seeded_vector(d, 12)), 4)
    ref2 = eo.indicator_squared(s, prob, eo.to_oracle(s, d.keys(), x), Q)
    worst = ratio(estimate(op, x, Q), ref2)
    print(f"FP32 p={p}: |eta^2 - ref| / max ref {worst:.2e}")
    assert worst <= TOL


def test_finest_level_of_a_pmg_hierarchy(mgamd, ctx):
    prob = Problem(**MIXED)
    h = mgamd.Hierarchy(ctx, tria_of(mgamd, mesh("quadrant", 3), prob), degree=4, mg_type="PMG")
    d, op, s = h.dofs[-1], h.operators[-1], eo.nodal_space(mesh("quadrant", 3), 4)
    x = seeded_vector(d, 13)
    ref2 = eo.indicator_squared(s, eo.on(prob, s.cells), eo.to_oracle(s, d.keys(), x), Q)
    worst = ratio(estimate(op, x, Q), ref2)
    print(f"PMG finest level: |eta^2 - ref| / max ref {worst:.2e}")
    assert worst <= TOL
    assert all(o._estimator_info()[0] == 0 for o in h.operators[:-1])  # the levels that were never asked hold no tables


def test_bit_identical_hanging_entries_unread_and_negative_control(mgamd, oracle, ctx):
    t, d, op, s, prob = build(mgamd, ctx, mesh("quadrant", 3), 3, Problem(**MIXED))
    assert op._estimator_info() == (0, 0.0, 0.0)  # nothing is built before the first call
    x = np.random.default_rng(14).standard_normal(d.n_dofs)
    a, b = estimate(op, x, Q), estimate(op, x, Q)
    assert np.array_equal(a, b)
    nan = x.copy()
    nan[d.n_dofs - d.info.n_hanging:] = np.nan
    assert d.info.n_hanging > 0 and np.array_equal(estimate(op, nan, Q), a)
    nbytes, build_ms, kernel_ms = op._estimator_info()
    n = 4
    assert nbytes == 120 * (4 * n ** 3 + 48 * n ** 2 + 128) and build_ms > 0 and kernel_ms > 0
    # negative control: the reference with ONE coefficient value changed is outside the tolerance
    xo = eo.to_oracle(s, d.keys(), x)
    assert ratio(a, eo.indicator_squared(s, prob, xo, Q)) <= TOL
    cell = s.cells[60]
    wrong = dataclasses.replace(prob, coefficient={**prob.coefficient, cell: prob.coefficient[cell] * (1 + 1e-9)})
    bad = ratio(a, eo.indicator_squared(s, wrong, xo, Q))
    print(f"negative control: one coefficient off by 1e-9 gives {bad:.2e}")
    assert bad > TOL


def test_refusals(mgamd, ctx):
    t = mgamd.Triangulation("quadrant", 3)
    t.set_dirichlet_faces(0b111110)
    d = mgamd.DoFs(t, 2)
    op = mgamd.Operator(ctx, d)
    u = op.initialize_dof_vector()
    with pytest.raises(mgamd.MgamdError, match="vector size mismatch"):
        op.estimate_error(mgamd.Vector(ctx, d.n_dofs + 1))
    with pytest.raises(mgamd.MgamdError, match="number type"):
        op.estimate_error(mgamd.Vector(ctx, d.n_dofs, mgamd.F32))
    with pytest.raises(mgamd.MgamdError, match=r"boundary flux on face 0 \(x=-1\) is not finite"):
        op.estimate_error(u, [np.inf, 0, 0, 0, 0, 0])
    with pytest.raises(mgamd.MgamdError) as flux:
        op.estimate_error(u, {3: 2.0})
    with pytest.raises(mgamd.MgamdError) as load:
        op.rhs_boundary_flux(op.initialize_dof_vector(), {3: 2.0})
    assert str(flux.value) == str(load.value) and "the face is Dirichlet" in str(flux.value)  # worded as rhs_boundary_flux words it
    lib = C.CDLL(mgamd._LIB_PATH)
    lib.mgamd_last_error.restype = C.c_char_p
    assert lib.mgamd_level_op_estimate_error(op._h, u._h, None, None) == 3 and b"eta is null" in lib.mgamd_last_error()
    assert op._estimator_info()[0] == 0  # a refused call builds nothing
    # the operator of a local-smoothing level
    plain = mgamd.Triangulation("quadrant", 3)
    ls = mgamd.Operator(ctx, mgamd.DoFs(plain.level_mesh(2), 2, local_smoothing_level=True))
    with pytest.raises(mgamd.MgamdError, match="local-smoothing"):
        ls.estimate_error(ls.initialize_dof_vector())
    # a distributed operator
    trias = mgamd.create_geometric_coarsening_sequence(plain)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    sharded = mgamd.DoFs(trias[-1], 2, 0, partition=part, level=len(trias) - 1, rank=0)
    group = mgamd.SimGroup(2)
    dist = mgamd.Operator(ctx, sharded, mgamd.F64, comm=group.comm(0))
    with pytest.raises(mgamd.MgamdError, match="not implemented: sharded"):
        dist.estimate_error(dist.initialize_dof_vector())


def test_carry_over_to_the_refined_mesh(mgamd, oracle, ctx):
    """(old mesh, refined mesh) is a pair the per-cell transfer tables describe: no old leaf is split twice.  prolongate_and_add from
    the old operator to the new one interpolates the nodal vector of a function (Dirichlet entries are zeroed by the transfer)."""
    for p, frac in ((1, 0.2), (2, 0.15)):
        old = mgamd.Triangulation("quadrant", 3)
        new = old.refine(np.random.default_rng(p).random(old.n_cells) < frac)
        dc, df = mgamd.DoFs(old, p), mgamd.DoFs(new, p)
        oc, of = mgamd.Operator(ctx, dc), mgamd.Operator(ctx, df)
        lc = mgoracle.Level(set(po.product_cells(old)), p, numbering_keys=dc.keys())
        lf = mgoracle.Level(set(po.product_cells(new)), p, numbering_keys=df.keys())
        P = mgoracle.build_transfer(lf, lc)
        x, y, z = dc.node_positions().T
        uc = np.sin(2 * x) * np.cos(y) + z * z
        vf = of.initialize_dof_vector()
        vf.set(0.0)
        mgamd.MGTwoLevelTransfer(of, oc).prolongate_and_add(vf, oc.initialize_dof_vector().from_host(uc))
        ref = P @ uc
        err = np.abs(vf.to_host() - ref).max() / np.abs(ref).max()
        print(f"carry-over p={p}: {old.n_cells} -> {new.n_cells} cells, max error {err:.2e}")
        assert new.n_cells > old.n_cells and err <= 1e-13


def exact_error(positions, u):
    return np.abs(u - mgoracle.gaussian_solution(*positions.T)).max()


@pytest.fixture(scope="module")
def loop(mgamd, ctx):
    """the adaptive loop on the device: p = 2 from hypercube 2, theta = 0.5, CG to 1e-10, four solves"""
    t, out = mgamd.Triangulation("hypercube", 2), []
    for cycle in range(4):
        h = mgamd.Hierarchy(ctx, t, degree=2, mg_type="HMG-global")
        op, d = h.fine_operator, h.dofs[-1]
        b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
        op.rhs(b, 1)
        mgamd.solve_cg(op, h.mg, x, b, 1e-10)
        op.distribute(x, 1)
        eta = op.estimate_error(x)
        flags = mgamd.mark_maximum(eta, 0.5)
        out.append(dict(cells=po.product_cells(t), n_dofs=d.n_dofs, eta=eta, flags=flags, error=exact_error(d.node_positions(), x.to_host())))
        t = t.refine(flags)
    return out


def test_adaptive_loop(mgamd, oracle, ctx, loop):
    import scipy.sparse.linalg as spla

    errors, sums = [], []
    for cycle, dev in enumerate(loop):
        lv = oracle.Level(set(dev["cells"]), 2)
        assert [tuple(c) for c in lv.cells] == dev["cells"]
        x = spla.spsolve(lv.A.tocsc(), lv.rhs_function(oracle.gaussian_rhs, oracle.gaussian_solution))
        x = lv.distribute(x, oracle.gaussian_solution)
        eta2 = eo.indicator_squared(eo.nodal_space(lv.leaves, 2), Problem(), x)
        thr = 0.25 * eta2.max()
        print(f"cycle {cycle}: {len(lv.cells)} cells, {lv.n} DoFs, sum eta^2 {eta2.sum():.4g} (device {np.sum(dev['eta'] ** 2):.4g}), max nodal error "
              f"{exact_error(lv.node_positions(), x):.4g} (device {dev['error']:.4g}), closest eta^2 to the threshold "
              f"{np.abs(eta2 / thr - 1).min():.3g}")
        assert np.array_equal(dev["flags"], (np.sqrt(eta2) >= 0.5 * np.sqrt(eta2.max())).astype(np.uint8))  # no exclusion
        assert dev["n_dofs"] == lv.n
        errors.append(exact_error(lv.node_positions(), x))
        sums.append(np.sum(dev["eta"] ** 2))
        assert abs(dev["error"] / errors[-1] - 1.0) <= 1e-6
    assert [len(d["cells"]) for d in loop] == [64, 120, 176, 232]
    assert all(sums[c + 1] < sums[c] for c in range(3))
    # against the device's own uniform mesh of 4096 cells
    h = mgamd.Hierarchy(ctx, "hypercube", 4, 2, "HMG-global")
    op = h.fine_operator
    b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
    op.rhs(b, 1)
    mgamd.solve_cg(op, h.mg, x, b, 1e-10)
    op.distribute(x, 1)
    uniform = exact_error(h.dofs[-1].node_positions(), x.to_host())
    print(f"uniform hypercube 4, p = 2: {h.n_dofs} DoFs, max nodal error {uniform:.4g}; adaptive: {loop[-1]['n_dofs']} DoFs, {loop[-1]['error']:.4g}")
    assert loop[-1]["error"] < uniform


def test_example_prints_the_loop(loop):
    r = subprocess.run([os.path.join(ROOT, "bin", "adaptive_gaussian"), "2", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l.split() for l in r.stdout.strip().split("\n")]
    assert len(lines) == 4
    for l, dev in zip(lines, loop):
        rec = dict(zip(l[0::2], l[1::2]))
        assert int(rec["cells"]) == len(dev["cells"]) and int(rec["dofs"]) == dev["n_dofs"]
        assert abs(float(rec["max_nodal_error"]) / dev["error"] - 1.0) <= 1e-5  # (six printed digits)
        assert abs(float(rec["sum_eta2"]) / np.sum(dev["eta"] ** 2) - 1.0) <= 1e-5
