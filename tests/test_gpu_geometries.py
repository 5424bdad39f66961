"""The `circle` and `quadrant_flexible` meshes on the device.  Every other GPU module builds `quadrant`, `annulus` or `hypercube`;
these are the two remaining GeometryType values (octree.hpp create_mesh), `quadrant_flexible` being the harness's default.

circle L: three global refinements plus L - 3 point refinements at the origin, entirely in the interior.  circle 5 has 624 cells on
levels 3, 4, 5 and the coarsening sequence 1, 8, 64, 120, 176, 624: one step from the finest mesh removes 72 % of the cells (the
whole background coarsens, the centre keeps three levels of hanging nodes), the steps below it change only the centre.  circle 7
keeps the background one step longer (232, 960, 2976).  quadrant_flexible (g, l): g global refinements plus l refinements of the
octant x, y, z <= 0; (3, 1) is a mesh `quadrant` cannot produce, (2, 2) is the mesh of `quadrant` 4 reached through NRefLocal.

Everything is held against the numpy oracle (oracle/mgoracle.py, built once per case in the numbering of the product's max_brick=0
tables and permuted through the DoF keys for the default slot policy max_brick=-1), with the project's own bounds: operator, inverse
diagonal and transfers <= 1e-13, Chebyshev <= 1e-12, V-cycle <= 1e-11, CG iterates <= 1e-10 with equal iteration counts; FP32
levels as in test_gpu_float_levels.py (single kernels 2e-6, cycle 16 e_ref from oracle/f32_emulation.py and 5e-5); the sharded
cases as in test_gpu_distributed_sim.py; the physics case as test_gpu_robin.py::test_random_octree.

Oracle times on a CPU (hierarchy, V-cycle, PCG): the circle rows 0.5 - 2.6 s, circle 4 p = 4 PMG 11 s (the only p = 4 solve of this
module); quadrant_flexible (2, 2) p = 1, 2: 0.3, 1.6 s, (3, 1) p = 1, 2: 0.2, 1.8 s, (3, 1) p = 2 HPMG 1.9 s.  p = 4 on quadrant_flexible
needs 31 s and 36 s (HMG-global), 11 s and 17 s (HPMG): no hierarchy is built there; (3, 1) p = 4 runs the operator and inverse
diagonal of its finest level alone.  No hierarchy of this module has plain 17-point bricks (the centre of circle cuts every 8^3 and
4^3 block of its background), so none has fused transfer bricks: the default transfers and MGAMD_NO_FUSED_TRANSFER both run the
separate kernels here; fused bricks stay with the hypercube cases of test_gpu_parity.py and test_gpu_boundary.py.

The local-smoothing cases of these meshes are in test_gpu_local_smoothing.py (its CASES and test_hpmg_local).

Largest relative errors measured on an MI355X (over every level, both slot policies and the separate transfer kernels; every case
prints its own); bounds 1e-13 (operator, inverse diagonal, transfer), 1e-11 (V-cycle), 1e-10 (CG iterate), CG counts equal:

  case                                   operator  inv.diag  transfer  V-cycle  iterate  CG its
  circle 5 p=1 HMG-global                3.4e-16   2.1e-16   1.7e-16   6.3e-16  1.1e-15  3
  circle 5 p=2 HMG-global                3.3e-16   6.5e-16   2.3e-16   2.3e-15  8.4e-15  4
  circle 4 p=2 HMG-global                3.3e-16   6.3e-16   2.3e-16   1.2e-15  5.9e-15  4
  circle 6 p=1 HMG-global                3.4e-16   2.4e-16   1.4e-16   1.8e-15  2.5e-15  4
  circle 7 p=1 HMG-global                3.4e-16   2.4e-16   1.4e-16   1.4e-15  5.2e-15  4
  circle 6 p=2 HPMG                      3.4e-16   6.6e-16   2.2e-16   9.9e-16  2.2e-14  4
  circle 4 p=4 PMG                       1.0e-15   1.1e-15   1.3e-15   1.7e-15  5.1e-14  4
  quadrant_flexible (2, 2) p=1 HMG       3.4e-16   2.4e-16   2.2e-16   6.9e-16  1.4e-15  4
  quadrant_flexible (2, 2) p=2 HMG       3.2e-16   6.5e-16   2.2e-16   1.6e-15  9.0e-15  4
  quadrant_flexible (3, 1) p=1 HMG       3.4e-16   2.3e-16   1.7e-16   6.4e-16  1.1e-15  4
  quadrant_flexible (3, 1) p=2 HMG       3.2e-16   6.5e-16   2.2e-16   1.4e-15  9.0e-15  4
  quadrant_flexible (3, 1) p=2 HPMG      3.4e-16   6.5e-16   1.9e-16   8.3e-16  8.6e-15  4

Chebyshev <= 1.6e-15 (bound 1e-12); FP32 V-cycle 1.41 e_ref (circle 5 p=2) and 1.27 e_ref (circle 4 p=4 PMG), bound 16 e_ref; 3 and 4
simulated ranks and the two-tier case: operator <= 2.4e-16, V-cycle <= 2.3e-15, iterate <= 2.4e-14; the physics case: V-cycle
8.5e-16, iterate 3.9e-14, 5 CG iterations."""
import json
import os

import numpy as np
import pytest

import physics_oracle as po
import support as su
from _degree_cases import float_cycle_reference, round32
from conftest import rel_err
from physics_oracle import Problem
from support import GOLDEN, emu, final_table, key_vector, keyset, run_harness, run_ranks  # noqa: F401

pytestmark = pytest.mark.gpu

TOL_OP, TOL_CHEB, TOL_VCYCLE, TOL_SOL = 1e-13, 1e-12, 1e-11, 1e-10
TOL_OP_F32, MARGIN_F32, CAP_F32 = 2e-6, 16, 5e-5  # test_gpu_float_levels.py

CIRCLE_5_P1 = ("circle", 5, 1, "HMG-global")
CIRCLE_5_P2 = ("circle", 5, 2, "HMG-global")
CIRCLE_6_P1 = ("circle", 6, 1, "HMG-global")
CIRCLE_7_P1 = ("circle", 7, 1, "HMG-global")
CIRCLE_6_P2_HPMG = ("circle", 6, 2, "HPMG")
CIRCLE_4_P4_PMG = ("circle", 4, 4, "PMG")
FLEXIBLE_22_P2 = ("quadrant_flexible", (2, 2), 2, "HMG-global")
CASES = [CIRCLE_5_P1, CIRCLE_5_P2, ("circle", 4, 2, "HMG-global"), CIRCLE_6_P1, CIRCLE_7_P1, CIRCLE_6_P2_HPMG, CIRCLE_4_P4_PMG,
         ("quadrant_flexible", (2, 2), 1, "HMG-global"), FLEXIBLE_22_P2, ("quadrant_flexible", (3, 1), 1, "HMG-global"),
         ("quadrant_flexible", (3, 1), 2, "HMG-global"), ("quadrant_flexible", (3, 1), 2, "HPMG")]
FINE_DOFS = {CIRCLE_5_P1: 925, CIRCLE_5_P2: 6265, ("circle", 4, 2, "HMG-global"): 5589, CIRCLE_6_P1: 1761, CIRCLE_7_P1: 3967,
             CIRCLE_6_P2_HPMG: 12305, CIRCLE_4_P4_PMG: 40481}
POLICIES = [0, -1]  # max_brick: bricks wherever they fit; the default: single-cell slots on the latency-bound small levels


def refs(L):
    """(n_ref_global, n_ref_local): a tuple for quadrant_flexible, NRefGlobal alone elsewhere"""
    return L if isinstance(L, tuple) else (L, 0)


def case_id(c):
    return "-".join(["+".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c]) if isinstance(c, tuple) else str(c)


class Renumbered:
    """an oracle level in the numbering of another DoF handler of the same space (matched through the geometric DoF keys)"""

    def __init__(self, lv, perm, keys):
        self.n, self.p, self.keys = lv.n, lv.p, keys
        self.A, self.inv_diag = lv.A[perm][:, perm].tocsr(), lv.inv_diag[perm]
        self.rhs_constant, self.constrained = lv.rhs_constant[perm], lv.constrained[perm]


def renumber(levels, P, dofs):
    perms = []
    for lv, d in zip(levels, dofs):
        pos = {k: i for i, k in enumerate(keyset(lv.keys))}
        perm = np.array([pos[k] for k in keyset(d.keys())])
        assert len(perm) == lv.n and len(set(perm.tolist())) == lv.n
        perms.append(perm)
    new = [Renumbered(lv, perm, keyset(d.keys())) for lv, perm, d in zip(levels, perms, dofs)]
    return new, [None] + [P[l][perms[l]][:, perms[l - 1]].tocsr() for l in range(1, len(levels))]


@pytest.fixture(scope="module")
def hierarchies(mgamd, oracle, ctx):
    """(Hierarchy, oracle levels, oracle transfers) of a case under a slot policy; the oracle hierarchy of a case is built once, in
    the numbering of the max_brick=0 tables"""
    cache, built = {}, {}

    def get(case, max_brick):
        if (case, max_brick) not in cache:
            geo, L, p, mg_type = case
            g, loc = refs(L)
            h = mgamd.Hierarchy(ctx, geo, g, p, mg_type, n_ref_local=loc, coarse_solver="amg", max_brick=max_brick)
            if case not in built:
                h0 = h if max_brick == 0 else get(case, 0)[0]
                built[case] = oracle.build_hierarchy(geo, g, p, mg_type, n_ref_local=loc, numbering_keys=[d.keys() for d in h0.dofs])
            lv, P = built[case] if max_brick == 0 else renumber(*built[case], h.dofs)
            assert [l.n for l in lv] == [d.n_dofs for d in h.dofs]
            cache[(case, max_brick)] = (h, lv, P)
        return cache[(case, max_brick)]

    return get


@pytest.fixture(scope="module")
def oracle_solves(oracle, hierarchies):
    """the oracle's multigrid and preconditioned solve of a case under a slot policy (the numbering enters through the index-based
    start vector of the eigenvalue estimates), computed once"""
    cache = {}

    def get(case, max_brick):
        if (case, max_brick) not in cache:
            h, lv, P = hierarchies(case, max_brick)
            mg = oracle.Multigrid(lv, P, 3, coarse="direct")
            cache[(case, max_brick)] = (mg,) + tuple(oracle.pcg(lv[-1].A, lv[-1].rhs_constant, mg.vcycle, 1e-4))
        return cache[(case, max_brick)]

    return get


def check_level(op, lv, tag):
    rng = np.random.default_rng(3)
    worst = 0.0
    for trial in range(2):  # (twice: the tail accumulator must be clean after a pass)
        x = rng.standard_normal(lv.n)
        src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector()
        dst.set(7.0)  # vmult must overwrite
        op.vmult(dst, src)
        worst = max(worst, rel_err(dst.to_host(), lv.A @ x))
        assert np.array_equal(src.to_host(), x)
    diag = op.initialize_dof_vector()
    op.compute_inverse_diagonal(diag)
    ed = rel_err(diag.to_host(), lv.inv_diag)
    print(f"{tag}: {lv.n} DoFs, vmult {worst:.2e} inverse diagonal {ed:.2e}")
    assert worst < TOL_OP and ed < TOL_OP
    return worst, ed


def check_transfers(h, lv, P, tag, tol=TOL_OP, rounded=False):
    """both directions accumulate into a non-zero vector (test_gpu_local_smoothing.py)"""
    rng = np.random.default_rng(6)
    draw = (lambda n: round32(rng.standard_normal(n))) if rounded else rng.standard_normal
    worst = 0.0
    for l in range(1, len(lv)):
        xc, xf0 = draw(lv[l - 1].n), draw(lv[l].n)
        vc, vf = h.operators[l - 1].initialize_dof_vector().from_host(xc), h.operators[l].initialize_dof_vector().from_host(xf0)
        h.transfers[l].prolongate_and_add(vf, vc)
        e1 = rel_err(vf.to_host(), xf0 + P[l] @ xc)
        rf, dc0 = draw(lv[l].n), draw(lv[l - 1].n)
        vr, vd = h.operators[l].initialize_dof_vector().from_host(rf), h.operators[l - 1].initialize_dof_vector().from_host(dc0)
        h.transfers[l].restrict_and_add(vd, vr)
        e2 = rel_err(vd.to_host(), dc0 + P[l].T @ rf)
        print(f"{tag} transfer {l - 1} -> {l} ({h.trias[l - 1].n_cells} -> {h.trias[l].n_cells} cells, p {lv[l - 1].p} -> {lv[l].p}): "
              f"prolongate {e1:.2e} restrict {e2:.2e}")
        assert e1 < tol and e2 < tol
        assert np.array_equal(vc.to_host(), xc) and np.array_equal(vr.to_host(), rf)
        worst = max(worst, e1, e2)
    return worst


# ------------------------------------------------------------------ operator, inverse diagonal and transfers on every level
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_operator_inverse_diagonal_and_transfers(mgamd, ctx, hierarchies, monkeypatch, case):
    geo, L, p, mg_type = case
    groups = {}
    for max_brick in POLICIES:
        h, lv, P = hierarchies(case, max_brick)
        if case in FINE_DOFS:
            assert h.n_dofs == lv[-1].n == FINE_DOFS[case]
        groups[max_brick] = [[(B, n) for B, n in d.groups() if n] for d in h.dofs]
        tag = f"{case_id(case)} max_brick={max_brick}"
        errs = [check_level(op, l, f"{tag} level {i}") for i, (op, l) in enumerate(zip(h.operators, lv))]
        et = check_transfers(h, lv, P, f"{tag} ({sum(t.n_fused_bricks() for t in h.transfers[1:])} fused bricks)")
        print(f"{tag} WORST: operator {max(e[0] for e in errs):.2e} inverse diagonal {max(e[1] for e in errs):.2e} transfer {et:.2e}")
    print(f"{case_id(case)} slot groups: max_brick=0 {groups[0]}  max_brick=-1 {groups[-1]}")
    if geo == "circle" and L in (5, 6):
        if p >= 2:
            assert groups[0] != groups[-1]  # the two runs are not the same tables twice
        else:
            # p = 1: LevelTables::build leaves every cell to the single-cell cluster kernel, so both policies give single-cell slots
            # only; said here so that the equality is a stated fact and not an accident
            assert groups[0] == groups[-1] and all(B == 1 for g in groups[0] for B, _ in g)
    if geo == "quadrant_flexible":
        assert groups[0] != groups[-1]
    h, lv, P = hierarchies(case, 0)
    if case in (CIRCLE_5_P1, CIRCLE_5_P2):
        # the 5 -> 4 step of the sequence, 624 -> 176 cells: a step that coarsens most cells (its transfer is the last one above)
        assert [t.n_cells for t in h.trias] == [1, 8, 64, 120, 176, 624] and h.trias[-2].n_cells < 0.3 * h.trias[-1].n_cells
    if case == CIRCLE_7_P1:
        assert [t.n_cells for t in h.trias][-3:] == [232, 960, 2976]
    # separate transfer kernels
    monkeypatch.setenv("MGAMD_NO_FUSED_TRANSFER", "1")
    g, loc = refs(L)
    h0 = mgamd.Hierarchy(ctx, geo, g, p, mg_type, n_ref_local=loc, coarse_solver="amg", max_brick=0)
    monkeypatch.delenv("MGAMD_NO_FUSED_TRANSFER")
    assert sum(t.n_fused_bricks() for t in h0.transfers[1:]) == 0
    assert all(np.array_equal(a.keys(), b.keys()) for a, b in zip(h.dofs, h0.dofs))
    et = check_transfers(h0, lv, P, f"{case_id(case)} max_brick=0 separate transfer kernels")
    print(f"{case_id(case)} separate transfer kernels WORST: transfer {et:.2e}")


def test_operator_at_degree_four_on_quadrant_flexible(mgamd, oracle, ctx):
    """quadrant_flexible (3, 1) p = 4, 67,717 DoFs: the oracle's hierarchy and solve need 17 - 36 s there (the transfer to the mesh
    below alone 25 s), its finest level alone is assembled here: operator and inverse diagonal under both slot policies (4^3 bricks
    of the seven unrefined octants, the refined octant's cells next to them)"""
    geo, (g, loc), p = "quadrant_flexible", (3, 1), 4
    t = mgamd.Triangulation(geo, g, loc)
    d0, d1 = mgamd.DoFs(t, p, 0), mgamd.DoFs(t, p, -1)
    assert max(B for B, n in d0.groups() if n) * p + 1 == 17  # 17-point lattice bricks
    lv0 = oracle.Level(oracle.create_mesh(geo, g, loc), p, numbering_keys=d0.keys())
    assert lv0.n == 67717
    lv1 = renumber([lv0], [None], [d1])[0][0]
    for d, lv, mb in ((d0, lv0, 0), (d1, lv1, -1)):
        check_level(mgamd.Operator(ctx, d), lv, f"quadrant_flexible-3+1-4 max_brick={mb} finest level")


# ------------------------------------------------------------------ V-cycle and CG
@pytest.mark.parametrize("max_brick", POLICIES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_vcycle_and_cg(mgamd, oracle, ctx, hierarchies, oracle_solves, case, max_brick):
    h, lv, P = hierarchies(case, max_brick)
    mg, xref, itref, hist = oracle_solves(case, max_brick)
    assert h.mg.coarse_solver_used() == "direct"
    for l, s in enumerate(h.smoothers):
        assert s.eigenvalue_estimates()[1] == pytest.approx(mg.sm[l].max_ev, rel=1e-9)
    Lf, n = lv[-1], lv[-1].n
    r = np.random.default_rng(42).standard_normal(n)
    r[Lf.constrained] = 0.0
    vr, vz = mgamd.Vector(ctx, n).from_host(r), mgamd.Vector(ctx, n).from_host(np.full(n, np.nan))
    h.mg.vmult(vz, vr)
    z, zref = vz.to_host(), mg.vcycle(r)
    ez = rel_err(z, zref)
    assert np.array_equal(vr.to_host(), r)
    u = np.random.default_rng(43).standard_normal(n)
    u[Lf.constrained] = 0.0
    vu, vw = mgamd.Vector(ctx, n).from_host(u), mgamd.Vector(ctx, n)
    h.mg.vmult(vw, vu)
    sym = abs(u @ z - r @ vw.to_host()) / abs(u @ z)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    ex = rel_err(x.to_host(), xref)
    print(f"{case_id(case)} max_brick={max_brick} WORST: V-cycle {ez:.2e}, u.Mr - r.Mu {sym:.2e}, CG iterations {it} (oracle {itref}), "
          f"iterate {ex:.2e}")
    assert ez < TOL_VCYCLE
    assert sym < 1e-10  # a symmetric preconditioner
    assert it == itref and res == pytest.approx(hist[-1], rel=1e-6) and ex < TOL_SOL
    # graph replay gives the same vector
    assert h.mg.time_vcycles(vz, vr, 2, True) > 0 and rel_err(vz.to_host(), zref) < TOL_VCYCLE


# ------------------------------------------------------------------ Chebyshev
@pytest.mark.parametrize("degree", [1, 3])
@pytest.mark.parametrize("level", [-1, -2], ids=["finest", "intermediate"])
@pytest.mark.parametrize("max_brick", POLICIES)
@pytest.mark.parametrize("case", [CIRCLE_5_P2, CIRCLE_6_P1], ids=case_id)
def test_chebyshev(mgamd, oracle, ctx, hierarchies, case, max_brick, level, degree):
    """vmult from a zero start and step (test_gpu_high_degree.py::test_chebyshev) on the finest mesh and on the one below it, which on
    circle is the centre's three hanging-node shells in a background of level-2 cells"""
    h, levels, P = hierarchies(case, max_brick)
    op, lv = h.operators[level], levels[level]
    assert h.dofs[level].info.n_hanging > 0
    ch = mgamd.PreconditionChebyshev(op, degree, 20.0, 20)
    ref = oracle.Chebyshev(lv.A, lv.inv_diag, degree, 20.0, 20)
    assert ch.eigenvalue_estimates()[1] == pytest.approx(ref.max_ev, rel=1e-9)
    rng = np.random.default_rng(5)
    b, x0 = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
    vb, vx = op.initialize_dof_vector().from_host(b), op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
    ch.vmult(vx, vb)
    e1 = rel_err(vx.to_host(), ref.vmult(b))
    vx.from_host(x0)
    ch.step(vx, vb)
    e2 = rel_err(vx.to_host(), ref.step(x0, b))
    print(f"chebyshev {case_id(case)} max_brick={max_brick} level {level} ({lv.n} DoFs) degree={degree}: vmult {e1:.2e} step {e2:.2e}")
    assert e1 < TOL_CHEB and e2 < TOL_CHEB


# ------------------------------------------------------------------ FP32 levels under the FP64 outer CG
@pytest.mark.parametrize("case", [CIRCLE_5_P2, CIRCLE_4_P4_PMG], ids=case_id)
def test_float_levels(mgamd, oracle, emu, ctx, hierarchies, oracle_solves, case):
    """MGNumberType float: single kernels at the project's FP32 bound, the cycle within 16 e_ref of the FP64 oracle carrying the
    product's eigenvalue estimates (e_ref: the distance of the float32 emulation from it) and within 5e-5, the CG count of the
    emulated cycle: the bounds of test_gpu_float_levels.py"""
    geo, L, p, mg_type = case
    h64, lv, P = hierarchies(case, 0)
    mg, xref, it64, _ = oracle_solves(case, 0)
    h = mgamd.Hierarchy(ctx, geo, L, p, mg_type, coarse_solver="amg", number_type=mgamd.F32, max_brick=0)
    assert all(np.array_equal(a.keys(), b.keys()) for a, b in zip(h.dofs, h64.dofs))  # numbered like the FP64 tables
    rng = np.random.default_rng(3)
    for l, op in enumerate(h.operators):
        x = round32(rng.standard_normal(lv[l].n))
        src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector()
        op.vmult(dst, src)
        diag = op.initialize_dof_vector()
        op.compute_inverse_diagonal(diag)
        ev, ed = rel_err(dst.to_host(), lv[l].A @ x), rel_err(diag.to_host(), lv[l].inv_diag)
        print(f"FP32 {case_id(case)} level {l}: vmult {ev:.2e} inverse diagonal {ed:.2e}")
        assert ev < TOL_OP_F32 and ed < TOL_OP_F32
    check_transfers(h, lv, P, f"FP32 {case_id(case)}", TOL_OP_F32, rounded=True)
    n = lv[-1].n
    r = np.random.default_rng(7).standard_normal(n)
    mgp, ref, e_ref = float_cycle_reference(emu, mg, [s.eigenvalue_estimates()[1] for s in h.smoothers], r)
    vr, vz = mgamd.Vector(ctx, n).from_host(r), mgamd.Vector(ctx, n).from_host(np.full(n, np.nan))
    h.mg.vmult(vz, vr)  # double in, float V-cycle, double out
    z = vz.to_host()
    assert np.isfinite(z).all() and np.array_equal(vr.to_host(), r)
    err = rel_err(z, ref)
    print(f"FP32 V-cycle {case_id(case)}: rel.err {err:.2e}, e_ref {e_ref:.2e}, ratio {err / e_ref:.2f}")
    assert err <= MARGIN_F32 * e_ref
    assert rel_err(z, mg.vcycle(r)) < CAP_F32
    Lf = lv[-1]
    x32, it32, _ = oracle.pcg(Lf.A, Lf.rhs_constant, lambda v: emu.vcycle(mg, v, np.float32).astype(np.float64), 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    ex = rel_err(x.to_host(), xref)
    print(f"FP32 CG {case_id(case)}: iterations gpu {it}, float32 emulation {it32}, FP64 oracle {it64}, rel.err {ex:.2e}")
    assert it == it32
    assert ex < 1e-3


# ------------------------------------------------------------------ simulated ranks
@pytest.fixture(scope="module")
def sharded_references(oracle, hierarchies):
    """the oracle's levels, cycle and solve with the numbering-independent start vectors of the sharded path, once per case"""
    cache = {}

    def get(case):
        if case not in cache:
            geo, L, p, mg_type = case
            levels, P = hierarchies(case, 0)[1:] if case in CASES else oracle.build_hierarchy(geo, L, p, mg_type)
            omg = oracle.Multigrid(levels, P, 3, coarse="direct", start_vectors=[oracle.key_hash_start_vector(lv) for lv in levels])
            Lf = levels[-1]
            u, r = key_vector(Lf.keys, 1), key_vector(Lf.keys, 2)
            r[Lf.constrained] = 0.0
            cache[case] = dict(levels=levels, kf={k: i for i, k in enumerate(keyset(Lf.keys))}, u=u, r=r, Au=Lf.A @ u, z=omg.vcycle(r),
                               solve=oracle.pcg(Lf.A, Lf.rhs_constant, omg.vcycle, 1e-4))
        return cache[case]

    return get


def sharded_run(mgamd, ref, case, n_ranks, **kw):
    geo, L, p, mg_type = case
    group = mgamd.SimGroup(n_ranks)

    def rank_main(rk):
        c = mgamd.Context(0)
        h = mgamd.DistributedHierarchy(c, group.comm(rk), geo, L, p, coarse_solver="amg", max_brick=0, mg_type=mg_type, **kw)
        idx = np.array([ref["kf"][k] for k in keyset(h.dofs[-1].keys())])
        op = h.fine_operator
        vu, vA = op.initialize_dof_vector().from_host(ref["u"][idx]), op.initialize_dof_vector()
        op.vmult(vA, vu)
        vr, vz = op.initialize_dof_vector().from_host(ref["r"][idx]), op.initialize_dof_vector()
        h.mg.vmult(vz, vr)
        b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
        op.rhs(b)
        it, res = mgamd.solve_cg(op, h.mg, x, b, 1e-4)
        return dict(idx=idx, Au=vA.to_host(), z=vz.to_host(), x=x.to_host(), b=b.to_host(), it=it, n_dofs=h.n_dofs, dist=list(h.distributed),
                    used=h.mg.coarse_solver_used(), peers=h.dofs[-1].info.n_peers, layout=h.layout(), level_dofs=h.global_level_dofs(c),
                    group=h.partition.group)

    out = run_ranks(n_ranks, rank_main)
    Lf = ref["levels"][-1]
    xref, itref, _ = ref["solve"]
    for rk, o in enumerate(out):
        eA, ez, ex = rel_err(o["Au"], ref["Au"][o["idx"]]), rel_err(o["z"], ref["z"][o["idx"]]), rel_err(o["x"], xref[o["idx"]])
        print(f"{case_id(case)} rank {rk} of {n_ranks}: layout {o['layout']}, {len(o['idx'])} local DoFs, {o['peers']} peers, operator {eA:.2e}, "
              f"V-cycle {ez:.2e}, CG iterations {o['it']} (oracle {itref}), iterate {ex:.2e}")
        assert o["n_dofs"] == Lf.n and o["peers"] >= 1 and o["dist"][-1] and o["used"] == "direct"
        assert o["level_dofs"] == [lv.n for lv in ref["levels"]]  # every DoF of every level owned exactly once
        assert eA < TOL_OP and np.abs(o["b"] - Lf.rhs_constant[o["idx"]]).max() < 1e-14
        assert ez < TOL_VCYCLE and o["it"] == itref and ex < TOL_SOL
    # copies of shared DoFs agree across ranks (bitwise: ascending-rank combination order)
    seen = {}
    for o in out:
        for i, v in zip(o["idx"], o["x"]):
            if i in seen:
                assert seen[i] == v
            seen[i] = v
    assert len(seen) == Lf.n
    return out


@pytest.mark.parametrize("case,n_ranks", [(("circle", 6, 2, "HMG-global"), 3), (("circle", 6, 2, "HMG-global"), 4), (CIRCLE_5_P1, 4)], ids=case_id)
def test_simulated_ranks(mgamd, sharded_references, monkeypatch, case, n_ranks):
    """n ranks as host threads over the in-process communicator (test_gpu_distributed_sim.py), min_root_dofs = 0: the fine level's
    weight sits in the small central region that the space-filling-curve cut has to split.  Operator, V-cycle, solve and iteration
    count against the numpy oracle"""
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")  # the sharded path's start vector hashes the DoF key; the oracle takes the same
    out = sharded_run(mgamd, sharded_references(case), case, n_ranks, min_root_dofs=0)
    # a level is cut only from 32 cells per piece: the 1-, 8- and 64-cell meshes stay replicated, the meshes above them are cut
    assert all(o["layout"] == out[0]["layout"] and o["layout"][0] == 1 and o["layout"][-1] == n_ranks for o in out)
    assert out[0]["layout"].count(n_ranks) >= 2


def test_two_tier_simulated_ranks(mgamd, sharded_references, monkeypatch):
    """circle 7 p = 1 on 4 ranks in groups of 2, the thresholds chosen by size as in test_two_tier_hierarchy_matches_numpy_oracle: the two
    finest meshes (2976, 960 cells) on all ranks, the two below them (232, 176) on the two parts, the rest replicated: all three tiers"""
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")
    case, n_ranks, group = CIRCLE_7_P1, 4, 2
    seq = mgamd.create_geometric_coarsening_sequence(mgamd.Triangulation(case[0], case[1]))
    n_cells = [t.n_cells for t in seq]
    out = sharded_run(mgamd, sharded_references(case), case, n_ranks, subset_group=group, min_root_dofs=n_cells[-2], min_subset_dofs=n_cells[-4])
    for o in out:
        assert o["group"] == group and n_ranks // group in o["layout"] and o["layout"][0] == 1 and o["layout"][-1] == n_ranks
        assert o["layout"] == [1, 1, 1, 1, 2, 2, 4, 4]


# ------------------------------------------------------------------ physics on the circle
def test_coefficient_mass_term_and_robin_face(mgamd, oracle, emu, ctx):
    """circle 5 p = 2 HMG-global with a = 50 on the leaves whose centre lies within 0.3 of the origin (112 of the 120 refined leaves:
    the inclusion sits inside the refined region, and the coarse coefficients are means across the hanging-node shells), sigma = 7.5,
    Dirichlet on face 0 only, a convective face 1 with beta = 2, the rest natural: operator and inverse diagonal on every level,
    V-cycle, CG count and solution at the bounds of test_gpu_robin.py::test_random_octree"""
    case, sigma, setup = CIRCLE_5_P2, 7.5, (0b000001, (0.0, 2.0, 0.0, 0.0, 0.0, 0.0))
    geo, L, p, mg_type = case
    inside = lambda x, y, z: np.sqrt(x * x + y * y + z * z) <= 0.3  # noqa: E731
    h = mgamd.Hierarchy(ctx, geo, L, p, mg_type, coarse_solver="amg", max_brick=0, mass_coefficient=sigma, dirichlet_faces=setup[0],
                        robin=setup[1], coefficient=lambda x, y, z: np.where(inside(x, y, z), 50.0, 1.0))
    assert all(np.array_equal(t.robin_coefficients(), setup[1]) and t.dirichlet_faces() == setup[0] for t in h.trias)
    meshes, degs = po.level_plan(geo, L, p, mg_type)
    finest = po.field_on(meshes[-1], lambda c: 50.0 if inside(*po._centre(c)) else 1.0)
    refined = {c for c in meshes[-1] if c[0] > 3}
    assert {c for c, a in finest.items() if a == 50.0} < refined and (sum(a == 50.0 for a in finest.values()), len(refined)) == (112, 120)
    coeffs = [finest if len(m) == len(finest) else po.restrict_field(finest, m) for m in meshes]
    for t, c in zip(h.trias, coeffs):
        want = po.product_values(t, c)
        assert np.abs(t.coefficient() - want).max() <= 1e-14 * 50.0
    assert any(1.0 < a < 50.0 for c in coeffs[:-1] for a in c.values())  # coarse cells across the inclusion's rim
    levels, P = su.oracle_hierarchy_on(h.dofs, meshes, degs, Problem(sigma, finest, *setup))
    assert all(lv.coefficient == c for lv, c in zip(levels, coeffs))
    for l, (op, lv) in enumerate(zip(h.operators, levels)):
        x = np.random.default_rng(3).standard_normal(lv.n)
        diag = op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
        op.compute_inverse_diagonal(diag)
        ev, ed = rel_err(su.apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x), rel_err(diag.to_host(), lv.inv_diag)
        print(f"circle 5 p=2 a=50|1 sigma={sigma} mask={setup[0]:#04x} beta={setup[1]} level {l}: vmult {ev:.2e} inverse diagonal {ed:.2e}")
        assert ev < TOL_OP and ed < TOL_OP
    su.vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"circle 5 p=2 a=50|1 sigma={sigma} mask={setup[0]:#04x} beta={setup[1]}")


# ------------------------------------------------------------------ harness
def test_harness_circle_and_default_geometry(oracle, hierarchies, oracle_solves, tmp_path):
    """the JSON-driven harness binary on GeometryType circle, and without a GeometryType key (the default, quadrant_flexible) with
    NRefLocal 2: mesh, DoF and CG iteration columns of the oracle (double levels; written like test_harness_degree_six)"""
    base = json.load(open(os.path.join(GOLDEN, "input_0003.json")))
    base = dict(base, Type="HMG-global", Degree=2, MGNumberType="double", Verbosity=False)
    cfgs = [dict(base, GeometryType="circle", NRefGlobal=5, NRefLocal=0), dict(base, NRefGlobal=2, NRefLocal=2)]
    del cfgs[1]["GeometryType"]
    files = []
    for i, cfg in enumerate(cfgs):
        files.append(str(tmp_path / f"geometry{i}.json"))
        json.dump(cfg, open(files[-1], "w"))
    rc, out, err = run_harness(*files)
    assert rc == 0, err
    _, rows = final_table(out)
    assert len(rows) == 2
    for row, case in zip(rows, (CIRCLE_5_P2, FLEXIBLE_22_P2)):
        geo, L, p, mg_type = case
        g, loc = refs(L)
        mesh = oracle.create_mesh(geo, g, loc)
        lv = hierarchies(case, -1)[1]
        itref = oracle_solves(case, -1)[2]
        print(f"harness {case_id(case)}: n_cells {row['n_cells']} n_cells_hn {row['n_cells_hn']} n_dofs {row['n_dofs']} n_ref_local "
              f"{row['n_ref_local']} n_levels {row['n_levels']} n_iterations {row['n_iterations']} (oracle {itref})")
        assert int(row["n_cells"]) == len(mesh) and int(row["n_cells_hn"]) == sum(oracle.is_cell_constrained(mesh, c) for c in mesh)
        assert (int(row["degree"]), int(row["n_ref_global"]), int(row["n_ref_local"])) == (p, g, loc)
        assert int(row["n_dofs"]) == lv[-1].n and int(row["n_levels"]) == len(lv)
        assert int(row["n_iterations"]) == itref and row["coarse_solver"] == "direct"
