"""The piecewise-constant diffusion coefficient on the GPU: operators, smoothers, multigrid, CG, AMG and the time stepper for
A = K_a + sigma M (-div(a grad u) + sigma u, a constant on every leaf) against the numpy oracle oracle/physics_oracle.py (sum
a_c h_c Kc in place of the stiffness matrix).

Fields (physics_oracle.FIELDS): uniform 3.5 (the slot structure of the mesh without a coefficient: every kernel family with
a != 1), octants (1 + 0.75 octant index: jumps on the planes through 0, bricks survive inside the octants), inclusion (1000 in
[-0.5, 0]^3: high contrast), per_cell (no two neighbours agree: single-cell slots only, hundreds of distinct diagonals).
sigma in {0, 7.5}: the Laplace kernels, which only see the scale a h, and the kernels of the mass term, which also need h^2 / a.

Bounds are those of test_gpu_helmholtz.py: operator <= 1e-13, Chebyshev <= 1e-12, V-cycle <= 1e-11, CG iterates <= 1e-10 with equal
iteration counts, FP32 single kernels <= 2e-6, FP32 V-cycle <= 16 e_ref with e_ref from oracle/f32_emulation.py on the test's own
levels plus the 5e-5 cap.  Every constraint search is made once per session (support.py).  The coarse
coefficients of every hierarchy are checked against the oracle's own restatement before they are used."""
import threading

import numpy as np
import pytest

import physics_oracle as po
import support as su
import time_stepping_oracle as ts
from conftest import rel_err
from physics_oracle import Problem
from support import OP_CASES, TOL_CHEB, TOL_CYCLE, TOL_F32, TOL_OP, TOL_SOL, apply_nan, assert_level_coefficients, emu  # noqa: F401

pytestmark = pytest.mark.gpu

SIGMAS = [0.0, 7.5]


def bricks_with_a_coefficient(d, t):
    """slots of B >= 2 whose cells carry a != 1, as (B, a)"""
    grp, _ = d.cell_slots()
    B, a = list(d.info.group_B), t.coefficient()
    return {(B[g], a[c]) for c, g in enumerate(grp) if B[g] >= 2 and a[c] != 1.0}


# ------------------------------------------------------------------ 1. operator and inverse diagonal
def plain_bricks_where_a_is_not_one(plain, t):
    """does a brick (B >= 2) of the mesh WITHOUT a coefficient hold a family (the eight children of one cell) that carries ONE
    value a != 1 of the field on t?  Then the tables built with the field keep at least that family as a brick with a != 1.
    Computed from the tables, so a change in brick formation cannot make the assertion below vacuous."""
    grp, _ = plain.cell_slots()
    B, a = list(plain.info.group_B), t.coefficient()
    lev, i, j, k, _ = t.cells()
    fam = {}
    for c in range(len(grp)):
        if B[int(grp[c])] >= 2:
            fam.setdefault((int(lev[c]), int(i[c]) >> 1, int(j[c]) >> 1, int(k[c]) >> 1), []).append(a[c])
    return any(len(v) == 8 and len(set(v)) == 1 and v[0] != 1.0 for v in fam.values())


@pytest.mark.parametrize("name", ["uniform", "octants"])
@pytest.mark.parametrize("geo,L,p,max_brick", OP_CASES)
def test_vmult_and_inverse_diagonal(mgamd, oracle, ctx, geo, L, p, max_brick, name):
    t = su.tria(mgamd, geo, L, Problem(coefficient=name))
    d = mgamd.DoFs(t, p, max_brick)
    plain = mgamd.DoFs(mgamd.Triangulation(geo, L), p, max_brick)
    if plain_bricks_where_a_is_not_one(plain, t):
        assert bricks_with_a_coefficient(d, t)  # a brick kernel cannot pass vacuously
    rng = np.random.default_rng(3)
    for sigma in SIGMAS:
        d.set_mass_coefficient(sigma)
        op = mgamd.Operator(ctx, d)
        lv = su.oracle_level(d, geo, L, p, Problem(sigma, name))
        for trial in range(2):  # twice: a dirty tail accumulator shows in the second pass
            x = rng.standard_normal(lv.n)
            err = rel_err(apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x)
            print(f"vmult {geo} L={L} p={p} max_brick={max_brick} {name} sigma={sigma}: rel.err {err:.2e}")
            assert err < TOL_OP
        diag = op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
        op.compute_inverse_diagonal(diag)
        err = rel_err(diag.to_host(), lv.inv_diag)
        print(f"inverse diagonal {geo} L={L} p={p} max_brick={max_brick} {name} sigma={sigma}: rel.err {err:.2e}")
        assert err < TOL_OP
    # the operator keeps the coefficient it was built with
    t.set_coefficient(None)
    assert rel_err(apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x) < TOL_OP


# ------------------------------------------------------------------ 2. a different value in every cell
@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 1), ("quadrant", 3, 2), ("quadrant", 3, 4), ("quadrant", 2, 7)])
def test_per_cell_field(mgamd, oracle, ctx, geo, L, p):
    """every brick is split: single-cell slots only.  p = 4: thousands of tail DoFs with hundreds of distinct diagonals, so the
    one-byte D^-1 codes of the tail and their overflow code 255 run"""
    t = su.tria(mgamd, geo, L, Problem(coefficient="per_cell"))
    d = mgamd.DoFs(t, p, 0)
    assert all(list(d.info.group_B)[int(g)] == 1 for g in set(d.cell_slots()[0].tolist()))
    if p == 4:
        assert d.n_dofs - d.info.n_interior >= 4096
    rng = np.random.default_rng(9)
    for sigma in SIGMAS:
        d.set_mass_coefficient(sigma)
        op = mgamd.Operator(ctx, d)
        lv = su.oracle_level(d, geo, L, p, Problem(sigma, "per_cell"))
        x = rng.standard_normal(lv.n)
        ev = rel_err(apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x)
        diag = op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
        op.compute_inverse_diagonal(diag)
        ed = rel_err(diag.to_host(), lv.inv_diag)
        ch = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
        ref = oracle.Chebyshev(lv.A, lv.inv_diag, 3, 20.0, 20)
        assert ch.eigenvalue_estimates()[1] == pytest.approx(ref.max_ev, rel=1e-10)
        b = rng.standard_normal(lv.n)
        ec = rel_err(apply_nan(mgamd, ctx, ch.vmult, b), ref.vmult(b))
        n_distinct = len(np.unique(lv.inv_diag[d.info.n_interior:d.info.n_interior + d.info.n_tail]))
        print(f"per-cell {geo} L={L} p={p} sigma={sigma}: vmult {ev:.2e}, inverse diagonal {ed:.2e}, Chebyshev {ec:.2e}; "
              f"{n_distinct} distinct D^-1 values on {d.info.n_tail} tail DoFs")
        assert ev < TOL_OP and ed < TOL_OP and ec < TOL_CHEB
        if p == 4:
            assert n_distinct > 255


# ------------------------------------------------------------------ 3., 4. what must not change
def compare_by_the_bitwise_rule(d, pairs):
    """test_sigma_zero_is_bitwise_the_laplace_path's rule: bit for bit on the DoFs whose value does not depend on the order of
    floating-point atomics (slot-interior, constrained, shell DoFs of at most two slots), 1e-14 on the rest and on a V-cycle"""
    cnt = su.atomic_contributions(d)
    det = cnt <= 2
    assert det.sum() > 0.5 * d.n_dofs
    for name, a, b in pairs:
        print(f"{name}: max |difference| {np.abs(a - b).max():.2e}, on the {int(det.sum())} order-independent DoFs {np.abs(a[det] - b[det]).max():.2e}")
        if name != "V-cycle":
            assert np.array_equal(a[det], b[det]), name
        assert rel_err(a, b) < 1e-14, name


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 4), ("hypercube", 3, 4), ("quadrant", 4, 1), ("hypercube", 3, 2)])
@pytest.mark.parametrize("name", ["uniform", "octants"])
def test_mass_operator_does_not_see_the_coefficient(mgamd, ctx, geo, L, p, name):
    """vmult_mass under a coefficient is vmult_mass without one (M does not depend on a).  Where the coefficient leaves the slots
    as they are the two run the same kernels on the same tables: the bitwise rule.  Where it splits bricks (octants on a mesh whose
    bricks straddle the planes through 0) the numbering differs: matched by the DoF keys, 1e-14."""
    t = su.tria(mgamd, geo, L, Problem(coefficient=name))
    d, d0 = mgamd.DoFs(t, p, 0), mgamd.DoFs(mgamd.Triangulation(geo, L), p, 0)
    d.set_mass_coefficient(7.5)
    d0.set_mass_coefficient(7.5)
    op, op0 = mgamd.Operator(ctx, d), mgamd.Operator(ctx, d0)
    x0 = np.random.default_rng(19).standard_normal(d0.n_dofs)
    same = all(np.array_equal(u, v) for u, v in zip(d.cell_slots(), d0.cell_slots()))
    assert same == (name == "uniform" or (geo, L, p) != ("hypercube", 3, 2))  # octants split the one 8^3 brick of hypercube L=3 p=2
    if same:
        assert np.array_equal(d.keys(), d0.keys())
        for trial in range(2):
            compare_by_the_bitwise_rule(d, [(f"vmult_mass {geo} p={p} {name}", apply_nan(mgamd, ctx, op.vmult_mass, x0),
                                             apply_nan(mgamd, ctx, op0.vmult_mass, x0))])
            apply_nan(mgamd, ctx, op.vmult, x0)  # an operator pass in between: the two scales of a slot do not get mixed up
    else:
        k0 = {tuple(int(v) for v in k): i for i, k in enumerate(d0.keys())}
        idx = np.array([k0[tuple(int(v) for v in k)] for k in d.keys()])
        assert rel_err(apply_nan(mgamd, ctx, op.vmult_mass, x0[idx]), apply_nan(mgamd, ctx, op0.vmult_mass, x0)[idx]) < 1e-14


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 4), ("hypercube", 3, 4), ("quadrant", 4, 1)])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_ones_are_no_coefficient(mgamd, ctx, geo, L, p, sigma):
    """set_coefficient(ones) against no coefficient set: the same tables and the same scales bit for bit, hence the same results
    under the bitwise rule"""
    t = mgamd.Triangulation(geo, L)
    t.set_coefficient(np.ones(t.n_cells))
    assert t.has_coefficient()
    ha = mgamd.Hierarchy(ctx, t, L, p, "HMG-global", coarse_solver="amg", max_brick=0, mass_coefficient=sigma)
    hb = mgamd.Hierarchy(ctx, geo, L, p, "HMG-global", coarse_solver="amg", max_brick=0, mass_coefficient=sigma)
    assert all(m.has_coefficient() for m in ha.trias) and not any(m.has_coefficient() for m in hb.trias)
    d = ha.dofs[-1]
    assert np.array_equal(d.keys(), hb.dofs[-1].keys())
    x = np.random.default_rng(13).standard_normal(ha.n_dofs)
    res = []
    for h in (ha, hb):
        op = h.operators[-1]
        diag = op.initialize_dof_vector()
        op.compute_inverse_diagonal(diag)
        res.append((apply_nan(mgamd, ctx, op.vmult, x), diag.to_host(), apply_nan(mgamd, ctx, op.vmult_mass, x),
                    apply_nan(mgamd, ctx, h.mg.vmult, x)))
    compare_by_the_bitwise_rule(d, list(zip(("vmult", "inverse diagonal", "vmult_mass", "V-cycle"), res[0], res[1])))


# ------------------------------------------------------------------ 5. Chebyshev
@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 1), ("quadrant", 3, 2), ("quadrant", 3, 4), ("quadrant", 2, 5)])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_chebyshev(mgamd, oracle, ctx, geo, L, p, sigma):
    d = mgamd.DoFs(su.tria(mgamd, geo, L, Problem(coefficient="octants")), p, 0)
    d.set_mass_coefficient(sigma)
    op = mgamd.Operator(ctx, d)
    lv = su.oracle_level(d, geo, L, p, Problem(sigma, "octants"))
    ch = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
    ref = oracle.Chebyshev(lv.A, lv.inv_diag, 3, 20.0, 20)
    assert ch.eigenvalue_estimates()[1] == pytest.approx(ref.max_ev, rel=1e-10)
    rng = np.random.default_rng(5)
    b, x0 = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
    ev = rel_err(apply_nan(mgamd, ctx, ch.vmult, b), ref.vmult(b))
    vb, vx = op.initialize_dof_vector().from_host(b), op.initialize_dof_vector().from_host(x0)
    ch.step(vx, vb)
    es = rel_err(vx.to_host(), ref.step(x0, b))
    print(f"chebyshev {geo} L={L} p={p} octants sigma={sigma}: vmult {ev:.2e} step {es:.2e}")
    assert ev < TOL_CHEB and es < TOL_CHEB


# ------------------------------------------------------------------ 6. V-cycle and CG
@pytest.mark.parametrize("case", [("quadrant", 3, 4, "HMG-global"), ("quadrant", 3, 4, "PMG"), ("hypercube", 4, 2, "HMG-global"),
                                  ("quadrant", 4, 1, "HPMG")], ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("name", ["octants", "inclusion"])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_vcycle_and_cg(mgamd, oracle, emu, ctx, case, name, sigma):
    h = su.hierarchy(mgamd, ctx, case, Problem(sigma, name), max_brick=0)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma, name))
    assert_level_coefficients(h, levels)
    su.vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{case} {name} sigma={sigma}")


# ------------------------------------------------------------------ 7. fused transfers
@pytest.mark.parametrize("sigma", SIGMAS)
def test_fused_transfers(mgamd, oracle, emu, ctx, sigma, monkeypatch):
    """hypercube L=3 p=4, octants: eight 17^3 bricks with eight coefficient values restrict and prolongate inside the operator
    passes (MODE_RESIDUAL_RESTRICT, MODE_CHEB_PROLONGATE); equal to the separate transfer kernels and to the oracle"""
    case = ("hypercube", 3, 4, "HMG-global")
    h = su.hierarchy(mgamd, ctx, case, Problem(sigma, "octants"), max_brick=0)
    assert sum(t.n_fused_bricks() for t in h.transfers[1:]) > 0
    assert len(bricks_with_a_coefficient(h.dofs[-1], h.trias[-1])) >= 4
    monkeypatch.setenv("MGAMD_NO_FUSED_TRANSFER", "1")
    h0 = su.hierarchy(mgamd, ctx, case, Problem(sigma, "octants"), max_brick=0)
    monkeypatch.delenv("MGAMD_NO_FUSED_TRANSFER")
    assert sum(t.n_fused_bricks() for t in h0.transfers[1:]) == 0
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma, "octants"))
    assert_level_coefficients(h, levels)
    su.vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{case} octants sigma={sigma} fused")
    r = np.random.default_rng(11).standard_normal(levels[-1].n)
    z, z0 = apply_nan(mgamd, ctx, h.mg.vmult, r), apply_nan(mgamd, ctx, h0.mg.vmult, r)
    assert rel_err(z, z0) < 1e-13
    z1 = apply_nan(mgamd, ctx, h.mg.vmult, r)
    assert np.array_equal(z1, z) or rel_err(z1, z) < 1e-14  # (atomic summation order)


# ------------------------------------------------------------------ 8. collapsed coarse levels
@pytest.mark.parametrize("sigma", SIGMAS)
def test_collapsed_coarse_levels(mgamd, oracle, emu, ctx, sigma, monkeypatch):
    """quadrant L=4 p=1: the levels up to 2048 DoFs as one tabulated matrix, formed through the operators with their coefficient"""
    case = ("quadrant", 4, 1, "HMG-global")
    ha = su.hierarchy(mgamd, ctx, case, Problem(sigma, "octants"))
    monkeypatch.setenv("MGAMD_COLLAPSE_MAX_DOFS", "0")
    hb = su.hierarchy(mgamd, ctx, case, Problem(sigma, "octants"))
    monkeypatch.delenv("MGAMD_COLLAPSE_MAX_DOFS")
    assert ha.mg.set_collapse(True) > 0 and hb.mg.set_collapse(True) == 0
    for h, tag in ((ha, "collapsed"), (hb, "kernel by kernel")):
        levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma, "octants"))
        su.vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{case} octants sigma={sigma} {tag}")


# ------------------------------------------------------------------ 9., 10. AMG
@pytest.mark.parametrize("sigma", SIGMAS)
def test_assembled_matrix_amg_and_cg(mgamd, oracle, ctx, sigma):
    """SparseMatrix + PreconditionAMG + solve_cg (Type "AMG") on quadrant L=3 p=2, octants"""
    import amg_oracle as ao

    geo, L, p = "quadrant", 3, 2
    h = mgamd.Hierarchy(ctx, geo, L, p, "AMG", mass_coefficient=sigma, coefficient=po.octants_xyz)
    d = h.dofs[0]
    assert d.coefficient_range() == (1.0, 6.25)
    lv = su.oracle_level(d, geo, L, p, Problem(sigma, "octants"))
    x = np.random.default_rng(4).standard_normal(lv.n)
    assert rel_err(apply_nan(mgamd, ctx, h.system_matrix.vmult, x), lv.A @ x) < TOL_OP
    o = ao.SmoothedAggregation(d.matrix())
    xref, itref, _ = oracle.pcg(lv.A, lv.rhs_constant, o.precondition(1), 1e-4)
    b, xv = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.system_matrix, h.amg, xv, b, 1e-4)
    print(f"Type AMG octants sigma={sigma}: CG iterations {it} (oracle {itref}), iterate {rel_err(xv.to_host(), xref):.2e}")
    assert it == itref and rel_err(xv.to_host(), xref) < TOL_SOL


def test_pmg_with_amg_coarse_solver(mgamd, oracle, ctx):
    """annulus L=6 p=2, PMG, coarse_solver="amg", octants, sigma = 7.5: the p = 1 level has 9763 DoFs and its coarse solver is the
    smoothed-aggregation AMG of the assembled K_a + sigma M"""
    import amg_oracle as ao

    sigma, case = 7.5, ("annulus", 6, 2, "PMG")
    h = su.hierarchy(mgamd, ctx, case, Problem(sigma, "octants"), coarse_n_cycles=2)
    assert h.mg.coarse_solver_used() == "amg"
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma, "octants"))
    A0 = ao.csr(*h.dofs[0].matrix())
    assert abs(A0 - levels[0].A).max() <= 1e-13 * abs(levels[0].A).max()
    mg = oracle.Multigrid(levels, P, 3, coarse=ao.SmoothedAggregation(h.dofs[0].matrix()).precondition(2))
    r = np.random.default_rng(2).standard_normal(h.n_dofs)
    err = rel_err(apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r))
    Lf = levels[-1]
    xref, itref, _ = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    print(f"PMG + amg octants: V-cycle {err:.2e}, CG iterations {it} (oracle {itref}), iterate {rel_err(x.to_host(), xref):.2e}")
    assert err <= TOL_CYCLE
    assert it == itref and rel_err(x.to_host(), xref) <= TOL_SOL


# ------------------------------------------------------------------ 11. Gaussian data
@pytest.mark.parametrize("sigma", SIGMAS)
def test_gaussian_simulation_type(mgamd, oracle, emu, ctx, sigma):
    """Dirichlet lifting with the unconstrained K_a + sigma M, solve, constraints.distribute"""
    case = ("quadrant", 3, 4, "HMG-global")
    h = su.hierarchy(mgamd, ctx, case, Problem(sigma, "octants"), max_brick=0)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma, "octants"))
    _, x, xref = su.vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"Gaussian {case} octants sigma={sigma}", rhs_kind=1)
    h.fine_operator.distribute(x, 1)
    assert rel_err(x.to_host(), levels[-1].distribute(xref, oracle.gaussian_solution)) < 10 * TOL_SOL


# ------------------------------------------------------------------ 12. FP32 levels
@pytest.mark.parametrize("sigma", SIGMAS)
def test_float_levels(mgamd, oracle, emu, ctx, sigma):
    case = ("quadrant", 3, 4, "HMG-global")
    h = su.hierarchy(mgamd, ctx, case, Problem(sigma, "octants"), number_type=mgamd.F32, max_brick=0)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma, "octants"))
    rng = np.random.default_rng(21)
    for l, op in enumerate(h.operators):
        lv = levels[l]
        x = rng.standard_normal(lv.n).astype(np.float32).astype(np.float64)
        src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
        op.vmult(dst, src)
        diag = op.initialize_dof_vector()
        op.compute_inverse_diagonal(diag)
        ev, ed = rel_err(dst.to_host(), lv.A @ x), rel_err(diag.to_host(), lv.inv_diag)
        print(f"FP32 level {l} octants sigma={sigma}: vmult {ev:.2e} inverse diagonal {ed:.2e}")
        assert ev < TOL_F32 and ed < TOL_F32
    mg = oracle.Multigrid(levels, P, 3, coarse="direct")
    mgp = emu.with_max_evs(mg, [s.eigenvalue_estimates()[1] for s in h.smoothers])
    Lf = levels[-1]
    r = rng.standard_normal(Lf.n)
    ref = mgp.vcycle(r)
    e_ref = rel_err(emu.vcycle(mgp, r, np.float32).astype(np.float64), ref)
    err = rel_err(apply_nan(mgamd, ctx, h.mg.vmult, r), ref)
    print(f"FP32 V-cycle octants sigma={sigma}: rel.err {err:.2e}, e_ref {e_ref:.2e}, ratio {err / e_ref:.2f}")
    assert err <= 16 * e_ref
    assert rel_err(apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r)) < 5e-5
    xref, it64, _ = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    print(f"FP32 CG octants sigma={sigma}: iterations {it}, FP64 oracle {it64}")
    assert it == it64


# ------------------------------------------------------------------ 13. two simulated ranks
def test_two_simulated_ranks(mgamd, oracle, monkeypatch):
    """quadrant L=4 p=2 HMG-global cut over two ranks: the local tables take the coefficient from the partition's meshes"""
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")  # the sharded path's start vector hashes the DoF key; the oracle takes the same
    sigma, case, n_ranks = 7.5, ("quadrant", 4, 2, "HMG-global"), 2
    levels, P = su.oracle_hierarchy(None, case, Problem(sigma, "octants"))
    omg = oracle.Multigrid(levels, P, 3, coarse="direct", start_vectors=[oracle.key_hash_start_vector(lv) for lv in levels])
    Lf = levels[-1]
    kf = {tuple(int(v) for v in k): i for i, k in enumerate(Lf.keys)}
    r = np.sin(np.arange(Lf.n) * 0.37) + 0.25
    r[Lf.constrained] = 0.0
    zref = omg.vcycle(r)
    xref, itref, _ = oracle.pcg(Lf.A, Lf.rhs_constant, omg.vcycle, 1e-4)
    group = mgamd.SimGroup(n_ranks)
    out, errs = [None] * n_ranks, [None] * n_ranks

    def rank_main(rk):
        try:
            c = mgamd.Context(0)
            h = mgamd.DistributedHierarchy(c, group.comm(rk), *case[:3], coarse_solver="amg", max_brick=0, min_root_dofs=0,
                                           mg_type=case[3], mass_coefficient=sigma, coefficient=po.octants_xyz)
            idx = np.array([kf[tuple(int(v) for v in k)] for k in h.dofs[-1].keys()])
            op = h.fine_operator
            vr, vz = op.initialize_dof_vector().from_host(r[idx]), op.initialize_dof_vector()
            h.mg.vmult(vz, vr)
            b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
            op.rhs(b)
            it, _ = mgamd.solve_cg(op, h.mg, x, b, 1e-4)
            out[rk] = dict(idx=idx, z=vz.to_host(), x=x.to_host(), it=it, dist=h.distributed[-1], rng=h.dofs[-1].coefficient_range())
        except BaseException as e:  # noqa
            errs[rk] = e

    threads = [threading.Thread(target=rank_main, args=(rk,)) for rk in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    for e in errs:
        if e is not None:
            raise e
    seen = {}
    assert max(o["rng"][1] for o in out) == 6.25 and min(o["rng"][0] for o in out) == 1.0
    for o in out:
        assert o["dist"]
        ez, ex = rel_err(o["z"], zref[o["idx"]]), rel_err(o["x"], xref[o["idx"]])
        print(f"two ranks octants: V-cycle {ez:.2e}, CG iterations {o['it']} (oracle {itref}), iterate {ex:.2e}")
        assert ez < TOL_CYCLE and o["it"] == itref and ex < TOL_SOL
        for i, v in zip(o["idx"], o["x"]):
            assert seen.setdefault(i, v) == v  # copies of shared DoFs: bitwise identical
    assert len(seen) == Lf.n


# ------------------------------------------------------------------ 14. the time stepper
def test_time_stepper_two_materials(mgamd, oracle, emu, ctx):
    """three Crank-Nicolson steps with a source on quadrant L=3 p=2, a = 1000 in the inclusion: TimeStepper is unchanged and
    works on the hierarchy; equal CG counts in every step"""
    case, theta, dt, n_steps, reltol = ("quadrant", 3, 2, "HMG-global"), 0.5, 0.02, 3, 1e-6
    sigma = mgamd.TimeStepper.mass_coefficient(theta, dt)
    h = su.hierarchy(mgamd, ctx, case, Problem(sigma, "inclusion"), max_brick=0)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma, "inclusion"))
    assert_level_coefficients(h, levels)
    assert h.dofs[-1].coefficient_range() == (1.0, 1000.0)
    lv = levels[-1]
    u0 = np.random.default_rng(17).standard_normal(lv.n)
    u0[lv.constrained] = 0.0
    f0 = np.sin(0.37 * np.arange(lv.n)) + 0.25
    f = lambda n: (1.0 + n * dt) * f0  # noqa: E731
    op = h.fine_operator
    vec = lambda x: op.initialize_dof_vector().from_host(x)  # noqa: E731
    stepper = mgamd.TimeStepper(op, h.mg, theta, dt)
    u, its = vec(u0), []
    for n in range(n_steps):
        its.append(stepper.step(u, vec(f(n)), vec(f(n + 1)), reltol=reltol)[0])
    Mh, solve = ts.mass_matrix(lv), ts.pcg_solver(oracle, lv, su.injected(emu, oracle, levels, P, h).vcycle, reltol)
    uref, itref = u0.copy(), []
    for n in range(n_steps):
        uref, it = ts.theta_step(lv, uref, f(n), f(n + 1), theta, dt, solve, Mh)
        itref.append(it)
    err = rel_err(u.to_host(), uref)
    print(f"time stepper inclusion: CG iterations {its} (oracle {itref}), iterate {err:.2e}")
    assert its == itref
    assert err <= 3e-10


def test_example_program_with_two_materials(oracle):
    """bin/heat_equation 1000 (examples/heat_equation.cpp through the C++ classes: Triangulation::set_coefficient, has_coefficient,
    coefficient, DoFHandler::coefficient_range): hypercube L=3 p=2, a = 1000 in the inclusion, five Crank-Nicolson steps from
    u = 1 at reltol 1e-10; the printed norms are the oracle stepper's"""
    import os
    import re
    import subprocess

    from conftest import ROOT

    exe = os.path.join(ROOT, "bin", "heat_equation")
    assert os.path.exists(exe), "bin/heat_equation is missing: make all"
    run = subprocess.run(["timeout", "-k", "10", "120", exe, "1000"], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    assert "conductivity 1 ... 1000 on the finest mesh, 16.609375 on the one-cell mesh" in run.stdout  # 1 + 999 / 64
    norms = [float(m) for m in re.findall(r"\|u\| = (\S+)", run.stdout)]
    assert len(norms) == 5, run.stdout
    theta, dt = 0.5, 0.01
    levels, P = su.oracle_hierarchy(None, ("hypercube", 3, 2, "HMG-global"), Problem(ts.mass_coefficient(theta, dt), "inclusion"))
    lv = levels[-1]
    u = np.ones(lv.n)
    u[lv.constrained] = 0.0
    Mh, solve = ts.mass_matrix(lv), ts.pcg_solver(oracle, lv, oracle.Multigrid(levels, P, 3, coarse="direct").vcycle, 1e-10)
    for n, got in enumerate(norms):
        u, _ = ts.theta_step(lv, u, None, None, theta, dt, solve, Mh)
        print(f"heat_equation 1000 step {n + 1}: |u| {got:.12e}, oracle {np.linalg.norm(u):.12e}")
        assert got == pytest.approx(np.linalg.norm(u), rel=1e-9)
    bad = subprocess.run(["timeout", "-k", "10", "120", exe, "-1"], capture_output=True, text=True, cwd=ROOT)
    assert bad.returncode == 1 and "refused" in bad.stderr


# ------------------------------------------------------------------ 15. a coarse mesh overwritten by the caller
@pytest.mark.parametrize("sigma", SIGMAS)
def test_harmonic_mean_on_the_coarse_meshes(mgamd, oracle, emu, ctx, sigma):
    """the caller overwrites every coarse mesh with the harmonic mean of the finest field; the level operators use what the meshes
    hold when their DoFs are built, and the V-cycle follows an oracle hierarchy built with the same values"""
    case = ("quadrant", 3, 2, "HMG-global")
    fine = su.tria(mgamd, *case[:2], Problem(coefficient="inclusion"))
    finest = po.field_on(po.product_cells(fine), po.inclusion)

    def harmonic(t):
        return po.product_values(t, po.harmonic_restrict_field(finest, po.product_cells(t)))

    h = mgamd.Hierarchy(ctx, fine, case[1], case[2], case[3], coarse_solver="amg", max_brick=0, mass_coefficient=sigma,
                        coarse_coefficient=harmonic)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma, "inclusion"), restrict=po.harmonic_restrict_field)
    assert_level_coefficients(h, levels)
    # it is not the arithmetic mean: the one-cell mesh holds 64 / (63 + 1 / 1000), not 1 + 999 / 64
    mean = po.restrict_field(finest, po.product_cells(h.trias[0]))
    assert h.trias[0].n_cells == 1 and po.product_values(h.trias[0], mean)[0] - h.trias[0].coefficient()[0] > 10.0
    su.vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{case} inclusion, harmonic coarse means, sigma={sigma}")


# ------------------------------------------------------------------ 16. refusals
def test_refusals(mgamd, ctx):
    for mg_type in ("HMG-local", "HPMG-local"):
        with pytest.raises(mgamd.MgamdError, match="not implemented"):
            mgamd.Hierarchy(ctx, "quadrant", 3, 2, mg_type, coefficient=po.octants_xyz)
        with pytest.raises(mgamd.MgamdError, match="not implemented"):
            mgamd.Hierarchy(ctx, su.tria(mgamd, "quadrant", 3, Problem(coefficient="octants")), 3, 2, mg_type)
    with pytest.raises(mgamd.MgamdError, match="cell 0 is -1"):
        mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-global", coefficient=lambda x, y, z: np.full(x.shape, -1.0))
    with pytest.raises(mgamd.MgamdError, match="nan"):
        mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-global", coefficient=lambda x, y, z: np.where(x > 0, np.nan, 1.0))
    with pytest.raises(mgamd.MgamdError, match="no coarse meshes"):
        mgamd.Hierarchy(ctx, "quadrant", 3, 2, "PMG", coefficient=po.octants_xyz, coarse_coefficient=lambda m: np.ones(m.n_cells))
    mine = mgamd.Triangulation("quadrant", 3)
    mgamd.Hierarchy(ctx, mine, 3, 2, "HMG-global", coefficient=po.octants_xyz)
    assert mine.has_coefficient() and mine.coefficient().max() == 6.25  # the caller's mesh carries the values afterwards
    t = su.tria(mgamd, "quadrant", 3, Problem(coefficient="uniform"))
    with pytest.raises(mgamd.MgamdError, match="local smoothing"):
        t.level_mesh(1)
    # local smoothing without a coefficient stays what it was
    h = mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-local")
    assert not any(m.has_coefficient() for m in h.trias)
    # an operator keeps the coefficient of its tables, the tables that of their mesh when they were built
    d = mgamd.DoFs(t, 2, 0)
    op = mgamd.Operator(ctx, d)
    x = np.random.default_rng(1).standard_normal(d.n_dofs)
    y = apply_nan(mgamd, ctx, op.vmult, x)
    t.set_coefficient(None)
    assert d.coefficient_range() == (3.5, 3.5)
    y1 = apply_nan(mgamd, ctx, mgamd.Operator(ctx, d).vmult, x)
    assert np.array_equal(apply_nan(mgamd, ctx, op.vmult, x), y) or rel_err(apply_nan(mgamd, ctx, op.vmult, x), y) < 1e-14
    assert rel_err(y1, y) < 1e-14
