"""The mass term on the GPU: operators, smoothers, multigrid and CG for A = K + sigma M (-Laplace u + sigma u) against the
numpy oracle oracle/physics_oracle.py (sigma h^3 M (x) M (x) M added to mgoracle.Level's stiffness matrix).

sigma in {7.5, 3000}: no powers of two, so a wrong power of h cannot hide; the smaller is stiffness-dominated, the larger
mass-dominated at these mesh sizes, so a kernel family without the term cannot hide either.  Bounds are the project's own:
operator <= 1e-13, Chebyshev <= 1e-12 (test_chebyshev), V-cycle <= 1e-11, CG iterates <= 1e-10 with equal iteration counts, FP32
single kernels <= 2e-6, FP32 V-cycle <= 16 e_ref with e_ref from oracle/f32_emulation.py run on the helper's levels (its functions
take them unchanged).  Shapes are the smallest that reach each kernel (support.OP_CASES).  Each constraint search is made once
per session (support.py).

One case is added to the issue's list: PMG with coarse_solver="amg" runs on annulus L=6 as well as L=5 -- the p = 1 level of annulus
L=5 has 1965 DoFs, which the library solves exactly ("direct", up to 4096 DoFs), so the AMG only runs at L=6.  The sigma = 0
comparison is bit for bit where the product repeats its own bits and 1e-14 elsewhere (test_sigma_zero_is_bitwise_the_laplace_path)."""
import json
import os
import threading

import numpy as np
import pytest

import support as su
from conftest import rel_err
from physics_oracle import Problem
from support import (BIN, GOLDEN, OP_CASES, REFERENCE_COLUMNS, TOL_CHEB, TOL_CYCLE, TOL_F32, TOL_OP, TOL_SOL, apply_nan, atomic_contributions,
                     emu, final_table, run_harness, vcycle_and_solve)  # noqa: F401

pytestmark = pytest.mark.gpu

SIGMAS = [7.5, 3000.0]
# ------------------------------------------------------------------ operator and inverse diagonal
@pytest.mark.parametrize("geo,L,p,max_brick", OP_CASES)
def test_vmult_and_inverse_diagonal(mgamd, oracle, ctx, geo, L, p, max_brick):
    d = mgamd.DoFs(mgamd.Triangulation(geo, L), p, max_brick)
    rng = np.random.default_rng(3)
    for sigma in SIGMAS:
        d.set_mass_coefficient(sigma)
        op = mgamd.Operator(ctx, d)
        assert op.mass_coefficient() == sigma
        lv = su.oracle_level(d, geo, L, p, Problem(sigma))
        for trial in range(2):  # twice: a dirty tail accumulator shows in the second pass
            x = rng.standard_normal(lv.n)
            err = rel_err(apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x)
            print(f"vmult {geo} L={L} p={p} max_brick={max_brick} sigma={sigma}: rel.err {err:.2e}")
            assert err < TOL_OP
        diag = op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
        op.compute_inverse_diagonal(diag)
        err = rel_err(diag.to_host(), lv.inv_diag)
        print(f"inverse diagonal {geo} L={L} p={p} max_brick={max_brick} sigma={sigma}: rel.err {err:.2e}")
        assert err < TOL_OP
    # the operator keeps the sigma it was built with
    d.set_mass_coefficient(0.0)
    assert op.mass_coefficient() == SIGMAS[-1]
    assert rel_err(apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x) < TOL_OP


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 4), ("hypercube", 3, 2), ("quadrant", 3, 1)])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_chebyshev(mgamd, oracle, ctx, geo, L, p, sigma):
    d = mgamd.DoFs(mgamd.Triangulation(geo, L), p, 0)
    d.set_mass_coefficient(sigma)
    op = mgamd.Operator(ctx, d)
    lv = su.oracle_level(d, geo, L, p, Problem(sigma))
    ch = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
    ref = oracle.Chebyshev(lv.A, lv.inv_diag, 3, 20.0, 20)
    assert ch.eigenvalue_estimates()[1] == pytest.approx(ref.max_ev, rel=1e-10)
    rng = np.random.default_rng(5)
    b, x0 = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
    ev = rel_err(apply_nan(mgamd, ctx, ch.vmult, b), ref.vmult(b))
    vb, vx = op.initialize_dof_vector().from_host(b), op.initialize_dof_vector().from_host(x0)
    ch.step(vx, vb)
    es = rel_err(vx.to_host(), ref.step(x0, b))
    print(f"chebyshev {geo} L={L} p={p} sigma={sigma}: vmult {ev:.2e} step {es:.2e}")
    assert ev < TOL_CHEB and es < TOL_CHEB


# ------------------------------------------------------------------ V-cycle and CG
@pytest.mark.parametrize("case", [("quadrant", 3, 4, "HMG-global"), ("quadrant", 3, 4, "PMG"), ("quadrant", 3, 4, "HPMG"),
                                  ("hypercube", 5, 1, "HMG-global")], ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("sigma", SIGMAS)
def test_vcycle_and_cg(mgamd, oracle, emu, ctx, case, sigma):
    geo, L, p, mg_type = case
    h = mgamd.Hierarchy(ctx, geo, L, p, mg_type, coarse_solver="amg", max_brick=0, mass_coefficient=sigma)
    assert all(op.mass_coefficient() == sigma for op in h.operators)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma))
    vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{case} sigma={sigma}")


@pytest.mark.parametrize("sigma", SIGMAS)
def test_fused_transfers_under_the_mass_term(mgamd, oracle, emu, ctx, sigma, monkeypatch):
    """hypercube L=3 p=4: eight 17^3 bricks; restriction and prolongation run inside the operator passes (MODE_RESIDUAL_RESTRICT,
    MODE_CHEB_PROLONGATE) of the kernels that carry the mass term; equal to the separate transfer kernels and to the oracle"""
    case = ("hypercube", 3, 4, "HMG-global")
    h = mgamd.Hierarchy(ctx, *case, coarse_solver="amg", max_brick=0, mass_coefficient=sigma)
    assert sum(t.n_fused_bricks() for t in h.transfers[1:]) > 0
    monkeypatch.setenv("MGAMD_NO_FUSED_TRANSFER", "1")
    h0 = mgamd.Hierarchy(ctx, *case, coarse_solver="amg", max_brick=0, mass_coefficient=sigma)
    monkeypatch.delenv("MGAMD_NO_FUSED_TRANSFER")
    assert sum(t.n_fused_bricks() for t in h0.transfers[1:]) == 0
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma))
    vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{case} sigma={sigma} fused")
    r = np.random.default_rng(11).standard_normal(levels[-1].n)
    z, z0 = apply_nan(mgamd, ctx, h.mg.vmult, r), apply_nan(mgamd, ctx, h0.mg.vmult, r)
    assert rel_err(z, z0) < 1e-13
    z1 = apply_nan(mgamd, ctx, h.mg.vmult, r)  # repeated: no state left in the scratch vectors or the tail accumulator
    assert np.array_equal(z1, z) or rel_err(z1, z) < 1e-14  # (atomic summation order)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_collapsed_coarse_levels(mgamd, oracle, emu, ctx, sigma, monkeypatch):
    """quadrant L=4 p=1: the levels up to 2048 DoFs as one tabulated matrix, and kernel by kernel: both are the oracle's cycle"""
    case = ("quadrant", 4, 1, "HMG-global")
    ha = mgamd.Hierarchy(ctx, *case, coarse_solver="amg", mass_coefficient=sigma)
    monkeypatch.setenv("MGAMD_COLLAPSE_MAX_DOFS", "0")
    hb = mgamd.Hierarchy(ctx, *case, coarse_solver="amg", mass_coefficient=sigma)
    monkeypatch.delenv("MGAMD_COLLAPSE_MAX_DOFS")
    assert ha.mg.set_collapse(True) > 0 and hb.mg.set_collapse(True) == 0
    for h, tag in ((ha, "collapsed"), (hb, "kernel by kernel")):
        levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma))
        vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{case} sigma={sigma} {tag}")


@pytest.mark.parametrize("sigma", SIGMAS)
def test_gaussian_simulation_type(mgamd, oracle, emu, ctx, sigma):
    """load -Laplace u_g + sigma u_g, Dirichlet lifting with K + sigma M, solve, constraints.distribute"""
    case = ("quadrant", 3, 4, "HMG-global")
    h = mgamd.Hierarchy(ctx, *case, coarse_solver="amg", max_brick=0, mass_coefficient=sigma)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma))
    _, x, xref = vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"Gaussian {case} sigma={sigma}", rhs_kind=1)
    h.fine_operator.distribute(x, 1)
    assert rel_err(x.to_host(), levels[-1].distribute(xref, oracle.gaussian_solution)) < 10 * TOL_SOL


# ------------------------------------------------------------------ AMG
@pytest.mark.parametrize("L", [5, 6])
def test_pmg_with_amg_coarse_solver(mgamd, oracle, ctx, L):
    """annulus p=2, PMG, coarse_solver="amg", sigma = 7.5.  L=6: the p = 1 level has 9763 DoFs and the coarse solver is the
    smoothed-aggregation AMG of K + sigma M; the cycle against the oracle's Multigrid with amg_oracle, fed with the product's matrix,
    as its coarse solver (test_gpu_amg.py's tolerance).  L=5: that level has 1965 DoFs, which the library solves exactly (up to
    4096): sigma reaches the dense inverse of a PMG coarse level through the operator"""
    import amg_oracle as ao

    sigma, case = 7.5, ("annulus", L, 2, "PMG")
    h = mgamd.Hierarchy(ctx, *case, coarse_solver="amg", coarse_n_cycles=2, mass_coefficient=sigma)
    assert h.mg.coarse_solver_used() == ("amg" if L == 6 else "direct")
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma))
    A0 = ao.csr(*h.dofs[0].matrix())
    assert abs(A0 - levels[0].A).max() <= 1e-13 * abs(levels[0].A).max()
    mg = oracle.Multigrid(levels, P, 3, coarse=ao.SmoothedAggregation(h.dofs[0].matrix()).precondition(2) if L == 6 else "direct")
    r = np.random.default_rng(2).standard_normal(h.n_dofs)
    err = rel_err(apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r))
    Lf = levels[-1]
    xref, itref, _ = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    print(f"PMG + amg L={L} sigma={sigma}: V-cycle {err:.2e}, CG iterations {it} (oracle {itref}), iterate {rel_err(x.to_host(), xref):.2e}")
    assert err <= TOL_CYCLE
    assert it == itref and rel_err(x.to_host(), xref) <= TOL_SOL


@pytest.mark.parametrize("sigma", SIGMAS)
def test_assembled_matrix_amg_and_cg(mgamd, oracle, ctx, sigma):
    """SparseMatrix + PreconditionAMG + solve_cg (Type "AMG") on quadrant L=3 p=2: the matrix is the helper's, the solve the helper's
    pcg with the restated AMG: equal iteration counts"""
    import amg_oracle as ao

    geo, L, p = "quadrant", 3, 2
    h = mgamd.Hierarchy(ctx, geo, L, p, "AMG", mass_coefficient=sigma)
    d = h.dofs[0]
    assert d.mass_coefficient() == sigma and h.fine_operator.mass_coefficient() == sigma
    lv = su.oracle_level(d, geo, L, p, Problem(sigma))
    x = np.random.default_rng(4).standard_normal(lv.n)
    assert rel_err(apply_nan(mgamd, ctx, h.system_matrix.vmult, x), lv.A @ x) < TOL_OP
    o = ao.SmoothedAggregation(d.matrix())
    xref, itref, _ = oracle.pcg(lv.A, lv.rhs_constant, o.precondition(1), 1e-4)
    b, xv = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.system_matrix, h.amg, xv, b, 1e-4)
    print(f"Type AMG sigma={sigma}: CG iterations {it} (oracle {itref}), iterate {rel_err(xv.to_host(), xref):.2e}")
    assert it == itref and rel_err(xv.to_host(), xref) < TOL_SOL


# ------------------------------------------------------------------ FP32 levels
@pytest.mark.parametrize("sigma", SIGMAS)
def test_float_levels(mgamd, oracle, emu, ctx, sigma):
    """quadrant L=3 p=4 with MGNumberType float: single kernels <= 2e-6 against the FP64 helper; the V-cycle under the rule of
    test_gpu_float_levels.py, error <= 16 e_ref with e_ref from oracle/f32_emulation.py on the helper's levels (5e-5 stays as the
    outer cap); the outer CG needs the FP64 count"""
    case = ("quadrant", 3, 4, "HMG-global")
    h = mgamd.Hierarchy(ctx, *case, coarse_solver="amg", number_type=mgamd.F32, max_brick=0, mass_coefficient=sigma)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma))
    rng = np.random.default_rng(21)
    for l, op in enumerate(h.operators):
        lv = levels[l]
        x = rng.standard_normal(lv.n).astype(np.float32).astype(np.float64)
        src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
        op.vmult(dst, src)
        diag = op.initialize_dof_vector()
        op.compute_inverse_diagonal(diag)
        ev, ed = rel_err(dst.to_host(), lv.A @ x), rel_err(diag.to_host(), lv.inv_diag)
        print(f"FP32 level {l} sigma={sigma}: vmult {ev:.2e} inverse diagonal {ed:.2e}")
        assert ev < TOL_F32 and ed < TOL_F32
    mg = oracle.Multigrid(levels, P, 3, coarse="direct")
    mgp = emu.with_max_evs(mg, [s.eigenvalue_estimates()[1] for s in h.smoothers])
    Lf = levels[-1]
    r = rng.standard_normal(Lf.n)
    ref = mgp.vcycle(r)
    e_ref = rel_err(emu.vcycle(mgp, r, np.float32).astype(np.float64), ref)
    err = rel_err(apply_nan(mgamd, ctx, h.mg.vmult, r), ref)
    print(f"FP32 V-cycle sigma={sigma}: rel.err {err:.2e}, e_ref {e_ref:.2e}, ratio {err / e_ref:.2f}")
    assert err <= 16 * e_ref
    assert rel_err(apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r)) < 5e-5
    xref, it64, _ = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    print(f"FP32 CG sigma={sigma}: iterations {it}, FP64 oracle {it64}")
    assert it == it64


# ------------------------------------------------------------------ two simulated ranks
def test_two_simulated_ranks(mgamd, oracle, monkeypatch):
    """quadrant L=4 p=2 HMG-global cut over two ranks (host threads over the in-process communicator)"""
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")  # the sharded path's start vector hashes the DoF key; the oracle takes the same
    sigma, case, n_ranks = 7.5, ("quadrant", 4, 2, "HMG-global"), 2
    levels, P = su.oracle_hierarchy(None, case, Problem(sigma))
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
                                           mg_type=case[3], mass_coefficient=sigma)
            idx = np.array([kf[tuple(int(v) for v in k)] for k in h.dofs[-1].keys()])
            op = h.fine_operator
            vr, vz = op.initialize_dof_vector().from_host(r[idx]), op.initialize_dof_vector()
            h.mg.vmult(vz, vr)
            b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
            op.rhs(b)
            it, _ = mgamd.solve_cg(op, h.mg, x, b, 1e-4)
            out[rk] = dict(idx=idx, z=vz.to_host(), x=x.to_host(), it=it, dist=h.distributed[-1], sig=[o.mass_coefficient() for o in h.operators])
        except BaseException as e:  # noqa
            errs[rk] = e

    th = [threading.Thread(target=rank_main, args=(rk,)) for rk in range(n_ranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    for e in errs:
        if e is not None:
            raise e
    seen = {}
    for o in out:
        assert o["dist"] and all(s == sigma for s in o["sig"])
        ez, ex = rel_err(o["z"], zref[o["idx"]]), rel_err(o["x"], xref[o["idx"]])
        print(f"two ranks sigma={sigma}: V-cycle {ez:.2e}, CG iterations {o['it']} (oracle {itref}), iterate {ex:.2e}")
        assert ez < TOL_CYCLE and o["it"] == itref and ex < TOL_SOL
        for i, v in zip(o["idx"], o["x"]):
            assert seen.setdefault(i, v) == v  # copies of shared DoFs: bitwise identical
    assert len(seen) == Lf.n


# ------------------------------------------------------------------ sigma = 0 is today's code path
@pytest.mark.parametrize("geo", ["quadrant", "hypercube"])
def test_sigma_zero_is_bitwise_the_laplace_path(mgamd, ctx, geo):
    """mass_coefficient=0.0 passed explicitly and the argument left out, L=3 p=4.  vmult and the stored inverse diagonal are
    bit-identical wherever the product repeats its own bits: on the slot-interior DoFs (one thread completes them), on the
    constrained rows, and on the shell DoFs that at most two slots add to (a sum of two terms does not depend on their order).
    Shell DoFs shared by three or more slots are sums of floating-point atomic adds whose order the hardware chooses: there,
    and in a V-cycle, which chains such passes, the SAME build on the SAME input does not repeat its bits -- the two hierarchies
    of this test run identical code, and differ there (measured on an MI355X: max |difference| of vmult 5.6e-17 on quadrant,
    2.8e-17 on hypercube).  Those entries and the V-cycle are held to 1e-14, the bound
    test_fused_transfers_match_separate_transfers has for the summation order.  DESIGN.md, "Mass term", records this deviation
    from a comparison of all entries bit for bit."""
    ha = mgamd.Hierarchy(ctx, geo, 3, 4, "HMG-global", coarse_solver="amg", max_brick=0, mass_coefficient=0.0)
    hb = mgamd.Hierarchy(ctx, geo, 3, 4, "HMG-global", coarse_solver="amg", max_brick=0)
    d = ha.dofs[-1]
    n = ha.n_dofs
    assert np.array_equal(d.keys(), hb.dofs[-1].keys())
    cnt = atomic_contributions(d)
    det = cnt <= 2
    assert d.info.n_interior > 0 and (cnt == 2).any() and det.sum() > 0.8 * n
    x = np.random.default_rng(13).standard_normal(n)
    res = []
    for h in (ha, hb):
        op = h.operators[-1]
        assert op.mass_coefficient() == 0.0
        diag = op.initialize_dof_vector()
        op.compute_inverse_diagonal(diag)
        res.append((apply_nan(mgamd, ctx, op.vmult, x), diag.to_host(), apply_nan(mgamd, ctx, h.mg.vmult, x)))
    for name, a, b in zip(("vmult", "inverse diagonal", "V-cycle"), res[0], res[1]):
        print(f"{geo} sigma=0 {name}: max |difference| {np.abs(a - b).max():.2e}; {int(det.sum())} of {n} DoFs order-independent "
              f"({int((cnt == 1).sum())} / {int((cnt == 2).sum())} shell DoFs of one / two slots), there {np.abs(a[det] - b[det]).max():.2e}; "
              f"{int((~det).sum())} DoFs of three or more slots")
        if name != "V-cycle":
            assert np.array_equal(a[det], b[det]), name
        assert rel_err(a, b) < 1e-14, name


def test_stale_mass_coefficient_is_refused(mgamd, ctx):
    """an operator keeps the sigma it was built with; what would assemble ANOTHER operator's matrix from its tables is refused"""
    d = mgamd.DoFs(mgamd.Triangulation("quadrant", 3), 2, 0)
    d.set_mass_coefficient(7.5)
    op = mgamd.Operator(ctx, d)
    assert op.get_system_matrix().n_rows == d.n_dofs
    d.set_mass_coefficient(3000.0)
    with pytest.raises(mgamd.MgamdError, match="mass coefficient"):
        op.get_system_matrix()
    d.set_mass_coefficient(7.5)
    assert op.get_system_matrix().n_rows == d.n_dofs


# ------------------------------------------------------------------ refusals
def test_local_smoothing_refuses_the_mass_term(mgamd, ctx):
    for mg_type in ("HMG-local", "HPMG-local"):
        with pytest.raises(mgamd.MgamdError, match="local"):
            mgamd.Hierarchy(ctx, "quadrant", 3, 2, mg_type, mass_coefficient=7.5)
    t = mgamd.Triangulation("quadrant", 3)
    dl = mgamd.DoFs(t.level_mesh(t.n_levels - 1), 2, 0, local_smoothing_level=True)
    with pytest.raises(mgamd.MgamdError, match="local-smoothing"):
        dl.set_mass_coefficient(7.5)
    assert mgamd.Operator(ctx, dl).mass_coefficient() == 0.0  # sigma = 0 stays what it was
    h = mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-local", mass_coefficient=0.0)
    assert all(op.mass_coefficient() == 0.0 for op in h.operators)


def test_operator_reports_what_it_was_built_with(mgamd, ctx):
    d = mgamd.DoFs(mgamd.Triangulation("quadrant", 3), 2, 0)
    op0 = mgamd.Operator(ctx, d)
    d.set_mass_coefficient(7.5)
    op1 = mgamd.Operator(ctx, d, mgamd.F32)
    d.set_mass_coefficient(3000.0)
    assert (op0.mass_coefficient(), op1.mass_coefficient(), d.mass_coefficient()) == (0.0, 7.5, 3000.0)


# ------------------------------------------------------------------ harness
def test_harness_mass_coefficient(oracle, tmp_path):
    """input_0003.json (octant, NRefGlobal 3, p = 4, HMG-global) with "MassCoefficient": 7.5: the helper's iteration count, the
    table unchanged in columns and order, the value echoed; a local-smoothing Type: "not implemented", exit code 1"""
    base = json.load(open(os.path.join(GOLDEN, "input_0003.json")))
    f = str(tmp_path / "mass.json")
    json.dump(dict(base, MassCoefficient=7.5), open(f, "w"))
    rc, out, err = run_harness(f)
    assert rc == 0, err
    assert "MassCoefficient: 7.5" in out
    header, rows = final_table(out)
    assert header[:len(REFERENCE_COLUMNS)] == REFERENCE_COLUMNS
    assert header[len(REFERENCE_COLUMNS):] == ["workload_eff", "workload_path_max", "vertical_eff", "horizontal_eff", "mem_total",
                                               "dofs_per_s_per_vcycle", "coarse_solver"]
    case = (base["GeometryType"], int(base["NRefGlobal"]), int(base["Degree"]), base["Type"])
    assert case == ("quadrant", 3, 4, "HMG-global")
    levels, P = su.oracle_hierarchy(None, case, Problem(7.5))  # (iteration counts do not depend on the numbering)
    itref = oracle.pcg(levels[-1].A, levels[-1].rhs_constant, oracle.Multigrid(levels, P, 3, coarse="direct").vcycle, 1e-4)[1]
    print(f"harness MassCoefficient 7.5: n_iterations {rows[0]['n_iterations']}, helper {itref}")
    assert int(rows[0]["n_iterations"]) == itref
    rc0, out0, _ = run_harness(os.path.join(GOLDEN, "input_0003.json"))
    assert rc0 == 0 and "MassCoefficient" not in out0  # echoed only when non-zero
    assert final_table(out0)[0] == header
    g = str(tmp_path / "mass_local.json")
    json.dump(dict(base, MassCoefficient=7.5, Type="HMG-local"), open(g, "w"))
    rc, out, err = run_harness(g)
    assert rc == 1 and "not implemented" in err
