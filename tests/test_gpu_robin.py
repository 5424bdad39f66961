"""Convective (Robin) faces on the GPU: robin_face_kernel adds the face term  sum_f beta_f B_f x  into the accumulator of the tail
rows in every operator pass (product, residual, the three Chebyshev passes, the diagonal) of both number types; the mass pass has
none.  Everything is held against the numpy oracle oracle/physics_oracle.py (the surface mass matrices of the convective faces
in Kraw), with the helpers and the cached spaces of support.py.

Setups (physics_oracle): R1 only x = +1 Dirichlet, beta = 2.5 on x = -1 (hanging nodes on quadrant) and 0.75 on y = +1; R2 no
Dirichlet face, sigma = 0, beta = 1.5 on y = -1 and 4 on z = +1, regular only through the faces.  Bounds are the project's own:
operator <= 1e-13, Chebyshev <= 1e-12, V-cycle <= 1e-11, CG iterates <= 1e-10 with equal iteration counts, FP32 single kernels
<= 2e-6, FP32 V-cycle <= 16 e_ref (oracle/f32_emulation.py on the Robin levels) and <= 5e-5."""
import json
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import random_mesh_physics as rp
import support as su
import time_stepping_oracle as ts
from conftest import ROOT, rel_err
from physics_oracle import R1, R2, Problem
from support import GOLDEN, TOL_CHEB, TOL_CYCLE, TOL_F32, TOL_OP, TOL_SOL, emu, final_table, run_harness  # noqa: F401

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ operator and inverse diagonal, both number types
OP_CASES = [(c, s) for c in su.OP_CASES for s in ("R1", "R2")] + [(("hypercube", 5, 1, 0), "R2")]


@pytest.mark.parametrize("case,setup", OP_CASES, ids=lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else c)
def test_vmult_and_inverse_diagonal(mgamd, oracle, ctx, case, setup):
    """hypercube L=5 p=1 under R2 has 2 x 1024 face cells: 32 groups of 64 faces, 16 workgroups with a grid stride of 2"""
    geo, L, p, max_brick = case
    setup = {"R1": R1, "R2": R2}[setup]
    d = mgamd.DoFs(su.tria(mgamd, geo, L, Problem(0.0, None, *setup)), p, max_brick)
    lv = su.oracle_level(d, geo, L, p, Problem(0.0, None, *setup))
    n_faces = len(d.robin_faces()[2])
    assert n_faces > 0
    rng = np.random.default_rng(3)
    for number_type, tol in ((mgamd.F64, TOL_OP), (mgamd.F32, TOL_F32)):
        op = mgamd.Operator(ctx, d, number_type)
        for trial in range(2):  # twice: a dirty tail accumulator shows in the second pass
            x = rng.standard_normal(lv.n).astype(np.float32).astype(np.float64)
            src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
            op.vmult(dst, src)
            diag = op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
            op.compute_inverse_diagonal(diag)
            y, dg = dst.to_host().astype(np.float64), diag.to_host().astype(np.float64)
            assert np.isfinite(y).all() and np.isfinite(dg).all()
            ev, ed = rel_err(y, lv.A @ x), rel_err(dg, lv.inv_diag)
            print(f"{geo} L={L} p={p} max_brick={max_brick} mask={setup[0]:#04x} beta={setup[1]} {n_faces} face cells, "
                  f"{'FP64' if number_type == mgamd.F64 else 'FP32'} pass {trial}: vmult {ev:.2e} inverse diagonal {ed:.2e}")
            assert ev < tol and ed < tol
    # the face term is what is being measured: without it the product is off by far more than the bound
    assert rel_err(lv.A @ x, (lv.A - lv.C.T @ lv.Braw @ lv.C) @ x) > 1e-4


def test_the_mass_product_has_no_face_term(mgamd, oracle, ctx):
    geo, L, p = "quadrant", 3, 2
    d1, d0 = mgamd.DoFs(su.tria(mgamd, geo, L, Problem(0.0, None, *R1)), p, 0), mgamd.DoFs(su.tria(mgamd, geo, L, Problem(dirichlet_faces=R1[0])), p, 0)
    assert np.array_equal(d0.keys(), d1.keys())
    x = np.random.default_rng(13).standard_normal(d0.n_dofs)
    a, b = (su.apply_nan(mgamd, ctx, mgamd.Operator(ctx, d).vmult_mass, x) for d in (d0, d1))
    det = su.atomic_contributions(d0) <= 2  # (sums of three or more atomic adds do not repeat their bits: test_gpu_helmholtz)
    assert det.sum() > 0.5 * d0.n_dofs and np.array_equal(a[det], b[det]) and rel_err(a, b) < 1e-14
    lv = su.oracle_level(d1, geo, L, p, Problem(0.0, None, *R1))
    assert rel_err(b, ts.mass_matrix(lv) @ x) < TOL_OP


# ------------------------------------------------------------------ Chebyshev: the X_FROM_B variant, the plain one, the byte codes
@pytest.mark.parametrize("p", [2, 5])
def test_chebyshev(mgamd, oracle, ctx, p):
    geo, L = "quadrant", 3
    d = mgamd.DoFs(su.tria(mgamd, geo, L, Problem(0.0, None, *R1)), p, 0)
    op = mgamd.Operator(ctx, d)
    lv = su.oracle_level(d, geo, L, p, Problem(0.0, None, *R1))
    ch = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
    ref = oracle.Chebyshev(lv.A, lv.inv_diag, 3, 20.0, 20)
    assert ch.eigenvalue_estimates()[1] == pytest.approx(ref.max_ev, rel=1e-10)
    rng = np.random.default_rng(5)
    b, x0 = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
    ev = rel_err(su.apply_nan(mgamd, ctx, ch.vmult, b), ref.vmult(b))
    vb, vx = op.initialize_dof_vector().from_host(b), op.initialize_dof_vector().from_host(x0)
    ch.step(vx, vb)
    es = rel_err(vx.to_host(), ref.step(x0, b))
    print(f"chebyshev {geo} L={L} p={p} R1 ({d.n_dofs - d.info.n_interior} rows outside the slots): vmult {ev:.2e} step {es:.2e}")
    assert ev < TOL_CHEB and es < TOL_CHEB


def test_chebyshev_through_the_byte_codes(mgamd, oracle, ctx, monkeypatch):
    """hypercube L=5 p=1 under R2: 6000 and more tail rows, above the 4096 from which the tail rows, and with them the face kernel's
    x = c0 D^-1 b, read D^-1 through one-byte codes; against the oracle and against the vector read (MGAMD_NO_DINV_CODES)"""
    geo, L, p = "hypercube", 5, 1
    d = mgamd.DoFs(su.tria(mgamd, geo, L, Problem(0.0, None, *R2)), p, 0)
    assert d.n_dofs - d.info.n_interior >= 4096
    lv = su.oracle_level(d, geo, L, p, Problem(0.0, None, *R2))
    ref = oracle.Chebyshev(lv.A, lv.inv_diag, 3, 20.0, 20)
    b = np.random.default_rng(9).standard_normal(lv.n)
    outs = []
    for no_codes in (False, True):
        if no_codes:
            monkeypatch.setenv("MGAMD_NO_DINV_CODES", "1")
        op = mgamd.Operator(ctx, d)
        ch = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
        outs.append(su.apply_nan(mgamd, ctx, ch.vmult, b))
        assert rel_err(outs[-1], ref.vmult(b)) < TOL_CHEB
    monkeypatch.delenv("MGAMD_NO_DINV_CODES")
    assert rel_err(outs[0], outs[1]) < 1e-12


# ------------------------------------------------------------------ V-cycle and CG, eager and by graph replay
CYCLE_CASES = [(("quadrant", 3, 2, "HMG-global"), "R1"), (("quadrant", 3, 4, "HPMG"), "R1"), (("hypercube", 4, 1, "HMG-global"), "R2")]


@pytest.mark.parametrize("case,setup", CYCLE_CASES, ids=lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else c)
def test_vcycle_and_cg(mgamd, oracle, emu, ctx, case, setup):
    setup = {"R1": R1, "R2": R2}[setup]
    h = su.hierarchy(mgamd, ctx, case, Problem(0.0, None, *setup), max_brick=0, coarse_solver="direct")
    assert h.mg.coarse_solver_used() == "direct"
    n_fused = sum(t.n_fused_bricks() for t in h.transfers[1:])
    assert n_fused == 0  # levels with a convective face run their transfers un-fused
    if case[0] == "hypercube":  # the same meshes and mask without a convective face (sigma = 1 keeps it regular) do fuse
        h1 = mgamd.Hierarchy(ctx, *case, coarse_solver="direct", max_brick=0, mass_coefficient=1.0, dirichlet_faces=setup[0])
        assert sum(t.n_fused_bricks() for t in h1.transfers[1:]) > 0
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(0.0, None, *setup))
    su.check_transfers(h, levels, P, f"{case} beta={setup[1]}")
    mg, _, _ = su.vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{case} mask={setup[0]:#04x} beta={setup[1]} eager")
    r = np.random.default_rng(12).standard_normal(levels[-1].n)
    vr, vz = h.fine_operator.initialize_dof_vector().from_host(r), h.fine_operator.initialize_dof_vector().from_host(np.full(len(r), np.nan))
    h.mg.time_vcycles(vz, vr, 2, True)
    err = rel_err(vz.to_host(), mg.vcycle(r))
    print(f"{case} beta={setup[1]} graph replay: V-cycle {err:.2e}")
    assert err < TOL_CYCLE
    # the stage callbacks (HIP-event stage timing): the same cycle, stages recorded (on these small hierarchies the levels are
    # collapsed into the coarse solve of the collapse level: test_gpu_parity.test_event_stage_timing)
    h.mg.stage_timing(True)
    zs = su.apply_nan(mgamd, ctx, h.mg.vmult, r)
    ms = h.mg.stage_times()
    h.mg.stage_timing(False)
    assert rel_err(zs, mg.vcycle(r)) < TOL_CYCLE and (ms >= 0).all() and ms.sum() > 0


def test_coarse_solver_cg_with_chebyshev(mgamd, oracle, emu, ctx):
    """PMG on quadrant L=3 p=2 under R1: the p = 1 level with hanging nodes and convective faces is the coarse problem"""
    case, coarse = ("quadrant", 3, 2, "PMG"), "cg_with_chebyshev"
    h = su.hierarchy(mgamd, ctx, case, Problem(0.0, None, *R1), max_brick=0, coarse_solver=coarse)
    assert h.mg.coarse_solver_used() == coarse
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(0.0, None, *R1))
    mg = emu.with_max_evs(oracle.Multigrid(levels, P, 3, coarse=coarse), [s.eigenvalue_estimates()[1] for s in h.smoothers])
    Lf = levels[-1]
    r = np.random.default_rng(7).standard_normal(Lf.n)
    ez = rel_err(su.apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r))
    xref, itref, _ = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    ex = rel_err(x.to_host(), xref)
    print(f"{case} R1 {coarse}: V-cycle {ez:.2e}, CG iterations {it} (oracle {itref}), iterate {ex:.2e}")
    assert ez < 1e-4 and it == itref and ex < 1e-5  # (an inner CG stops on a tolerance: test_gpu_distributed_sim's bounds)


# ------------------------------------------------------------------ AMG
def test_solve_with_amg(mgamd, oracle, ctx):
    """Type "AMG" on quadrant L=3 p=2 under R1: the assembled matrix and the AMG built on it carry the face term"""
    import amg_oracle as ao

    geo, L, p = "quadrant", 3, 2
    h = mgamd.Hierarchy(ctx, geo, L, p, "AMG", dirichlet_faces=R1[0], robin=R1[1])
    d = h.dofs[0]
    lv = su.oracle_level(d, geo, L, p, Problem(0.0, None, *R1))
    x = np.random.default_rng(4).standard_normal(lv.n)
    assert rel_err(su.apply_nan(mgamd, ctx, h.system_matrix.vmult, x), lv.A @ x) < TOL_OP
    xref, itref, _ = oracle.pcg(lv.A, lv.rhs_constant, ao.SmoothedAggregation(d.matrix()).precondition(1), 1e-4)
    b, xv = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.system_matrix, h.amg, xv, b, 1e-4)
    print(f"Type AMG R1: CG iterations {it} (oracle {itref}), iterate {rel_err(xv.to_host(), xref):.2e}")
    assert it == itref and rel_err(xv.to_host(), xref) < TOL_SOL


def test_pmg_with_amg_coarse_solver(mgamd, oracle, ctx):
    """annulus L=6 p=2 PMG under R1 (test_gpu_boundary's shape, the smallest PMG case whose p = 1 level is above 4096 DoFs): the
    coarse solver is the smoothed-aggregation AMG of the matrix with the face term"""
    import amg_oracle as ao

    case = ("annulus", 6, 2, "PMG")
    h = su.hierarchy(mgamd, ctx, case, Problem(0.0, None, *R1), max_brick=0, coarse_n_cycles=2)
    assert h.mg.coarse_solver_used() == "amg"
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(0.0, None, *R1))
    A0 = ao.csr(*h.dofs[0].matrix())
    assert abs(A0 - levels[0].A).max() <= 1e-13 * abs(levels[0].A).max()
    mg = oracle.Multigrid(levels, P, 3, coarse=ao.SmoothedAggregation(h.dofs[0].matrix()).precondition(2))
    r = np.random.default_rng(2).standard_normal(h.n_dofs)
    err = rel_err(su.apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r))
    Lf = levels[-1]
    xref, itref, _ = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    print(f"PMG + amg annulus L=6 R1: V-cycle {err:.2e}, CG iterations {it} (oracle {itref}), iterate {rel_err(x.to_host(), xref):.2e}")
    assert err <= TOL_CYCLE and it == itref and rel_err(x.to_host(), xref) <= TOL_SOL


# ------------------------------------------------------------------ FP32 levels
def test_float_levels(mgamd, oracle, emu, ctx):
    case = ("quadrant", 3, 4, "HMG-global")
    h = su.hierarchy(mgamd, ctx, case, Problem(0.0, None, *R1), max_brick=0, number_type=mgamd.F32)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(0.0, None, *R1))
    mg = oracle.Multigrid(levels, P, 3, coarse="direct")
    mgp = emu.with_max_evs(mg, [s.eigenvalue_estimates()[1] for s in h.smoothers])
    Lf = levels[-1]
    r = np.random.default_rng(21).standard_normal(Lf.n)
    ref = mgp.vcycle(r)
    e_ref = rel_err(emu.vcycle(mgp, r, np.float32).astype(np.float64), ref)
    err = rel_err(su.apply_nan(mgamd, ctx, h.mg.vmult, r), ref)
    print(f"FP32 V-cycle R1: rel.err {err:.2e}, e_ref {e_ref:.2e}, ratio {err / e_ref:.2f}")
    assert err <= 16 * e_ref and err <= 5e-5
    xref, it64, _ = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    assert it == it64


# ------------------------------------------------------------------ two simulated ranks
def test_two_simulated_ranks(mgamd, oracle, monkeypatch):
    """R1 on quadrant L=3 p=2 HMG-global cut over two ranks (host threads over the in-process communicator): each rank's face kernel
    runs over its own cells' faces with the halo slots and the exchange sums what the ranks add to shared boundary DoFs; operator,
    V-cycle and CG against the one-rank numpy oracle through the DoF keys"""
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")  # the sharded path's start vector hashes the DoF key; the oracle takes the same
    case, n_ranks = ("quadrant", 3, 2, "HMG-global"), 2
    levels, P = su.oracle_hierarchy(None, case, Problem(0.0, None, *R1))
    omg = oracle.Multigrid(levels, P, 3, coarse="direct", start_vectors=[oracle.key_hash_start_vector(lv) for lv in levels])
    Lf = levels[-1]
    kf = {tuple(int(v) for v in k): i for i, k in enumerate(Lf.keys)}
    r = np.sin(np.arange(Lf.n) * 0.37) + 0.25
    r[Lf.constrained] = 0.0
    yref, zref = Lf.A @ r, omg.vcycle(r)
    xref, itref, _ = oracle.pcg(Lf.A, Lf.rhs_constant, omg.vcycle, 1e-4)
    group = mgamd.SimGroup(n_ranks)
    out, errs = [None] * n_ranks, [None] * n_ranks

    def rank_main(rk):
        try:
            c = mgamd.Context(0)
            h = mgamd.DistributedHierarchy(c, group.comm(rk), *case[:3], coarse_solver="amg", max_brick=0, min_root_dofs=0,
                                           mg_type=case[3], dirichlet_faces=R1[0], robin=R1[1])
            idx = np.array([kf[tuple(int(v) for v in k)] for k in h.dofs[-1].keys()])
            op = h.fine_operator
            vr, vy, vz = op.initialize_dof_vector().from_host(r[idx]), op.initialize_dof_vector(), op.initialize_dof_vector()
            op.vmult(vy, vr)
            h.mg.vmult(vz, vr)
            b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
            op.rhs(b)
            it, _ = mgamd.solve_cg(op, h.mg, x, b, 1e-4)
            out[rk] = dict(idx=idx, y=vy.to_host(), z=vz.to_host(), x=x.to_host(), it=it, dist=h.distributed[-1],
                           faces=len(h.dofs[-1].robin_faces()[2]))
        except BaseException as e:  # noqa
            errs[rk] = e

    threads = [threading.Thread(target=rank_main, args=(rk,)) for rk in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in threads)
    for e in errs:
        if e is not None:
            raise e
    for o in out:
        free = ~Lf.constrained[o["idx"]]
        ey, ez, ex = rel_err(o["y"][free], yref[o["idx"]][free]), rel_err(o["z"], zref[o["idx"]]), rel_err(o["x"], xref[o["idx"]])
        print(f"two ranks R1: {o['faces']} face cells, operator {ey:.2e}, V-cycle {ez:.2e}, CG iterations {o['it']} (oracle {itref}), "
              f"iterate {ex:.2e}")
        assert o["dist"] and o["faces"] > 0
        assert ey < TOL_OP and ez < TOL_CYCLE and o["it"] == itref and ex < TOL_SOL


# ------------------------------------------------------------------ random octree
def test_random_octree(mgamd, oracle, emu, ctx):
    """mesh M of random_mesh_physics at p = 2 with R1, sigma = 7.5 and the per_family coefficient: operator, inverse diagonal,
    V-cycle and CG"""
    name, p, mg_type, field, sigma = "M", 2, "HMG-global", "per_family", 7.5
    t = su.tria_of(mgamd, rp.leaves_of(oracle, name), Problem(coefficient=field))
    h = mgamd.Hierarchy(ctx, t, 0, p, mg_type, coarse_solver="amg", max_brick=0, mass_coefficient=sigma, dirichlet_faces=R1[0], robin=R1[1])
    assert np.array_equal(t.robin_coefficients(), R1[1]) and h.dofs[-1].info.n_hanging > 0
    levels, P = su.oracle_hierarchy_on(h.dofs, *rp.level_plan(oracle, name, p, mg_type), Problem(sigma, field, *R1))
    lv, op = levels[-1], h.fine_operator
    x = np.random.default_rng(3).standard_normal(lv.n)
    diag = op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
    op.compute_inverse_diagonal(diag)
    ev, ed = rel_err(su.apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x), rel_err(diag.to_host(), lv.inv_diag)
    print(f"random octree {name} p={p} {field} R1 sigma={sigma}: vmult {ev:.2e} inverse diagonal {ed:.2e}")
    assert ev < TOL_OP and ed < TOL_OP
    su.vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"random octree {name} p={p} {field} R1 sigma={sigma}")


# ------------------------------------------------------------------ known answer
@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 2), ("hypercube", 2, 3)])
def test_convective_wall_known_answer(mgamd, oracle, ctx, geo, L, p):
    """three layers 1 | 5 | 0.2, f = 0, u = 0 on x = -1, a convective face at x = +1 with beta = 2 and u_ext = 7: the solution is q
    times the resistance between x = -1 and x, q = beta u_ext / (1 + beta R); it lies in the FE space.  solve_cg with the multigrid
    at reltol 1e-12, then distribute: only the solver tolerance times the conditioning of these small meshes remains"""
    planes, values, beta, u_ext = [-0.5, 0.0], [1.0, 5.0, 0.2], 2.0, 7.0
    h = mgamd.Hierarchy(ctx, mgamd.Triangulation(geo, L), 0, p, "HMG-global", coarse_solver="amg", max_brick=0, dirichlet_faces=0b000001,
                        robin={1: beta}, coefficient=lambda x, y, z: su.layers(x, planes, values))
    op = h.fine_operator
    b, u = op.initialize_dof_vector(), op.initialize_dof_vector()
    op.rhs_boundary_flux(b, {1: beta * u_ext})
    it, _ = mgamd.solve_cg(op, h.mg, u, b, 1e-12)
    op.distribute(u)
    x = su.oracle_level(h.dofs[-1], geo, L, p).node_positions()[:, 0]
    edges = np.concatenate(([-1.0], planes, [1.0]))
    R = sum((hi - lo) / a for lo, hi, a in zip(edges[:-1], edges[1:], values))
    q = beta * u_ext / (1.0 + beta * R)
    ref = q * sum((np.clip(x, lo, hi) - lo) / a for lo, hi, a in zip(edges[:-1], edges[1:], values))
    err = np.abs(u.to_host() - ref).max() / np.abs(ref).max()
    print(f"{geo} {L} p={p} convective wall: CG iterations {it}, face temperature {q * R:.8f}, relative nodal error {err:.2e}")
    assert err <= 1e-8


def test_convective_wall_example_program():
    """bin/convective_wall (examples/convective_wall.cpp, the C++ classes): the same wall with beta = 2, u_ext = 7: the face
    temperature is q R = 14 * 5.6 / 12.2"""
    exe = os.path.join(ROOT, "bin", "convective_wall")
    assert os.path.exists(exe), "bin/convective_wall is missing: make all"
    run = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    m = re.search(r"face temperature computed (\S+) \.\.\. (\S+)\s+analytic (\S+)", run.stdout)
    assert m, run.stdout
    lo, hi, exact = (float(v) for v in m.groups())
    print(run.stdout.strip())
    assert exact == pytest.approx(14.0 * 5.6 / 12.2, rel=1e-14) and abs(lo - exact) <= 1e-8 * exact and abs(hi - exact) <= 1e-8 * exact
    assert re.search(r"analytic \d+\.\d{10}", run.stdout)


# ------------------------------------------------------------------ time stepper
def test_a_box_with_two_convective_faces_cools(mgamd, oracle, emu, ctx):
    """mask 0, beta on two faces, u_ext = 0, f = 0, Crank-Nicolson, five steps on quadrant L=3 p=2 from a positive start: the
    iterates are the oracle stepper's on the Robin level (n steps x 1e-10, equal CG counts at reltol 1e-6), and the total heat
    1^T M^ u decreases in every step"""
    case, theta, dt, n_steps, reltol = ("quadrant", 3, 2, "HMG-global"), 0.5, 0.02, 5, 1e-6
    setup = (0, (0.0, 3.0, 0.0, 0.0, 1.0, 0.0))
    sigma = mgamd.TimeStepper.mass_coefficient(theta, dt)
    h = su.hierarchy(mgamd, ctx, case, Problem(sigma, None, *setup), max_brick=0)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma, None, *setup))
    lv, op = levels[-1], h.fine_operator
    Mh = ts.mass_matrix(lv)
    u0 = 1.0 + np.random.default_rng(17).random(lv.n)
    u0[lv.constrained] = 0.0
    stepper = mgamd.TimeStepper(op, h.mg, theta, dt)
    mg = emu.with_max_evs(oracle.Multigrid(levels, P, 3, coarse="direct"), [s.eigenvalue_estimates()[1] for s in h.smoothers])
    solve = ts.pcg_solver(oracle, lv, mg.vcycle, reltol)
    one = np.ones(lv.n)
    u, uref, its, itref, heat = op.initialize_dof_vector().from_host(u0), u0.copy(), [], [], [one @ (Mh @ u0)]
    for n in range(n_steps):
        its.append(stepper.step(u, reltol=reltol)[0])
        uref, it = ts.theta_step(lv, uref, None, None, theta, dt, solve, Mh)
        itref.append(it)
        heat.append(one @ (Mh @ u.to_host()))
    err = rel_err(u.to_host(), uref)
    print(f"cooling box {case}: CG iterations {its} (oracle {itref}), iterate {err:.2e}, heat {['%.6f' % v for v in heat]}")
    assert its == itref and err <= n_steps * TOL_SOL
    assert all(b < a for a, b in zip(heat[:-1], heat[1:]))


# ------------------------------------------------------------------ refusals and the regular Neumann box
def test_device_side_refusals(mgamd, ctx):
    for mg_type in ("HMG-local", "HPMG-local"):
        with pytest.raises(mgamd.MgamdError, match=f"Type '{mg_type}' with the Robin coefficients.*local"):
            mgamd.Hierarchy(ctx, "quadrant", 3, 2, mg_type, dirichlet_faces=0x3E, robin={0: 1.0})
    with pytest.raises(mgamd.MgamdError, match="on face 1 refused: the face is Dirichlet"):
        mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-global", dirichlet_faces=R1[0], robin={1: 1.0})
    with pytest.raises(mgamd.MgamdError, match="singular: dirichlet_faces mask 0.*sigma = 0"):
        mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-global", dirichlet_faces=0)
    # one convective face makes mask 0 with sigma 0 regular: every solver entry accepts it
    h = su.hierarchy(mgamd, ctx, ("quadrant", 3, 2, "HMG-global"), Problem(0.0, None, *R2), max_brick=0)
    op = h.fine_operator
    b, v = op.initialize_dof_vector(), op.initialize_dof_vector()
    op.rhs(b)
    assert mgamd.solve_cg(op, h.mg, v, b, 1e-4)[0] > 0
    assert mgamd.SparseMatrix(ctx, h.dofs[-1]) is not None and len(h.dofs[0].amg_setup_info()) >= 1
    with pytest.raises(mgamd.MgamdError, match="SimulationType 1 with Robin coefficients.*not implemented"):
        op.rhs(b, 1)


# ------------------------------------------------------------------ harness
def test_harness_robin_coefficients(mgamd, oracle, ctx, tmp_path):
    """input_0003.json (quadrant, NRefGlobal 3, p = 4, HMG-global) with "NeumannFaces": "023" and "RobinCoefficients" on faces 0
    and 3: the CG count of the Python solve and of the oracle, the value echoed; a local-smoothing Type and a coefficient on a
    Dirichlet face: "not implemented", exit code 1"""
    base = json.load(open(os.path.join(GOLDEN, "input_0003.json")))
    case = (base["GeometryType"], int(base["NRefGlobal"]), int(base["Degree"]), base["Type"])
    assert case == ("quadrant", 3, 4, "HMG-global")
    setup = (0x3F & ~0b001101, (2.5, 0.0, 0.0, 0.75, 0.0, 0.0))
    f = str(tmp_path / "robin.json")
    json.dump(dict(base, NeumannFaces="023", RobinCoefficients="2.5,0,0,0.75,0,0"), open(f, "w"))
    rc, out, err = run_harness(f)
    assert rc == 0, err
    assert "RobinCoefficients: 2.5,0,0,0.75,0,0" in out
    _, rows = final_table(out)
    number_type = mgamd.F32 if base.get("MGNumberType", "float") == "float" else mgamd.F64
    h = su.hierarchy(mgamd, ctx, case, Problem(0.0, None, *setup), max_brick=0, number_type=number_type)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, float(base.get("RelativeTolerance", 1e-4)))
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(0.0, None, *setup))
    itref = oracle.pcg(levels[-1].A, levels[-1].rhs_constant, oracle.Multigrid(levels, P, 3, coarse="direct").vcycle, 1e-4)[1]
    print(f"harness RobinCoefficients: n_iterations {rows[0]['n_iterations']}, Python solve {it}, oracle {itref}")
    assert int(rows[0]["n_iterations"]) == it == itref
    rc0, out0, _ = run_harness(os.path.join(GOLDEN, "input_0003.json"))
    assert rc0 == 0 and "RobinCoefficients" not in out0  # echoed only when set
    for extra in (dict(NeumannFaces="023", RobinCoefficients="2.5,0,0,0.75,0,0", Type="HMG-local"),
                  dict(NeumannFaces="0", RobinCoefficients="0,1,0,0,0,0"), dict(NeumannFaces="0", RobinCoefficients="1,2,3"),
                  dict(NeumannFaces="0", RobinCoefficients="-1,0,0,0,0,0")):
        g = str(tmp_path / "refused.json")
        json.dump(dict(base, **extra), open(g, "w"))
        rc, out, err = run_harness(g)
        assert rc == 1 and "not implemented" in err and "RobinCoefficients" in err, (extra, err)
