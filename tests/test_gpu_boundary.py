"""Per-face boundary conditions on the GPU: the kernels are the ones that ran before, the tables are new.  With natural (Neumann)
faces the boundary shell gathers and atomic scatters of every kernel family, the coarse boundary DoFs of the fused transfers, the
D^-1 byte codes of many more tail rows and levels without any constrained DoF carry live rows for the first time.  Everything is
held against the numpy oracle oracle/physics_oracle.py (Dirichlet DoFs chosen by face).

Masks (physics_oracle): M1 only x = -1 is Dirichlet (on quadrant the refined corner touches it: hanging nodes on both kinds of
face), M2 the three "+" faces (hanging nodes on Neumann faces, a Neumann-Neumann edge and corner in the refined region), M0 none,
with sigma = 7.5.  Bounds are the project's own: operator <= 1e-13, Chebyshev <= 1e-12, V-cycle <= 1e-11, CG iterates <= 1e-10 with
equal iteration counts, FP32 single kernels <= 2e-6, FP32 V-cycle <= 16 e_ref with e_ref from oracle/f32_emulation.py run on the
levels of the mask.  Shapes are support.OP_CASES.

The numpy hierarchies come from support.py: one constraint search per (mesh, degree) in the oracle's own numbering, the transfers
once under mask 0; a case permutes them into the numbering of the product's tables (which changes with the mask: tail and
Dirichlet DoFs are numbered apart) and forms the levels of its problem (physics_oracle.Level, mask_transfers, held against
spaces built directly by test_boundary_host.py)."""
import json
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import physics_oracle as po
import random_mesh_physics as rp
import support as su
import time_stepping_oracle as ts
from conftest import ROOT, rel_err
from physics_oracle import M0, M1, M2, Problem
from support import GOLDEN, OP_CASES, TOL_CHEB, TOL_CYCLE, TOL_F32, TOL_OP, TOL_SOL, check_transfers, emu, final_table, run_harness, vcycle_and_solve  # noqa: F401

pytestmark = pytest.mark.gpu

MASKS = [(M1, 0.0), (M2, 0.0), (M0, 7.5)]

# ------------------------------------------------------------------ operator, mass operator, inverse diagonal
@pytest.mark.parametrize("geo,L,p,max_brick", OP_CASES)
def test_vmult_mass_and_inverse_diagonal(mgamd, oracle, ctx, geo, L, p, max_brick):
    rng = np.random.default_rng(3)
    for mask, sigma in MASKS:
        d = mgamd.DoFs(su.tria(mgamd, geo, L, Problem(dirichlet_faces=mask)), p, max_brick)
        d.set_mass_coefficient(sigma)
        op = mgamd.Operator(ctx, d)
        lv = su.oracle_level(d, geo, L, p, Problem(sigma, dirichlet_faces=mask))
        assert d.info.n_dirichlet == int((lv.dirichlet & ~lv.hanging).sum())
        Mh, c = ts.mass_matrix(lv), lv.constrained
        for trial in range(2):  # twice: a dirty tail accumulator shows in the second pass
            x = rng.standard_normal(lv.n)
            ev = rel_err(su.apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x)
            y = su.apply_nan(mgamd, ctx, op.vmult_mass, x)
            em = rel_err(y, Mh @ x)
            diag = op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
            op.compute_inverse_diagonal(diag)
            ed = rel_err(diag.to_host(), lv.inv_diag)
            print(f"{geo} L={L} p={p} max_brick={max_brick} mask={mask:#04x} sigma={sigma} pass {trial}: vmult {ev:.2e} vmult_mass {em:.2e} "
                  f"inverse diagonal {ed:.2e}")
            assert ev < TOL_OP and em < TOL_OP and ed < TOL_OP
            assert (y[c] == 0.0).all()
        # rows of DoFs on natural faces are live in the mass operator
        top = p << oracle.LMAX
        k = np.array(lv.keys)[:, :3]
        natural = ((k == 0) | (k == top)).any(axis=1) & ~c
        assert natural.any() and (np.abs(Mh @ x)[natural] > 0).all() and (y[natural] != 0.0).all()


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 4), ("hypercube", 3, 2), ("quadrant", 4, 1)])
def test_default_mask_set_explicitly_is_bitwise_the_unset_mesh(mgamd, ctx, geo, L, p):
    d0, d1 = mgamd.DoFs(mgamd.Triangulation(geo, L), p, 0), mgamd.DoFs(su.tria(mgamd, geo, L, Problem(dirichlet_faces=0x3F)), p, 0)
    assert np.array_equal(d0.keys(), d1.keys()) and np.array_equal(d0.cell_dofs(), d1.cell_dofs())
    x = np.random.default_rng(13).standard_normal(d0.n_dofs)
    a, b = (su.apply_nan(mgamd, ctx, mgamd.Operator(ctx, d).vmult, x) for d in (d0, d1))
    det = su.atomic_contributions(d0) <= 2  # (sums of three or more atomic adds do not repeat their bits: test_gpu_helmholtz)
    assert det.sum() > 0.8 * d0.n_dofs and np.array_equal(a[det], b[det]) and rel_err(a, b) < 1e-14


# ------------------------------------------------------------------ V-cycle and CG
@pytest.mark.parametrize("case", [("hypercube", 3, 2, "HMG-global"), ("hypercube", 4, 1, "HMG-global")], ids=lambda c: "-".join(map(str, c)))
def test_levels_without_a_constrained_row(mgamd, oracle, emu, ctx, case):
    """hypercube under M0: no Dirichlet and no hanging DoF on any level, level 0 is one cell whose DoFs are all free"""
    h = su.hierarchy(mgamd, ctx, case, Problem(7.5, dirichlet_faces=M0), max_brick=0)
    assert all(d.info.n_dirichlet == 0 and d.info.n_hanging == 0 for d in h.dofs)
    assert h.dofs[0].info.n_cells == 1 and h.dofs[0].n_dofs == (case[2] + 1) ** 3
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(7.5, dirichlet_faces=M0))
    rng = np.random.default_rng(5)
    for l, (op, lv) in enumerate(zip(h.operators, levels)):
        x = rng.standard_normal(lv.n)
        assert rel_err(su.apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x) < TOL_OP
        ch, ref = mgamd.PreconditionChebyshev(op, 3, 20.0, 20), oracle.Chebyshev(lv.A, lv.inv_diag, 3, 20.0, 20)
        assert ch.eigenvalue_estimates()[1] == pytest.approx(ref.max_ev, rel=1e-10)
        assert rel_err(su.apply_nan(mgamd, ctx, ch.vmult, x), ref.vmult(x)) < TOL_CHEB
    check_transfers(h, levels, P, f"{case} M0")
    vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{case} M0 sigma=7.5")


def test_dinv_byte_codes_of_natural_boundary_rows(mgamd, oracle, emu, ctx, monkeypatch):
    """hypercube L=5 p=1 under M2: 5768 tail rows (all-Dirichlet: 2791), above the 4096 from which tail_kernel reads D^-1 through
    one-byte codes; against the oracle and against the vector read (MGAMD_NO_DINV_CODES)"""
    case = ("hypercube", 5, 1, "HMG-global")
    h = su.hierarchy(mgamd, ctx, case, Problem(dirichlet_faces=M2), max_brick=0)
    i = h.dofs[-1].info
    assert i.n_tail > 4096 and i.n_dofs - i.n_interior >= 4096
    assert i.n_tail > mgamd.DoFs(mgamd.Triangulation("hypercube", 5), 1, 0).info.n_tail
    monkeypatch.setenv("MGAMD_NO_DINV_CODES", "1")
    h0 = su.hierarchy(mgamd, ctx, case, Problem(dirichlet_faces=M2), max_brick=0)
    monkeypatch.delenv("MGAMD_NO_DINV_CODES")
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(0.0, dirichlet_faces=M2))
    lv, rng = levels[-1], np.random.default_rng(9)
    b, x0 = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
    ref = oracle.Chebyshev(lv.A, lv.inv_diag, 3, 20.0, 20)
    outs = []
    for hh in (h, h0):
        op = hh.operators[-1]
        ch = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
        v = su.apply_nan(mgamd, ctx, ch.vmult, b)
        vx, vb = op.initialize_dof_vector().from_host(x0), op.initialize_dof_vector().from_host(b)
        ch.step(vx, vb)
        z = su.apply_nan(mgamd, ctx, hh.mg.vmult, b)
        assert rel_err(v, ref.vmult(b)) < TOL_CHEB and rel_err(vx.to_host(), ref.step(x0, b)) < TOL_CHEB
        outs.append((v, vx.to_host(), z))
    for a, c in zip(*outs):
        assert rel_err(a, c) < 1e-12
    vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{case} M2 byte codes")


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 4), ("hypercube", 3, 2), ("quadrant", 3, 1)])
@pytest.mark.parametrize("mask", [M1, M2])
def test_chebyshev(mgamd, oracle, ctx, geo, L, p, mask):
    d = mgamd.DoFs(su.tria(mgamd, geo, L, Problem(dirichlet_faces=mask)), p, 0)
    op = mgamd.Operator(ctx, d)
    lv = su.oracle_level(d, geo, L, p, Problem(0.0, dirichlet_faces=mask))
    ch = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
    ref = oracle.Chebyshev(lv.A, lv.inv_diag, 3, 20.0, 20)
    assert ch.eigenvalue_estimates()[1] == pytest.approx(ref.max_ev, rel=1e-10)
    rng = np.random.default_rng(5)
    b, x0 = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
    ev = rel_err(su.apply_nan(mgamd, ctx, ch.vmult, b), ref.vmult(b))
    vb, vx = op.initialize_dof_vector().from_host(b), op.initialize_dof_vector().from_host(x0)
    ch.step(vx, vb)
    es = rel_err(vx.to_host(), ref.step(x0, b))
    print(f"chebyshev {geo} L={L} p={p} mask={mask:#04x}: vmult {ev:.2e} step {es:.2e}")
    assert ev < TOL_CHEB and es < TOL_CHEB


FUSED = [("hypercube", 3, 4, "HMG-global"), ("hypercube", 4, 2, "HMG-global"), ("hypercube", 5, 1, "HMG-global")]
TRANSFER_CASES = [(("quadrant", 3, 4, "HMG-global"), M1, 0.0), (("quadrant", 3, 4, "HMG-global"), M2, 0.0),
                  (("hypercube", 3, 4, "HMG-global"), M2, 0.0), (("hypercube", 4, 2, "HMG-global"), M0, 7.5),
                  (("hypercube", 5, 1, "HMG-global"), M1, 0.0), (("quadrant", 3, 4, "PMG"), M2, 0.0), (("quadrant", 3, 2, "HPMG"), M1, 0.0)]


@pytest.mark.parametrize("case,mask,sigma", TRANSFER_CASES, ids=lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_transfers_vcycle_and_cg(mgamd, oracle, emu, ctx, case, mask, sigma, monkeypatch):
    """restriction and prolongation against the oracle's P^T and P, then the V-cycle and CG; with the default path (fused into the
    operator passes where the level has 17-point bricks: the coarse boundary DoFs are live there) and with separate transfer kernels"""
    h = su.hierarchy(mgamd, ctx, case, Problem(sigma, dirichlet_faces=mask), max_brick=0)
    monkeypatch.setenv("MGAMD_NO_FUSED_TRANSFER", "1")
    h0 = su.hierarchy(mgamd, ctx, case, Problem(sigma, dirichlet_faces=mask), max_brick=0)
    monkeypatch.delenv("MGAMD_NO_FUSED_TRANSFER")
    n_fused = sum(t.n_fused_bricks() for t in h.transfers[1:])
    assert (n_fused > 0) == (case in FUSED) and sum(t.n_fused_bricks() for t in h0.transfers[1:]) == 0
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma, dirichlet_faces=mask))
    for hh, tag in ((h, f"{n_fused} fused bricks"), (h0, "separate transfers")):
        check_transfers(hh, levels, P, f"{case} mask={mask:#04x} {tag}")
        vcycle_and_solve(mgamd, oracle, emu, ctx, hh, levels, P, f"{case} mask={mask:#04x} sigma={sigma} {tag}")


def test_graph_replay_and_kernel_by_kernel(mgamd, oracle, emu, ctx, monkeypatch):
    """hypercube L=4 p=2 under M2: the captured cycle replayed, and the coarse levels kernel by kernel instead of collapsed"""
    case = ("hypercube", 4, 2, "HMG-global")
    h = su.hierarchy(mgamd, ctx, case, Problem(dirichlet_faces=M2), max_brick=0)
    monkeypatch.setenv("MGAMD_COLLAPSE_MAX_DOFS", "0")
    hb = su.hierarchy(mgamd, ctx, case, Problem(dirichlet_faces=M2), max_brick=0)
    monkeypatch.delenv("MGAMD_COLLAPSE_MAX_DOFS")
    assert h.mg.set_collapse(True) > 0 and hb.mg.set_collapse(True) == 0
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(0.0, dirichlet_faces=M2))
    mg, _, _ = vcycle_and_solve(mgamd, oracle, emu, ctx, hb, levels, P, f"{case} M2 kernel by kernel")
    r = np.random.default_rng(12).standard_normal(levels[-1].n)
    vr, vz = h.fine_operator.initialize_dof_vector().from_host(r), h.fine_operator.initialize_dof_vector().from_host(np.full(len(r), np.nan))
    h.mg.time_vcycles(vz, vr, 2, True)
    err = rel_err(vz.to_host(), mg.vcycle(r))
    print(f"{case} M2 graph replay: V-cycle {err:.2e}")
    assert err < TOL_CYCLE


# ------------------------------------------------------------------ coarse solvers
@pytest.mark.parametrize("coarse", ["direct", "cg_with_chebyshev"])
def test_coarse_solvers(mgamd, oracle, emu, ctx, coarse):
    """PMG on quadrant L=3: the p = 1 level is the coarse problem, with hanging nodes and natural faces"""
    case = ("quadrant", 3, 4, "PMG")
    h = su.hierarchy(mgamd, ctx, case, Problem(dirichlet_faces=M2), max_brick=0, coarse_solver=coarse)
    assert h.mg.coarse_solver_used() == coarse
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(0.0, dirichlet_faces=M2))
    if coarse == "direct":
        vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{case} M2 {coarse}")
        return
    mg = emu.with_max_evs(oracle.Multigrid(levels, P, 3, coarse=coarse), [s.eigenvalue_estimates()[1] for s in h.smoothers])
    Lf = levels[-1]
    r = np.random.default_rng(7).standard_normal(Lf.n)
    ez = rel_err(su.apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r))
    xref, itref, _ = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    ex = rel_err(x.to_host(), xref)
    print(f"{case} M2 {coarse}: V-cycle {ez:.2e}, CG iterations {it} (oracle {itref}), iterate {ex:.2e}")
    assert ez < 1e-4 and it == itref and ex < 1e-5  # (an inner CG stops on a tolerance: test_gpu_distributed_sim's bounds)


def test_pmg_with_amg_coarse_solver(mgamd, oracle, ctx):
    """annulus L=6 p=2 PMG under M2 (test_gpu_helmholtz's shape): the p = 1 level is above 4096 DoFs, its coarse solver the
    smoothed-aggregation AMG of the matrix with natural boundary rows; against the oracle's cycle with amg_oracle fed that matrix"""
    import amg_oracle as ao

    case = ("annulus", 6, 2, "PMG")
    h = su.hierarchy(mgamd, ctx, case, Problem(dirichlet_faces=M2), max_brick=0, coarse_n_cycles=2)
    assert h.mg.coarse_solver_used() == "amg"
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(0.0, dirichlet_faces=M2))
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
    print(f"PMG + amg annulus L=6 M2: V-cycle {err:.2e}, CG iterations {it} (oracle {itref}), iterate {rel_err(x.to_host(), xref):.2e}")
    assert err <= TOL_CYCLE and it == itref and rel_err(x.to_host(), xref) <= TOL_SOL


def test_solve_with_amg_follows_the_mesh(mgamd, oracle, ctx):
    """Type "AMG" on quadrant L=3 p=2 under M1: the assembled matrix and the AMG built on it carry the natural rows"""
    import amg_oracle as ao

    geo, L, p = "quadrant", 3, 2
    h = mgamd.Hierarchy(ctx, geo, L, p, "AMG", dirichlet_faces=M1)
    d = h.dofs[0]
    assert d.dirichlet_faces() == M1
    lv = su.oracle_level(d, geo, L, p, Problem(0.0, dirichlet_faces=M1))
    x = np.random.default_rng(4).standard_normal(lv.n)
    assert rel_err(su.apply_nan(mgamd, ctx, h.system_matrix.vmult, x), lv.A @ x) < TOL_OP
    xref, itref, _ = oracle.pcg(lv.A, lv.rhs_constant, ao.SmoothedAggregation(d.matrix()).precondition(1), 1e-4)
    b, xv = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.system_matrix, h.amg, xv, b, 1e-4)
    print(f"Type AMG M1: CG iterations {it} (oracle {itref}), iterate {rel_err(xv.to_host(), xref):.2e}")
    assert it == itref and rel_err(xv.to_host(), xref) < TOL_SOL


# ------------------------------------------------------------------ FP32 levels
def test_float_levels(mgamd, oracle, emu, ctx):
    case = ("quadrant", 3, 4, "HMG-global")
    h = su.hierarchy(mgamd, ctx, case, Problem(dirichlet_faces=M2), max_brick=0, number_type=mgamd.F32)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(0.0, dirichlet_faces=M2))
    rng = np.random.default_rng(21)
    for l, op in enumerate(h.operators):
        lv = levels[l]
        x = rng.standard_normal(lv.n).astype(np.float32).astype(np.float64)
        src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
        op.vmult(dst, src)
        diag = op.initialize_dof_vector()
        op.compute_inverse_diagonal(diag)
        ev, ed = rel_err(dst.to_host(), lv.A @ x), rel_err(diag.to_host(), lv.inv_diag)
        print(f"FP32 level {l} M2: vmult {ev:.2e} inverse diagonal {ed:.2e}")
        assert ev < TOL_F32 and ed < TOL_F32
    mg = oracle.Multigrid(levels, P, 3, coarse="direct")
    mgp = emu.with_max_evs(mg, [s.eigenvalue_estimates()[1] for s in h.smoothers])
    Lf = levels[-1]
    r = rng.standard_normal(Lf.n)
    ref = mgp.vcycle(r)
    e_ref = rel_err(emu.vcycle(mgp, r, np.float32).astype(np.float64), ref)
    err = rel_err(su.apply_nan(mgamd, ctx, h.mg.vmult, r), ref)
    print(f"FP32 V-cycle M2: rel.err {err:.2e}, e_ref {e_ref:.2e}, ratio {err / e_ref:.2f}")
    assert err <= 16 * e_ref
    xref, it64, _ = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    assert it == it64


# ------------------------------------------------------------------ two simulated ranks
@pytest.mark.parametrize("case", [("quadrant", 4, 2, "HMG-global"), ("hypercube", 4, 2, "PMG")], ids=lambda c: "-".join(map(str, c)))
def test_two_simulated_ranks(mgamd, oracle, case, monkeypatch):
    """under M1 cut over two ranks (host threads over the in-process communicator): V-cycle, CG and the flux load against the numpy
    oracle through the DoF keys.  quadrant L=4 p=2 HMG-global has hanging nodes on both kinds of face.  hypercube L=4 p=2 PMG: every
    level lives on the finest mesh and is sharded, the p = 1 level has 4913 DoFs, so the AMG choice runs the sharded geometric
    stand-in ("gmg_vcycle", test_gpu_distributed_sim): the cycle is the oracle's HPMG cycle"""
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")  # the sharded path's start vector hashes the DoF key; the oracle takes the same
    n_ranks, mg_type = 2, case[3]
    ocase = case[:3] + ("HPMG" if mg_type == "PMG" else mg_type,)
    levels, P = su.oracle_hierarchy(None, ocase, Problem(dirichlet_faces=M1))
    omg = oracle.Multigrid(levels, P, 3, coarse="direct", start_vectors=[oracle.key_hash_start_vector(lv) for lv in levels])
    Lf = levels[-1]
    kf = {tuple(int(v) for v in k): i for i, k in enumerate(Lf.keys)}
    r = np.sin(np.arange(Lf.n) * 0.37) + 0.25
    r[Lf.constrained] = 0.0
    zref = omg.vcycle(r)
    xref, itref, _ = oracle.pcg(Lf.A, Lf.rhs_constant, omg.vcycle, 1e-4)
    q = np.array([0.0, 1.5, -2.0, 0.5, 3.0, 1.0])
    qref = po.flux_load(Lf, q)
    group = mgamd.SimGroup(n_ranks)
    out, errs = [None] * n_ranks, [None] * n_ranks

    def rank_main(rk):
        try:
            c = mgamd.Context(0)
            h = mgamd.DistributedHierarchy(c, group.comm(rk), *case[:3], coarse_solver="amg", max_brick=0, min_root_dofs=0,
                                           mg_type=mg_type, dirichlet_faces=M1)
            idx = np.array([kf[tuple(int(v) for v in k)] for k in h.dofs[-1].keys()])
            op = h.fine_operator
            vr, vz = op.initialize_dof_vector().from_host(r[idx]), op.initialize_dof_vector()
            h.mg.vmult(vz, vr)
            b, x, vq = op.initialize_dof_vector(), op.initialize_dof_vector(), op.initialize_dof_vector()
            op.rhs(b)
            op.rhs_boundary_flux(vq, q)
            it, _ = mgamd.solve_cg(op, h.mg, x, b, 1e-4)
            out[rk] = dict(idx=idx, z=vz.to_host(), x=x.to_host(), q=vq.to_host(), it=it, dist=h.distributed[-1],
                           masks=[d.dirichlet_faces() for d in h.dofs], used=h.mg.coarse_solver_used())
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
    seen = {}
    for o in out:
        assert o["dist"] and all(m == M1 for m in o["masks"]) and o["used"] == ("gmg_vcycle" if mg_type == "PMG" else "direct")
        ez, ex = rel_err(o["z"], zref[o["idx"]]), rel_err(o["x"], xref[o["idx"]])
        eq = np.abs(o["q"] - qref[o["idx"]]).max() / np.abs(qref).max()
        print(f"two ranks {mg_type} M1: V-cycle {ez:.2e}, CG iterations {o['it']} (oracle {itref}), iterate {ex:.2e}, flux load {eq:.2e}")
        assert ez < TOL_CYCLE and o["it"] == itref and ex < TOL_SOL and eq < TOL_OP
        for i, v in zip(o["idx"], o["x"]):
            assert seen.setdefault(i, v) == v  # copies of shared DoFs: bitwise identical
    assert len(seen) == Lf.n


# ------------------------------------------------------------------ random octree
def test_random_octree(mgamd, oracle, emu, ctx):
    """mesh M of random_mesh_physics at p = 2 with M2, sigma = 7.5 and the per_family coefficient: operator, mass operator, inverse
    diagonal, V-cycle and CG"""
    name, p, mg_type, field, sigma = "M", 2, "HMG-global", "per_family", 7.5
    t = su.tria_of(mgamd, rp.leaves_of(oracle, name), Problem(coefficient=field))
    h = mgamd.Hierarchy(ctx, t, 0, p, mg_type, coarse_solver="amg", max_brick=0, mass_coefficient=sigma, dirichlet_faces=M2)
    assert t.dirichlet_faces() == M2 and h.dofs[-1].info.n_hanging > 0
    levels, P = su.oracle_hierarchy_on(h.dofs, *rp.level_plan(oracle, name, p, mg_type), Problem(sigma, field, M2))
    lv, op = levels[-1], h.fine_operator
    x = np.random.default_rng(3).standard_normal(lv.n)
    diag = op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
    op.compute_inverse_diagonal(diag)
    ev, em = rel_err(su.apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x), rel_err(su.apply_nan(mgamd, ctx, op.vmult_mass, x), ts.mass_matrix(lv) @ x)
    ed = rel_err(diag.to_host(), lv.inv_diag)
    print(f"random octree {name} p={p} {field} M2 sigma={sigma}: vmult {ev:.2e} vmult_mass {em:.2e} inverse diagonal {ed:.2e}")
    assert ev < TOL_OP and em < TOL_OP and ed < TOL_OP
    vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"random octree {name} p={p} {field} M2 sigma={sigma}")


# ------------------------------------------------------------------ known answer
def _exact(x, planes, values, q, dirichlet_face):
    edges = np.concatenate(([-1.0], planes, [1.0]))
    out = np.zeros_like(x)
    for lo, hi, a in zip(edges[:-1], edges[1:], values):
        out += (np.clip(x, lo, hi) - lo) / a if dirichlet_face == 0 else (hi - np.clip(x, lo, hi)) / a
    return q * out


@pytest.mark.parametrize("dirichlet_face", [0, 1])
@pytest.mark.parametrize("geo,L,p,planes,values", [("quadrant", 3, 2, [0.0], [1.0, 4.0]), ("quadrant", 3, 4, [0.0], [1.0, 4.0]),
                                                   ("hypercube", 2, 3, [-0.5, 0.0], [1.0, 5.0, 0.2])])
def test_layered_wall_known_answer(mgamd, oracle, ctx, geo, L, p, planes, values, dirichlet_face):
    """f = 0, u = 0 on one x face, flux 3 through the opposite one, a constant between planes that are faces of every leaf: the
    exact solution is piecewise linear in x and lies in the FE space.  solve_cg with the multigrid at reltol 1e-12, then distribute:
    only the solver tolerance times the conditioning of these small meshes remains (the host test's figure with a direct solve is
    1e-13)"""
    q = 3.0
    t = mgamd.Triangulation(geo, L)
    h = mgamd.Hierarchy(ctx, t, 0, p, "HMG-global", coarse_solver="amg", max_brick=0, dirichlet_faces=1 << dirichlet_face,
                        coefficient=lambda x, y, z: su.layers(x, planes, values))
    op = h.fine_operator
    b, u = op.initialize_dof_vector(), op.initialize_dof_vector()
    op.rhs_boundary_flux(b, {1 - dirichlet_face: q})
    assert np.abs(b.to_host() - h.dofs[-1].rhs_boundary_flux({1 - dirichlet_face: q})).max() == 0.0
    it, _ = mgamd.solve_cg(op, h.mg, u, b, 1e-12)
    op.distribute(u)
    x = su.oracle_level(h.dofs[-1], geo, L, p).node_positions()[:, 0]
    ref = _exact(x, planes, values, q, dirichlet_face)
    err = np.abs(u.to_host() - ref).max() / np.abs(ref).max()
    print(f"{geo} {L} p={p} layers {values}, Dirichlet face {dirichlet_face}: CG iterations {it}, relative nodal error {err:.2e}")
    assert err <= 1e-8


def test_layered_wall_example_program():
    """bin/layered_wall (examples/layered_wall.cpp, the C++ classes): three layers 1 | 5 | 0.2, flux 3 through x = +1: the face
    temperature is q sum d_i / a_i = 3 (0.5 / 1 + 0.5 / 5 + 1 / 0.2) = 16.8"""
    exe = os.path.join(ROOT, "bin", "layered_wall")
    assert os.path.exists(exe), "bin/layered_wall is missing: make all"
    run = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    m = re.search(r"face temperature computed (\S+) \.\.\. (\S+)\s+analytic (\S+)", run.stdout)
    assert m, run.stdout
    lo, hi, exact = (float(v) for v in m.groups())
    print(run.stdout.strip())
    assert exact == pytest.approx(16.8, rel=1e-14) and abs(lo - exact) <= 1e-8 * exact and abs(hi - exact) <= 1e-8 * exact


# ------------------------------------------------------------------ time stepper
def test_insulated_box_conserves_heat(mgamd, oracle, emu, ctx):
    """M0, f = 0, Crank-Nicolson, five steps on quadrant L=3 p=2 from a random start: the iterates are the oracle stepper's on the
    re-masked level (test_gpu_time_stepping's bound: n steps x 1e-10, equal CG counts at reltol 1e-6), and the total heat 1^T M^ u
    drifts by no more than ten times the oracle stepper's own drift at the same tolerances"""
    case, theta, dt, n_steps, reltol = ("quadrant", 3, 2, "HMG-global"), 0.5, 0.02, 5, 1e-6
    sigma = mgamd.TimeStepper.mass_coefficient(theta, dt)
    h = su.hierarchy(mgamd, ctx, case, Problem(sigma, dirichlet_faces=M0), max_brick=0)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma, dirichlet_faces=M0))
    lv, op = levels[-1], h.fine_operator
    Mh = ts.mass_matrix(lv)
    u0 = np.random.default_rng(17).standard_normal(lv.n)
    u0[lv.constrained] = 0.0
    stepper = mgamd.TimeStepper(op, h.mg, theta, dt)
    mg = emu.with_max_evs(oracle.Multigrid(levels, P, 3, coarse="direct"), [s.eigenvalue_estimates()[1] for s in h.smoothers])
    solve = ts.pcg_solver(oracle, lv, mg.vcycle, reltol)
    one, scale = np.ones(lv.n), np.ones(lv.n) @ (Mh @ np.abs(u0))
    u, uref, its, itref, heat, heat_ref = op.initialize_dof_vector().from_host(u0), u0.copy(), [], [], [one @ (Mh @ u0)], [one @ (Mh @ u0)]
    for n in range(n_steps):
        its.append(stepper.step(u, reltol=reltol)[0])
        uref, it = ts.theta_step(lv, uref, None, None, theta, dt, solve, Mh)
        itref.append(it)
        heat.append(one @ (Mh @ u.to_host()))
        heat_ref.append(one @ (Mh @ uref))
    err = rel_err(u.to_host(), uref)
    drift = np.abs(np.array(heat) - heat[0]).max() / scale
    drift_ref = np.abs(np.array(heat_ref) - heat_ref[0]).max() / scale
    print(f"insulated box {case}: CG iterations {its} (oracle {itref}), iterate {err:.2e}, heat {heat[0]:.6e}, relative drift {drift:.2e} "
          f"(oracle stepper {drift_ref:.2e})")
    assert its == itref and err <= n_steps * TOL_SOL
    assert drift <= 10 * drift_ref


# ------------------------------------------------------------------ refusals
def test_the_singular_operator_is_refused_by_every_solver(mgamd, ctx):
    """mask 0 with sigma = 0: operators, mass products, inverse diagonals and Chebyshev stay available; what solves refuses"""
    singular = "singular: dirichlet_faces mask 0.*sigma = 0"
    t = su.tria(mgamd, "quadrant", 3, Problem(dirichlet_faces=M0))
    d = mgamd.DoFs(t, 2, 0)
    op = mgamd.Operator(ctx, d)
    x = np.random.default_rng(1).standard_normal(d.n_dofs)
    free = np.arange(d.n_dofs) < d.info.n_interior + d.info.n_tail
    y = su.apply_nan(mgamd, ctx, op.vmult, np.where(free, 1.0, 0.0))
    assert np.abs(y[free]).max() <= 1e-12  # the constants are in the kernel
    assert np.isfinite(su.apply_nan(mgamd, ctx, op.vmult_mass, x)).all()
    diag = op.initialize_dof_vector()
    op.compute_inverse_diagonal(diag)
    ch = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
    assert np.isfinite(su.apply_nan(mgamd, ctx, ch.vmult, x)).all()
    for mg_type in ("HMG-global", "PMG", "HPMG", "AMG"):
        with pytest.raises(mgamd.MgamdError, match=singular):
            mgamd.Hierarchy(ctx, "quadrant", 3, 2, mg_type, dirichlet_faces=M0)
    with pytest.raises(mgamd.MgamdError, match=singular):
        mgamd.PreconditionMG(ctx, [op], [None], [ch], "direct")
    with pytest.raises(mgamd.MgamdError, match=singular):
        mgamd.SparseMatrix(ctx, d)
    with pytest.raises(mgamd.MgamdError, match=singular):
        d.amg_setup_info()
    b, v = op.initialize_dof_vector(), op.initialize_dof_vector()
    with pytest.raises(mgamd.MgamdError, match=singular):
        mgamd.solve_cg(op, None, v, b, 1e-4)
    with pytest.raises(mgamd.MgamdError, match=singular):
        mgamd.TimeStepper(op, None, 0.5, 0.02)
    # with a mass term the same mask solves
    h = mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-global", mass_coefficient=7.5, dirichlet_faces=M0)
    h.fine_operator.rhs(b)
    assert mgamd.solve_cg(h.fine_operator, h.mg, v, b, 1e-4)[0] > 0


def test_local_smoothing_and_flux_refusals(mgamd, ctx):
    for mg_type in ("HMG-local", "HPMG-local"):
        with pytest.raises(mgamd.MgamdError, match=f"Type '{mg_type}' with the dirichlet_faces mask 1.*local smoothing"):
            mgamd.Hierarchy(ctx, "quadrant", 3, 2, mg_type, dirichlet_faces=M1)
        with pytest.raises(mgamd.MgamdError, match="local smoothing"):
            mgamd.Hierarchy(ctx, su.tria(mgamd, "quadrant", 3, Problem(dirichlet_faces=M1)), 3, 2, mg_type)
        assert mgamd.Hierarchy(ctx, "quadrant", 3, 2, mg_type, dirichlet_faces=0x3F).n_dofs > 0
    op = mgamd.Operator(ctx, mgamd.DoFs(su.tria(mgamd, "quadrant", 3, Problem(dirichlet_faces=M2)), 2, 0))
    b = op.initialize_dof_vector()
    with pytest.raises(mgamd.MgamdError, match=r"face 3 \(y=\+1\) refused: the face is Dirichlet"):
        op.rhs_boundary_flux(b, {0: 1.0, 3: 2.0})
    op.rhs_boundary_flux(b, {0: 1.0})
    assert np.abs(b.to_host()).max() > 0


# ------------------------------------------------------------------ harness
def test_harness_neumann_faces(mgamd, oracle, ctx, tmp_path):
    """input_0003.json (quadrant, NRefGlobal 3, p = 4, HMG-global) with "NeumannFaces": "135" (mask 0b010101) and MassCoefficient 0:
    the CG count of the Python solve and of the oracle, the value echoed; a local-smoothing Type and the singular combination:
    "not implemented", exit code 1"""
    base = json.load(open(os.path.join(GOLDEN, "input_0003.json")))
    case = (base["GeometryType"], int(base["NRefGlobal"]), int(base["Degree"]), base["Type"])
    assert case == ("quadrant", 3, 4, "HMG-global")
    mask = 0b010101
    f = str(tmp_path / "neumann.json")
    json.dump(dict(base, NeumannFaces="135", MassCoefficient=0), open(f, "w"))
    rc, out, err = run_harness(f)
    assert rc == 0, err
    assert f"NeumannFaces: 135 (dirichlet_faces mask {mask})" in out and "MassCoefficient" not in out
    _, rows = final_table(out)
    number_type = mgamd.F32 if base.get("MGNumberType", "float") == "float" else mgamd.F64
    h = su.hierarchy(mgamd, ctx, case, Problem(dirichlet_faces=mask), max_brick=0, number_type=number_type)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, float(base.get("RelativeTolerance", 1e-4)))
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(0.0, dirichlet_faces=mask))
    itref = oracle.pcg(levels[-1].A, levels[-1].rhs_constant, oracle.Multigrid(levels, P, 3, coarse="direct").vcycle, 1e-4)[1]
    print(f"harness NeumannFaces 135: n_iterations {rows[0]['n_iterations']}, Python solve {it}, oracle {itref}")
    assert int(rows[0]["n_iterations"]) == it == itref
    rc0, out0, _ = run_harness(os.path.join(GOLDEN, "input_0003.json"))
    assert rc0 == 0 and "NeumannFaces" not in out0  # echoed only when set
    for extra in (dict(NeumannFaces="135", Type="HMG-local"), dict(NeumannFaces="135", Type="HPMG-local"),
                  dict(NeumannFaces="012345", MassCoefficient=0), dict(NeumannFaces="6")):
        g = str(tmp_path / "refused.json")
        json.dump(dict(base, **extra), open(g, "w"))
        rc, out, err = run_harness(g)
        assert rc == 1 and "not implemented" in err and "NeumannFaces" in err, (extra, err)
