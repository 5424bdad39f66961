"""Mass term, diffusion coefficient and mass operator on caller-built RANDOM octrees with coefficient fields that differ from brick
to brick: A = K_a + sigma M through the operators of every level, Chebyshev, V-cycle and CG (HMG-global, PMG, HPMG), FP32 levels,
the theta time stepper and simulated ranks, against the numpy oracle on the same leaves (oracle/physics_oracle.py).

Why these fields.  The kernels that hold several slots in one workgroup (three 2^3 families, four wave-scoped cells, the p = 1
pair and cluster launches, the per-slot D^-1 table of the persistent kernels) read the scale a h and the ratio h^2 / a by the slot
of the line.  A wrong slot index there reads in bounds and only changes numbers, and it is invisible whenever the slots that share a
workgroup carry the same a and h: uniform and octants give long runs of equal slots, inclusion differs at one box, per_cell splits
every brick.  per_family keeps the 2^3 bricks and gives every family its own value, per_block4 does so for aligned 4^3 blocks, and
on a random octree consecutive slots also differ in the cell level.  assert_slots_differ computes that from the tables of every
case and asserts it.

Meshes S, M, B, R: random_mesh_physics.  sigma in {0, 7.5, 3000}.  Bounds are the project's (support.py): operator
<= 1e-13, Chebyshev <= 1e-12, V-cycle <= 1e-11, CG iterates <= 1e-10 with equal iteration counts, FP32 single kernels <= 2e-6, FP32
V-cycle <= 16 e_ref (oracle/f32_emulation.py on the test's own levels) and <= 5e-5.  Every constraint search is made once per
session (support.py)."""
import numpy as np
import pytest

import physics_oracle as po
import random_mesh_physics as rm
import support as su
import time_stepping_oracle as ts
from conftest import rel_err
from physics_oracle import Problem
from support import (TOL_CHEB, TOL_CYCLE, TOL_F32, TOL_OP, TOL_SOL, apply_nan, assert_level_coefficients, emu, key_vector, keyset,  # noqa: F401
                     linear_source, oracle_steps, run_ranks, run_steps)

pytestmark = pytest.mark.gpu

SIGMAS = [0.0, 7.5, 3000.0]


def oracle_hierarchy(oracle, name, p, mg_type, field, sigma, dofs):
    return su.oracle_hierarchy_on(dofs, *rm.level_plan(oracle, name, p, mg_type), Problem(sigma, field))


def hierarchy(mgamd, ctx, oracle, name, p, mg_type, field, sigma, **kw):
    t = su.tria_of(mgamd, rm.leaves_of(oracle, name), Problem(coefficient=field))
    h = mgamd.Hierarchy(ctx, t, None, p, mg_type, coarse_solver="amg", max_brick=0, mass_coefficient=sigma, **kw)
    assert h.mg.coarse_solver_used() == "direct"
    return h


# ------------------------------------------------------------------ (a) the operator trio on every level
# S holds one family per octant, so octants gives its tables what per_family gives them (five 2^3 bricks with five values): all four
# fields at p = 5, the two that differ in the slots at p = 6, 7, where one oracle level costs several seconds per field
OP_CASES = ([("S", 5, f, 0) for f in (None, "per_family", "per_cell", "octants")]
            + [("S", p, f, 0) for p in (6, 7) for f in ("per_family", "per_cell")]
            + [("M", p, f, 0) for p in (1, 2, 3, 4) for f in (None, "per_family", "per_cell", "octants")]
            + [("M", p, "per_family", 1) for p in (1, 2, 3, 4)]  # max_brick = 1: single cells only, the wave-scoped cell kernel
            + [("B", p, f, 0) for p in (1, 2, 3) for f in (None, "per_family", "per_cell", "octants")]
            + [("B", p, "per_block4", 0) for p in (1, 2)]
            + [("R", p, f, 0) for p in (1, 2) for f in ("uniform", "octants", "per_block4")])


@pytest.mark.parametrize("name,p,field,max_brick", OP_CASES)
def test_operator_trio_on_every_level(mgamd, oracle, ctx, name, p, field, max_brick):
    """vmult, compute_inverse_diagonal and vmult_mass on EVERY level of the HMG-global hierarchy (the coarse levels carry restricted,
    mixed coefficients), each twice into a NaN-prefilled destination; vmult_mass against C^T Mraw C"""
    fine = su.tria_of(mgamd, rm.leaves_of(oracle, name), Problem(coefficient=field))
    seq = mgamd.create_geometric_coarsening_sequence(fine)
    dofs = [mgamd.DoFs(t, p, max_brick) for t in seq]
    if max_brick == 0:
        rm.assert_slots_differ(mgamd, name, p, field, dofs[-1], fine)
    else:
        assert {B for B, n in dofs[-1].groups() if n} == {1}
    levels0, _ = oracle_hierarchy(oracle, name, p, "HMG-global", field, 0.0, dofs)
    if field is not None:
        for t, d, lv in zip(seq, dofs, levels0):
            assert np.abs(t.coefficient() / po.product_values(t, lv.coefficient) - 1.0).max() <= 1e-15
            assert d.coefficient_range() == (t.coefficient().min(), t.coefficient().max())
    rng = np.random.default_rng(3)
    worst = dict(vmult=0.0, diag=0.0, mass=0.0)
    for l, (d, lv0) in enumerate(zip(dofs, levels0)):
        M, c = ts.mass_matrix(lv0), lv0.constrained
        for sigma in SIGMAS:
            d.set_mass_coefficient(sigma)
            op = mgamd.Operator(ctx, d)
            lv = lv0 if sigma == 0.0 else po.changed(lv0, sigma=sigma)
            for trial in range(2):  # twice: a dirty tail accumulator shows in the second pass
                x = rng.standard_normal(lv.n)
                ev = rel_err(apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x)
                diag = op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
                op.compute_inverse_diagonal(diag)
                ed = rel_err(diag.to_host(), lv.inv_diag)
                y = apply_nan(mgamd, ctx, op.vmult_mass, x)
                em = rel_err(y, M @ x)
                print(f"{name} p={p} {field} max_brick={max_brick} level {l} ({lv.n} DoFs) sigma={sigma} pass {trial}: vmult {ev:.2e}, "
                      f"inverse diagonal {ed:.2e}, vmult_mass {em:.2e}")
                worst = dict(vmult=max(worst["vmult"], ev), diag=max(worst["diag"], ed), mass=max(worst["mass"], em))
                assert ev < TOL_OP and ed < TOL_OP and em <= TOL_OP
                assert (y[c] == 0.0).all()
    print(f"{name} p={p} {field} max_brick={max_brick}: worst over {len(dofs)} levels {worst}")


# ------------------------------------------------------------------ (b) Chebyshev
# R p = 1 under octants: two plain 8^3 bricks with different a in one workgroup of the 9-point lattice kernel, whose Chebyshev
# modes tabulate D^-1 per slot from h^2 / a
@pytest.mark.parametrize("name,p,field", [("M", p, "per_family") for p in (1, 2, 3, 4)] + [("S", 5, "per_family"), ("S", 7, "per_family"),
                                          ("R", 1, "octants")])
@pytest.mark.parametrize("sigma", [0.0, 7.5])
def test_chebyshev(mgamd, oracle, ctx, name, p, field, sigma):
    t = su.tria_of(mgamd, rm.leaves_of(oracle, name), Problem(coefficient=field))
    d = mgamd.DoFs(t, p, 0)
    rm.assert_slots_differ(mgamd, name, p, field, d, t)
    d.set_mass_coefficient(sigma)
    op = mgamd.Operator(ctx, d)
    lv = su.oracle_level_on(d, rm.leaves_of(oracle, name), p, Problem(sigma, field))
    ch = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
    ref = oracle.Chebyshev(lv.A, lv.inv_diag, 3, 20.0, 20)
    assert ch.eigenvalue_estimates()[1] == pytest.approx(ref.max_ev, rel=1e-10)
    rng = np.random.default_rng(5)
    b, x0 = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
    ev = rel_err(apply_nan(mgamd, ctx, ch.vmult, b), ref.vmult(b))
    vb, vx = op.initialize_dof_vector().from_host(b), op.initialize_dof_vector().from_host(x0)
    ch.step(vx, vb)
    es = rel_err(vx.to_host(), ref.step(x0, b))
    print(f"chebyshev {name} p={p} {field} sigma={sigma}: vmult {ev:.2e} step {es:.2e}")
    assert ev < TOL_CHEB and es < TOL_CHEB


# ------------------------------------------------------------------ (c) V-cycle and CG
# R p = 1 under octants: the smoothers of the finest level run the 9-point lattice kernel's Chebyshev modes on two bricks per workgroup
VCYCLE_CASES = ([(n, p, t, f) for n, p, t in (("M", 4, "HMG-global"), ("M", 4, "PMG"), ("M", 4, "HPMG"), ("B", 3, "HMG-global"), ("S", 6, "HPMG"))
                 for f in ("per_family", "inclusion")] + [("R", 1, "HMG-global", "octants")])


@pytest.mark.parametrize("name,p,mg_type,field", VCYCLE_CASES)
@pytest.mark.parametrize("sigma", [0.0, 7.5])
def test_vcycle_and_cg(mgamd, oracle, emu, ctx, name, p, mg_type, field, sigma):
    h = hierarchy(mgamd, ctx, oracle, name, p, mg_type, field, sigma)
    if field == "inclusion":
        assert h.dofs[-1].coefficient_range() == (1.0, 1000.0)
    else:
        rm.assert_slots_differ(mgamd, name, p, field, h.dofs[-1], h.trias[-1])
    levels, P = oracle_hierarchy(oracle, name, p, mg_type, field, sigma, h.dofs)
    assert_level_coefficients(h, levels)
    su.vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, f"{name} p={p} {mg_type} {field} sigma={sigma}")


# ------------------------------------------------------------------ (d) FP32 levels
@pytest.mark.parametrize("name,p", [("M", 4), ("S", 5)])
def test_float_levels(mgamd, oracle, emu, ctx, name, p):
    field, sigma = "per_family", 7.5
    h = hierarchy(mgamd, ctx, oracle, name, p, "HMG-global", field, sigma, number_type=mgamd.F32)
    rm.assert_slots_differ(mgamd, name, p, field, h.dofs[-1], h.trias[-1])
    levels, P = oracle_hierarchy(oracle, name, p, "HMG-global", field, sigma, h.dofs)
    assert_level_coefficients(h, levels)
    rng = np.random.default_rng(21)
    for l, op in enumerate(h.operators):
        lv = levels[l]
        x = rng.standard_normal(lv.n).astype(np.float32).astype(np.float64)
        src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
        op.vmult(dst, src)
        diag = op.initialize_dof_vector()
        op.compute_inverse_diagonal(diag)
        dmass = op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
        op.vmult_mass(dmass, src)
        ev, ed, em = rel_err(dst.to_host(), lv.A @ x), rel_err(diag.to_host(), lv.inv_diag), rel_err(dmass.to_host(), ts.mass_matrix(lv) @ x)
        print(f"FP32 {name} p={p} level {l} {field} sigma={sigma}: vmult {ev:.2e} inverse diagonal {ed:.2e} vmult_mass {em:.2e}")
        assert ev < TOL_F32 and ed < TOL_F32 and em <= TOL_F32
    mg = oracle.Multigrid(levels, P, 3, coarse="direct")
    mgp = emu.with_max_evs(mg, [s.eigenvalue_estimates()[1] for s in h.smoothers])
    Lf = levels[-1]
    r = rng.standard_normal(Lf.n)
    ref = mgp.vcycle(r)
    e_ref = rel_err(emu.vcycle(mgp, r, np.float32).astype(np.float64), ref)
    err = rel_err(apply_nan(mgamd, ctx, h.mg.vmult, r), ref)
    print(f"FP32 V-cycle {name} p={p} {field} sigma={sigma}: rel.err {err:.2e}, e_ref {e_ref:.2e}, ratio {err / e_ref:.2f}")
    assert err <= 16 * e_ref
    assert rel_err(apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r)) < 5e-5
    _, it64, _ = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    _, it32, _ = oracle.pcg(Lf.A, Lf.rhs_constant, lambda v: emu.vcycle(mg, v, np.float32).astype(np.float64), 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    print(f"FP32 CG {name} p={p} {field} sigma={sigma}: iterations {it}, float32 emulation {it32}, FP64 oracle {it64}")
    assert it == it32  # test_gpu_float_levels.test_cg_iteration_count_of_the_emulated_cycle


# ------------------------------------------------------------------ (e) the time stepper
@pytest.mark.parametrize("theta,n_steps", [(0.5, 2), (1.0, 1)])
def test_time_stepper(mgamd, oracle, emu, ctx, theta, n_steps):
    """Crank-Nicolson and implicit Euler steps with a source term on M p = 2 under per_family; test_gpu_time_stepping.test_source_term"""
    name, p, field, dt, reltol = "M", 2, "per_family", 0.02, 1e-6
    sigma = mgamd.TimeStepper.mass_coefficient(theta, dt)
    h = hierarchy(mgamd, ctx, oracle, name, p, "HMG-global", field, sigma)
    rm.assert_slots_differ(mgamd, name, p, field, h.dofs[-1], h.trias[-1])
    levels, P = oracle_hierarchy(oracle, name, p, "HMG-global", field, sigma, h.dofs)
    assert_level_coefficients(h, levels)
    lv = levels[-1]
    u0 = np.random.default_rng(17).standard_normal(lv.n)
    u0[lv.constrained] = 0.0
    f = linear_source(lv.n, dt)
    u, its = run_steps(mgamd, h, mgamd.TimeStepper(h.fine_operator, h.mg, theta, dt), u0, n_steps, reltol, f)
    uref, itref = oracle_steps(oracle, lv, su.injected(emu, oracle, levels, P, h).vcycle, u0, theta, dt, n_steps, reltol, f)
    err = rel_err(u, uref)
    print(f"time stepper {name} p={p} {field} theta={theta}: CG iterations {its} (oracle {itref}), iterate {err:.2e}")
    assert its == itref
    assert err <= n_steps * TOL_SOL


# ------------------------------------------------------------------ (f) simulated ranks
@pytest.mark.parametrize("name,p,n_ranks", [("M", 4, 2), ("B", 2, 3)])
def test_simulated_ranks(mgamd, oracle, name, p, n_ranks, monkeypatch):
    """the sharded path (test_gpu_random_meshes.test_random_octree_sharded) under per_family and sigma = 7.5: the halo-first slot
    permutation of the local tables carries a and h^2 / a with the slot"""
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")  # numbering-independent Chebyshev start vector (the sharded path has no global index)
    field, sigma = "per_family", 7.5
    leaves = rm.leaves_of(oracle, name)
    levels, P = oracle_hierarchy(oracle, name, p, "HMG-global", field, sigma, None)
    omg = oracle.Multigrid(levels, P, 3, coarse="direct", start_vectors=[oracle.key_hash_start_vector(lv) for lv in levels])
    Lf = levels[-1]
    kf = {tuple(int(v) for v in k): i for i, k in enumerate(Lf.keys)}
    r = key_vector(Lf.keys, 2)
    r[Lf.constrained] = 0.0
    zref = omg.vcycle(r)
    xref, itref, _ = oracle.pcg(Lf.A, Lf.rhs_constant, omg.vcycle, 1e-4)
    sim = mgamd.SimGroup(n_ranks)

    def rank_main(rk):
        c = mgamd.Context(0)
        h = mgamd.DistributedHierarchy(c, sim.comm(rk), su.tria_of(mgamd, leaves, Problem(coefficient=field)), None, p, coarse_solver="amg", max_brick=0,
                                       min_root_dofs=0, min_subset_dofs=0, mass_coefficient=sigma)
        idx = np.array([kf[k] for k in keyset(h.dofs[-1].keys())])
        op = h.fine_operator
        vr, vz = op.initialize_dof_vector().from_host(r[idx]), op.initialize_dof_vector()
        h.mg.vmult(vz, vr)
        b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
        op.rhs(b)
        it, _ = mgamd.solve_cg(op, h.mg, x, b, 1e-4)
        return dict(idx=idx, z=vz.to_host(), x=x.to_host(), it=it, n_dofs=h.n_dofs, layout=h.layout(), groups=h.dofs[-1].groups(),
                    rng=h.dofs[-1].coefficient_range())

    for rk, o in enumerate(run_ranks(n_ranks, rank_main)):
        assert o["n_dofs"] == Lf.n and o["layout"][-1] == n_ranks
        ez, ex = rel_err(o["z"], zref[o["idx"]]), rel_err(o["x"], xref[o["idx"]])
        print(f"{name} p={p} rank {rk} of {n_ranks} {field}: slot groups (B, slots) {o['groups']}, a in {o['rng']}; V-cycle {ez:.2e}, "
              f"CG iterations {o['it']} (oracle {itref}), iterate {ex:.2e}")
        assert sum(n for B, n in o["groups"] if B == 2) >= 2 and o["rng"][0] < o["rng"][1]  # local families with different values
        assert ez < TOL_CYCLE
        assert o["it"] == itref
        assert ex < TOL_SOL
