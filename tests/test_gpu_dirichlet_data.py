"""Non-zero Dirichlet data on the GPU: the lifting kernel (dirichlet_lift_kernel, every degree and both number types), the device
distribute_values, the known answer, the example program, the convective wall with a hot wall, the time stepper with time-dependent
Dirichlet values and a boundary load, two simulated ranks and the refusals.  Oracle: oracle/physics_oracle.py, and
tests/dirichlet_data_oracle.py for the theta steppers; the numpy spaces are shared with every other file through support.py.

Shapes are the smallest that reach every branch of the kernel: quadrant 3 (120 cells) at p = 1, 2, 4 and quadrant 2 (15 cells) at
p = 3, 5, 6, 7, where a cell has more nodes than the workgroup has threads, and the one-cell coarsest level.  Bounds are the
project's: 1e-13 for one kernel in FP64, 2e-6 in FP32, 1e-10 per step of a solver, 1e-14 between two runs of one kernel."""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import dirichlet_data_oracle as do
import physics_oracle as po
import support as su
import time_stepping_oracle as ts
from conftest import ROOT, rel_err
from physics_oracle import ALL, M1, Problem
from support import emu, vec  # noqa: F401

pytestmark = pytest.mark.gpu

TOL_OP, TOL_ORDER, TOL_SOL, TOL_F32 = 1e-13, 1e-14, 1e-10, 2e-6
SIGMA = 7.5


def product(mgamd, L, p, mask, sigma, field=None):
    t = su.tria(mgamd, "quadrant", L, Problem(dirichlet_faces=mask))
    if field is not None:
        t.set_coefficient_function(po.XYZ[field])
    d = mgamd.DoFs(t, p, 0)
    d.set_mass_coefficient(sigma)
    return d


def oracle_level(oracle, L, p, mask, sigma, d, field=None):
    return su.oracle_level(d, "quadrant", L, p, Problem(sigma, field, mask))


def lift(op, g, include_mass=True):
    b = vec(op, np.full(len(g), np.nan))
    op.rhs_dirichlet(b, vec(op, g), include_mass)
    return b.to_host()


def cells_per_workgroup(p):
    return max(1, 256 // (p + 1) ** 3)  # kernels_boundary.hpp dirichlet_cells_per_workgroup


def table_facts(oracle, d, lv, mask):
    """from the exported table: (entries, entries with a hanging flag and a Dirichlet node, cells that lie on two Dirichlet faces)"""
    p, i = d.degree, d.info
    idx, hmask, _ = d.dirichlet_cells()
    first_d = i.n_interior + i.n_tail + i.n_edge
    dn = (idx >= first_d) & (idx < first_d + i.n_dirichlet)
    keys, top = np.array(lv.keys)[:, :3], p << oracle.LMAX
    two = 0
    for row, sel in zip(idx, dn):
        k = keys[row[sel]]
        faces = [f for f in range(6) if (mask >> f) & 1 and int((k[:, f >> 1] == (top if f & 1 else 0)).sum()) >= (p + 1) ** 2]
        two += len(faces) >= 2
    return len(idx), int((((hmask >> 3) != 0) & dn.any(axis=1)).sum()), two


# ------------------------------------------------------------------ the lifting kernel
LIFT_CASES = [(3, 1), (3, 2), (3, 4), (2, 3), (2, 5), (2, 6), (2, 7)]


@pytest.mark.parametrize("L,p", LIFT_CASES)
def test_lift_against_the_oracle(mgamd, oracle, ctx, L, p):
    """The table of every case holds an entry with a hanging flag and a Dirichlet node, and under ALL a cell on two Dirichlet faces
    (the edge and corner case; M1 has one Dirichlet face).  The last workgroup is partial where the kernel packs more than one cell
    (p <= 4) for at least one mask of the degree: quadrant 3 has 98 entries under ALL and 35 under M1, quadrant 2 has 15 and 10,
    against 32, 9, 4, 2 cells per workgroup at p = 1..4 (98 is even: at p = 4 it is M1 that leaves a group half full)."""
    rng = np.random.default_rng(7)
    cpw, partial = cells_per_workgroup(p), []
    for mask in (ALL, M1):
        for field in (None, "octants"):
            d = product(mgamd, L, p, mask, SIGMA, field)
            lv = oracle_level(oracle, L, p, mask, SIGMA, d, field)
            n, n_hanging, n_two = table_facts(oracle, d, lv, mask)
            assert n == po.n_cells_with_dirichlet_dof(lv) and n_hanging >= 1 and (n_two >= 1 or mask == M1)
            partial.append(n % cpw != 0)
            g = rng.standard_normal(lv.n).astype(np.float32).astype(np.float64)
            for number_type, tol in ((mgamd.F64, TOL_OP), (mgamd.F32, TOL_F32)):
                op = mgamd.Operator(ctx, d, number_type)
                for include_mass in (True, False):
                    got, ref = lift(op, g, include_mass), po.lift(lv, g, include_mass)
                    e = rel_err(got, ref)
                    print(f"quadrant {L} p={p} mask={mask:#04x} {field} {'FP64' if number_type == mgamd.F64 else 'FP32'} mass={include_mass}: "
                          f"{n} entries ({n_hanging} hanging with a Dirichlet node, {n_two} on two faces), {cpw} per workgroup, lift {e:.2e}")
                    assert np.isfinite(got).all() and e < tol and np.all(got[lv.constrained] == 0.0)
            # the mass part is what include_mass switches: far above both tolerances, so a kernel that ignored the flag would fail
            assert rel_err(po.lift(lv, g, True), po.lift(lv, g, False)) > 100 * TOL_F32
    assert cpw == 1 or any(partial)


@pytest.mark.parametrize("p", [1, 2])
def test_lift_on_the_one_cell_coarsest_level(mgamd, oracle, ctx, p):
    """quadrant 0 is one cell.  Under ALL at p = 1 every node is Dirichlet and nothing is scattered: the result is 0.  Under M1 (and
    at p = 2, whose centre node is free) it has free rows."""
    for mask in (ALL, M1):
        d = product(mgamd, 0, p, mask, SIGMA)
        lv = oracle_level(oracle, 0, p, mask, SIGMA, d)
        assert d.info.n_cells == 1 and len(d.dirichlet_cells()[0]) == 1
        g = np.random.default_rng(1).standard_normal(lv.n)
        got, ref = lift(mgamd.Operator(ctx, d), g), po.lift(lv, g)
        if mask == ALL and p == 1:
            assert d.info.n_dirichlet == d.n_dofs == 8 and np.all(ref == 0.0) and np.all(got == 0.0)
        else:
            assert np.abs(ref).max() > 0 and rel_err(got, ref) < TOL_OP


def test_mask_zero_host_agreement_and_overwrite(mgamd, oracle, ctx):
    p = 2
    d0 = product(mgamd, 3, p, 0, SIGMA)
    assert len(d0.dirichlet_cells()[0]) == 0
    assert np.all(lift(mgamd.Operator(ctx, d0), np.ones(d0.n_dofs)) == 0.0)  # nothing is launched, the vector is zero-filled
    for mask in (ALL, M1):
        d = product(mgamd, 3, p, mask, SIGMA, "octants")
        op = mgamd.Operator(ctx, d)
        g = np.random.default_rng(3).standard_normal(d.n_dofs)
        for include_mass in (True, False):
            host = d.rhs_dirichlet(g, include_mass)
            b, vg = vec(op, np.full(d.n_dofs, np.nan)), vec(op, g)
            op.rhs_dirichlet(b, vg, include_mass)
            first = b.to_host()
            op.rhs_dirichlet(b, vg, include_mass)  # a second call into the same vector: the lift overwrites
            second = b.to_host()
            e, e2 = rel_err(first, host), rel_err(second, first)
            print(f"quadrant 3 p={p} mask={mask:#04x} mass={include_mass}: device against host {e:.2e}, second call {e2:.2e}")
            assert e < TOL_OP and e2 <= TOL_ORDER
            assert np.array_equal(vg.to_host(), g)


# ------------------------------------------------------------------ distribute_values
@pytest.mark.parametrize("L,p", [(3, 1), (3, 2), (3, 4), (2, 5)])
def test_distribute_values(mgamd, oracle, ctx, L, p):
    rng = np.random.default_rng(11)
    for mask in (ALL, M1):
        d = product(mgamd, L, p, mask, 0.0)
        lv = oracle_level(oracle, L, p, mask, 0.0, d)
        assert d.info.n_hanging > 0
        for number_type, tol in ((mgamd.F64, 1e-15), (mgamd.F32, TOL_F32)):
            op = mgamd.Operator(ctx, d, number_type)
            g = rng.standard_normal(lv.n).astype(np.float32).astype(np.float64)
            x = rng.standard_normal(lv.n).astype(np.float32).astype(np.float64)
            ref = po.distribute_values(lv, x, g)
            x[lv.constrained] = 1e30  # hanging and Dirichlet entries hold garbage beforehand
            vx, vg = vec(op, x), vec(op, g)
            op.distribute_values(vx, vg)
            got = vx.to_host()
            e = rel_err(got, ref)
            print(f"distribute_values quadrant {L} p={p} mask={mask:#04x} {'FP64' if number_type == mgamd.F64 else 'FP32'}: {e:.2e}")
            assert e <= tol and np.array_equal(got[~lv.constrained], x[~lv.constrained]) and np.array_equal(vg.to_host(), g)
            if number_type == mgamd.F64:
                assert np.abs(got - d.distribute_values(x, g)).max() <= 1e-15 * np.abs(ref).max()


@pytest.mark.parametrize("p", [1, 2, 4])
def test_distribute_of_the_gaussian_is_distribute_values(mgamd, oracle, ctx, p):
    """Operator.distribute(x, 1) uploads the Gaussian at the Dirichlet support points and runs the kernels of distribute_values: the
    same bits as distribute_values with those values (read off the host distribute of a zero vector, whose Dirichlet entries are
    exactly them), in both number types.  Quadrant 3 is the smallest mesh with hanging nodes whose parents are Dirichlet DoFs, under
    both masks.  Constrained entries hold NaN beforehand: a row that is not written shows.  Bounds: test_distribute_values'."""
    rng = np.random.default_rng(13)
    for mask in (ALL, M1):
        d = product(mgamd, 3, p, mask, 0.0)
        lv = oracle_level(oracle, 3, p, mask, 0.0, d)
        bd = po.dirichlet_dofs(lv)
        assert d.info.n_hanging > 0 and lv.Ch.tocsr()[np.flatnonzero(lv.hanging)][:, np.flatnonzero(bd)].nnz > 0
        g = d.distribute(np.zeros(lv.n), 1)
        assert np.abs(g[bd]).max() > 0
        x = rng.standard_normal(lv.n).astype(np.float32).astype(np.float64)
        ref = lv.distribute(x, oracle.gaussian_solution)
        x[lv.constrained] = np.nan
        for number_type, tol in ((mgamd.F64, 1e-15), (mgamd.F32, TOL_F32)):
            op = mgamd.Operator(ctx, d, number_type)
            va, vb, v0 = vec(op, x), vec(op, x), vec(op, x)
            op.distribute(va, 1)
            op.distribute_values(vb, vec(op, g))
            op.distribute(v0, 0)
            a, b, zero = va.to_host(), vb.to_host(), v0.to_host()
            e = rel_err(a, ref)
            print(f"distribute(x, 1) quadrant 3 p={p} mask={mask:#04x} {'FP64' if number_type == mgamd.F64 else 'FP32'}: {e:.2e}")
            assert np.isfinite(a).all() and np.array_equal(a, b) and e <= tol
            assert np.array_equal(a[~lv.constrained], x[~lv.constrained])
            assert np.isfinite(zero).all() and np.all(zero[bd] == 0.0)  # kind 0: exact zeros, nothing evaluated


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("p", [1, 2])
def test_linear_function_is_reproduced(mgamd, oracle, ctx, p):
    """g = the nodal values of 1 + 2x - 3y + 0.5z on all six faces, f = 0, sigma = 0: solve_cg with the multigrid at reltol 1e-12, then
    distribute_values; the result is the function at every node, hanging ones included, within test_gpu_boundary's
    test_layered_wall_known_answer bound (1e-8 after a solve at 1e-12; the host test's direct solve holds 1e-12)"""
    h = su.hierarchy(mgamd, ctx, ("quadrant", 3, p, "HMG-global"), Problem(), max_brick=0)
    op, d = h.fine_operator, h.dofs[-1]
    pos = d.node_positions()
    exact = 1.0 + 2.0 * pos[:, 0] - 3.0 * pos[:, 1] + 0.5 * pos[:, 2]
    g, b, u = vec(op, exact), op.initialize_dof_vector(), op.initialize_dof_vector()
    op.rhs_dirichlet(b, g)
    it, _ = mgamd.solve_cg(op, h.mg, u, b, 1e-12)
    op.distribute_values(u, g)
    err = np.abs(u.to_host() - exact).max() / np.abs(exact).max()
    print(f"quadrant 3 p={p}: n_hanging {d.info.n_hanging}, CG iterations {it}, relative nodal error {err:.2e}")
    assert d.info.n_hanging > 0 and err <= 1e-8


def test_heated_wall_example_program():
    """bin/heated_wall (examples/heated_wall.cpp, the C++ classes): three layers 1 | 5 | 0.2 between 300 on x = -1 and 400 on x = +1:
    q = 100 / (0.5 / 1 + 0.5 / 5 + 1 / 0.2) = 100 / 5.6, interface temperatures 300 + 0.5 q and 300 + 0.6 q, under
    test_layered_wall_example_program's bound (1e-8 relative)"""
    exe = os.path.join(ROOT, "bin", "heated_wall")
    assert os.path.exists(exe), "bin/heated_wall is missing: make all"
    run = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    rows = re.findall(r"interface x = (\S+) temperature computed (\S+) \.\.\. (\S+)\s+analytic (\S+)", run.stdout)
    assert len(rows) == 2, run.stdout
    print(run.stdout.strip())
    q = 100.0 / 5.6
    for (x, lo, hi, exact), want in zip(rows, (300.0 + 0.5 * q, 300.0 + 0.6 * q)):
        lo, hi, exact = float(lo), float(hi), float(exact)
        assert exact == pytest.approx(want, rel=1e-11) and abs(lo - exact) <= 1e-8 * exact and abs(hi - exact) <= 1e-8 * exact


# ------------------------------------------------------------------ convective faces
def test_convective_wall_with_a_hot_wall(mgamd, oracle, ctx):
    """beta > 0 on x = +1 with the value T on x = -1 (the face opposite: no DoF is shared) is accepted: the lift is the oracle's, whose
    levels carry the surface matrix (physics_oracle.Level.Braw), and the solve with the load of u_ext is the oracle's direct solve.  beta > 0 on
    y = +1 with x = -1 Dirichlet shares an edge and is refused by name."""
    case, T, u_ext = ("quadrant", 3, 2, "HMG-global"), 350.0, 290.0
    setup = (M1, (0.0, 2.5, 0.0, 0.0, 0.0, 0.0))
    h = su.hierarchy(mgamd, ctx, case, Problem(0.0, None, *setup), max_brick=0)
    op, d = h.fine_operator, h.dofs[-1]
    lv = su.oracle_level(d, "quadrant", 3, 2, Problem(0.0, None, *setup))
    g = d.dirichlet_face_values({0: T})
    ref = po.lift(lv, g)
    e = rel_err(lift(op, g), ref)
    flux = po.flux_load(lv, [0.0, 2.5 * u_ext, 0.0, 0.0, 0.0, 0.0])
    b, q, u = (op.initialize_dof_vector() for _ in range(3))
    op.rhs_dirichlet(b, vec(op, g))
    op.rhs_boundary_flux(q, {1: 2.5 * u_ext})
    b.from_host(b.to_host() + q.to_host())
    it, _ = mgamd.solve_cg(op, h.mg, u, b, 1e-12)
    op.distribute_values(u, vec(op, g))
    uref = po.distribute_values(lv, spla.spsolve(lv.A.tocsc(), ref + flux), g)
    eu = np.abs(u.to_host() - uref).max() / np.abs(uref).max()
    print(f"convective wall with a hot wall: lift {e:.2e}, CG iterations {it}, solution {eu:.2e}, range {uref.min():.3f} .. {uref.max():.3f}")
    assert np.abs(ref).max() > 0 and e < TOL_OP and eu <= 1e-8
    t = su.tria(mgamd, "quadrant", 3, Problem(0.0, None, M1, (0.0, 0.0, 0.0, 0.75, 0.0, 0.0)))
    bad = mgamd.Operator(ctx, mgamd.DoFs(t, 2, 0))
    v, w = bad.initialize_dof_vector(), bad.initialize_dof_vector()
    with pytest.raises(mgamd.MgamdError, match=r"convective face 3 \(y=\+1.*shares an edge with the Dirichlet face 0 \(x=-1\)"):
        bad.rhs_dirichlet(v, w)


# ------------------------------------------------------------------ the time stepper
CASE, THETA, DT, RELTOL = ("quadrant", 3, 2, "HMG-global"), 0.5, 0.02, 1e-6
_stepping = {}


def stepping(mgamd, oracle, emu, ctx, mask):
    """(hierarchy, oracle level, its mass matrix, the oracle's PCG with the multigrid at the product's eigenvalue estimates)"""
    if mask not in _stepping:
        sigma = mgamd.TimeStepper.mass_coefficient(THETA, DT)
        h = su.hierarchy(mgamd, ctx, CASE, Problem(sigma, dirichlet_faces=mask), max_brick=0)
        levels, P = su.oracle_hierarchy(h.dofs, CASE, Problem(sigma, dirichlet_faces=mask))
        mg = emu.with_max_evs(oracle.Multigrid(levels, P, 3, coarse="direct"), [s.eigenvalue_estimates()[1] for s in h.smoothers])
        _stepping[mask] = (h, levels[-1], ts.mass_matrix(levels[-1]), ts.pcg_solver(oracle, levels[-1], mg.vcycle, RELTOL))
    return _stepping[mask]


def linear(pos):
    return 1.0 + 2.0 * pos[:, 0] - 3.0 * pos[:, 1] + 0.5 * pos[:, 2]


def test_stepper_preserves_a_steady_state(mgamd, oracle, emu, ctx):
    """u_I = L with g_old = g_new = L (L linear: K L = 0 on the free rows) stays L over three Crank-Nicolson steps"""
    h, lv, Mh, solve = stepping(mgamd, oracle, emu, ctx, ALL)
    op, n_steps = h.fine_operator, 3
    L = linear(h.dofs[-1].node_positions())
    u0 = np.where(lv.constrained, 0.0, L)
    u, g = vec(op, u0), vec(op, L)
    stepper = mgamd.TimeStepper(op, h.mg, THETA, DT)
    for n in range(n_steps):
        stepper.step(u, reltol=RELTOL, g_old=g, g_new=g)
    got = u.to_host()
    err = rel_err(got, u0)
    print(f"steady state over {n_steps} steps: {err:.2e}")
    assert err <= n_steps * TOL_SOL and np.all(got[lv.constrained] == 0.0)
    op.distribute_values(u, g)
    assert np.abs(u.to_host() - L).max() <= n_steps * TOL_SOL * np.abs(L).max()


def test_stepper_with_time_dependent_values(mgamd, oracle, emu, ctx):
    """g(t) = (1 + t) L on the boundary, f = 0, zero initial data: three steps against the oracle stepper"""
    h, lv, Mh, solve = stepping(mgamd, oracle, emu, ctx, ALL)
    op, n_steps = h.fine_operator, 3
    L = linear(h.dofs[-1].node_positions())
    g = lambda n: (1.0 + n * DT) * L
    u, uref, its, itref = op.initialize_dof_vector(), np.zeros(lv.n), [], []
    stepper = mgamd.TimeStepper(op, h.mg, THETA, DT)
    for n in range(n_steps):
        its.append(stepper.step(u, reltol=RELTOL, g_old=vec(op, g(n)), g_new=vec(op, g(n + 1)))[0])
        uref, it = do.theta_step_data(lv, uref, None, None, g(n), g(n + 1), None, THETA, DT, solve, Mh)
        itref.append(it)
    err = rel_err(u.to_host(), uref)
    print(f"time-dependent values: CG iterations {its} (oracle {itref}), iterate {err:.2e}, |u| {np.linalg.norm(uref):.3e}")
    assert its == itref and err <= n_steps * TOL_SOL and np.linalg.norm(uref) > 0


def test_stepper_with_a_boundary_load_and_a_source(mgamd, oracle, emu, ctx):
    """M1: values (1 + t) L on x = -1, the flux load of the natural face x = +1 and a source, three steps against the oracle stepper"""
    h, lv, Mh, solve = stepping(mgamd, oracle, emu, ctx, M1)
    op, n_steps = h.fine_operator, 3
    L = linear(h.dofs[-1].node_positions())
    g = lambda n: (1.0 + n * DT) * L
    f = lambda n: (1.0 + n * DT) * (np.sin(0.37 * np.arange(lv.n)) + 0.25)
    load = op.initialize_dof_vector()
    op.rhs_boundary_flux(load, {1: 1.5})
    lref = po.flux_load(lv, [0.0, 1.5, 0.0, 0.0, 0.0, 0.0])
    assert rel_err(load.to_host(), lref) < TOL_OP
    u0 = np.random.default_rng(17).standard_normal(lv.n)
    u0[lv.constrained] = 0.0
    u, uref, its, itref = vec(op, u0), u0.copy(), [], []
    stepper = mgamd.TimeStepper(op, h.mg, THETA, DT)
    for n in range(n_steps):
        its.append(stepper.step(u, vec(op, f(n)), vec(op, f(n + 1)), reltol=RELTOL, g_old=vec(op, g(n)), g_new=vec(op, g(n + 1)), load=load)[0])
        uref, it = do.theta_step_data(lv, uref, f(n), f(n + 1), g(n), g(n + 1), lref, THETA, DT, solve, Mh)
        itref.append(it)
    err = rel_err(u.to_host(), uref)
    print(f"boundary load and source: CG iterations {its} (oracle {itref}), iterate {err:.2e}")
    assert its == itref and err <= n_steps * TOL_SOL


def test_step_data_without_data_is_the_old_step(mgamd, oracle, emu, ctx):
    """mgamd_time_stepper_step and mgamd_time_stepper_step_data with NULL g_old, g_new and load run the same launches: the same bits
    wherever the old step repeats its own bits from run to run (its atomic sums need not), and TOL_ORDER otherwise"""
    h, lv, Mh, solve = stepping(mgamd, oracle, emu, ctx, ALL)
    op = h.fine_operator
    u0 = np.random.default_rng(17).standard_normal(lv.n)
    f0, f1 = vec(op, np.sin(0.37 * np.arange(lv.n))), vec(op, np.cos(0.11 * np.arange(lv.n)))

    def run(entry):
        stepper, u = mgamd.TimeStepper(op, h.mg, THETA, DT), vec(op, u0)
        it, res = C.c_uint(), C.c_double()
        args = (C.c_double(RELTOL), C.c_double(1e-20), 10000, C.byref(it), C.byref(res))
        if entry == "step":
            mgamd._chk(mgamd._lib.mgamd_time_stepper_step(stepper._h, u._h, f0._h, f1._h, *args))
        else:
            mgamd._chk(mgamd._lib.mgamd_time_stepper_step_data(stepper._h, u._h, f0._h, f1._h, None, None, None, *args))
        return u.to_host(), it.value

    (a, ita), (a2, _), (b, itb) = run("step"), run("step"), run("step_data")
    repeats = np.array_equal(a, a2)
    print(f"step against step_data with NULL data: iterations {ita} / {itb}, the old step repeats its bits: {repeats}, "
          f"difference {rel_err(b, a):.2e}")
    assert ita == itb and (np.array_equal(a, b) if repeats else rel_err(b, a) <= TOL_ORDER)


# ------------------------------------------------------------------ two simulated ranks
def test_two_simulated_ranks(mgamd, oracle, ctx, monkeypatch):
    """quadrant 3 p=2 under M1 cut over two ranks (host threads over the in-process communicator): the lift and one stepper step
    against the one-rank result"""
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")  # a start vector of the smoothers' eigenvalue estimate that does not depend on the numbering
    n_ranks, sigma = 2, mgamd.TimeStepper.mass_coefficient(THETA, DT)
    h1 = su.hierarchy(mgamd, ctx, CASE, Problem(sigma, dirichlet_faces=M1), max_brick=0)
    op1, d1 = h1.fine_operator, h1.dofs[-1]
    kf = {tuple(int(v) for v in k): i for i, k in enumerate(d1.keys())}
    rng = np.random.default_rng(23)
    g0, g1, u0 = rng.standard_normal(d1.n_dofs), rng.standard_normal(d1.n_dofs), rng.standard_normal(d1.n_dofs)
    lift1 = lift(op1, g0)
    u = vec(op1, u0)
    it1 = mgamd.TimeStepper(op1, h1.mg, THETA, DT).step(u, reltol=RELTOL, g_old=vec(op1, g0), g_new=vec(op1, g1))[0]
    step1 = u.to_host()
    group = mgamd.SimGroup(n_ranks)
    out, errs = [None] * n_ranks, [None] * n_ranks

    def rank_main(rk):
        try:
            c = mgamd.Context(0)
            h = mgamd.DistributedHierarchy(c, group.comm(rk), *CASE[:3], coarse_solver="amg", max_brick=0, min_root_dofs=0, mg_type=CASE[3],
                                           mass_coefficient=sigma, dirichlet_faces=M1)
            idx = np.array([kf[tuple(int(v) for v in k)] for k in h.dofs[-1].keys()])
            op = h.fine_operator
            y = lift(op, g0[idx])
            v = vec(op, u0[idx])
            it = mgamd.TimeStepper(op, h.mg, THETA, DT).step(v, reltol=RELTOL, g_old=vec(op, g0[idx]), g_new=vec(op, g1[idx]))[0]
            out[rk] = dict(idx=idx, y=y, u=v.to_host(), it=it, dist=h.distributed[-1], n_table=len(h.dofs[-1].dirichlet_cells()[0]))
        except BaseException as e:  # noqa
            errs[rk] = e

    th = [threading.Thread(target=rank_main, args=(rk,)) for rk in range(n_ranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th)
    for e in errs:
        if e is not None:
            raise e
    assert sum(o["n_table"] for o in out) == len(d1.dirichlet_cells()[0])
    for o in out:
        assert o["dist"] and o["n_table"] > 0
        ey, eu = rel_err(o["y"], lift1[o["idx"]]), rel_err(o["u"], step1[o["idx"]])
        print(f"two ranks: {o['n_table']} table entries, lift {ey:.2e}, CG iterations {o['it']} (one rank {it1}), iterate {eu:.2e}")
        assert ey <= TOL_OP and o["it"] == it1 and eu <= TOL_SOL


# ------------------------------------------------------------------ refusals
def test_refusals(mgamd, ctx):
    sigma = mgamd.TimeStepper.mass_coefficient(THETA, DT)
    h = su.hierarchy(mgamd, ctx, CASE, Problem(sigma, dirichlet_faces=ALL), max_brick=0)
    op, n = h.fine_operator, h.n_dofs
    g, b = vec(op, np.ones(n)), op.initialize_dof_vector()
    with pytest.raises(mgamd.MgamdError, match="rhs_dirichlet: vector size mismatch"):
        op.rhs_dirichlet(mgamd.Vector(ctx, n + 1), g)
    with pytest.raises(mgamd.MgamdError, match="rhs_dirichlet: vector size mismatch"):
        op.rhs_dirichlet(b, mgamd.Vector(ctx, n - 1))
    with pytest.raises(mgamd.MgamdError, match="number type"):
        op.rhs_dirichlet(b, mgamd.Vector(ctx, n, mgamd.F32))
    with pytest.raises(mgamd.MgamdError, match="rhs and g must differ"):
        op.rhs_dirichlet(g, g)
    with pytest.raises(mgamd.MgamdError, match="distribute_values: vector size mismatch"):
        op.distribute_values(b, mgamd.Vector(ctx, n + 1))
    stepper = mgamd.TimeStepper(op, h.mg, THETA, DT)
    u0 = np.random.default_rng(1).standard_normal(n)
    u = vec(op, u0)
    with pytest.raises(mgamd.MgamdError, match="exactly one of g_old / g_new"):
        stepper.step(u, g_old=g)
    with pytest.raises(mgamd.MgamdError, match="exactly one of g_old / g_new"):
        stepper.step(u, g_new=g)
    with pytest.raises(mgamd.MgamdError, match="entries"):
        stepper.step(u, g_old=g, g_new=mgamd.Vector(ctx, n + 1))
    with pytest.raises(mgamd.MgamdError, match="entries"):
        stepper.step(u, load=mgamd.Vector(ctx, n, mgamd.F32))
    assert np.array_equal(u.to_host(), u0) and stepper.time() == 0.0 and stepper.n_steps() == 0
    # the operator of a local-smoothing level is refused by name; the active-mesh operator of that hierarchy works
    hl = mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-local")
    lop = hl.operators[-1]
    with pytest.raises(mgamd.MgamdError, match="rhs_dirichlet: refused on the level of a local-smoothing hierarchy"):
        lop.rhs_dirichlet(lop.initialize_dof_vector(), lop.initialize_dof_vector())
    with pytest.raises(mgamd.MgamdError, match="distribute_values: refused on the level of a local-smoothing hierarchy"):
        lop.distribute_values(lop.initialize_dof_vector(), lop.initialize_dof_vector())
    a = hl.fine_operator
    y = lift(a, np.ones(hl.n_dofs), False)
    assert np.isfinite(y).all() and np.abs(y).max() > 0.0
