"""The mass operator (Operator.vmult_mass, kernel mode MODE_MASS) and the theta time stepper (TimeStepper) on the GPU against
the numpy oracle tests/time_stepping_oracle.py, which tests/test_time_stepping_host.py pins first.

Bounds are the project's own: operator <= 1e-13, FP32 single kernels <= 2e-6, summation order (atomics) 1e-14, CG iterates
<= 1e-10 per solve with equal iteration counts at reltol 1e-6.  n steps are held to n x 1e-10: a theta step does not amplify
for theta >= 1/2.  The eigenmode runs stop at reltol 1e-10, where no test of the project pins counts: there the counts are held to
+-1 of the oracle's and the result to 1e-9 = reltol x 5 steps x 2 (residual against iterate), as in the host test.

Shapes: support.OP_CASES reach every kernel family the launch plan can choose; the numpy levels come from support.py (the mass
matrix does not depend on sigma)."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import physics_oracle as po
import support as su
import time_stepping_oracle as ts
from conftest import ROOT, rel_err
from physics_oracle import Problem
from support import OP_CASES, apply_nan, emu, injected, linear_source, oracle_steps, run_steps, vec  # noqa: F401

pytestmark = pytest.mark.gpu

TOL_OP, TOL_ORDER, TOL_SOL, TOL_F32 = 1e-13, 1e-14, 1e-10, 2e-6
_eig = {}


def level_and_mass(oracle, geo, L, p, d):
    """the oracle level numbered like d (any sigma) and its mass matrix"""
    lv = su.oracle_level(d, geo, L, p, Problem(7.5))
    return lv, ts.mass_matrix(lv)


# ------------------------------------------------------------------ the mass operator
@pytest.mark.parametrize("geo,L,p,max_brick", OP_CASES)
def test_vmult_mass(mgamd, oracle, ctx, geo, L, p, max_brick):
    d = mgamd.DoFs(mgamd.Triangulation(geo, L), p, max_brick)
    lv, M = level_and_mass(oracle, geo, L, p, d)
    c = lv.constrained
    rng = np.random.default_rng(3)
    outs = {}
    for sigma in (0.0, 7.5):
        d.set_mass_coefficient(sigma)
        op = mgamd.Operator(ctx, d)
        A = po.changed(lv, sigma=sigma).A
        x = np.random.default_rng(3).standard_normal(lv.n)
        for trial in range(2):  # twice in a row: the accumulator is left clean
            y = apply_nan(mgamd, ctx, op.vmult_mass, x)
            err = rel_err(y, M @ x)
            print(f"vmult_mass {geo} L={L} p={p} max_brick={max_brick} sigma={sigma} pass {trial}: rel.err {err:.2e}")
            assert err <= TOL_OP
            assert (y[c] == 0.0).all()
        outs[sigma] = y
        xd = x.copy()
        xd[c] = 1e30  # constrained input entries are never read
        yd = apply_nan(mgamd, ctx, op.vmult_mass, xd)
        assert rel_err(yd, y) <= TOL_ORDER and (yd[c] == 0.0).all()
        # vmult, vmult_mass, vmult interleaved
        x2 = rng.standard_normal(lv.n)
        for fn, ref in ((op.vmult, A @ x2), (op.vmult_mass, M @ x2), (op.vmult, A @ x2)):
            assert rel_err(apply_nan(mgamd, ctx, fn, x2), ref) <= TOL_OP
    assert rel_err(outs[0.0], outs[7.5]) <= TOL_ORDER  # sigma plays no role (bitwise but for the order of the atomic sums)


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 4), ("hypercube", 4, 1)])
def test_mass_symmetry(mgamd, oracle, ctx, geo, L, p):
    d = mgamd.DoFs(mgamd.Triangulation(geo, L), p, 0)
    op = mgamd.Operator(ctx, d)
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(d.n_dofs), rng.standard_normal(d.n_dofs)
    Mx, My = apply_nan(mgamd, ctx, op.vmult_mass, x), apply_nan(mgamd, ctx, op.vmult_mass, y)
    a, b = y @ Mx, x @ My
    print(f"mass symmetry {geo} L={L} p={p}: y.Mx {a:.15e} x.My {b:.15e}, x.Mx {x @ Mx:.3e}")
    assert abs(a - b) <= 1e-13 * abs(a)
    assert x @ Mx > 0.0 and y @ My > 0.0


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 4), ("hypercube", 4, 1), ("quadrant", 2, 7)])
def test_vmult_mass_float(mgamd, oracle, ctx, geo, L, p):
    d = mgamd.DoFs(mgamd.Triangulation(geo, L), p, 0)
    lv, M = level_and_mass(oracle, geo, L, p, d)
    op = mgamd.Operator(ctx, d, mgamd.F32)
    x = np.random.default_rng(3).standard_normal(lv.n).astype(np.float32).astype(np.float64)
    src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector().from_host(np.full(lv.n, np.nan))
    for trial in range(2):
        op.vmult_mass(dst, src)
        y = dst.to_host()
        err = rel_err(y, M @ x)
        print(f"FP32 vmult_mass {geo} L={L} p={p} pass {trial}: rel.err {err:.2e}")
        assert err <= TOL_F32 and (y[lv.constrained] == 0.0).all()
    assert np.array_equal(src.to_host(), x)


# ------------------------------------------------------------------ the stepper
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("case", [("hypercube", 2, 2, "HMG-global"), ("quadrant", 3, 2, "HMG-global"), ("quadrant", 3, 4, "HMG-global"),
                                  ("quadrant", 3, 4, "PMG")], ids=lambda c: "-".join(map(str, c)))
def test_eigenmode_decay(mgamd, oracle, emu, ctx, case, theta):
    geo, L, p, mg_type = case
    dt, n_steps, reltol = 0.01, 5, 1e-10
    sigma = mgamd.TimeStepper.mass_coefficient(theta, dt)
    assert sigma == ts.mass_coefficient(theta, dt)
    h = mgamd.Hierarchy(ctx, geo, L, p, mg_type, coarse_solver="amg", max_brick=0, mass_coefficient=sigma)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma))
    lv = levels[-1]
    hit = _eig.get((geo, L, p))
    if hit is None or not np.array_equal(hit[0], lv.keys):
        _eig[(geo, L, p)] = hit = (lv.keys,) + ts.lowest_eigenpair(lv)
    lam, phi = hit[1], hit[2]
    g = ts.growth_factor(lam, theta, dt)
    stepper = mgamd.TimeStepper(h.fine_operator, h.mg, theta, dt)
    u, its = run_steps(mgamd, h, stepper, phi, n_steps, reltol)
    assert stepper.time() == pytest.approx(n_steps * dt, rel=1e-14)
    uref, itref = oracle_steps(oracle, lv, injected(emu, oracle, levels, P, h).vcycle, phi, theta, dt, n_steps, reltol)
    dev = np.abs(u - g ** n_steps * phi).max() / np.abs(phi).max()
    dev_ref = np.abs(u - uref).max() / np.abs(phi).max()
    print(f"eigenmode {case} theta={theta}: lambda {lam:.4f} g {g:.6f}; CG iterations {its} (oracle {itref}); "
          f"|u - g^n phi| {dev:.2e}, |u - oracle stepper| {dev_ref:.2e}")
    assert dev <= 1e-9 and dev_ref <= 1e-9
    assert all(abs(a - b) <= 1 for a, b in zip(its, itref))
    assert (u[lv.constrained] == 0.0).all()


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("case", [("quadrant", 3, 4, "HMG-global"), ("hypercube", 5, 1, "HMG-global")], ids=lambda c: "-".join(map(str, c)))
def test_source_term(mgamd, oracle, emu, ctx, case, theta):
    dt, n_steps, reltol = 0.02, 3, 1e-6
    sigma = mgamd.TimeStepper.mass_coefficient(theta, dt)
    h = mgamd.Hierarchy(ctx, *case, coarse_solver="amg", max_brick=0, mass_coefficient=sigma)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma))
    lv = levels[-1]
    u0 = np.random.default_rng(17).standard_normal(lv.n)
    u0[lv.constrained] = 0.0
    f = linear_source(lv.n, dt)
    u, its = run_steps(mgamd, h, mgamd.TimeStepper(h.fine_operator, h.mg, theta, dt), u0, n_steps, reltol, f)
    uref, itref = oracle_steps(oracle, lv, injected(emu, oracle, levels, P, h).vcycle, u0, theta, dt, n_steps, reltol, f)
    err = rel_err(u, uref)
    print(f"source term {case} theta={theta}: CG iterations {its} (oracle {itref}), iterate {err:.2e}")
    assert its == itref
    assert err <= n_steps * TOL_SOL


def test_distributed_input(mgamd, oracle, emu, ctx):
    """hanging values are not state: the step from u and from distribute(u) is the same step"""
    case, theta, dt = ("quadrant", 3, 4, "HMG-global"), 0.5, 0.02
    sigma = mgamd.TimeStepper.mass_coefficient(theta, dt)
    h = mgamd.Hierarchy(ctx, *case, coarse_solver="amg", max_brick=0, mass_coefficient=sigma)
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma))
    lv, op = levels[-1], h.fine_operator
    u0 = np.random.default_rng(19).standard_normal(lv.n)
    u0[lv.constrained] = 0.0
    f = linear_source(lv.n, dt)
    stepper = mgamd.TimeStepper(op, h.mg, theta, dt)
    a, b = vec(op, u0), vec(op, u0)
    op.distribute(b)
    filled = b.to_host()
    assert np.abs(filled[lv.constrained]).max() > 0.0 and np.array_equal(filled[~lv.constrained], u0[~lv.constrained])
    ita, _ = stepper.step(a, vec(op, f(0)), vec(op, f(1)), reltol=1e-6)
    itb, _ = stepper.step(b, vec(op, f(0)), vec(op, f(1)), reltol=1e-6)
    ua, ub = a.to_host(), b.to_host()
    print(f"distributed input: iterations {ita} / {itb}, difference {rel_err(ub, ua):.2e}")
    assert ita == itb and rel_err(ub, ua) <= TOL_ORDER
    assert (ua[lv.constrained] == 0.0).all() and (ub[lv.constrained] == 0.0).all()
    uref, _ = oracle_steps(oracle, lv, injected(emu, oracle, levels, P, h).vcycle, u0, theta, dt, 1, 1e-6, f)
    op.distribute(a)
    assert rel_err(a.to_host(), lv.C @ uref) <= TOL_SOL


def test_float_levels(mgamd, oracle, emu, ctx):
    """FP32 levels under the FP64 outer operator: the CG of every step needs the FP64 oracle's iteration count"""
    case, theta, dt, n_steps, reltol = ("quadrant", 3, 4, "HMG-global"), 1.0, 0.02, 3, 1e-6
    sigma = mgamd.TimeStepper.mass_coefficient(theta, dt)
    h = mgamd.Hierarchy(ctx, *case, coarse_solver="amg", number_type=mgamd.F32, max_brick=0, mass_coefficient=sigma)
    assert h.fine_operator is not h.operators[-1]
    levels, P = su.oracle_hierarchy(h.dofs, case, Problem(sigma))
    lv = levels[-1]
    u0 = np.random.default_rng(17).standard_normal(lv.n)
    u0[lv.constrained] = 0.0
    f = linear_source(lv.n, dt)
    u, its = run_steps(mgamd, h, mgamd.TimeStepper(h.fine_operator, h.mg, theta, dt), u0, n_steps, reltol, f)
    mg = emu.with_max_evs(oracle.Multigrid(levels, P, 3, coarse="direct"), [s.eigenvalue_estimates()[1] for s in h.smoothers])
    uref, itref = oracle_steps(oracle, lv, mg.vcycle, u0, theta, dt, n_steps, reltol, f)
    err = rel_err(u, uref)
    print(f"FP32 levels: CG iterations {its} (FP64 oracle {itref}), iterate {err:.2e}")
    assert its == itref
    assert err <= 1e-5


def test_two_simulated_ranks(mgamd, oracle, monkeypatch):
    """quadrant L=4 p=2 HMG-global cut over two ranks (host threads over the in-process communicator)"""
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")  # the sharded path's start vector hashes the DoF key; the oracle takes the same
    case, n_ranks, theta, dt, n_steps, reltol = ("quadrant", 4, 2, "HMG-global"), 2, 1.0, 0.02, 2, 1e-6
    sigma = ts.mass_coefficient(theta, dt)
    levels, P = su.oracle_hierarchy(None, case, Problem(sigma))
    omg = oracle.Multigrid(levels, P, 3, coarse="direct", start_vectors=[oracle.key_hash_start_vector(lv) for lv in levels])
    Lf = levels[-1]
    kf = {tuple(int(v) for v in k): i for i, k in enumerate(Lf.keys)}
    M = ts.mass_matrix(Lf)
    x = np.random.default_rng(3).standard_normal(Lf.n)
    u0 = np.random.default_rng(17).standard_normal(Lf.n)
    u0[Lf.constrained] = 0.0
    f = linear_source(Lf.n, dt)
    Mx = M @ x
    uref, itref = oracle_steps(oracle, Lf, omg.vcycle, u0, theta, dt, n_steps, reltol, f)
    group = mgamd.SimGroup(n_ranks)
    out, errs = [None] * n_ranks, [None] * n_ranks

    def rank_main(rk):
        try:
            c = mgamd.Context(0)
            h = mgamd.DistributedHierarchy(c, group.comm(rk), *case[:3], coarse_solver="amg", max_brick=0, min_root_dofs=0,
                                           mg_type=case[3], mass_coefficient=sigma)
            idx = np.array([kf[tuple(int(v) for v in k)] for k in h.dofs[-1].keys()])
            op = h.fine_operator
            vx, vy = vec(op, x[idx]), vec(op, np.full(len(idx), np.nan))
            op.vmult_mass(vy, vx)
            stepper = mgamd.TimeStepper(op, h.mg, theta, dt)
            u, its = vec(op, u0[idx]), []
            for n in range(n_steps):
                its.append(stepper.step(u, vec(op, f(n)[idx]), vec(op, f(n + 1)[idx]), reltol=reltol)[0])
            out[rk] = dict(idx=idx, y=vy.to_host(), u=u.to_host(), its=its, dist=h.distributed[-1])
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
    seen = {}
    for o in out:
        assert o["dist"]
        ey, eu = rel_err(o["y"], Mx[o["idx"]]), rel_err(o["u"], uref[o["idx"]])
        print(f"two ranks: vmult_mass {ey:.2e}, CG iterations {o['its']} (oracle {itref}), iterate {eu:.2e}")
        assert ey <= TOL_OP and o["its"] == itref and eu <= n_steps * TOL_SOL
        for i, v in zip(o["idx"], o["u"]):
            assert seen.setdefault(i, v) == v  # copies of shared DoFs: bitwise identical
    assert len(seen) == Lf.n


# ------------------------------------------------------------------ refusals
def test_refusals(mgamd, ctx):
    theta, dt = 0.5, 0.02
    sigma = mgamd.TimeStepper.mass_coefficient(theta, dt)
    h = mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-global", coarse_solver="amg", mass_coefficient=sigma)
    op, n = h.fine_operator, h.n_dofs
    for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(mgamd.MgamdError, match="theta"):
            mgamd.TimeStepper(op, h.mg, bad, dt)
    for bad in (0.0, -0.02, float("nan"), float("inf")):
        with pytest.raises(mgamd.MgamdError, match="dt = "):
            mgamd.TimeStepper(op, h.mg, theta, bad)
    with pytest.raises(mgamd.MgamdError, match=r"sigma = 100\b.*theta = 1\b.*dt = 0\.02"):
        mgamd.TimeStepper(op, h.mg, 1.0, dt)  # sigma theta dt = 2
    op32 = mgamd.Operator(ctx, h.dofs[-1], mgamd.F32)
    with pytest.raises(mgamd.MgamdError, match="FP64"):
        mgamd.TimeStepper(op32, h.mg, theta, dt)
    stepper = mgamd.TimeStepper(op, h.mg, theta, dt)
    u0 = np.random.default_rng(1).standard_normal(n)
    u, f = vec(op, u0), vec(op, np.ones(n))
    with pytest.raises(mgamd.MgamdError, match="exactly one"):
        stepper.step(u, f, None)
    with pytest.raises(mgamd.MgamdError, match="exactly one"):
        stepper.step(u, None, f)
    with pytest.raises(mgamd.MgamdError, match="entries"):
        stepper.step(mgamd.Vector(ctx, n + 1))
    with pytest.raises(mgamd.MgamdError, match="entries"):
        stepper.step(u, f, mgamd.Vector(ctx, n - 1))
    with pytest.raises(mgamd.MgamdError, match="entries"):
        stepper.step(u, mgamd.Vector(ctx, n, mgamd.F32), f)
    assert np.array_equal(u.to_host(), u0) and stepper.time() == 0.0 and stepper.n_steps() == 0
    # vmult_mass
    with pytest.raises(mgamd.MgamdError, match="differ"):
        op.vmult_mass(u, u)
    with pytest.raises(mgamd.MgamdError, match="size"):
        op.vmult_mass(mgamd.Vector(ctx, n + 1), u)
    with pytest.raises(mgamd.MgamdError, match="number type"):
        op.vmult_mass(mgamd.Vector(ctx, n, mgamd.F32), u)
    assert np.array_equal(u.to_host(), u0)
    # the operator of a local-smoothing level is refused by name; the active-mesh operator of that hierarchy works
    hl = mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-local")
    lop = hl.operators[-1]
    with pytest.raises(mgamd.MgamdError, match="local-smoothing"):
        lop.vmult_mass(lop.initialize_dof_vector(), lop.initialize_dof_vector())
    a = hl.fine_operator
    y = apply_nan(mgamd, ctx, a.vmult_mass, np.ones(hl.n_dofs))
    assert np.isfinite(y).all() and y.sum() > 0.0


# ------------------------------------------------------------------ the example program
def test_example_program(oracle):
    """bin/heat_equation (examples/heat_equation.cpp, the C++ class): hypercube L=3 p=2, HMG-global, theta = 0.5, dt = 0.01, five
    steps from u = 1 at reltol 1e-10; the printed norms are the oracle stepper's"""
    exe = os.path.join(ROOT, "bin", "heat_equation")
    assert os.path.exists(exe), "bin/heat_equation is missing: make all"
    run = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    norms = [float(m) for m in re.findall(r"\|u\| = (\S+)", run.stdout)]
    assert len(norms) == 5, run.stdout
    theta, dt = 0.5, 0.01
    levels, P = su.oracle_hierarchy(None, ("hypercube", 3, 2, "HMG-global"), Problem(ts.mass_coefficient(theta, dt)))
    lv = levels[-1]
    u = np.ones(lv.n)
    u[lv.constrained] = 0.0
    Mh, solve = ts.mass_matrix(lv), ts.pcg_solver(oracle, lv, oracle.Multigrid(levels, P, 3, coarse="direct").vcycle, 1e-10)
    for n, got in enumerate(norms):
        u, _ = ts.theta_step(lv, u, None, None, theta, dt, solve, Mh)
        print(f"heat_equation step {n + 1}: |u| {got:.12e}, oracle {np.linalg.norm(u):.12e}")
        assert got == pytest.approx(np.linalg.norm(u), rel=1e-9)
