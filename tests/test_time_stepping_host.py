"""The oracle of the time stepper (tests/time_stepping_oracle.py) pinned on the host, before anything is compared with it: the
mass matrix C^T M C is symmetric, positive on the free DoFs, exactly zero on constrained rows and columns and integrates 1 to the
volume; theta steps from the lowest eigenmode of K phi = lambda M phi decay by the scheme's growth factor
g = (1 - (1 - theta) dt lambda) / (1 + theta dt lambda) per step.

Eigenmode bound 1e-9 = reltol 1e-10 x 5 steps x 2 (the CG stops on the residual, the error is measured in the iterate).  The
oracle alone shows <= 1.2e-11 against g^n phi and <= 1.7e-11 against the exact-solve stepper, 7-9 CG iterations per step, with
lambda = 7.406, 7.406, 7.402 on the three meshes (3 pi^2 / 4 = 7.402 on the cube of side 2)."""
import numpy as np
import pytest

import physics_oracle as po
import support as su
import time_stepping_oracle as ts
from physics_oracle import Problem

CASES = [("hypercube", 2, 2), ("quadrant", 3, 2), ("quadrant", 3, 4)]
THETAS = [1.0, 0.5]
DT, N_STEPS, RELTOL, TOL = 0.01, 5, 1e-10, 1e-9

_eig = {}  # case -> (lambda, phi), which do not depend on sigma


def hierarchy(oracle, case, theta):
    levels, P = su.oracle_hierarchy(None, case + ("HMG-global",), Problem(ts.mass_coefficient(theta, DT)))
    if case not in _eig:
        _eig[case] = ts.lowest_eigenpair(levels[-1])
    return (levels, P) + _eig[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_mass_matrix(oracle, case):
    lv = hierarchy(oracle, case, THETAS[0])[0][-1]
    M = ts.mass_matrix(lv)
    c, free = lv.constrained, np.flatnonzero(~lv.constrained)
    assert c.any() and (case[0] != "quadrant" or lv.C[c].nnz > 0)  # quadrant: hanging nodes with parents
    assert abs(M - M.T).max() <= 1e-15 * abs(M).max()
    assert M[c].nnz == 0 or abs(M[c]).max() == 0.0
    assert M[:, c].nnz == 0 or abs(M[:, c]).max() == 0.0
    rng = np.random.default_rng(1)
    for _ in range(3):
        x = rng.standard_normal(lv.n)
        assert x[free] @ (M[free][:, free] @ x[free]) > 0.0
    assert np.linalg.eigvalsh(M[free][:, free].toarray()).min() > 0.0 if len(free) < 1500 else True
    one = np.ones(lv.n)
    if case[0] == "hypercube":
        assert one @ (lv.Mraw @ one) == pytest.approx(8.0, rel=1e-13)  # the domain has side 2
    # sigma does not enter
    assert abs(ts.mass_matrix(po.changed(lv, sigma=7.5)) - M).max() == 0.0


@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_eigenmode_decay(oracle, case, theta):
    levels, P, lam, phi = hierarchy(oracle, case, theta)
    lv = levels[-1]
    assert lam == pytest.approx(0.75 * np.pi ** 2, rel=2e-3)
    g = ts.growth_factor(lam, theta, DT)
    Mh = ts.mass_matrix(lv)
    mg = oracle.Multigrid(levels, P, 3, coarse="direct")
    iterative, exact = ts.pcg_solver(oracle, lv, mg.vcycle, RELTOL), ts.exact_solver(lv)
    u, ue, its = phi.copy(), phi.copy(), []
    for _ in range(N_STEPS):
        u, it = ts.theta_step(lv, u, None, None, theta, DT, iterative, Mh)
        ue, _ = ts.theta_step(lv, ue, None, None, theta, DT, exact, Mh)
        its.append(it)
    dev = np.abs(u - g ** N_STEPS * phi).max() / np.abs(phi).max()
    dev_exact = np.abs(u - ue).max() / np.abs(phi).max()
    print(f"{case} theta={theta}: n={lv.n} lambda={lam:.4f} g={g:.6f} CG iterations {its}; |u - g^n phi| {dev:.2e}, "
          f"|u - exact-solve stepper| {dev_exact:.2e}")
    assert dev <= TOL and dev_exact <= TOL
    assert (u[lv.constrained] == 0.0).all()


def test_step_ignores_constrained_entries_and_takes_a_source(oracle):
    """entries of u and f on constrained DoFs are never used; with a source the exact-solve step satisfies the scheme's equation"""
    case, theta = ("quadrant", 3, 2), 0.5
    lv = hierarchy(oracle, case, theta)[0][-1]
    rng = np.random.default_rng(2)
    u, f0, f1 = (rng.standard_normal(lv.n) for _ in range(3))
    u[lv.constrained] = 0.0
    solve = ts.exact_solver(lv)
    a, _ = ts.theta_step(lv, u, f0, f1, theta, DT, solve)
    ud, f0d, f1d = u.copy(), f0.copy(), f1.copy()
    for v in (ud, f0d, f1d):
        v[lv.constrained] = 1e30
    b, _ = ts.theta_step(lv, ud, f0d, f1d, theta, DT, solve)
    assert np.array_equal(a, b)
    # (M/dt + theta K)(a - u) = M f_theta - K u on the free rows
    M, K, free = ts.mass_matrix(lv), ts.stiffness_matrix(lv), ~lv.constrained
    lhs = (M / DT + theta * K) @ (a - u)
    rhs = M @ (theta * f1 + (1 - theta) * f0) - K @ u
    assert np.abs(lhs - rhs)[free].max() <= 1e-11 * np.abs(rhs).max()
