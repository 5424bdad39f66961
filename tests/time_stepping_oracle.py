"""Test-side oracle of the mass matrix and the theta time stepper: pure numpy/scipy on the levels of oracle/physics_oracle.py,
which carry Mraw, K0raw, C, A and constrained.  Not a test module.

Semi-discrete heat equation with homogeneous Dirichlet data and constraints eliminated:  M^ u' + K^ u = M^ f(t),
M^ = C^T Mraw C, K^ = C^T K0raw C, f a vector of nodal values.  theta-scheme with constant dt for the increment
delta = u_new - u:  (M^/dt + theta K^) delta = M^ f_theta - K^ u,  f_theta = theta f_new + (1 - theta) f_old.  With
sigma = 1 / (theta dt) the left side is theta A^, A^ = K^ + sigma M^ (the level's A on the free DoFs), and K^ u = A^ u - sigma M^ u:

    1.  w = f_theta + sigma u              (w = sigma u without a source)
    2.  t = M^ w
    3.  r = t - A u, constrained rows of r set to 0
    4.  solve A delta = r / theta from delta = 0
    5.  u_new = u + delta, constrained entries 0

M^ has zero rows and columns on constrained DoFs (Dirichlet and hanging), so the entries of u and f there are never used.
"""
import numpy as np
import scipy.sparse.linalg as spla


def mass_matrix(lv):
    """C^T Mraw C: the mass matrix of the level's constrained space, zero rows and columns on constrained DoFs"""
    return (lv.C.T @ lv.Mraw @ lv.C).tocsr()


def stiffness_matrix(lv):
    """C^T K0raw C, likewise (no identity rows)"""
    return (lv.C.T @ lv.K0raw @ lv.C).tocsr()


def mass_coefficient(theta, dt):
    return 1.0 / (theta * dt)


def exact_solver(lv):
    """solve(b) -> (A^-1 b, 0) by sparse LU"""
    lu = spla.splu(lv.A.tocsc())
    return lambda b: (lu.solve(b), 0)


def pcg_solver(oracle, lv, precond, reltol, abstol=1e-20, maxiter=10000):
    """solve(b) -> (x, iterations) by mgoracle.pcg from x = 0"""
    def solve(b):
        x, it, _ = oracle.pcg(lv.A, b, precond, reltol, abstol, maxiter)
        return x, it
    return solve


def theta_step(lv, u, f_old, f_new, theta, dt, solve, Mh=None):
    """one step of the scheme above on the level lv, whose mass coefficient must be 1 / (theta dt); returns (u_new, iterations)"""
    sigma = mass_coefficient(theta, dt)
    assert abs(lv.mass_coefficient * theta * dt - 1.0) <= 1e-12
    assert (f_old is None) == (f_new is None)
    if Mh is None:
        Mh = mass_matrix(lv)
    w = sigma * u if f_new is None else theta * f_new + (1.0 - theta) * f_old + sigma * u
    t = Mh @ w
    r = t - lv.A @ u
    r[lv.constrained] = 0.0
    delta, it = solve(r / theta)
    u_new = u + delta
    u_new[lv.constrained] = 0.0
    return u_new, it


def lowest_eigenpair(lv):
    """(lambda, phi) of K^ phi = lambda M^ phi on the free DoFs, lowest lambda (shift-invert at 0); phi is extended by zeros to the
    constrained DoFs and scaled to max |phi| = 1"""
    free = np.flatnonzero(~lv.constrained)
    K = stiffness_matrix(lv)[free][:, free].tocsc()
    M = mass_matrix(lv)[free][:, free].tocsc()
    lam, vec = spla.eigsh(K, k=1, M=M, sigma=0.0, which="LM")
    phi = np.zeros(lv.n)
    phi[free] = vec[:, 0]
    phi /= phi[np.argmax(np.abs(phi))]
    return float(lam[0]), phi


def growth_factor(lam, theta, dt):
    """of one theta-step on an eigenmode: (1 - (1 - theta) dt lambda) / (1 + theta dt lambda)"""
    return (1.0 - (1.0 - theta) * dt * lam) / (1.0 + theta * dt * lam)
