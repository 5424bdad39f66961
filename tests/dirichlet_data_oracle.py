"""Test-side oracle of the theta stepper with non-zero Dirichlet data, on the levels of oracle/physics_oracle.py (which carry Ch, C, K0raw,
Braw, Mraw, dirichlet, hanging, constrained) and the solvers of tests/time_stepping_oracle.py.  Not a test module.

Dirichlet data is a vector g of n values of which only the entries at Dirichlet DoFs count:  g^ = physics_oracle.data(lv, g).  The
lifting, distribute_values and face_values of a level are physics_oracle's.

The stepper works on FULL nodal vectors N(u, g) = Ch (u + g^), u the free DoFs, K the raw stiffness matrix of the level with its
coefficient and the surface term of its convective faces (physics_oracle.stiffness_raw).  The semi-discrete equation on the free
rows i is [Ch^T (Mraw N' + K N)]_i = [C^T Mraw C f]_i + l_i (the source sees the free entries of f only, as the product's mass
pass).  One theta step with sigma = 1 / (theta dt), for the increment delta of the free DoFs:

    A delta = (M^ f_theta + l - [Ch^T K N(u, g_old)]) / theta - [Ch^T (K + sigma Mraw) Ch (g_new^ - g_old^)]     on free rows

theta_step_data forms that right-hand side from the raw matrices and hands it to the solver of time_stepping_oracle (exact or the
oracle's PCG, from delta = 0).  theta_step_direct solves the same step for u_new itself, (M^/dt + theta K^) u_new = ..., with
every term written out on full vectors: the check of the increment form (test_dirichlet_data_host.py).
"""
import numpy as np
import scipy.sparse.linalg as spla

import time_stepping_oracle as tso
from physics_oracle import data, stiffness_raw


def _nodal(lv, u, g):
    free = np.where(lv.constrained, 0.0, u)
    return lv.Ch @ (free + data(lv, g))


def theta_rhs_data(lv, u, f_old, f_new, g_old, g_new, load, theta, dt, Mh=None):
    """the right-hand side of A delta = ... above, constrained rows 0"""
    sigma = tso.mass_coefficient(theta, dt)
    assert abs(lv.mass_coefficient * theta * dt - 1.0) <= 1e-12
    if Mh is None:
        Mh = tso.mass_matrix(lv)
    K = stiffness_raw(lv)
    zero = np.zeros(lv.n)
    g_old = zero if g_old is None else g_old
    g_new = zero if g_new is None else g_new
    r = -(lv.Ch.T @ (K @ _nodal(lv, u, g_old)))
    if f_new is not None:
        r = r + Mh @ (theta * f_new + (1.0 - theta) * f_old)
    if load is not None:
        r = r + load
    r = r / theta - lv.Ch.T @ ((K + sigma * lv.Mraw) @ (lv.Ch @ (data(lv, g_new) - data(lv, g_old))))
    r[lv.constrained] = 0.0
    return r


def theta_step_data(lv, u, f_old, f_new, g_old, g_new, load, theta, dt, solve, Mh=None):
    """one step; returns (u_new, iterations), constrained entries of u_new 0 (distribute_values(lv, u_new, g_new) for output)"""
    delta, it = solve(theta_rhs_data(lv, u, f_old, f_new, g_old, g_new, load, theta, dt, Mh))
    u_new = u + delta
    u_new[lv.constrained] = 0.0
    return u_new, it


def theta_step_direct(lv, u, f_old, f_new, g_old, g_new, load, theta, dt):
    """the same step solved for u_new itself by sparse LU:
    Ch^T [Mraw (N_new - N_old) / dt + theta K N_new + (1 - theta) K N_old] = M^ f_theta + l  on the free rows"""
    K, M = stiffness_raw(lv), lv.Mraw
    free = np.flatnonzero(~lv.constrained)
    N_old = _nodal(lv, u, g_old)
    N_bnd = lv.Ch @ data(lv, g_new)  # N_new = Ch u_new + N_bnd
    rhs = lv.Ch.T @ (M @ (N_old - N_bnd) / dt - theta * (K @ N_bnd) - (1.0 - theta) * (K @ N_old))
    if f_new is not None:
        rhs = rhs + tso.mass_matrix(lv) @ (theta * f_new + (1.0 - theta) * f_old)
    if load is not None:
        rhs = rhs + load
    S = (lv.Ch.T @ (M / dt + theta * K) @ lv.Ch).tocsr()[free][:, free].tocsc()
    u_new = np.zeros(lv.n)
    u_new[free] = spla.spsolve(S, rhs[free])
    return u_new
