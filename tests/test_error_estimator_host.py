"""The numpy oracle of the jump error indicator (tests/error_estimator_oracle.py) against mathematics: closed forms on quadrant
NRefGlobal 3 (120 cells, hanging faces on the planes through 0), degrees 1 ... 7, each held to 1e-13 of the largest value.  The device
kernels are held against this oracle by test_gpu_error_estimator.py."""
import numpy as np
import pytest

import error_estimator_oracle as eo
import mgoracle
import physics_oracle as po
from physics_oracle import Problem
from support import mesh

TOL = 1e-13
DEGREES = (1, 2, 3, 4, 5, 6, 7)


def setup(p):
    s = eo.nodal_space(mesh("quadrant", 3), p)
    return s, mgoracle.Level.node_positions(s), np.array([2.0 / (1 << c[0]) for c in s.cells])


def on_face(s, f):
    """bool per cell: the cell has a face on face f of the cube"""
    return np.array([c[1 + (f >> 1)] == (((1 << c[0]) - 1) if f & 1 else 0) for c in s.cells])


def check(eta2, ref, h, tag):
    scale = ref.max() if ref.max() > 0 else (h ** 3 / 24.0).max()  # (all-zero closed forms: the size of one unit jump)
    err = np.abs(eta2 - ref).max() / scale
    print(f"{tag}: max |eta^2 - closed form| / scale = {err:.2e}")
    assert err <= TOL


@pytest.mark.parametrize("p", DEGREES)
def test_coefficient_jump_across_hanging_faces(p):
    """a = 1 for x < 0 and 3 for x > 0, u = x: the flux jumps by 2 on the plane x = 0, eta_K^2 = h_K / 24 * 4 h_K^2 = h_K^3 / 6 on
    the cells that touch it from either side (the fine cells see the coarse side on their own face, the coarse cell its four
    quarters), 0 elsewhere"""
    s, pos, h = setup(p)
    prob = Problem(coefficient={c: (1.0 if po._centre(c)[0] < 0 else 3.0) for c in s.cells})
    touches = np.array([(c[1] + 1) << (mgoracle.LMAX - c[0]) == 1 << (mgoracle.LMAX - 1) or c[1] << (mgoracle.LMAX - c[0]) == 1 << (mgoracle.LMAX - 1)
                        for c in s.cells])
    assert 0 < touches.sum() < len(s.cells) and len({c[0] for c, t in zip(s.cells, touches) if t}) == 2  # both levels meet there
    check(eo.indicator_squared(s, prob, pos[:, 0]), np.where(touches, h ** 3 / 6.0, 0.0), h, f"p={p} coefficient jump")


@pytest.mark.parametrize("p", DEGREES)
def test_global_q1_polynomial_has_no_jump(p):
    s, pos, h = setup(p)
    x, y, z = pos.T
    u = 0.5 - x + 2.0 * y + 0.25 * z + 0.75 * x * y - 1.5 * y * z + x * z + 0.5 * x * y * z
    eta2 = eo.indicator_squared(s, Problem(), u)
    gmax = 6.0  # a bound on |grad u| on the cube
    print(f"p={p} Q1: max eta^2 {eta2.max():.2e}")
    assert eta2.max() <= TOL * gmax ** 2 * (h ** 3 / 24.0).max()
    # and with the hanging entries overwritten: they are never read
    u2 = np.where(s.hanging, np.nan, u)
    assert np.array_equal(eo.indicator_squared(s, Problem(), u2), eta2)


@pytest.mark.parametrize("p", DEGREES)
def test_boundary_residuals(p):
    s, pos, h = setup(p)
    u = pos[:, 0]  # u = x: a d_n u = -1 on face 0, +1 on face 1
    f0, f1 = on_face(s, 0), on_face(s, 1)
    natural = Problem(dirichlet_faces=0b111100)
    # no q: no boundary term at all
    check(eo.indicator_squared(s, natural, u), np.zeros(len(h)), h, f"p={p} q = None")
    # q = 0 on the natural x-faces: r = -a d_n u = -+1, eta^2 = h^3 / 24 on the cells on those faces
    check(eo.indicator_squared(s, natural, u, np.zeros(6)), np.where(f0 | f1, h ** 3 / 24.0, 0.0), h, f"p={p} q = 0")
    # the exact flux
    check(eo.indicator_squared(s, natural, u, np.array([-1.0, 1.0, 0, 0, 0, 0])), np.zeros(len(h)), h, f"p={p} exact flux")
    # a convective face 1: a d_n u + beta (u - u_ext) = 0 holds for u_ext = 1 + 1 / beta, passed as q_1 = beta u_ext
    beta = 2.5
    robin = Problem(dirichlet_faces=0b111101, robin=(0, beta, 0, 0, 0, 0))
    check(eo.indicator_squared(s, robin, u, np.array([0, beta * (1.0 + 1.0 / beta), 0, 0, 0, 0])), np.zeros(len(h)), h, f"p={p} Robin exact")
    # another exterior temperature: r = beta u_ext - beta - 1 on face 1
    u_ext = -0.75
    r = beta * u_ext - beta - 1.0
    check(eo.indicator_squared(s, robin, u, np.array([0, beta * u_ext, 0, 0, 0, 0])), np.where(f1, h ** 3 / 24.0 * r * r, 0.0), h, f"p={p} Robin")
