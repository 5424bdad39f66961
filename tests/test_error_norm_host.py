"""The error norms on the host: mgamd_dofs_quadrature_points against the oracle's points, the numpy oracle (tests/error_norm_oracle.py)
against closed forms, compute_global_error and the host-side refusals.  The device kernel is held against this oracle and against the
same closed forms by test_gpu_error_norm.py.

Closed forms: for tensor polynomials v and w (polynomial_exactness.Poly3, monomial coefficients c[i, j, k]) the difference d = v - w is
one more Poly3, and on a leaf K = Ix x Iy x Iz
    int_K d^2        = sum c_ijk c_lmn Mx[i, l] My[j, m] Mz[k, n]
    int_K |grad d|^2 = the same with (K, M, M) + (M, K, M) + (M, M, K)
with M[a, b] = int_I t^a t^b and K[a, b] = int_I (t^a)' (t^b)' from polynomial_exactness.interval_integrals: no shape function and no
quadrature.

Points: the product forms corner + h x_q in double with its own rule (Newton on P_n in long double), the oracle with numpy's leggauss.
corner and h x_q are exact on both sides (h is a power of two), so the two differ by the two rules' x_q (asked to agree to 1 ulp of a
number below 1: 2^-53, times h) and by the final rounding of either sum (half an ulp of a number of size at most 1 each): the bound is
h 2^-53 + 2^-52.  Bit equality is NOT asserted: the two rules are computed independently."""
import ctypes as C

import numpy as np
import pytest

import error_estimator_oracle as eo
import error_norm_oracle as no
import mgoracle
import physics_oracle as po
import random_mesh_physics as rm
from support import mesh, tria_of

DEGREES = (1, 2, 3, 4, 5, 6, 7)
TOL = 1e-12  # the tolerance of test_gpu_error_norm.py: up to 1000 FP64 additions per leaf plus the sweeps


def leaves_of(oracle, name):
    named = dict(quadrant2=("quadrant", 2), quadrant3=("quadrant", 3), hypercube0=("hypercube", 0), hypercube1=("hypercube", 1))
    return mesh(*named[name]) if name in named else rm.leaves_of(oracle, name)


@pytest.mark.parametrize("name", ["quadrant2", "quadrant3", "S"])
def test_quadrature_points(mgamd, oracle, name):
    leaves = leaves_of(oracle, name)
    t = tria_of(mgamd, leaves)
    cells = po.product_cells(t)
    assert cells == [tuple(c) for c in mgoracle.sorted_cells(leaves)]
    h = no.cell_h(cells)[:, None, None, None, None]
    worst = 0.0
    for p in (1, 4, 7):
        d = mgamd.DoFs(t, p)
        assert np.array_equal(d.quadrature_points(0), d.quadrature_points(p + 2))
        for n_q in (p + 1, p + 2, p + 3):
            x, ref = d.quadrature_points(n_q), no.quadrature_points(cells, n_q)
            assert x.shape == ref.shape == (len(cells), n_q, n_q, n_q, 3)
            worst = max(worst, (np.abs(x - ref) / (h * 2.0 ** -53 + 2.0 ** -52)).max())
    print(f"{name}: {len(cells)} leaves, max |x - x_ref| / (h 2^-53 + 2^-52) = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("p", DEGREES)
def test_oracle_against_closed_forms(p):
    """u_h the nodal interpolant of v in Q_p (it lies in the conforming space, hanging nodes included), w of degree p + 1 per variable:
    the squared integrands have degree 2p + 2 <= 2 n_q - 1 for n_q = p + 2, so the rule is exact"""
    s = eo.nodal_space(mesh("quadrant", 2), p)
    pos = mgoracle.Level.node_positions(s)
    v, w = no.polynomial(p, 10 + p), no.polynomial(p + 1, 20 + p)
    a = np.array([1.0 + 0.5 * (t % 3) for t in range(len(s.cells))])
    x = np.where(s.hanging, np.nan, v(*pos.T))  # (the hanging entries are never used)
    forms = no.ClosedForms(p + 1)
    got = no.norms(s, x, p + 2, w, no.gradient_of(w), a, 3.0)
    ref = forms.norms(s.cells, no.difference(v, w), a, 3.0)
    size_v, size_w = forms.norms(s.cells, v, a, 3.0), forms.norms(s.cells, w, a, 3.0)
    for norm in (no.L2, no.H1, no.ENERGY):
        ratio = (np.abs(got[norm] - ref[norm]) / (size_v[norm] + size_w[norm])).max()
        print(f"p={p} norm {norm}: max |oracle - closed form| / (|v|_K + |w|_K) = {ratio:.2e}")
        assert ratio <= TOL
    # w = v: nothing is left; n_q = p + 1 and p + 3 integrate (v - 0)^2 of degree 2p exactly as well
    zero = no.norms(s, x, p + 2, v, no.gradient_of(v))
    assert all((zero[norm] <= 1e-13 * size_v[norm]).all() for norm in (no.L2, no.H1))
    plain = no.ClosedForms(p).norms(s.cells, v)
    for n_q in (p + 1, p + 3):
        own = no.norms(s, x, n_q)
        assert all((np.abs(own[norm] - plain[norm]) <= TOL * plain[norm]).all() for norm in (no.L2, no.H1))
    # Linfty is a maximum over the points: the points' own values
    pts = np.moveaxis(no.quadrature_points(s.cells, p + 2), -1, 0)
    linf = np.abs(v(*pts) - w(*pts)).reshape(len(s.cells), -1).max(axis=1)
    assert (np.abs(got[no.LINFTY] - linf) <= 1e-13 * linf).all()


def test_compute_global_error(mgamd):
    e = np.array([3.0, 4.0, 12.0])
    for norm in (mgamd.NORM_L2, mgamd.NORM_H1_SEMINORM, mgamd.NORM_ENERGY):
        assert mgamd.compute_global_error(e, norm) == 13.0 == no.global_error(e, norm)
    assert mgamd.compute_global_error(e, mgamd.NORM_LINFTY) == 12.0 == no.global_error(e, no.LINFTY)
    assert (mgamd.NORM_L2, mgamd.NORM_H1_SEMINORM, mgamd.NORM_ENERGY, mgamd.NORM_LINFTY) == (no.L2, no.H1, no.ENERGY, no.LINFTY)
    with pytest.raises(ValueError, match="unknown norm"):
        mgamd.compute_global_error(e, 4)


def test_host_refusals(mgamd):
    plain = mgamd.Triangulation("quadrant", 3)
    d = mgamd.DoFs(plain, 2)
    for n_q in (-1, 1, 2, 6, 11, 1000):
        with pytest.raises(mgamd.MgamdError, match=rf"quadrature_points: n_q = {n_q} refused"):
            d.quadrature_points(n_q)
    lib = C.CDLL(mgamd._LIB_PATH)
    lib.mgamd_last_error.restype = C.c_char_p
    assert lib.mgamd_dofs_quadrature_points(d._h, 0, None) == 3 and b"null argument" in lib.mgamd_last_error()
    ls = mgamd.DoFs(plain.level_mesh(2), 2, local_smoothing_level=True)
    with pytest.raises(mgamd.MgamdError, match="quadrature_points: refused on the level of a local-smoothing hierarchy"):
        ls.quadrature_points()
    trias = mgamd.create_geometric_coarsening_sequence(plain)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    sharded = mgamd.DoFs(trias[-1], 2, 0, partition=part, level=len(trias) - 1, rank=0)
    with pytest.raises(mgamd.MgamdError, match="quadrature_points: not implemented: sharded"):
        sharded.quadrature_points()
