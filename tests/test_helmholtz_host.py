"""The mass term on the host (no GPU): level tables carry sigma of A = K + sigma M; the assembled matrix, the Gaussian right-hand
side and the AMG set-up follow it; what is out of scope is refused by name.  Oracle: oracle/physics_oracle.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import physics_oracle as po
import support as su
from physics_oracle import Problem

SIGMAS = [7.5, 3000.0]  # no powers of two: a wrong power of h cannot hide; stiffness- and mass-dominated at these mesh sizes


def _csr(d):
    ptr, col, val = d.matrix()
    return sp.csr_matrix((val, col.astype(np.int64), ptr.astype(np.int64)), shape=(d.n_dofs, d.n_dofs))


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 1), ("quadrant", 3, 2), ("quadrant", 3, 4), ("hypercube", 2, 4)])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_assembled_matrix_is_helper_matrix(mgamd, oracle, geo, L, p, sigma):
    d = mgamd.DoFs(mgamd.Triangulation(geo, L), p, 0)
    d.set_mass_coefficient(sigma)
    lv = su.oracle_level(d, geo, L, p, Problem(sigma))
    A = _csr(d)
    diff = (A - lv.A).tocsr()
    err = (abs(diff).max() if diff.nnz else 0.0) / abs(lv.A).max()
    print(f"{geo} L={L} p={p} sigma={sigma}: max |A - A_ref| / max |A_ref| = {err:.2e}")
    assert err <= 1e-13
    assert abs(A - A.T).max() <= 1e-13 * abs(A).max()


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 2), ("hypercube", 2, 4)])
def test_mass_matrix_integrates_one_to_the_volume(mgamd, oracle, geo, L, p):
    """(A_sigma - A_0) / sigma is C^T M C on the unconstrained rows.  Two checks, which together give 1^T M 1 = |[-1, 1]^3| = 8 for
    the product's mass term: (1) the product's free-free block equals the helper's C^T M C to 1e-13; (2) the helper's full mass
    matrix, Dirichlet and hanging rows included, integrates the constant 1 to 8.  The Dirichlet rows and columns are not in an
    assembled matrix (C drops them), so the product alone cannot give the 8: step (2) is about the helper, step (1) ties the
    product to it."""
    sigma = 7.5
    d = mgamd.DoFs(mgamd.Triangulation(geo, L), p, 0)
    A0 = _csr(d)
    d.set_mass_coefficient(sigma)
    M = (_csr(d) - A0) / sigma
    hel = su.oracle_level(d, geo, L, p, Problem(1.0))
    free = ~hel.constrained
    Mref = (hel.C.T @ hel.Mraw @ hel.C).tocsr()
    assert abs((M - Mref)[free][:, free]).max() <= 1e-13 * abs(Mref).max()
    assert abs(M[~free]).max() == 0.0 and abs(M[:, ~free]).max() == 0.0  # identity rows carry no sigma
    one = np.ones(hel.n)
    assert one @ (hel.Mraw @ one) == pytest.approx(8.0, rel=1e-13)
    # a function that the constrained space holds exactly: 1_free has the nodal values Ch 1_free, and both sides integrate its square
    f = free.astype(float)
    nodal = hel.Ch @ f
    assert f @ (M @ f) == pytest.approx(nodal @ (hel.Mraw @ nodal), rel=1e-13)


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 1), ("quadrant", 3, 2), ("quadrant", 3, 4), ("hypercube", 2, 3)])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_gaussian_right_hand_side(mgamd, oracle, geo, L, p, sigma):
    d = mgamd.DoFs(mgamd.Triangulation(geo, L), p, 0)
    b0 = d.rhs_function(1)
    d.set_mass_coefficient(sigma)
    lv = su.oracle_level(d, geo, L, p, Problem(sigma))
    ref = lv.rhs_function(po.gaussian_load(sigma), oracle.gaussian_solution)
    got = d.rhs_function(1)
    assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)  # the bound of test_gaussian_right_hand_side_and_distribute
    assert np.abs(got - b0).max() > 1e-3 * np.abs(b0).max()  # the mass term is in it
    assert np.array_equal(d.rhs_function(0), d.rhs_constant())  # f = 1, g = 0: no lifting, no sigma
    d.set_mass_coefficient(0.0)
    assert np.array_equal(d.rhs_function(1), b0)


def test_getter_round_trip_and_refusals(mgamd):
    t = mgamd.Triangulation("quadrant", 3)
    d = mgamd.DoFs(t, 2, 0)
    assert d.mass_coefficient() == 0.0
    d.set_mass_coefficient(7.5)
    assert d.mass_coefficient() == 7.5
    for bad, word in ((-1.0, "-1"), (float("nan"), "nan"), (float("inf"), "inf"), (-0.25, "-0.25")):
        with pytest.raises(mgamd.MgamdError, match=word):
            d.set_mass_coefficient(bad)
        assert d.mass_coefficient() == 7.5  # a refused value changes nothing
    d.set_mass_coefficient(0.0)
    assert d.mass_coefficient() == 0.0


def test_local_smoothing_level_refuses_mass_term(mgamd):
    t = mgamd.Triangulation("quadrant", 3)
    dl = mgamd.DoFs(t.level_mesh(t.n_levels - 1), 2, 0, local_smoothing_level=True)
    dl.set_mass_coefficient(0.0)
    with pytest.raises(mgamd.MgamdError, match="local-smoothing"):
        dl.set_mass_coefficient(7.5)
    assert dl.mass_coefficient() == 0.0


def test_sharded_amg_plans_refuse_a_global_space_with_another_sigma(mgamd):
    fine = mgamd.Triangulation("quadrant", 4)
    trias = mgamd.create_geometric_coarsening_sequence(fine)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    glob = mgamd.DoFs(fine, 1, -1)
    loc = mgamd.DoFs(fine, 1, -1, part, len(trias) - 1, 1)
    rows = mgamd.amg_shard_match_rows(glob, loc)
    assert len(rows) == loc.n_dofs and len(set(rows.tolist())) == loc.n_dofs
    loc.set_mass_coefficient(7.5)
    with pytest.raises(mgamd.MgamdError, match="mass coefficient"):
        mgamd.amg_shard_match_rows(glob, loc)
    glob.set_mass_coefficient(3000.0)
    with pytest.raises(mgamd.MgamdError, match="mass coefficient"):
        mgamd.amg_shard_match_rows(glob, loc)
    glob.set_mass_coefficient(7.5)
    assert np.array_equal(mgamd.amg_shard_match_rows(glob, loc), rows)


def test_amg_setup_runs_on_the_shifted_matrix(mgamd):
    """SPD in, hierarchy out: the smoothed-aggregation set-up of the AMG coarse solver on K + sigma M"""
    d = mgamd.DoFs(mgamd.Triangulation("annulus", 5), 1, -1)
    base = d.amg_setup_info()
    for sigma in SIGMAS:
        d.set_mass_coefficient(sigma)
        info = d.amg_setup_info()
        assert len(info) >= 2 and info[0] == base[0]  # same pattern on the finest level
        assert all(info[l + 1][0] < info[l][0] for l in range(len(info) - 1))
        assert np.array_equal(d.amg_hierarchy().level(0)["A"][2], d.matrix()[2])  # built on THIS matrix
