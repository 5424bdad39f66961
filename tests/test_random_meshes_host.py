"""Mass term and diffusion coefficient on caller-built random octrees, on the host (no GPU): the assembled matrix of
A = K_a + sigma M, the constant and the Gaussian right-hand side, and the coarse coefficients of the coarsening sequence on the
meshes M (344 cells, levels 2-4) and S (50 cells, levels 1-3) of tests/random_mesh_physics.py, against oracle/physics_oracle.py
on the same leaves through the DoF keys.  Fields: none, per_family (2^3 bricks survive, neighbouring families differ) and per_cell.
On these meshes a coarse cell covers leaves of two or three levels, so the 8^-k weights of the mean are exercised.

The numpy levels come from support.oracle_level_on (one constraint search per mesh and degree, then permuted into the product's
numbering); test_the_renumbered_level_is_the_level_built_directly holds that against a space built directly in that numbering."""
import numpy as np
import pytest
import scipy.sparse as sp

import physics_oracle as po
import random_mesh_physics as rm
import support as su
from physics_oracle import Problem

SIGMAS = [0.0, 7.5, 3000.0]
CASES = [("M", 1), ("M", 2), ("M", 3), ("M", 4), ("S", 5)]
FIELDS = [None, "per_family", "per_cell"]


def _csr(d):
    ptr, col, val = d.matrix()
    return sp.csr_matrix((val, col.astype(np.int64), ptr.astype(np.int64)), shape=(d.n_dofs, d.n_dofs))


def _finest(oracle, name, p, field, sigma, d):
    return su.oracle_level_on(d, rm.leaves_of(oracle, name), p, Problem(sigma, field))


def test_the_renumbered_level_is_the_level_built_directly(mgamd, oracle):
    """the level formed on the cached space renumbered to the product's tables against the level formed on a space built directly
    with numbering_keys, M p = 2 per_family: the same tables, the same matrices up to the order of the sums over the cells; and the
    same path on the recorded mesh against the vectors recorded from a level that was built directly"""
    name, p, field, sigma = "M", 2, "per_family", 7.5
    leaves = rm.leaves_of(oracle, name)
    d = mgamd.DoFs(su.tria_of(mgamd, leaves, Problem(coefficient=field)), p, 0)
    a = _finest(oracle, name, p, field, sigma, d)
    b = po.Level(po.Space(leaves, p, numbering_keys=d.keys()), Problem(sigma, po.field_on(leaves, po.FIELDS[field])))
    assert a.keys == b.keys and a.key_to_dof == b.key_to_dof and np.array_equal(a.cell_dofs, b.cell_dofs)
    for attr in ("dirichlet", "hanging", "constrained"):
        assert np.array_equal(getattr(a, attr), getattr(b, attr)), attr
    for attr in ("Ch", "C", "Kraw", "K0raw", "Mraw", "A"):
        assert abs(getattr(a, attr) - getattr(b, attr)).max() <= 1e-15 * abs(getattr(b, attr)).max(), attr
    assert np.abs(a.inv_diag / b.inv_diag - 1.0).max() <= 1e-15 and np.abs(a.rhs_constant - b.rhs_constant).max() <= 1e-17
    assert a.mass_coefficient == b.mass_coefficient == sigma and a.coefficient == b.coefficient
    su.assert_recorded(su.oracle_level(None, "quadrant", 2, 1, Problem(7.5, "octants")), "octants_sigma")


@pytest.mark.parametrize("name,p", CASES)
@pytest.mark.parametrize("field", FIELDS)
def test_assembled_matrix_and_right_hand_sides(mgamd, oracle, name, p, field):
    leaves = rm.leaves_of(oracle, name)
    t = su.tria_of(mgamd, leaves, Problem(coefficient=field))
    d = mgamd.DoFs(t, p, 0)
    if field is not None:
        rm.assert_slots_differ(mgamd, name, p, field, d, t)
    for sigma in SIGMAS:
        d.set_mass_coefficient(sigma)
        lv = _finest(oracle, name, p, field, sigma, d)
        A = _csr(d)
        diff = (A - lv.A).tocsr()
        err = (abs(diff).max() if diff.nnz else 0.0) / abs(lv.A).max()
        ref = lv.rhs_function(po.gaussian_load(sigma), oracle.gaussian_solution)
        eg = np.abs(d.rhs_function(1) - ref).max() / np.abs(ref).max()
        ec = np.abs(d.rhs_constant() - lv.rhs_constant).max()
        print(f"{name} p={p} {field} sigma={sigma}: matrix {err:.2e}, rhs_function(1) {eg:.2e}, rhs_constant {ec:.2e}")
        assert err <= 1e-13  # test_helmholtz_host.test_assembled_matrix_is_helper_matrix
        assert abs(A - A.T).max() <= 1e-13 * abs(A).max()
        assert eg <= 1e-13  # test_coefficient_host.test_assembled_matrix_and_gaussian_right_hand_side
        assert ec < 1e-14  # test_gpu_random_meshes: f = 1, g = 0 sees neither sigma nor a
        assert np.array_equal(d.rhs_function(0), d.rhs_constant())


@pytest.mark.parametrize("name,p", [("M", 2), ("S", 5)])
@pytest.mark.parametrize("field", ["per_family", "per_cell", "per_block4", "octants"])
def test_coarse_coefficients(mgamd, oracle, name, p, field):
    """every mesh of the product's coarsening sequence against restrict_field of the FINEST field, and coefficient_range of the
    tables built on it"""
    leaves = rm.leaves_of(oracle, name)
    fine = su.tria_of(mgamd, leaves, Problem(coefficient=field))
    finest = po.field_on(leaves, po.FIELDS[field])
    seq = mgamd.create_geometric_coarsening_sequence(fine)
    assert [t.n_cells for t in seq] == [len(m) for m in oracle.coarsening_sequence(leaves)]
    worst, mixed = 0.0, 0
    for t in seq:
        cells = po.product_cells(t)
        cell_set = set(cells)
        ref = po.product_values(t, po.restrict_field(finest, cells))
        worst = max(worst, np.abs(t.coefficient() / ref - 1.0).max())
        # coarse cells that cover finest leaves of more than one level: the weights 8^-k differ inside one mean
        depth = {}
        for (l, i, j, k) in leaves:
            for up in range(l + 1):
                anc = (l - up, i >> up, j >> up, k >> up)
                if anc in cell_set:
                    depth.setdefault(anc, set()).add(up)
                    break
        mixed += sum(len(v) >= 2 for v in depth.values())
        assert mgamd.DoFs(t, p, 0).coefficient_range() == (t.coefficient().min(), t.coefficient().max())
    print(f"{name} {field}: {len(seq)} meshes, {mixed} coarse cells over leaves of several levels, worst relative difference {worst:.2e}")
    assert mixed > 0
    assert worst <= 1e-15
