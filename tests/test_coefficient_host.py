"""The diffusion coefficient on the host (no GPU): the triangulation carries one value per leaf, coarsening takes the mean over
each coarse leaf, level tables copy it and only form bricks of cells with the bit-identical value, the assembled matrix and the
Gaussian right-hand side follow it, and what is out of scope is refused by name.  Oracle: oracle/physics_oracle.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import physics_oracle as po
import support as su
from physics_oracle import Problem

SIGMAS = [0.0, 7.5]


def _csr(d):
    ptr, col, val = d.matrix()
    return sp.csr_matrix((val, col.astype(np.int64), ptr.astype(np.int64)), shape=(d.n_dofs, d.n_dofs))


def _tria(mgamd, geo, L, field):
    t = mgamd.Triangulation(geo, L)
    t.set_coefficient(po.product_values(t, po.field_on(po.product_cells(t), field)))
    return t


def _slots(d, t):
    """{(group, slot): values of its cells} and the brick size of every group"""
    grp, slot = d.cell_slots()
    a = t.coefficient()
    out = {}
    for c in range(len(grp)):
        out.setdefault((int(grp[c]), int(slot[c])), []).append(a[c])
    return out, list(d.info.group_B)


# ------------------------------------------------------------------ the triangulation
def test_round_trip_and_reset(mgamd):
    t = mgamd.Triangulation("quadrant", 3)
    assert not t.has_coefficient() and np.array_equal(t.coefficient(), np.ones(t.n_cells))
    a = np.linspace(0.5, 9.0, t.n_cells)
    t.set_coefficient(a)
    assert t.has_coefficient() and np.array_equal(t.coefficient(), a)
    t.set_coefficient(None)
    assert not t.has_coefficient() and np.array_equal(t.coefficient(), np.ones(t.n_cells))
    t.set_coefficient_function(lambda x, y, z: 2.0 + x)
    assert np.array_equal(t.coefficient(), 2.0 + t.cell_centres()[:, 0])


@pytest.mark.parametrize("geo,L", [("quadrant", 3), ("hypercube", 3), ("annulus", 5)])
@pytest.mark.parametrize("name", ["uniform", "octants", "inclusion", "per_cell"])
def test_coarsen_takes_the_mean_over_each_coarse_leaf(mgamd, geo, L, name):
    """every mesh of the coarsening sequence against the oracle's volume-weighted mean of the FINEST field"""
    fine = _tria(mgamd, geo, L, po.FIELDS[name])
    finest = po.field_on(po.product_cells(fine), po.FIELDS[name])
    seq = mgamd.create_geometric_coarsening_sequence(fine)
    assert len(seq) > 2
    worst = 0.0
    for t in seq[:-1]:
        assert t.has_coefficient()
        ref = po.product_values(t, po.restrict_field(finest, po.product_cells(t)))
        worst = max(worst, np.abs(t.coefficient() / ref - 1.0).max())
    print(f"{geo} L={L} {name}: {len(seq)} meshes, worst relative difference of a coarse coefficient {worst:.2e}")
    assert worst <= 1e-15
    if name == "uniform":
        assert all(np.array_equal(t.coefficient(), np.full(t.n_cells, 3.5)) for t in seq)


def test_coarsen_without_a_coefficient_carries_none(mgamd):
    assert not mgamd.Triangulation("quadrant", 3).coarsen().has_coefficient()


# ------------------------------------------------------------------ slots
@pytest.mark.parametrize("geo,L,p,max_brick", [("quadrant", 3, 1, 0), ("quadrant", 3, 2, 0), ("quadrant", 3, 4, 0), ("quadrant", 4, 1, 0),
                                               ("hypercube", 3, 2, 0), ("hypercube", 3, 4, 0), ("quadrant", 3, 4, 1)])
@pytest.mark.parametrize("name", ["uniform", "octants", "inclusion", "per_cell"])
def test_every_slot_has_one_bit_identical_value(mgamd, geo, L, p, max_brick, name):
    t = _tria(mgamd, geo, L, po.FIELDS[name])
    d = mgamd.DoFs(t, p, max_brick)
    slots, B = _slots(d, t)
    for (g, s), vals in slots.items():
        assert len(vals) == B[g] ** 3
        assert len(set(np.asarray(vals).view(np.uint64).tolist())) == 1, (g, s, vals)
    if name == "per_cell":
        assert all(B[g] == 1 for g, _ in slots)  # no two neighbours agree: every brick is split
    if name == "uniform":  # the slot structure is that of the mesh without a coefficient
        d0 = mgamd.DoFs(mgamd.Triangulation(geo, L), p, max_brick)
        assert all(np.array_equal(x, y) for x, y in zip(d.cell_slots(), d0.cell_slots()))
    assert d.coefficient_range() == (t.coefficient().min(), t.coefficient().max())


def test_octants_keep_the_eight_bricks_of_p4_and_split_the_brick_of_p2(mgamd):
    t = _tria(mgamd, "hypercube", 3, po.octants)
    slots, B = _slots(mgamd.DoFs(t, 4, 0), t)
    bricks = [vals[0] for (g, s), vals in slots.items() if B[g] == 4]
    assert len(bricks) == 8 and len(slots) == 8
    assert sorted(bricks) == [1.0 + 0.75 * o for o in range(8)] and sum(v != 1.0 for v in bricks) >= 4
    # p = 2: the mesh is ONE 8^3 brick without a coefficient; the jumps through 0 split it
    slots0, B0 = _slots(mgamd.DoFs(mgamd.Triangulation("hypercube", 3), 2, 0), t)
    assert len(slots0) == 1 and B0[next(iter(slots0))[0]] == 8
    slots2, B2 = _slots(mgamd.DoFs(t, 2, 0), t)
    assert len(slots2) > 1 and max(B2[g] for g, _ in slots2) < 8


# ------------------------------------------------------------------ assembled matrix and right-hand side
@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 1), ("quadrant", 3, 2), ("quadrant", 3, 4), ("hypercube", 2, 4)])
@pytest.mark.parametrize("name", ["uniform", "octants", "inclusion", "per_cell"])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_assembled_matrix_and_gaussian_right_hand_side(mgamd, oracle, geo, L, p, name, sigma):
    t = _tria(mgamd, geo, L, po.FIELDS[name])
    d = mgamd.DoFs(t, p, 0)
    d.set_mass_coefficient(sigma)
    lv = su.oracle_level(d, geo, L, p, Problem(sigma, name))
    A = _csr(d)
    diff = (A - lv.A).tocsr()
    err = (abs(diff).max() if diff.nnz else 0.0) / abs(lv.A).max()
    ref = lv.rhs_function(po.gaussian_load(sigma), oracle.gaussian_solution)
    got = d.rhs_function(1)
    eb = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{geo} L={L} p={p} {name} sigma={sigma}: matrix {err:.2e}, rhs_function(1) {eb:.2e}")
    assert err <= 1e-13 and eb <= 1e-13
    assert abs(A - A.T).max() <= 1e-13 * abs(A).max()
    assert np.array_equal(d.rhs_function(0), d.rhs_constant())  # f = 1, g = 0: no lifting, no coefficient


def test_a_coefficient_set_later_does_not_reach_existing_tables(mgamd):
    t = mgamd.Triangulation("quadrant", 3)
    d0 = mgamd.DoFs(t, 2, 0)
    A0, b0 = d0.matrix()[2].copy(), d0.rhs_function(1)
    t.set_coefficient(np.full(t.n_cells, 3.5))
    assert d0.coefficient_range() == (1.0, 1.0)
    assert np.array_equal(d0.matrix()[2], A0) and np.array_equal(d0.rhs_function(1), b0)
    d1 = mgamd.DoFs(t, 2, 0)
    assert d1.coefficient_range() == (3.5, 3.5)
    free = np.arange(d1.n_dofs) < d1.info.n_interior + d1.info.n_tail
    A1 = _csr(d1)
    assert abs(A1[free][:, free] - 3.5 * _csr(d0)[free][:, free]).max() <= 1e-13 * abs(A1).max()
    t.set_coefficient(None)
    assert d1.coefficient_range() == (3.5, 3.5)


# ------------------------------------------------------------------ refusals
def test_refused_values_name_the_index_and_the_value(mgamd):
    t = mgamd.Triangulation("quadrant", 3)
    good = np.linspace(1.0, 2.0, t.n_cells)
    t.set_coefficient(good)
    for at, bad, word in ((5, 0.0, "0.0"), (17, -2.5, "-2.5"), (0, float("nan"), "nan"), (t.n_cells - 1, float("inf"), "inf")):
        a = good.copy()
        a[at] = bad
        with pytest.raises(mgamd.MgamdError, match=f"cell {at} is {word}"):
            t.set_coefficient(a)
        assert np.array_equal(t.coefficient(), good)  # a refused field changes nothing
    with pytest.raises(ValueError):
        t.set_coefficient(good[:-1])


def test_local_smoothing_refuses_a_coefficient(mgamd):
    t = mgamd.Triangulation("quadrant", 3)
    t.set_coefficient(np.full(t.n_cells, 3.5))
    with pytest.raises(mgamd.MgamdError, match="local smoothing with a coefficient is not implemented"):
        t.level_mesh(t.n_levels - 1)
    t.set_coefficient(None)
    lm = t.level_mesh(t.n_levels - 1)
    lm.set_coefficient(np.full(lm.n_cells, 3.5))  # a level mesh is a triangulation; its local-smoothing tables refuse
    with pytest.raises(mgamd.MgamdError, match="not implemented"):
        mgamd.DoFs(lm, 2, 0, local_smoothing_level=True)


def test_sharded_amg_plans_refuse_a_global_space_with_another_coefficient(mgamd):
    fine = _tria(mgamd, "quadrant", 4, po.octants)
    trias = mgamd.create_geometric_coarsening_sequence(fine)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    loc = mgamd.DoFs(fine, 1, -1, part, len(trias) - 1, 1)
    glob = mgamd.DoFs(fine, 1, -1)
    rows = mgamd.amg_shard_match_rows(glob, loc)
    assert len(rows) == loc.n_dofs and len(set(rows.tolist())) == loc.n_dofs
    lo, hi = loc.coefficient_range()
    assert 1.0 <= lo < hi <= 6.25
    fine.set_coefficient(None)
    with pytest.raises(mgamd.MgamdError, match="diffusion coefficient"):
        mgamd.amg_shard_match_rows(mgamd.DoFs(fine, 1, -1), loc)
