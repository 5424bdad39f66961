"""Per-face boundary conditions on the host (no GPU): the triangulation carries a 6-bit mask of its Dirichlet faces, coarsening
inherits it, level tables copy it and classify boundary DoFs by it, the assembled matrix, the right-hand sides, distribute and the
boundary flux load follow, and what is out of scope is refused by name.  Oracle: oracle/physics_oracle.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import physics_oracle as po
import random_mesh_physics as rp
import support as su
from physics_oracle import Problem

# (mask, sigma): M0 has no Dirichlet DoF and needs the mass term
MASKS = [(po.M1, 0.0), (po.M2, 0.0), (po.M0, 7.5)]

def _csr(d):
    ptr, col, val = d.matrix()
    return sp.csr_matrix((val, col.astype(np.int64), ptr.astype(np.int64)), shape=(d.n_dofs, d.n_dofs))


def _info_tuple(d):
    i = d.info
    return (i.n_dofs, i.n_interior, i.n_tail, i.n_dirichlet, i.n_hanging, i.n_groups, list(i.group_B), list(i.group_slots), i.n_edge)


def _check_level(oracle, d, lv, tag):
    """the product's tables d against the re-masked oracle level lv in the same numbering"""
    i = d.info
    first_d = i.n_interior + i.n_tail + i.n_edge
    got_d = set(range(first_d, first_d + i.n_dirichlet))
    assert got_d == set(np.flatnonzero(lv.dirichlet & ~lv.hanging).tolist())
    assert set(range(first_d + i.n_dirichlet, i.n_dofs)) == set(np.flatnonzero(lv.hanging).tolist())
    A = _csr(d)
    diff = (A - lv.A).tocsr()
    e_A = (abs(diff).max() if diff.nnz else 0.0) / abs(lv.A).max()
    e_c = np.abs(d.rhs_function(0) - lv.rhs_constant).max() / np.abs(lv.rhs_constant).max()
    ref = lv.rhs_function(po.gaussian_load(lv.mass_coefficient), oracle.gaussian_solution)
    e_g = np.abs(d.rhs_function(1) - ref).max() / np.abs(ref).max()
    x = np.random.default_rng(3).standard_normal(lv.n)
    x[lv.constrained] = 0.0
    ref = lv.distribute(x, oracle.gaussian_solution)
    e_d = np.abs(d.distribute(x, 1) - ref).max() / np.abs(ref).max()
    q = np.array([0.0 if (lv.dirichlet_faces >> f) & 1 else 1.0 + 0.5 * f for f in range(6)])
    ref = po.flux_load(lv, q)
    got = d.rhs_boundary_flux(q)
    e_q = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{tag}: n_dirichlet {i.n_dirichlet} n_hanging {i.n_hanging} matrix {e_A:.2e} rhs Constant {e_c:.2e} Gaussian {e_g:.2e} "
          f"distribute {e_d:.2e} flux load {e_q:.2e}")
    assert e_A <= 1e-13 and e_c <= 1e-13 and e_g <= 1e-13 and e_d <= 1e-13 and e_q <= 1e-13
    assert np.all(got[lv.constrained] == 0.0) and np.abs(ref).max() > 0
    assert abs(A - A.T).max() <= 1e-13 * abs(A).max()


# ------------------------------------------------------------------ the triangulation
def test_mask_round_trip_defaults_and_coarsening(mgamd):
    t = mgamd.Triangulation("quadrant", 3)
    assert t.dirichlet_faces() == 63 == mgamd.ALL_DIRICHLET
    t.set_dirichlet_faces(po.M2)
    assert t.dirichlet_faces() == po.M2
    seq = mgamd.create_geometric_coarsening_sequence(t)
    assert len(seq) > 2 and all(s.dirichlet_faces() == po.M2 for s in seq)
    assert t.coarsen().coarsen().dirichlet_faces() == po.M2
    lev, i, j, k, _ = t.cells()
    assert mgamd.Triangulation.from_leaves(lev, i, j, k).dirichlet_faces() == 63
    d = mgamd.DoFs(t, 2, 0)
    assert d.dirichlet_faces() == po.M2
    t.set_dirichlet_faces(po.M1)  # tables that exist keep their copy
    assert d.dirichlet_faces() == po.M2 and mgamd.DoFs(t, 2, 0).dirichlet_faces() == po.M1


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 1), ("quadrant", 3, 2), ("quadrant", 3, 4), ("hypercube", 3, 2)])
def test_default_mask_set_explicitly_is_bit_identical(mgamd, geo, L, p):
    t0, t1 = mgamd.Triangulation(geo, L), mgamd.Triangulation(geo, L)
    t1.set_dirichlet_faces(0x3F)
    d0, d1 = mgamd.DoFs(t0, p, 0), mgamd.DoFs(t1, p, 0)
    assert np.array_equal(d0.keys(), d1.keys()) and np.array_equal(d0.cell_dofs(), d1.cell_dofs())
    assert _info_tuple(d0) == _info_tuple(d1)
    assert all(np.array_equal(a, b) for a, b in zip(d0.matrix(), d1.matrix()))
    assert np.array_equal(d0.rhs_function(1), d1.rhs_function(1))


# ------------------------------------------------------------------ tables, matrix, right-hand sides, distribute, flux load
@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("mask,sigma", MASKS)
def test_quadrant_against_the_oracle(mgamd, oracle, p, mask, sigma):
    t = mgamd.Triangulation("quadrant", 3)
    t.set_dirichlet_faces(mask)
    d = mgamd.DoFs(t, p, 0)
    d.set_mass_coefficient(sigma)
    lv = su.oracle_level(d, "quadrant", 3, p, Problem(sigma, dirichlet_faces=mask))
    if mask == po.M1:  # the refined corner touches x = -1: hanging nodes on both kinds of face
        top, k = p << oracle.LMAX, np.array(lv.keys)[lv.hanging]
        assert np.any(k[:, 0] == 0) and np.any((k[:, 1] == 0) | (k[:, 2] == 0))
    if mask == po.M0:
        assert d.info.n_dirichlet == 0
    _check_level(oracle, d, lv, f"quadrant 3 p={p} mask={mask:#04x} sigma={sigma}")


def test_remask_is_what_the_level_class_builds(mgamd, oracle):
    """the shortcut of this file (one constraint search in the oracle's own numbering, cached, renumbered to the product's tables,
    then the level formed with the mask) against a level formed on a space built directly in that numbering, and against the
    vectors recorded from the levels the mask was first written for"""
    mesh = oracle.create_mesh("quadrant", 3)
    for (mask, sigma), name in zip(MASKS, ("M1", "M2", "M0_sigma")):
        keys = mgamd.DoFs(su.tria(mgamd, "quadrant", 3, Problem(dirichlet_faces=mask)), 2, 0).keys()
        direct = po.Level(po.Space(mesh, 2, numbering_keys=keys), Problem(sigma, dirichlet_faces=mask))
        short = su.oracle_level(keys, "quadrant", 3, 2, Problem(sigma, dirichlet_faces=mask))
        assert np.array_equal(direct.dirichlet, short.dirichlet) and np.array_equal(direct.constrained, short.constrained)
        assert abs(direct.A - short.A).max() <= 1e-15 * abs(direct.A).max()
        assert np.abs(direct.rhs_constant - short.rhs_constant).max() <= 1e-15
        su.assert_recorded(su.oracle_level(None, "quadrant", 2, 1, Problem(sigma, dirichlet_faces=mask)), name)


@pytest.mark.parametrize("mg_type,p", [("HMG-global", 2), ("PMG", 2)])
def test_mask_transfers_is_what_build_transfer_gives(oracle, mg_type, p):
    """the transfers of a mask derived from those of mask 0 (physics_oracle.mask_transfers) against build_transfer on the levels
    of the mask"""
    meshes, degs = po.level_plan("quadrant", 3, p, mg_type)
    base = [su.space(m, q) for m, q in zip(meshes, degs)]
    P0 = po.natural_transfers(base)
    for mask, sigma in MASKS:
        levels = [po.Level(s, Problem(sigma, dirichlet_faces=mask)) for s in base]
        P, ref = po.mask_transfers(P0, levels), [None] + [oracle.build_transfer(levels[l], levels[l - 1]) for l in range(1, len(levels))]
        for l in range(1, len(levels)):
            assert P[l].shape == ref[l].shape and abs(P[l] - ref[l]).max() == 0.0 and ref[l].nnz > 0


@pytest.mark.parametrize("mask,sigma", MASKS)
def test_random_octree_against_the_oracle(mgamd, oracle, mask, sigma):
    name, p = "M", 2
    t = su.tria_of(mgamd, rp.leaves_of(oracle, name), Problem(coefficient="per_family"))
    t.set_dirichlet_faces(mask)
    d = mgamd.DoFs(t, p, 0)
    d.set_mass_coefficient(sigma)
    assert d.info.n_hanging > 0
    lv = su.oracle_level_on(d, rp.leaves_of(oracle, name), p, Problem(sigma, "per_family", mask))
    _check_level(oracle, d, lv, f"random octree {name} p={p} per_family mask={mask:#04x} sigma={sigma}")


# ------------------------------------------------------------------ partitions
def _classes(d):
    k, i = [tuple(r) for r in d.keys().tolist()], d.info
    first_d = i.n_interior + i.n_tail + i.n_edge
    return set(k[:i.n_interior + i.n_tail]), set(k[first_d:first_d + i.n_dirichlet]), set(k[first_d + i.n_dirichlet:])


@pytest.mark.parametrize("mask", [po.M1, po.M2, po.M0])
def test_two_rank_partition_classifies_like_the_global_level(mgamd, mask):
    fine = mgamd.Triangulation("quadrant", 3)
    fine.set_dirichlet_faces(mask)
    trias = mgamd.create_geometric_coarsening_sequence(fine)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    lvl, p = len(trias) - 1, 2
    full = mgamd.DoFs(trias[lvl], p, 0)
    loc = [mgamd.DoFs(trias[lvl], p, 0, part, lvl, r) for r in range(2)]
    assert all(d.dirichlet_faces() == mask for d in loc)
    free, dirichlet, hanging = _classes(full)
    parts = [_classes(d) for d in loc]
    assert set.union(*[c[0] for c in parts]) == free
    assert set.union(*[c[1] for c in parts]) == dirichlet
    assert set.union(*[c[2] for c in parts]) == hanging
    assert sum(d.info.n_interior + d.info.n_tail_owned for d in loc) == full.info.n_interior + full.info.n_tail
    assert sum(d.info.n_dirichlet_owned for d in loc) == full.info.n_dirichlet
    # the flux load, summed over the ranks through the keys, is the global one
    q = np.array([0.0 if (mask >> f) & 1 else 2.0 + f for f in range(6)])
    acc = {}
    for d in loc:
        for key, v in zip([tuple(r) for r in d.keys().tolist()], d.rhs_boundary_flux(q)):
            acc[key] = acc.get(key, 0.0) + v
    ref = full.rhs_boundary_flux(q)
    got = np.array([acc[tuple(r)] for r in full.keys().tolist()])
    assert np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max()


# ------------------------------------------------------------------ refusals
def test_refusals_by_message(mgamd):
    t = mgamd.Triangulation("quadrant", 3)
    with pytest.raises(mgamd.MgamdError, match="mask 64 refused.*at most 63"):
        t.set_dirichlet_faces(64)
    with pytest.raises(mgamd.MgamdError, match="refused"):
        t.set_dirichlet_faces(-1)
    assert t.dirichlet_faces() == 63
    t.set_dirichlet_faces(po.M1)
    d = mgamd.DoFs(t, 2, 0)
    with pytest.raises(mgamd.MgamdError, match=r"face 0 \(x=-1\) refused: the face is Dirichlet"):
        d.rhs_boundary_flux([1.0, 0, 0, 0, 0, 0])
    with pytest.raises(mgamd.MgamdError, match="faces are 0 to 5"):
        d.rhs_boundary_flux({6: 1.0})
    assert np.abs(d.rhs_boundary_flux({1: 1.0})).max() > 0
    with pytest.raises(mgamd.MgamdError, match="level_mesh: the triangulation carries the dirichlet_faces mask 1"):
        t.level_mesh(1)
    t.set_dirichlet_faces(63)
    assert t.level_mesh(1).n_cells > 0
    with pytest.raises(mgamd.MgamdError, match="face 3"):
        mgamd.DoFs(t, 2, 0).rhs_boundary_flux({3: 0.5})  # all Dirichlet: no face takes a flux


def test_amg_setup_refuses_the_singular_operator(mgamd):
    t = mgamd.Triangulation("hypercube", 2)
    t.set_dirichlet_faces(0)
    d = mgamd.DoFs(t, 1, 0)
    assert d.info.n_dirichlet == 0 and d.info.n_hanging == 0
    with pytest.raises(mgamd.MgamdError, match="singular: dirichlet_faces mask 0.*sigma = 0"):
        d.amg_setup_info()
    A = _csr(d)  # the matrix itself stays available: symmetric, the constants in its kernel
    assert np.abs(A @ np.ones(d.n_dofs)).max() <= 1e-13 * abs(A).max()
    d.set_mass_coefficient(7.5)
    assert len(d.amg_setup_info()) >= 1


# ------------------------------------------------------------------ known answer
def _exact(x, planes, values, q, dirichlet_face):
    """u(x) with a u' = q from u(-1) = 0 (dirichlet_face 0), or -a u' = q from u(+1) = 0 (dirichlet_face 1): q times the thermal
    resistance between the Dirichlet face and x"""
    edges = np.concatenate(([-1.0], planes, [1.0]))
    out = np.zeros_like(x)
    for lo, hi, a in zip(edges[:-1], edges[1:], values):
        out += (np.clip(x, lo, hi) - lo) / a if dirichlet_face == 0 else (hi - np.clip(x, lo, hi)) / a
    return q * out


@pytest.mark.parametrize("dirichlet_face", [0, 1])
@pytest.mark.parametrize("geo,L,p,planes,values", [("quadrant", 3, 2, [0.0], [1.0, 4.0]), ("quadrant", 3, 4, [0.0], [1.0, 4.0]),
                                                   ("hypercube", 2, 3, [-0.5, 0.0], [1.0, 5.0, 0.2])])
def test_layered_wall_known_answer(mgamd, oracle, geo, L, p, planes, values, dirichlet_face):
    """f = 0, u = 0 on one x face, flux 3 through the opposite one, a constant between planes that are faces of every leaf: the
    exact solution is piecewise linear in x and lies in the FE space, hanging nodes included.  The product's matrix and flux load,
    solved with scipy and distributed, reproduce it.  On quadrant the hanging nodes lie once on the Dirichlet and once on the flux
    face.  Measured with the oracle alone: 4e-14 (quadrant p = 2), 1.2e-13 (p = 4), 1.3e-14 (hypercube 2 p = 3)."""
    q = 3.0
    t = mgamd.Triangulation(geo, L)
    t.set_dirichlet_faces(1 << dirichlet_face)
    t.set_coefficient_function(lambda x, y, z: su.layers(x, planes, values))
    d = mgamd.DoFs(t, p, 0)
    b = d.rhs_boundary_flux({1 - dirichlet_face: q})
    u = d.distribute(spla.spsolve(_csr(d).tocsc(), b), 0)
    x = su.oracle_level(d, geo, L, p).node_positions()[:, 0]
    ref = _exact(x, planes, values, q, dirichlet_face)
    err = np.abs(u - ref).max() / np.abs(ref).max()
    print(f"{geo} {L} p={p} layers {values}, Dirichlet face {dirichlet_face}: n_hanging {d.info.n_hanging}, face temperature "
          f"{ref.max():.6f}, relative nodal error {err:.2e}")
    assert err <= 1e-12
