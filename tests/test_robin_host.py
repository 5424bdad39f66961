"""Convective (Robin) faces on the host (no GPU): the triangulation carries six Robin coefficients, coarsening inherits them, level
tables copy them and build the table of convective cell faces, the assembled matrix carries the face term, a convective face makes
the pure-Neumann box regular, and what is out of scope is refused by name.  Oracle: oracle/physics_oracle.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import physics_oracle as po
import random_mesh_physics as rp
import support as su
from physics_oracle import Problem

SETUPS = [po.R1, po.R2]

def _csr(d):
    ptr, col, val = d.matrix()
    return sp.csr_matrix((val, col.astype(np.int64), ptr.astype(np.int64)), shape=(d.n_dofs, d.n_dofs))


def _tria(mgamd, geo, L, mask, beta):
    t = mgamd.Triangulation(geo, L)
    t.set_dirichlet_faces(mask)
    t.set_robin_coefficients(beta)
    return t


def _info_tuple(d):
    i = d.info
    return (i.n_dofs, i.n_interior, i.n_tail, i.n_dirichlet, i.n_hanging, i.n_groups, list(i.group_B), list(i.group_slots), i.n_edge)


def _check_level(d, lv, tag):
    """index sets and assembled matrix of the product's tables d against the oracle level lv in the same numbering"""
    i = d.info
    first_d = i.n_interior + i.n_tail + i.n_edge
    assert set(range(first_d, first_d + i.n_dirichlet)) == set(np.flatnonzero(lv.dirichlet & ~lv.hanging).tolist())
    assert set(range(first_d + i.n_dirichlet, i.n_dofs)) == set(np.flatnonzero(lv.hanging).tolist())
    A = _csr(d)
    diff = (A - lv.A).tocsr()
    e_A = (abs(diff).max() if diff.nnz else 0.0) / abs(lv.A).max()
    print(f"{tag}: n_dirichlet {i.n_dirichlet} n_hanging {i.n_hanging} face entries {len(d.robin_faces()[2])} matrix {e_A:.2e}")
    assert e_A <= 1e-13
    assert abs(A - A.T).max() <= 1e-13 * abs(A).max()
    return A


# ------------------------------------------------------------------ the triangulation
def test_round_trip_defaults_coarsening_and_copies(mgamd):
    t = mgamd.Triangulation("quadrant", 3)
    assert np.array_equal(t.robin_coefficients(), np.zeros(6))
    mask, beta = po.R1
    t.set_dirichlet_faces(mask)
    t.set_robin_coefficients(beta)
    assert np.array_equal(t.robin_coefficients(), beta)
    seq = mgamd.create_geometric_coarsening_sequence(t)
    assert len(seq) > 2 and all(np.array_equal(s.robin_coefficients(), beta) and s.dirichlet_faces() == mask for s in seq)
    assert np.array_equal(t.coarsen().coarsen().robin_coefficients(), beta)
    lev, i, j, k, _ = t.cells()
    assert np.array_equal(mgamd.Triangulation.from_leaves(lev, i, j, k).robin_coefficients(), np.zeros(6))
    d = mgamd.DoFs(t, 2, 0)
    assert np.array_equal(d.robin_coefficients(), beta)
    t.set_robin_coefficients({0: 1.0})  # tables that exist keep their copy; the dict form sets the other faces to 0
    assert np.array_equal(d.robin_coefficients(), beta)
    assert np.array_equal(mgamd.DoFs(t, 2, 0).robin_coefficients(), [1.0, 0, 0, 0, 0, 0])


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 1), ("quadrant", 3, 2), ("quadrant", 3, 4), ("hypercube", 3, 2)])
def test_zero_coefficients_set_explicitly_are_bit_identical(mgamd, geo, L, p):
    t0, t1 = mgamd.Triangulation(geo, L), mgamd.Triangulation(geo, L)
    for t in (t0, t1):
        t.set_dirichlet_faces(po.M1)
    t1.set_robin_coefficients(np.zeros(6))
    d0, d1 = mgamd.DoFs(t0, p, 0), mgamd.DoFs(t1, p, 0)
    assert np.array_equal(d0.keys(), d1.keys()) and np.array_equal(d0.cell_dofs(), d1.cell_dofs())
    assert _info_tuple(d0) == _info_tuple(d1)
    assert all(np.array_equal(a, b) for a, b in zip(d0.matrix(), d1.matrix()))
    assert np.array_equal(d0.rhs_function(1), d1.rhs_function(1))
    assert len(d0.robin_faces()[2]) == 0 and len(d1.robin_faces()[2]) == 0


# ------------------------------------------------------------------ tables and matrix
@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("setup", SETUPS, ids=["R1", "R2"])
def test_quadrant_against_the_oracle(mgamd, oracle, p, setup):
    mask, beta = setup
    d = mgamd.DoFs(_tria(mgamd, "quadrant", 3, mask, beta), p, 0)
    lv = su.oracle_level(d, "quadrant", 3, p, Problem(0.0, None, mask, beta))
    idx, flags, scale = d.robin_faces()
    assert len(scale) > 0 and (scale > 0).all() and idx.shape == (len(scale), (p + 1) ** 2)
    if setup is po.R1:  # the refined corner touches x = -1: the convective face 0 carries hanging nodes, face 3 none
        assert np.any(flags & 3) and np.any((flags & 3) == 0)
        k = np.array(lv.keys)[lv.hanging]
        assert np.any(k[:, 0] == 0)
        assert np.any(idx == mgamd.INVALID_DOF)  # the edge shared with the Dirichlet face x = +1 (face 3 touches it)
    else:
        assert d.info.n_dirichlet == 0 and not np.any(idx == mgamd.INVALID_DOF)
    A = _check_level(d, lv, f"quadrant 3 p={p} mask={mask:#04x} beta={beta}")
    if setup is po.R2:  # regular only through the faces: without them the constants are in the kernel
        one = np.where(lv.constrained, 0.0, 1.0)
        K = _csr(mgamd.DoFs(_tria(mgamd, "quadrant", 3, mask, np.zeros(6)), p, 0))
        assert np.abs(K @ one).max() <= 1e-12 * abs(K).max() and np.abs(A @ one).max() > 1e-3 * abs(A).max()
        assert one @ (A @ one) == pytest.approx(4.0 * sum(beta), rel=1e-12)  # 1^T B 1 = sum_f beta_f |face f|


def test_face_table_areas(mgamd):
    """the scales of the table are beta_f h^2: per convective face of the cube they add up to beta_f times its area 4"""
    mask, beta = po.R1
    d = mgamd.DoFs(_tria(mgamd, "quadrant", 3, mask, beta), 2, 0)
    _, _, scale = d.robin_faces()
    assert scale.sum() == pytest.approx(4.0 * sum(beta), rel=1e-14)


def test_random_octree_against_the_oracle(mgamd, oracle):
    name, p, sigma = "M", 2, 7.5
    mask, beta = po.R1
    t = su.tria_of(mgamd, rp.leaves_of(oracle, name), Problem(coefficient="per_family"))
    t.set_dirichlet_faces(mask)
    t.set_robin_coefficients(beta)
    d = mgamd.DoFs(t, p, 0)
    d.set_mass_coefficient(sigma)
    assert d.info.n_hanging > 0
    lv = su.oracle_level_on(d, rp.leaves_of(oracle, name), p, Problem(sigma, "per_family", mask, beta))
    _check_level(d, lv, f"random octree {name} p={p} per_family sigma={sigma} R1")


# ------------------------------------------------------------------ partitions
def test_two_rank_partition_covers_every_boundary_face_once(mgamd):
    mask, beta = po.R1
    fine = _tria(mgamd, "quadrant", 3, mask, beta)
    trias = mgamd.create_geometric_coarsening_sequence(fine)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    lvl, p = len(trias) - 1, 2
    full = mgamd.DoFs(trias[lvl], p, 0)
    loc = [mgamd.DoFs(trias[lvl], p, 0, part, lvl, r) for r in range(2)]
    assert all(np.array_equal(d.robin_coefficients(), beta) for d in loc)

    def faces(d):
        k = d.keys()
        idx, flags, scale = d.robin_faces()
        out = []
        for e in range(len(scale)):
            valid = idx[e][idx[e] != mgamd.INVALID_DOF]
            out.append((tuple(sorted(tuple(r) for r in k[valid].tolist())), int(flags[e]), float(scale[e])))
        return out

    ref, parts = faces(full), [faces(d) for d in loc]
    assert all(len(q) > 0 for q in parts)  # both ranks hold convective faces
    assert len(set(ref)) == len(ref) and sorted(parts[0] + parts[1]) == sorted(ref)


# ------------------------------------------------------------------ refusals
def test_refusals_by_message(mgamd):
    t = mgamd.Triangulation("quadrant", 3)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(mgamd.MgamdError, match=r"Robin coefficient \S+ on face 2 refused: it must be finite and >= 0"):
            t.set_robin_coefficients([0, 0, bad, 0, 0, 0])
    with pytest.raises(mgamd.MgamdError, match="Robin coefficient 2.5\\d* on face 0 refused: the face is Dirichlet"):
        t.set_robin_coefficients(po.R1[1])  # the default mask: every face is Dirichlet
    with pytest.raises(mgamd.MgamdError, match="faces are 0 to 5"):
        t.set_robin_coefficients({6: 1.0})
    assert np.array_equal(t.robin_coefficients(), np.zeros(6))
    t.set_dirichlet_faces(po.R1[0])
    t.set_robin_coefficients(po.R1[1])
    with pytest.raises(mgamd.MgamdError, match="mask 63 refused: face 0 carries the Robin coefficient 2.5"):
        t.set_dirichlet_faces(63)  # the other order
    assert t.dirichlet_faces() == po.R1[0]
    with pytest.raises(mgamd.MgamdError, match="level_mesh: the triangulation carries Robin coefficients"):
        t.level_mesh(1)
    with pytest.raises(mgamd.MgamdError, match="local-smoothing level tables of a triangulation with Robin coefficients"):
        mgamd.DoFs(t, 2, 0, local_smoothing_level=True)
    d = mgamd.DoFs(t, 2, 0)
    with pytest.raises(mgamd.MgamdError, match="SimulationType 1 with Robin coefficients.*not implemented"):
        d.rhs_function(1)
    assert np.abs(d.rhs_function(0)).max() > 0
    # the load of u_ext is the flux load on the convective face; only Dirichlet faces refuse one
    assert np.abs(d.rhs_boundary_flux({0: 2.5 * 3.0})).max() > 0
    with pytest.raises(mgamd.MgamdError, match=r"face 1 \(x=\+1\) refused: the face is Dirichlet"):
        d.rhs_boundary_flux({1: 1.0})
    t.set_robin_coefficients(np.zeros(6))
    t.set_dirichlet_faces(63)
    assert t.level_mesh(1).n_cells > 0


def test_sharded_amg_plans_refuse_a_global_space_with_other_robin_coefficients(mgamd):
    mask, beta = po.R1
    fine = _tria(mgamd, "quadrant", 4, mask, beta)
    trias = mgamd.create_geometric_coarsening_sequence(fine)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    glob = mgamd.DoFs(fine, 1, -1)
    loc = mgamd.DoFs(fine, 1, -1, part, len(trias) - 1, 1)
    rows = mgamd.amg_shard_match_rows(glob, loc)
    assert len(rows) == loc.n_dofs and len(set(rows.tolist())) == loc.n_dofs
    fine.set_robin_coefficients({0: 2.5, 3: 1.0})
    with pytest.raises(mgamd.MgamdError, match="Robin coefficient 1.0\\d* on face 3, the local level 0.75"):
        mgamd.amg_shard_match_rows(mgamd.DoFs(fine, 1, -1), loc)


def test_a_convective_face_makes_the_neumann_box_regular(mgamd):
    """mask 0, sigma 0: refused as singular with every beta 0, accepted by the matrix and AMG-setup entries with R2"""
    t = mgamd.Triangulation("hypercube", 2)
    t.set_dirichlet_faces(0)
    d = mgamd.DoFs(t, 1, 0)
    with pytest.raises(mgamd.MgamdError, match="singular: dirichlet_faces mask 0.*sigma = 0"):
        d.amg_setup_info()
    t.set_robin_coefficients(po.R2[1])
    with pytest.raises(mgamd.MgamdError, match="singular"):
        d.amg_setup_info()  # the tables keep their copy
    d = mgamd.DoFs(t, 1, 0)
    assert len(d.amg_setup_info()) >= 1
    A = _csr(d)
    assert np.linalg.eigvalsh(A.toarray()).min() > 1e-3


# ------------------------------------------------------------------ known answer
@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 2), ("hypercube", 2, 3)])
def test_convective_wall_known_answer(mgamd, oracle, geo, L, p):
    """three layers 1 | 5 | 0.2 between planes that are faces of every leaf, f = 0, u = 0 on x = -1, a convective face at x = +1 with
    beta and u_ext: the flux is q = beta u_ext / (1 + beta R), R = sum d_k / a_k the wall's resistance, the solution q times the
    resistance between x = -1 and x: piecewise linear, in the FE space, hanging nodes included.  The product's matrix and flux load
    (q_f = beta u_ext), solved with scipy and distributed, reproduce it."""
    planes, values, beta, u_ext = [-0.5, 0.0], [1.0, 5.0, 0.2], 2.0, 7.0
    t = mgamd.Triangulation(geo, L)
    t.set_dirichlet_faces(0b000001)
    t.set_robin_coefficients({1: beta})
    t.set_coefficient_function(lambda x, y, z: su.layers(x, planes, values))
    d = mgamd.DoFs(t, p, 0)
    b = d.rhs_boundary_flux({1: beta * u_ext})
    u = d.distribute(spla.spsolve(_csr(d).tocsc(), b), 0)
    x = su.oracle_level(d, geo, L, p).node_positions()[:, 0]
    edges = np.concatenate(([-1.0], planes, [1.0]))
    R = sum((hi - lo) / a for lo, hi, a in zip(edges[:-1], edges[1:], values))
    q = beta * u_ext / (1.0 + beta * R)
    ref = q * sum((np.clip(x, lo, hi) - lo) / a for lo, hi, a in zip(edges[:-1], edges[1:], values))
    err = np.abs(u - ref).max() / np.abs(ref).max()
    print(f"{geo} {L} p={p} layers {values} beta {beta} u_ext {u_ext}: n_hanging {d.info.n_hanging}, face temperature {q * R:.6f}, "
          f"relative nodal error {err:.2e}")
    assert ref.max() == pytest.approx(q * R, rel=1e-14) and err <= 1e-12
