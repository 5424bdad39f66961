"""Non-zero Dirichlet data on the host (no GPU): the table of cells that gather a Dirichlet DoF, the lifting b_I -= A_ID g, the
distribute for caller data, the per-face constants, a two-rank partition and what is refused, by name.
Oracle: oracle/physics_oracle.py, and tests/dirichlet_data_oracle.py for the theta steppers."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import dirichlet_data_oracle as do
import physics_oracle as po
import support as su
import time_stepping_oracle as tso
from conftest import ROOT, rel_err
from physics_oracle import Problem

TOL_LOAD = 1e-13  # test_boundary_host.py's bound for loads
MASKS = [po.ALL, po.M1, po.M2]


def _product(mgamd, geo, L, p, mask, sigma, field=None, robin=None):
    t = mgamd.Triangulation(geo, L)
    t.set_dirichlet_faces(mask)
    if field is not None:
        t.set_coefficient_function(po.XYZ[field])
    if robin is not None:
        t.set_robin_coefficients(robin)
    d = mgamd.DoFs(t, p, 0)
    d.set_mass_coefficient(sigma)
    return d


def _oracle_level(oracle, geo, L, p, mask, sigma, d, field=None):
    return su.oracle_level(d, geo, L, p, Problem(sigma, field, mask))


def _csr(d):
    ptr, col, val = d.matrix()
    return sp.csr_matrix((val, col.astype(np.int64), ptr.astype(np.int64)), shape=(d.n_dofs, d.n_dofs))


# ------------------------------------------------------------------ table, lifting, distribute
@pytest.mark.parametrize("L,p", [(2, 1), (2, 2), (2, 4), (3, 1), (3, 2), (3, 4)])
def test_table_lift_and_distribute_against_the_oracle(mgamd, oracle, L, p):
    rng = np.random.default_rng(5)
    n_cells = {2: 15, 3: 120}[L]
    for mask in MASKS:
        for field in (None, "octants"):
            for sigma in (0.0, 7.5):
                d = _product(mgamd, "quadrant", L, p, mask, sigma, field)
                lv = _oracle_level(oracle, "quadrant", L, p, mask, sigma, d, field)
                assert len(lv.cells) == n_cells == d.info.n_cells
                i = d.info
                first_d = i.n_interior + i.n_tail + i.n_edge
                # the table: as many cells as gather a Dirichlet DoF, their Dirichlet entries in the Dirichlet range
                idx, hmask, scale = d.dirichlet_cells()
                assert len(idx) == po.n_cells_with_dirichlet_dof(lv) and 0 < len(idx) <= n_cells
                in_range = (idx >= first_d) & (idx < first_d + i.n_dirichlet)
                assert in_range.any(axis=1).all() and (idx < d.n_dofs).all()
                cd = d.cell_dofs()  # INVALID_DOF exactly where the table holds a Dirichlet index
                cd, ti = cd.astype(np.int64), idx.astype(np.int64)
                cd[cd == mgamd.INVALID_DOF], ti[in_range] = -1, -1
                gathers = (cd == -1).any(axis=1)  # (Morton order, as the cells)
                assert np.array_equal(cd[gathers], ti) and np.array_equal(hmask, d.tria.cells()[4][gathers])
                assert np.all(scale[:, 1] > 0) and (np.all(scale[:, 0] >= scale[:, 1]) if field else np.array_equal(scale[:, 0], scale[:, 1]))
                if L == 2:
                    hang = np.array(lv.keys)[lv.hanging]
                    on_boundary = ((hang[:, :3] == 0) | (hang[:, :3] == p << oracle.LMAX)).any(axis=1)
                    assert on_boundary.sum() >= 6
                # g is random on EVERY DoF: the entries at free and hanging DoFs are not read
                g = rng.standard_normal(lv.n)
                for include_mass in (True, False):
                    ref, got = po.lift(lv, g, include_mass), d.rhs_dirichlet(g, include_mass)
                    e = rel_err(got, ref)
                    print(f"quadrant {L} p={p} mask={mask:#04x} {field} sigma={sigma} mass={include_mass}: table {len(idx)} of {n_cells} cells, "
                          f"lift {e:.2e}")
                    assert np.abs(ref).max() > 0
                    assert e <= TOL_LOAD and np.all(got[lv.constrained] == 0.0)
                g2 = g.copy()
                g2[~po.dirichlet_dofs(lv)] = 0.0
                assert np.array_equal(d.rhs_dirichlet(g2), d.rhs_dirichlet(g))
                x = rng.standard_normal(lv.n)
                ref, got = po.distribute_values(lv, x, g), d.distribute_values(x, g)
                free = ~lv.constrained
                assert rel_err(got, ref) <= TOL_LOAD and np.array_equal(got[free], x[free])
                assert np.array_equal(got[po.dirichlet_dofs(lv)], g[po.dirichlet_dofs(lv)])


def test_lift_is_the_matrix_block(mgamd, oracle):
    """on a mesh without a coefficient the lifting is -A_ID g with A_ID from the assembled matrix of the all-natural mesh, in which
    the Dirichlet DoFs of the masked mesh are ordinary unknowns: the product against itself"""
    p, sigma = 2, 7.5
    d = _product(mgamd, "quadrant", 3, p, po.M1, sigma)
    n = _product(mgamd, "quadrant", 3, p, 0, sigma)
    key_n = {tuple(k): i for i, k in enumerate(n.keys().tolist())}
    perm = np.array([key_n[tuple(k)] for k in d.keys().tolist()])
    A = _csr(n)[perm][:, perm]
    i = d.info
    first_d, n_free = i.n_interior + i.n_tail, i.n_interior + i.n_tail
    g = np.zeros(d.n_dofs)
    g[first_d:first_d + i.n_dirichlet] = np.random.default_rng(2).standard_normal(i.n_dirichlet)
    ref = -(A @ g)
    ref[n_free:] = 0.0
    assert rel_err(d.rhs_dirichlet(g), ref) <= TOL_LOAD


def test_gaussian_values_give_the_gaussian_distribute(mgamd, oracle):
    for p in (1, 2, 4):
        for mask in MASKS:
            d = _product(mgamd, "quadrant", 3, p, mask, 0.0)
            pos = d.node_positions()
            lv = _oracle_level(oracle, "quadrant", 3, p, mask, 0.0, d)
            assert np.abs(pos - lv.node_positions()).max() <= 1e-15
            g = oracle.gaussian_solution(pos[:, 0], pos[:, 1], pos[:, 2])
            x = np.random.default_rng(8).standard_normal(d.n_dofs)
            a, b = d.distribute_values(x, g), d.distribute(x, 1)
            assert np.abs(a - b).max() <= 1e-15 * np.abs(b).max()
            # and the lifting of these values is what the Gaussian right-hand side carries on top of its load
            zero_g = po.changed(lv, sigma=0.0)
            load = zero_g.rhs_function(oracle.gaussian_rhs, lambda x, y, z: 0.0 * x)
            full = d.rhs_function(1)  # (the Gaussian is tiny on the boundary: the bound is the rounding of the load it is added to)
            assert np.linalg.norm(d.rhs_dirichlet(g) + load - full) <= TOL_LOAD * np.linalg.norm(full)


def test_gaussian_data_on_a_local_smoothing_level_is_the_recorded_one(mgamd):
    """The Gaussian right-hand side and distribute on the tables of a local-smoothing level (quadrant 3, p = 2, the finest refinement
    level: 64 cells with refinement-edge DoFs, gathered as ordinary indices, their rows constrained), which no oracle test covers.
    tests/golden/ls_level_quadrant3_p2_gaussian.npz holds x and both results as computed before the Gaussian data went through the
    Dirichlet-data path (load and lifting summed per cell); 1e-13 of the largest entry allows the reordered sum and nothing more."""
    fix = np.load(os.path.join(ROOT, "tests", "golden", "ls_level_quadrant3_p2_gaussian.npz"))
    t = mgamd.Triangulation("quadrant", 3)
    d = mgamd.DoFs(t.level_mesh(t.n_levels - 1), 2, 0, local_smoothing_level=True)
    i = d.info
    assert i.n_cells == 64 and i.n_edge > 0 and i.n_dirichlet > 0 and d.n_dofs == len(fix["x"])
    b = d.rhs_function(1)
    for name, got in (("rhs_function_1", b), ("distribute_1", d.distribute(fix["x"], 1))):
        want = fix[name]
        e = np.abs(got - want).max() / np.abs(want).max()
        print(f"local-smoothing level, {name}: {e:.2e} of the largest entry {np.abs(want).max():.3e}")
        assert e <= 1e-13
    assert np.all(b[i.n_interior + i.n_tail:] == 0.0)  # (refinement-edge rows too)


def test_dirichlet_face_values_on_shared_edges_and_corners(mgamd, oracle):
    p = 2
    v = np.array([300.0, 400.0, 5.0, 0.0, 0.0, -7.0])
    mask = 0b100111  # x = -1, x = +1, y = -1, z = +1
    d = _product(mgamd, "quadrant", 3, p, mask, 0.0)
    lv = _oracle_level(oracle, "quadrant", 3, p, mask, 0.0, d)
    g = d.dirichlet_face_values(v)
    assert np.array_equal(g, po.face_values(lv, v))
    assert np.array_equal(g, d.dirichlet_face_values({0: 300.0, 1: 400.0, 2: 5.0, 5: -7.0}))
    keys, top = np.array(lv.keys), p << oracle.LMAX
    edge = np.flatnonzero((keys[:, 0] == 0) & (keys[:, 1] == 0) & (keys[:, 2] > 0) & (keys[:, 2] < top) & ~lv.hanging)
    corner = np.flatnonzero((keys[:, 0] == top) & (keys[:, 1] == 0) & (keys[:, 2] == top))
    edge_yz = np.flatnonzero((keys[:, 0] > 0) & (keys[:, 0] < top) & (keys[:, 1] == 0) & (keys[:, 2] == top) & ~lv.hanging)
    assert len(edge) and len(corner) == 1 and len(edge_yz)
    assert np.all(g[edge] == 300.0) and g[corner[0]] == 400.0 and np.all(g[edge_yz] == 5.0)
    assert np.all(g[~po.dirichlet_dofs(lv)] == 0.0)
    natural = np.flatnonzero((keys[:, 1] == top) & (keys[:, 0] > 0) & (keys[:, 0] < top) & (keys[:, 2] > 0) & (keys[:, 2] < top))
    assert len(natural) and np.all(g[natural] == 0.0)


# ------------------------------------------------------------------ known answer
@pytest.mark.parametrize("p", [1, 2])
def test_linear_function_is_reproduced(mgamd, oracle, p):
    """g = nodal values of 1 + 2x - 3y + 0.5z on all six faces, f = 0, sigma = 0: the solution is that function, at hanging nodes
    too.  The product's matrix and lifting, solved with scipy and distributed (test_boundary_host's known-answer bound, 1e-12)"""
    d = _product(mgamd, "quadrant", 3, p, po.ALL, 0.0)
    pos = d.node_positions()
    exact = 1.0 + 2.0 * pos[:, 0] - 3.0 * pos[:, 1] + 0.5 * pos[:, 2]
    u = d.distribute_values(spla.spsolve(_csr(d).tocsc(), d.rhs_dirichlet(exact)), exact)
    err = np.abs(u - exact).max() / np.abs(exact).max()
    print(f"quadrant 3 p={p}: n_hanging {d.info.n_hanging}, relative nodal error {err:.2e}")
    assert d.info.n_hanging > 0 and err <= 1e-12


# ------------------------------------------------------------------ partitions
@pytest.mark.parametrize("mask", MASKS)
def test_two_rank_partition_sums_to_the_global_lift(mgamd, mask):
    fine = mgamd.Triangulation("quadrant", 3)
    fine.set_dirichlet_faces(mask)
    trias = mgamd.create_geometric_coarsening_sequence(fine)
    part = mgamd.Partition(trias, 2, 2.0, 0)
    lvl, p, sigma = len(trias) - 1, 2, 7.5
    full = mgamd.DoFs(trias[lvl], p, 0)
    loc = [mgamd.DoFs(trias[lvl], p, 0, part, lvl, r) for r in range(2)]
    for d in [full] + loc:
        d.set_mass_coefficient(sigma)
    assert sum(len(d.dirichlet_cells()[0]) for d in loc) == len(full.dirichlet_cells()[0])
    gk = {tuple(k): v for k, v in zip(full.keys().tolist(), np.random.default_rng(4).standard_normal(full.n_dofs))}
    acc = {}
    for d in loc:
        keys = [tuple(r) for r in d.keys().tolist()]
        for key, v in zip(keys, d.rhs_dirichlet(np.array([gk[k] for k in keys]))):
            acc[key] = acc.get(key, 0.0) + v
    ref = full.rhs_dirichlet(np.array([gk[tuple(k)] for k in full.keys().tolist()]))
    got = np.array([acc[tuple(r)] for r in full.keys().tolist()])
    assert np.abs(ref).max() > 0 and np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


# ------------------------------------------------------------------ convective faces, refusals
def test_convective_wall_with_a_hot_wall_is_accepted(mgamd, oracle):
    """beta > 0 on x = +1, the only Dirichlet face x = -1 opposite: no DoF is shared and the face term of the lifting vanishes (the
    oracle's lifting carries the surface matrix and shows it)"""
    p, mask, beta = 2, po.M1, (0.0, 2.5, 0.0, 0.0, 0.0, 0.0)
    d = _product(mgamd, "quadrant", 3, p, mask, 0.0, robin=beta)
    lv = su.oracle_level(d, "quadrant", 3, p, Problem(0.0, None, mask, beta))
    g = d.dirichlet_face_values({0: 350.0})
    ref = po.lift(lv, g)
    assert np.abs(ref).max() > 0 and rel_err(d.rhs_dirichlet(g), ref) <= TOL_LOAD
    with pytest.raises(mgamd.MgamdError, match="SimulationType 1 with Robin coefficients"):
        d.rhs_function(1)  # (the Gaussian lifting keeps its refusal)


def test_refusals_by_message(mgamd):
    d = _product(mgamd, "quadrant", 3, 2, po.M1, 0.0, robin=(0.0, 0.0, 0.0, 0.75, 0.0, 0.0))
    g = np.zeros(d.n_dofs)
    with pytest.raises(mgamd.MgamdError, match=r"convective face 3 \(y=\+1, Robin coefficient 0.75\d*\) shares an edge with the Dirichlet "
                                               r"face 0 \(x=-1\)"):
        d.rhs_dirichlet(g)
    d = _product(mgamd, "quadrant", 3, 2, po.M1, 0.0)
    with pytest.raises(mgamd.MgamdError, match=r"Dirichlet value 2.0\d* on face 3 \(y=\+1\) refused: the face is natural"):
        d.dirichlet_face_values({0: 1.0, 3: 2.0})
    with pytest.raises(mgamd.MgamdError, match=r"face 0 \(x=-1\) is not finite"):
        d.dirichlet_face_values({0: np.nan})
    with pytest.raises(mgamd.MgamdError, match="faces are 0 to 5"):
        d.dirichlet_face_values({6: 1.0})
    with pytest.raises(ValueError, match="values for"):
        d.rhs_dirichlet(np.zeros(d.n_dofs + 1))
    assert np.all(d.dirichlet_face_values({0: 1.0, 3: 0.0})[d.info.n_interior + d.info.n_tail:][:d.info.n_dirichlet] == 1.0)
    t = mgamd.Triangulation("quadrant", 3)
    lvl = mgamd.DoFs(t.level_mesh(2), 2, 0, local_smoothing_level=True)
    assert len(lvl.dirichlet_cells()[0]) > 0  # (the level's own Gaussian right-hand side walks it; caller data stays refused)
    with pytest.raises(mgamd.MgamdError, match="rhs_dirichlet: refused on the level of a local-smoothing hierarchy"):
        lvl.rhs_dirichlet(np.zeros(lvl.n_dofs))
    # mask 0: no Dirichlet DoF, an empty table and a zero lifting
    n = _product(mgamd, "quadrant", 3, 2, 0, 7.5)
    assert len(n.dirichlet_cells()[0]) == 0 and np.all(n.rhs_dirichlet(np.ones(n.n_dofs)) == 0.0)


# ------------------------------------------------------------------ the oracle stepper
def test_increment_form_of_the_oracle_stepper_is_the_direct_step(oracle):
    """dirichlet_data_oracle.theta_step_data (the increment, as the product solves it) against theta_step_direct (u_new itself, every
    term on full vectors), with a source, time-dependent values and a flux load"""
    p, theta, dt, mask = 2, 0.5, 0.05, po.M1
    lv = su.oracle_level(None, "quadrant", 2, p, Problem(tso.mass_coefficient(theta, dt), dirichlet_faces=mask))
    rng = np.random.default_rng(9)
    u = rng.standard_normal(lv.n)
    u[lv.constrained] = 0.0
    f0, f1, g0, g1 = (rng.standard_normal(lv.n) for _ in range(4))
    load = po.flux_load(lv, [0.0, 1.5, 0.0, 0.0, 0.0, 0.0])
    a, _ = do.theta_step_data(lv, u, f0, f1, g0, g1, load, theta, dt, tso.exact_solver(lv))
    b = do.theta_step_direct(lv, u, f0, f1, g0, g1, load, theta, dt)
    assert rel_err(a, b) <= 1e-12
    # without data it is time_stepping_oracle's step
    c, _ = do.theta_step_data(lv, u, f0, f1, None, None, None, theta, dt, tso.exact_solver(lv))
    e, _ = tso.theta_step(lv, u, f0, f1, theta, dt, tso.exact_solver(lv))
    assert rel_err(c, e) <= 1e-12
