"""Known-answer tests that pin the oracle (the reference ships no golden vectors,
so the oracle is pinned against mathematics, not against deal.II output: 'parity unpinned')."""
import numpy as np
import pytest

# Appendix B of SURVEY.md (derived independently during the survey)
QUADRANT_CELLS = {0: 1, 1: 8, 2: 15, 3: 120, 4: 701}
QUADRANT_DOFS = {1: {0: 8, 1: 27, 2: 46, 3: 223, 4: 1008}, 2: {0: 27, 1: 125, 2: 235, 3: 1375}, 4: {0: 125, 1: 729, 2: 1387, 3: 9295}}
QUADRANT_HN = {3: 37, 4: 260}


def test_q1_element_matrix(oracle):
    fe = oracle.FE1D(1)
    K = np.kron(np.kron(fe.M, fe.M), fe.K) + np.kron(np.kron(fe.M, fe.K), fe.M) + np.kron(np.kron(fe.K, fe.M), fe.M)
    # cube of side h=1: diag 1/3, edge neighbour 0, face diagonal -1/12, body diagonal -1/12
    assert K[0, 0] == pytest.approx(1 / 3, abs=1e-15)
    assert K[0, 1] == pytest.approx(0.0, abs=1e-15)
    assert K[0, 3] == pytest.approx(-1 / 12, abs=1e-15)
    assert K[0, 7] == pytest.approx(-1 / 12, abs=1e-15)


def test_q1_27_point_stencil(oracle):
    lv = oracle.Level(oracle.create_mesh("hypercube", 2), 1)
    h = 0.5
    centre = lv.key_to_dof[(2 << oracle.LMAX >> 2, 2 << oracle.LMAX >> 2, 2 << oracle.LMAX >> 2, 0, 0)]
    row = lv.Kraw[centre].toarray().ravel()
    row[np.abs(row) < 1e-13] = 0.0
    vals = sorted(np.round(row[row != 0] / h, 12))
    assert row[centre] == pytest.approx(8 * h / 3)
    assert vals.count(round(-1 / 6, 12)) == 12  # edge neighbours
    assert vals.count(round(-1 / 12, 12)) == 8  # corner neighbours
    assert np.count_nonzero(row) == 21  # face neighbours vanish


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7])
def test_fe_tables(oracle, p):
    fe = oracle.FE1D(p)
    assert fe.M.sum() == pytest.approx(1.0)  # partition of unity
    assert np.abs(fe.K.sum(axis=1)).max() < 1e-12  # constants in the kernel
    assert fe.m.sum() == pytest.approx(1.0)
    # GLL nodes are symmetric, Gauss rule integrates x^(2p+1) exactly
    assert np.allclose(fe.nodes + fe.nodes[::-1], 1.0)
    assert (fe.wq * fe.xq ** (2 * p + 1)).sum() == pytest.approx(1 / (2 * p + 2))


def test_mesh_counts(oracle):
    for L, n in QUADRANT_CELLS.items():
        m = oracle.create_mesh("quadrant", L)
        assert len(m) == n
        if L in QUADRANT_HN:
            assert sum(oracle.is_cell_constrained(m, c) for c in m) == QUADRANT_HN[L]
    seq = oracle.coarsening_sequence(oracle.create_mesh("quadrant", 4))
    assert [len(s) for s in seq] == [1, 8, 15, 120, 701]
    ann = oracle.create_mesh("annulus", 5)
    assert len(ann) == 1184 and sum(oracle.is_cell_constrained(ann, c) for c in ann) == 816
    assert len(oracle.create_mesh("hypercube", 3)) == 512


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7])
def test_dof_counts(oracle, p):
    """the SURVEY's counts where it lists the degree; the uniform meshes at every degree (hypercube 1 from p = 5: 8 cells)"""
    for L, n in QUADRANT_DOFS.get(p, {}).items():
        if n > 2000 and p == 4:
            continue
        assert oracle.Level(oracle.create_mesh("quadrant", L), p).n == n
    L = 2 if p <= 4 else 1
    assert oracle.Level(oracle.create_mesh("hypercube", L), p).n == ((1 << L) * p + 1) ** 3


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7])
def test_operator_properties(oracle, p):
    lv = oracle.Level(oracle.create_mesh("quadrant", 3 if p < 4 else 2), p)
    A = lv.A
    assert abs(A - A.T).max() < 1e-13
    free = ~lv.constrained
    Af = A.toarray()[np.ix_(free, free)]
    if p <= 4:
        assert np.linalg.eigvalsh(Af).min() > 0  # SPD on free DoFs
    else:
        np.linalg.cholesky(Af)  # the same statement at the cost of one factorisation: it raises unless Af is positive definite
    assert np.abs(lv.Kraw @ np.ones(lv.n)).max() < 1e-12  # constants in the null space of unconstrained K
    # polynomial exactness: for u = x (degree 1 <= p), C^T K u_h vanishes at free DoFs away from constraints?  use
    # energy instead: u^T K u = int |grad u|^2 = volume = 8 for u = x
    top = p << oracle.LMAX
    x = np.array([-1.0 + 2.0 * k[0] / top for k in lv.keys])
    # node coordinates are GLL, not equispaced: interpolate x through the element basis instead
    fe = lv.fe
    xs = np.zeros(lv.n)
    for ci, cell in enumerate(lv.cells):
        l, i, j, k = cell
        h = 2.0 / (1 << l)
        for t, d in enumerate(lv.cell_dofs[ci]):
            a = t % (p + 1)
            xs[d] = -1.0 + (i + fe.nodes[a]) * h
    assert xs @ (lv.Kraw @ xs) == pytest.approx(8.0, rel=1e-12)


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6])  # p = 7 costs a dense 4913^2 product; its transfers are held to polynomials instead
def test_galerkin_identity(oracle, p):
    """A_c = P^T A_f P on free DoFs: ties operator, transfer and hanging-node constraints together."""
    levels, P = oracle.build_hierarchy("quadrant", 3 if p < 4 else 2, p)
    for l in range(1, len(levels)):
        f, c = levels[l], levels[l - 1]
        G = (P[l].T @ f.A @ P[l]).toarray()
        fr = ~c.constrained
        if fr.any():
            assert np.abs(G[np.ix_(fr, fr)] - c.A.toarray()[np.ix_(fr, fr)]).max() < 1e-12


def test_transfer_reproduces_polynomials(oracle):
    levels, P = oracle.build_hierarchy("quadrant", 3, 2)
    f, c = levels[-1], levels[-2]

    def interp(lv, fn):
        v = np.zeros(lv.n)
        for ci, cell in enumerate(lv.cells):
            l, i, j, k = cell
            h = 2.0 / (1 << l)
            n1 = lv.p + 1
            for t, d in enumerate(lv.cell_dofs[ci]):
                a, b, cc = t % n1, (t // n1) % n1, t // (n1 * n1)
                v[d] = fn(-1 + (i + lv.fe.nodes[a]) * h, -1 + (j + lv.fe.nodes[b]) * h, -1 + (k + lv.fe.nodes[cc]) * h)
        return v

    fn = lambda x, y, z: (1 - x * x) * (1 - y * y) * (1 - z * z)  # in Q2, zero on the boundary
    uf, uc = interp(f, fn), interp(c, fn)
    free = ~f.constrained
    assert np.abs((P[-1] @ uc) - uf)[free].max() < 1e-12


def test_chebyshev_eigenvalue_estimate(oracle):
    lv = oracle.Level(oracle.create_mesh("hypercube", 2), 2)
    ch = oracle.Chebyshev(lv.A, lv.inv_diag, 3)
    ev = np.linalg.eigvalsh((np.diag(lv.inv_diag) @ lv.A.toarray() + (np.diag(lv.inv_diag) @ lv.A.toarray()).T) / 2)
    lam = np.linalg.eigvals(np.diag(lv.inv_diag) @ lv.A.toarray()).real.max()
    assert 0.8 * lam <= ch.max_ev_raw <= lam * (1 + 1e-10)  # Lanczos approaches from below


def test_cg_iteration_counts(oracle):
    # the only correctness evidence the reference prints is n_iterations (ref:multigrid_throughput.cc:1279)
    for geo, L, p, expect in (("quadrant", 3, 1, 4), ("hypercube", 3, 1, 4), ("quadrant", 4, 1, 4)):
        r = oracle.solve(geo, L, p)
        assert r["n_iterations"] == expect
        assert r["history"][-1] < 1e-4 * r["history"][0]
