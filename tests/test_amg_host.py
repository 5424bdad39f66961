"""Host setup of the algebraic multigrid behind the coarse solvers "amg", "cg_with_amg", "amg_petsc" (csrc/amg.hpp) against the
independent numpy/scipy restatement oracle/amg_oracle.py, level by level, plus the assembled level matrix it starts from
(mgamd_dofs_matrix) against the numpy multigrid oracle's Level.A.  CPU only: the hierarchy is host code (mgamd_dev.h).

Both sides start from the product's own assembled matrix, so strength, aggregates and the power iteration see identical numbers;
the oracle sums its power-iteration norms in index order, and its prolongator and Galerkin products then agree with the product's
to the last bit on every tested mesh (the tolerances below leave room for a different but equally valid summation order)."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import amg_oracle as ao
from support import random_mesh

TOL_MAT = 1e-13

# (geometry, NRefGlobal) or ("random", random_mesh's (seed, global refinements, rounds, fraction)): p = 1, > 1000 DoFs
HIERARCHY_CASES = [("annulus", 6), ("annulus", 7), ("quadrant", 6), ("hypercube", 5), ("random", (4, 4, 1, 0.004)),
                   ("random", (8, 4, 2, 0.002))]


def _tria(mgamd, oracle, geo, L):
    if geo == "random":
        arr = np.array(sorted(random_mesh(oracle, *L)), dtype=np.int64)
        return mgamd.Triangulation.from_leaves(arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3]), {tuple(int(v) for v in c) for c in arr}
    return mgamd.Triangulation(geo, L), None


@pytest.fixture(scope="module")
def setups(mgamd, oracle):
    cache = {}

    def get(geo, L):
        key = (geo, str(L))
        if key not in cache:
            t, _ = _tria(mgamd, oracle, geo, L)
            d = mgamd.DoFs(t, 1, 0)
            H = d.amg_hierarchy()
            cache[key] = (d, [H.level(l) for l in range(H.n_levels)], ao.SmoothedAggregation(d.matrix()))
        return cache[key]

    return get


CASE_IDS = [f"{g}-{L}" if g != "random" else f"random-seed{L[0]}" for g, L in HIERARCHY_CASES]


def _strength_graph(A, theta=ao.THETA):
    """strong couplings, stated here once more so that the aggregate properties do not rest on the oracle's code"""
    d = np.abs(A.diagonal())
    C = A.tocoo()
    keep = (C.row != C.col) & (C.data != 0) & (np.abs(C.data) >= theta * np.sqrt(d[C.row] * d[C.col]))
    return sp.csr_matrix((np.ones(keep.sum()), (C.row[keep], C.col[keep])), shape=A.shape)


def _same_pattern(X, Y):
    X, Y = X.tocsr(), Y.tocsr()
    X.sort_indices()
    Y.sort_indices()
    return X.shape == Y.shape and np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)


def _rel_errors(X, Y):
    """(Frobenius, max-entry) relative difference"""
    D = (X - Y).tocsr()
    return sp.linalg.norm(D) / sp.linalg.norm(Y), abs(D).max() / abs(Y).max()


# ------------------------------------------------------------------ the assembled matrix
@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("geo,L", [("quadrant", 3), ("random", (5, 2, 2, 0.05))], ids=["quadrant-3", "random-seed5"])
def test_assembled_matrix_equals_oracle(mgamd, oracle, geo, L, p):
    """d.matrix() (Operator::get_trilinos_system_matrix) IS the oracle's C^T K C + I on the constrained rows, on meshes with
    hanging nodes: the symbolic pattern of the cell couplings, and every entry within TOL_MAT of its row's largest entry"""
    t, leaves = _tria(mgamd, oracle, geo, L)
    d = mgamd.DoFs(t, p, 0)
    assert d.info.n_hanging > 0
    lv = oracle.Level(leaves if leaves is not None else oracle.create_mesh(geo, L), p, numbering_keys=d.keys())
    A = ao.csr(*d.matrix())
    ones = lambda M: sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
    C = lv.C.tocsr()
    pattern = ones(C.T.tocsr()) @ ones(lv.Kraw.tocsr()) @ ones(C) + sp.diags(lv.constrained.astype(float))
    assert _same_pattern(A, pattern)
    D = (A - lv.A).tocsr()
    rowmax = np.asarray(abs(lv.A).max(axis=1).todense()).ravel()
    assert (np.asarray(abs(D).max(axis=1).todense()).ravel() <= TOL_MAT * rowmax).all()


# ------------------------------------------------------------------ the smoothed-aggregation hierarchy
@pytest.mark.parametrize("geo,L", HIERARCHY_CASES, ids=CASE_IDS)
def test_hierarchy_sizes(setups, geo, L):
    d, H, o = setups(geo, L)
    assert d.n_dofs > 1000 and len(H) >= 2
    assert [(len(h["A"][0]) - 1, len(h["A"][1])) for h in H] == [(lv.n, lv.A.nnz) for lv in o.levels]
    assert [(len(h["A"][0]) - 1, len(h["A"][1])) for h in H] == [tuple(s) for s in d.amg_setup_info()]


@pytest.mark.parametrize("geo,L", HIERARCHY_CASES, ids=CASE_IDS)
def test_aggregates_equal_oracle(setups, geo, L):
    """aggregates and their count on every level: from the product's own level matrix, and as the oracle's own hierarchy has them"""
    d, H, o = setups(geo, L)
    for h, lv in zip(H[:-1], o.levels):
        agg, na = ao.aggregate(ao.csr(*h["A"]))
        assert h["n_aggregates"] == na == lv.n_aggregates
        assert np.array_equal(h["agg"], agg) and np.array_equal(h["agg"], lv.agg)


@pytest.mark.parametrize("geo,L", HIERARCHY_CASES, ids=CASE_IDS)
def test_aggregate_properties(setups, geo, L):
    """independent of any restatement: each row with a strong coupling lies in exactly one aggregate, each row without one (the
    identity rows of constrained DoFs) in none, every aggregate is non-empty and connected in the strength graph"""
    d, H, o = setups(geo, L)
    for h in H[:-1]:
        A, agg, na = ao.csr(*h["A"]), h["agg"].astype(np.int64), h["n_aggregates"]
        S = _strength_graph(A)
        coupled = np.diff(S.indptr) > 0
        assert (agg[coupled] >= 0).all() and (agg[coupled] < na).all() and (agg[~coupled] == -1).all()
        assert (np.bincount(agg[coupled], minlength=na) > 0).all()
        # keep only the strong couplings inside one aggregate: exactly na components on the coupled rows
        Sc = S.tocoo()
        inside = (agg[Sc.row] == agg[Sc.col]) & coupled[Sc.row]
        G = sp.csr_matrix((np.ones(inside.sum()), (Sc.row[inside], Sc.col[inside])), shape=A.shape)
        idx = np.flatnonzero(coupled)
        n_comp, labels = connected_components(G[idx][:, idx], directed=False)
        assert n_comp == na
        assert len({(a, c) for a, c in zip(agg[idx].tolist(), labels.tolist())}) == na


@pytest.mark.parametrize("geo,L", HIERARCHY_CASES, ids=CASE_IDS)
def test_prolongator_and_coarse_matrix(setups, geo, L):
    """P = (I - omega D^-1 A) P_t and A_c = P^T A P: the same pattern as the oracle's, values within TOL_MAT relative (Frobenius
    and largest entry) on every level"""
    d, H, o = setups(geo, L)
    for l, (h, lv) in enumerate(zip(H, o.levels)):
        A = ao.csr(*h["A"])
        assert _same_pattern(A, lv.A), l
        fro, mx = _rel_errors(A, lv.A)
        assert fro <= TOL_MAT and mx <= TOL_MAT, (l, fro, mx)
        if h["P"] is not None:
            P = ao.csr(*h["P"], shape=(len(h["P"][0]) - 1, h["n_cols_P"]))
            assert _same_pattern(P, lv.P), l
            fro, mx = _rel_errors(P, lv.P)
            assert fro <= TOL_MAT and mx <= TOL_MAT, (l, fro, mx)


@pytest.mark.parametrize("geo,L", HIERARCHY_CASES, ids=CASE_IDS)
def test_lambda_max(setups, geo, L):
    """lambda_max of every level is the oracle's 1.1 x power iteration, and lies ABOVE the true lambda_max(D^-1 A) (scipy Lanczos):
    the Chebyshev smoother of the cycle works on [lambda_max / 20, lambda_max], which must cover the spectrum.  Measured ratios
    lambda_max / true per level (finest first): annulus-6 1.069 1.065, annulus-7 1.041 1.071, quadrant-6 1.065 1.076 1.094,
    hypercube-5 1.062 1.075, random-seed4 1.035 1.097, random-seed8 1.050 1.091."""
    d, H, o = setups(geo, L)
    for l, (h, lv) in enumerate(zip(H, o.levels)):
        assert abs(h["lambda_max"] - lv.lambda_max) <= 1e-12 * lv.lambda_max, l
        true = ao.true_lambda_max(ao.csr(*h["A"]))
        assert h["lambda_max"] >= true, (l, h["lambda_max"], true)
