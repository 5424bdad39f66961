"""Host side of FE degrees 5, 6 and 7 (no GPU): the assembled level matrix, the polynomial coarsening sequences and the
patch sizes of the transfer tables on the smallest mesh with hanging faces and edges (quadrant, NRefGlobal 2).  The device
tests of these degrees (test_gpu_high_degree.py) stand on these tables."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import oracle_level

DEGREES = [5, 6, 7]
N_DOFS = {5: 2530, 6: 4171, 7: 6400}


@pytest.fixture(scope="module")
def host_levels(mgamd, oracle):
    cache = {}

    def get(p):
        if p not in cache:
            t = mgamd.Triangulation("quadrant", 2)
            d = mgamd.DoFs(t, p)
            cache[p] = (t, d, oracle_level(oracle, d, "quadrant", 2, p))
        return cache[p]

    return get


@pytest.mark.parametrize("p", DEGREES)
def test_assembled_matrix_matches_oracle(mgamd, host_levels, p):
    t, d, lv = host_levels(p)
    assert d.n_dofs == lv.n == N_DOFS[p]
    ptr, col, val = d.matrix()
    A = sp.csr_matrix((val, col, ptr), shape=(d.n_dofs, d.n_dofs))
    diff = (A - sp.csr_matrix(lv.A)).tocoo()
    err = np.abs(diff.data).max() if diff.nnz else 0.0
    print(f"p={p}: n_dofs={d.n_dofs} nnz={A.nnz} max |A - A_oracle| / max |A_oracle| = {err / np.abs(lv.A).max():.2e}")
    assert err < 1e-13 * np.abs(lv.A).max()
    # the largest brick of these degrees is 2^3 cells: 11-, 13- and 15-point lattices, and single cells
    assert {B for B, n in d.groups() if n} <= {1, 2}


@pytest.mark.parametrize("p,seq", [(5, [1, 2, 5]), (6, [1, 3, 6]), (7, [1, 3, 7])])
def test_polynomial_coarsening_sequences(mgamd, p, seq):
    assert list(mgamd.create_polynomial_coarsening_sequence(p)) == seq


@pytest.mark.parametrize("p", DEGREES)
def test_transfer_patch_sizes(mgamd, p):
    """h-transfer: identity patches of p + 1 points and embedding patches of 2 p + 1 = 11 / 13 / 15 points; the first
    p-transfer of the bisection sequence (from p // 2): patches of p + 1 = 6 / 7 / 8 points"""
    t = mgamd.Triangulation("quadrant", 2)
    fine = mgamd.DoFs(t, p)

    def patch_sizes(coarse):
        return [(kind, nf) for kind, nf, ci, cm, fi in mgamd.transfer_tables(fine, coarse) if ci.shape[0]]

    h = patch_sizes(mgamd.DoFs(t.coarsen(), p))
    assert (1, 2 * p + 1) in h and all(nf == p + 1 for kind, nf in h if kind == 0) and all(kind in (0, 1) for kind, nf in h)
    pt = patch_sizes(mgamd.DoFs(t, p // 2))
    assert pt == [(2, p + 1)]


def test_degree_eight_is_refused(mgamd):
    t = mgamd.Triangulation("quadrant", 2)
    with pytest.raises(mgamd.MgamdError):
        mgamd.DoFs(t, 8)
