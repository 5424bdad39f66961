"""Host side of Type "AMG" (CG on the assembled matrix with the AMG preconditioner), CPU only:
  * assemble_level_matrix (csrc/amg.hpp) now counts the entries of a row in 64 bits; its output on a valid input is unchanged:
    DoFs.matrix() is still the numpy multigrid oracle's Level.A, at degree 3 on a mesh with hanging nodes, matched through the
    geometric DoF keys as test_amg_host.py does;
  * the counting function it builds its 32-bit row pointers with (csr_row_pointers, through mgamd_debug_csr_row_pointers) refuses a
    matrix of more than 2^32 - 1 entries instead of wrapping, on fabricated row counts: no large mesh is built."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_oracle as ao

TOL_MAT = 1e-13  # test_amg_host.py's: every entry within this of its row's largest entry


def test_assembled_matrix_unchanged(mgamd, oracle):
    d = mgamd.DoFs(mgamd.Triangulation("quadrant", 2), 3, 0)
    assert d.info.n_hanging > 0
    lv = oracle.Level(oracle.create_mesh("quadrant", 2), 3, numbering_keys=d.keys())
    ptr, col, val = d.matrix()
    # the row pointers are the running sum of the row lengths, the columns of a row sorted and distinct
    assert ptr[0] == 0 and ptr[-1] == len(col) == len(val) and (np.diff(ptr.astype(np.int64)) > 0).all()
    for i in (0, d.n_dofs // 2, d.n_dofs - 1):
        assert (np.diff(col[ptr[i]:ptr[i + 1]].astype(np.int64)) > 0).all()
    A = ao.csr(ptr, col, val)
    ones = lambda M: sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)  # noqa: E731
    C = lv.C.tocsr()
    pattern = (ones(C.T.tocsr()) @ ones(lv.Kraw.tocsr()) @ ones(C) + sp.diags(lv.constrained.astype(float))).tocsr()
    pattern.sort_indices()
    assert np.array_equal(A.indptr, pattern.indptr) and np.array_equal(A.indices, pattern.indices)
    D = (A - lv.A).tocsr()
    rowmax = np.asarray(abs(lv.A).max(axis=1).todense()).ravel()
    assert (np.asarray(abs(D).max(axis=1).todense()).ravel() <= TOL_MAT * rowmax).all()


def test_row_pointers_of_valid_counts(mgamd):
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 2000, 1000).astype(np.uint64)
    ptr = mgamd.csr_row_pointers(counts)
    assert ptr.dtype == np.uint32 and np.array_equal(ptr.astype(np.uint64), np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64))
    assert np.array_equal(mgamd.csr_row_pointers([]), np.zeros(1, np.uint32))
    # exactly 2^32 - 1 entries still fit
    ptr = mgamd.csr_row_pointers(np.array([2 ** 31, 0, 2 ** 31 - 1], np.uint64))
    assert [int(v) for v in ptr] == [0, 2 ** 31, 2 ** 31, 2 ** 32 - 1]


@pytest.mark.parametrize("counts", [[2 ** 31, 2 ** 31], [2 ** 32 - 1, 0, 1], [1561] * 2_800_000, [2 ** 32, 5]],
                         ids=["two-halves", "one-past", "many-long-rows", "one-row-too-long"])
def test_row_pointers_refuse_overflow(mgamd, counts):
    """sums that wrap 32 bits (to 0, to 0, to a small number, to 5): an error that names the count, never wrapped pointers"""
    total = sum(counts)
    assert total > 2 ** 32 - 1
    with pytest.raises(mgamd.MgamdError, match=str(total)):
        mgamd.csr_row_pointers(np.array(counts, np.uint64))
