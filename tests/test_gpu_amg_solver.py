"""Type "AMG": CG on the assembled system matrix with the AMG preconditioner built on it (solve_with_amg,
ref:multigrid_throughput.cc:1877-1966; runtime.hip AssembledMatrix, kernels_amg.hpp K8 and SPMV_DOT) on the GPU:
  * the wavefront-per-row kernel K8 (lanes = 64) in all five modes and SPMV_DOT at every lane count, through the production
    launcher (mgamd_debug_csr_spmv_ex), against float64 numpy on synthetic CSR matrices; a row's result at two grid sizes;
  * SparseMatrix.vmult against the matrix-free Operator.vmult and against scipy on DoFs.matrix();
  * PreconditionAMG.vmult against oracle/amg_oracle.py's SmoothedAggregation.apply on the product's matrix;
  * Hierarchy(..., "AMG") + solve_cg against the oracle's pcg with the restated AMG, with and without the fused p . A p, and
    without a preconditioner;
  * the refusals.
Every output vector is filled with NaN before the call that must overwrite it."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import amg_oracle as ao
from conftest import rel_err

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
TOL_VMULT = 1e-13  # assembled against matrix-free operator
TOL_CYCLE = 1e-11  # test_gpu_amg.py's: FP64 AMG application against the oracle
TOL_SOL = 1e-10
TOL_FUSED = 1e-12
K7_LANES = (4, 8, 16, 32)


# ------------------------------------------------------------------ K8 and SPMV_DOT against float64 numpy
def _csr_case(rng, row_lengths):
    """square CSR matrix with the given row lengths (random columns; a column may repeat within a row, which the kernels sum like
    any other entry)"""
    n = len(row_lengths)
    ptr = np.concatenate([[0], np.cumsum(row_lengths)]).astype(np.uint32)
    return ptr, rng.integers(0, n, int(ptr[-1])).astype(np.uint32), rng.standard_normal(int(ptr[-1]))


EDGE_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1561]  # around one pass of 64 lanes, one unrolled pass of 256, the longest p = 4 row


def _spmv_matrices():
    rng = np.random.default_rng(11)
    mats = [("rows1", _csr_case(rng, [1561])),
            ("rows3", _csr_case(rng, [65, 0, 256])),
            ("rows5", _csr_case(rng, [64, 255, 1, 257, 0])),  # not a multiple of the 4 rows per block
            ("rows9", _csr_case(rng, EDGE_LENGTHS))]
    L = rng.integers(2, 130, 257)
    L[rng.permutation(257)[:len(EDGE_LENGTHS)]] = EDGE_LENGTHS
    mats.append(("rows257", _csr_case(rng, L)))
    # 5000 rows: 1250 blocks of 4 rows, more than the 1024 partials of SPMV_DOT, so its grid is capped and strides
    L = rng.integers(55, 85, 5000)
    L[::97] = 0
    L[7::211] = 300
    mats.append(("rows5000", _csr_case(rng, L)))
    return mats


SPMV_MATRICES = _spmv_matrices()


def _reference(mat, seed):
    ptr, col, val = mat
    n = len(ptr) - 1
    rng = np.random.default_rng(seed)
    x, b, xold, dinv, y0 = (rng.standard_normal(n) for _ in range(5))
    dinv = 1.0 + np.abs(dinv)
    A = sp.csr_matrix((val, col.astype(np.int64), ptr.astype(np.int64)), shape=(n, n))
    Aabs = sp.csr_matrix((np.abs(val), col.astype(np.int64), ptr.astype(np.int64)), shape=(n, n))
    return n, x, b, xold, dinv, y0, A @ x, Aabs @ np.abs(x)


@pytest.mark.parametrize("name,mat", SPMV_MATRICES, ids=[m[0] for m in SPMV_MATRICES])
def test_wave_per_row_kernel(mgamd, ctx, name, mat):
    """lanes = 64 in the four modes of K7 (Chebyshev with xold null, given, and aliased to the output): per row within
    4 eps sum |a||x| (test_gpu_amg.py's bound)"""
    ptr, col, val = mat
    n, x, b, xold, dinv, y0, s, sabs = _reference(mat, 100 + len(ptr))
    f1, f2 = 0.37, 1.3
    nan = np.full(n, np.nan)
    cheb = lambda xo: x + f1 * (x - xo) + f2 * dinv * (b - s)  # noqa: E731
    bound = lambda xo: np.abs(x) + abs(f1) * (np.abs(x) + np.abs(xo)) + abs(f2) * dinv * (np.abs(b) + sabs)  # noqa: E731
    z = np.zeros(n)
    cases = [(mgamd.SPMV_PLAIN, nan, {}, s, sabs),
             (mgamd.SPMV_ADD, y0, {}, y0 + s, np.abs(y0) + sabs),
             (mgamd.SPMV_RESID, nan, dict(b=b), b - s, np.abs(b) + sabs),
             (mgamd.SPMV_CHEB, nan, dict(b=b, dinv=dinv, f1=f1, f2=f2), cheb(z), bound(z)),
             (mgamd.SPMV_CHEB, nan, dict(b=b, dinv=dinv, f1=f1, f2=f2, xold=xold), cheb(xold), bound(xold)),
             (mgamd.SPMV_CHEB, xold, dict(b=b, dinv=dinv, f1=f1, f2=f2, xold_is_y=True), cheb(xold), bound(xold))]
    for mode, yin, kw, ref, mag in cases:
        y, used, blocks, _ = mgamd.debug_csr_spmv_ex(ctx, mode, 64, ptr, col, val, x, yin, **kw)
        assert used == 64 and blocks == min((n + 3) // 4, 4096)
        err = np.abs(y - ref)
        print(f"{name} mode {mode}: max err / bound {float(np.max(err / np.maximum(4 * EPS * mag, 1e-300))):.3f}")
        assert np.isfinite(y).all() and (err <= 4 * EPS * mag).all(), (mode, float(np.max(err / np.maximum(mag, 1e-300))))


@pytest.mark.parametrize("lanes", [4, 8, 16, 32, 64, 0])
@pytest.mark.parametrize("name,mat", SPMV_MATRICES, ids=[m[0] for m in SPMV_MATRICES])
def test_spmv_dot(mgamd, ctx, name, mat, lanes):
    """SPMV_DOT at K7's lane counts, at 64 and at the automatic choice: y = A x per row as above; x . y within
    (4 + n) eps sum_i |x_i| sum_j |a_ij||x_j|: every term x_i y_i carries y_i's 4 eps sum_j |a_ij||x_j| (and its own rounding), and
    summing the n terms in any order adds at most (n - 1) eps sum_i |x_i y_i|"""
    ptr, col, val = mat
    n, x, _, _, _, _, s, sabs = _reference(mat, 200 + len(ptr))
    y, used, blocks, dot = mgamd.debug_csr_spmv_ex(ctx, mgamd.SPMV_DOT, lanes, ptr, col, val, x, np.full(n, np.nan))
    avg = len(col) / n
    assert used == (lanes or (4 if avg <= 6 else (8 if avg <= 24 else (16 if avg <= 64 else 32))))
    assert blocks == min((n * used + 255) // 256, 1024)  # one partial per block: never more than the 1024 the context holds
    assert np.isfinite(y).all() and (np.abs(y - s) <= 4 * EPS * sabs).all()
    bound = (4 + n) * EPS * float(np.abs(x) @ sabs)
    print(f"{name} lanes {used}: dot error {abs(dot - float(x @ s)):.3e}, bound {bound:.3e}")
    assert np.isfinite(dot) and abs(dot - float(x @ s)) <= bound


@pytest.mark.parametrize("lanes", [64, 32])
def test_row_results_do_not_depend_on_the_grid(mgamd, ctx, lanes):
    """the 5000-row matrix at the launcher's grid, at 7 blocks and at 1 block (every row through the grid-stride loop): bitwise the
    same y in every mode; the dot product, whose partials are cut by the grid, within its bound"""
    name, mat = SPMV_MATRICES[-1]
    ptr, col, val = mat
    n, x, b, xold, dinv, y0, s, sabs = _reference(mat, 300)
    for mode, yin, kw in [(mgamd.SPMV_PLAIN, np.full(n, np.nan), {}), (mgamd.SPMV_ADD, y0, {}), (mgamd.SPMV_RESID, np.full(n, np.nan), dict(b=b)),
                          (mgamd.SPMV_CHEB, xold, dict(b=b, dinv=dinv, f1=0.37, f2=1.3, xold_is_y=True)),
                          (mgamd.SPMV_DOT, np.full(n, np.nan), {})]:
        full = mgamd.debug_csr_spmv_ex(ctx, mode, lanes, ptr, col, val, x, yin, **kw)
        assert full[2] > 7
        for max_blocks in (7, 1):
            part = mgamd.debug_csr_spmv_ex(ctx, mode, lanes, ptr, col, val, x, yin, max_blocks=max_blocks, **kw)
            assert part[2] == max_blocks and np.array_equal(full[0], part[0]), (mode, max_blocks)
            if mode == mgamd.SPMV_DOT:
                assert abs(part[3] - float(x @ s)) <= (4 + n) * EPS * float(np.abs(x) @ sabs)


def test_debug_entry_refuses_what_the_kernels_lack(mgamd, ctx):
    ptr, col, val = SPMV_MATRICES[1][1]
    x = np.ones(3)
    for kw in (dict(lanes=64, mode=mgamd.SPMV_PLAIN, number_type=mgamd.F32), dict(lanes=16, mode=mgamd.SPMV_DOT, number_type=mgamd.F32),
               dict(lanes=48, mode=mgamd.SPMV_PLAIN), dict(lanes=64, mode=5)):
        with pytest.raises(mgamd.MgamdError):
            mgamd.debug_csr_spmv_ex(ctx, kw.pop("mode"), kw.pop("lanes"), ptr, col, val, x, np.zeros(3), **kw)
    # lanes = 0 keeps meaning the coarse solver's choice, through the old entry and the new
    assert mgamd.debug_csr_spmv(ctx, mgamd.F64, mgamd.SPMV_PLAIN, 0, ptr, col, val, x, np.zeros(3))[1] == 32
    assert mgamd.debug_csr_spmv_ex(ctx, mgamd.SPMV_PLAIN, 0, ptr, col, val, x, np.zeros(3))[1] == 32


# ------------------------------------------------------------------ the assembled operator
@pytest.fixture(scope="module")
def levels(mgamd, ctx):
    """per (geometry, NRefGlobal, degree): the Hierarchy of Type "AMG" and its host matrix, built once.  p < 0: degree -p with
    MGAMD_SPMV_WAVE_MIN_MEAN_ROW=40 while it is built: the operator and every AMG matrix with a mean row above 40 take K8, the
    wavefront-per-row kernel, which the default threshold (144) gives to larger meshes only (quadrant L=4 p=4: mean row 157)"""
    cache = {}

    def get(geo, L, p):
        if (geo, L, p) not in cache:
            if p < 0:
                os.environ["MGAMD_SPMV_WAVE_MIN_MEAN_ROW"] = "40"
            try:
                h = mgamd.Hierarchy(ctx, geo, L, abs(p), "AMG")
            finally:
                os.environ.pop("MGAMD_SPMV_WAVE_MIN_MEAN_ROW", None)
            assert h.system_matrix.lanes == 64 or p > 0
            assert h.mg is None and len(h.dofs) == 1 and h.n_dofs == h.dofs[0].n_dofs == h.system_matrix.n_rows
            cache[(geo, L, p)] = (h, ao.csr(*h.dofs[0].matrix()))
        return cache[(geo, L, p)]

    return get


@pytest.fixture(scope="module")
def oracles(levels):
    """the oracle's hierarchy on the product's matrix (the product's numbering), built once per case and left unchanged"""
    cache = {}

    def get(geo, L, p):
        if (geo, L, p) not in cache:
            cache[(geo, L, p)] = cache.get((geo, L, -p)) or ao.SmoothedAggregation(levels(geo, L, p)[1])
        return cache[(geo, L, p)]

    return get


def _nan_vector(mgamd, ctx, n):
    v = mgamd.Vector(ctx, n)
    v.set(np.nan)
    return v


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 4), ("quadrant", 3, -4), ("hypercube", 2, 4), ("hypercube", 2, -4), ("quadrant", 6, 1), ("quadrant", 4, 4)],
                         ids=["quadrant-3-p4", "quadrant-3-p4-K8", "hypercube-2-p4", "hypercube-2-p4-K8", "quadrant-6-p1", "quadrant-4-p4"])
def test_matrix_vmult(mgamd, ctx, levels, geo, L, p):
    """SparseMatrix.vmult against the matrix-free operator on the same DoFs and against scipy on DoFs.matrix(): rows to about 1280
    entries with hanging nodes at p = 4, through K7 (the lane choice's pick below a mean row of 144) and through K8; quadrant L=4
    p=4 (mean row 157) takes K8 by that choice; p = 1: short rows, K7"""
    h, A = levels(geo, L, p)
    M = h.system_matrix
    assert (M.n_rows, M.nnz) == (A.shape[0], A.nnz) and M.m() == h.n_dofs
    mean = M.nnz / M.n_rows
    if p > 0:
        assert M.lanes == mgamd.csr_spmv_lanes_long(M.n_rows, M.nnz) == (64 if mean > 144 else (32 if mean > 64 else (16 if mean > 24 else 8)))
        assert (M.lanes == 64) == ((geo, L, p) == ("quadrant", 4, 4))
    p = abs(p)
    x = np.random.default_rng(L * 10 + p).standard_normal(h.n_dofs)
    vx, vy, vf = mgamd.Vector(ctx, h.n_dofs).from_host(x), _nan_vector(mgamd, ctx, h.n_dofs), _nan_vector(mgamd, ctx, h.n_dofs)
    M.vmult(vy, vx)
    h.fine_operator.vmult(vf, vx)
    y = vy.to_host()
    err = rel_err(y, vf.to_host())
    print(f"{geo} L={L} p={p}: {M.n_rows} rows, mean row {M.nnz / M.n_rows:.0f}, max row {int(np.diff(A.indptr).max())}, lanes {M.lanes}; "
          f"assembled vs matrix-free {err:.2e}")
    assert np.isfinite(y).all() and err <= TOL_VMULT
    # scipy sums a row of n products one after the other: its own result carries up to (n - 1) eps sum |a||x| (the a-priori bound
    # of recursive summation), on top of the kernel's 4 eps
    bound = (4 + np.diff(A.indptr)) * EPS * (abs(A) @ np.abs(x))
    err = np.abs(y - A @ x)
    print(f"against scipy: max error / (eps sum |a||x|) {float(np.max(err / np.maximum(EPS * (abs(A) @ np.abs(x)), 1e-300))):.2f}")
    assert (err <= bound).all()


AMG_CASES = [("quadrant", 3, 4), ("quadrant", 3, -4), ("annulus", 5, 3), ("annulus", 5, -3), ("quadrant", 6, 1)]
AMG_IDS = ["quadrant-3-p4", "quadrant-3-p4-K8", "annulus-5-p3", "annulus-5-p3-K8", "quadrant-6-p1"]


def _rhs(d, rng, constrained):
    """random right-hand side; constrained=False: zero on the constrained DoFs (the last rows)"""
    r = rng.standard_normal(d.n_dofs)
    if not constrained:
        r[d.info.n_interior + d.info.n_tail:] = 0.0
    return r


@pytest.mark.parametrize("geo,L,p", AMG_CASES, ids=AMG_IDS)
def test_amg_vmult_equals_oracle(mgamd, ctx, levels, oracles, geo, L, p):
    """PreconditionAMG.vmult with 1 and 2 cycles against the oracle's apply, right-hand sides with and without non-zero
    constrained entries; quadrant L=6 p=1 has three AMG levels"""
    h, A = levels(geo, L, p)
    o = oracles(geo, L, p)
    assert h.amg.layout() == [lv.n for lv in o.levels] and h.amg.layout()[0] == h.n_dofs
    if (geo, L, p) == ("quadrant", 6, 1):
        assert len(o.levels) == 3
    rng = np.random.default_rng(12)
    for n_cycles in (1, 2):
        amg = h.amg if n_cycles == 1 else mgamd.PreconditionAMG(h.system_matrix, n_cycles)
        for constrained in (False, True):
            r = _rhs(h.dofs[0], rng, constrained)
            vz = _nan_vector(mgamd, ctx, h.n_dofs)
            amg.vmult(vz, mgamd.Vector(ctx, h.n_dofs).from_host(r))
            err = rel_err(vz.to_host(), o.apply(r, n_cycles))
            print(f"{geo} L={L} p={p} cycles={n_cycles} constrained rhs={constrained}: rel. error {err:.2e}")
            assert err <= TOL_CYCLE, (n_cycles, constrained, err)


def _solve(mgamd, ctx, h, precond, reltol):
    b = h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    x = _nan_vector(mgamd, ctx, h.n_dofs)
    it, res = mgamd.solve_cg(h.system_matrix, precond, x, b, reltol)
    return b.to_host(), x.to_host(), it, res


@pytest.mark.parametrize("geo,L,p", AMG_CASES, ids=AMG_IDS)
def test_solve_equals_oracle(mgamd, oracle, ctx, levels, oracles, monkeypatch, geo, L, p):
    """CG to reltol 1e-4 and 1e-6 with one AMG cycle: the oracle's pcg with the restated AMG takes the same iterations and reaches
    the same solution; with the fused p . A p switched off (product, then inner product) the same again"""
    h, A = levels(geo, L, p)
    o = oracles(geo, L, p)
    for reltol in (1e-4, 1e-6):
        bh, x, it, _ = _solve(mgamd, ctx, h, h.amg, reltol)
        xref, itref, _ = oracle.pcg(A, bh, o.precondition(1), reltol)
        monkeypatch.setenv("MGAMD_NO_FUSED_DOT", "1")
        _, x2, it2, _ = _solve(mgamd, ctx, h, h.amg, reltol)
        monkeypatch.delenv("MGAMD_NO_FUSED_DOT")
        print(f"{geo} L={L} p={p} reltol {reltol:g}: {it} iterations (oracle {itref}, separate dot {it2}), solution rel. error "
              f"{rel_err(x, xref):.2e}, fused vs separate {rel_err(x, x2):.2e}")
        assert it == itref and rel_err(x, xref) <= TOL_SOL, (it, itref)
        assert it2 == it and rel_err(x2, x) <= TOL_FUSED


def test_solve_without_preconditioner(mgamd, oracle, ctx, levels):
    """solve_cg(matrix, None): the oracle's pcg with the identity.  Rounding differences of relative size eps per step grow by at
    most the condition number over the run; on hypercube L=2 p=4 (4913 DoFs, a few dozen iterations, condition number of order 10^3)
    that stays below TOL_SOL"""
    h, A = levels("hypercube", 2, 4)
    bh, x, it, _ = _solve(mgamd, ctx, h, None, 1e-4)
    xref, itref, _ = oracle.pcg(A, bh, lambda r: r.copy(), 1e-4)
    print(f"no preconditioner: {it} iterations (oracle {itref}), solution rel. error {rel_err(x, xref):.2e}")
    assert it == itref and rel_err(x, xref) <= TOL_SOL


# ------------------------------------------------------------------ refusals
def test_refusals(mgamd, ctx, levels):
    h, _ = levels("hypercube", 2, 4)
    n = h.n_dofs
    f32, f64 = mgamd.Vector(ctx, n, mgamd.F32), mgamd.Vector(ctx, n)
    for call in (lambda: h.system_matrix.vmult(f32, f64), lambda: h.system_matrix.vmult(f64, f32), lambda: h.amg.vmult(f32, f64),
                 lambda: mgamd.solve_cg(h.system_matrix, h.amg, f32, f64), lambda: mgamd.solve_cg(h.system_matrix, None, f64, f32),
                 lambda: h.system_matrix.vmult(mgamd.Vector(ctx, n + 1), f64), lambda: mgamd.PreconditionAMG(h.system_matrix, 0)):
        with pytest.raises(mgamd.MgamdError):
            call()
    # an AMG goes with the matrix it was built on
    other = mgamd.SparseMatrix(ctx, h.dofs[0])
    with pytest.raises(mgamd.MgamdError):
        mgamd.solve_cg(other, h.amg, f64, f64)
    # a local-smoothing level
    fine = mgamd.Triangulation("quadrant", 3)
    with pytest.raises(mgamd.MgamdError):
        mgamd.SparseMatrix(ctx, mgamd.DoFs(fine.level_mesh(fine.n_levels - 1), 2, 0, local_smoothing_level=True))
    # the DoFs of a Partition
    seq = mgamd.create_geometric_coarsening_sequence(mgamd.Triangulation("hypercube", 3))
    part = mgamd.Partition(seq, 2)
    local = mgamd.DoFs(seq[-1], 2, 0, part, len(seq) - 1, 0)
    assert local.info.n_peers > 0
    with pytest.raises(mgamd.MgamdError):
        mgamd.SparseMatrix(ctx, local)
    # still in working order after the refusals
    x = np.random.default_rng(1).standard_normal(n)
    h.system_matrix.vmult(f64, mgamd.Vector(ctx, n).from_host(x))
    assert np.isfinite(f64.to_host()).all()
