"""The algebraic multigrid of the coarse solvers "amg", "cg_with_amg" (csrc/amg.hpp, runtime.hip AmgCycle, kernel K7 of
kernels_amg.hpp) on the GPU against the independent numpy restatement oracle/amg_oracle.py:
  * K7 through its production launcher (mgamd_debug_csr_spmv) against float64 numpy: every mode, 4/8/16/32 lanes and the
    automatic choice, double and float, on CSR matrices with empty, 1-entry and long rows and on one large enough for the
    grid-stride loop;
  * the one-level AMG (a p = 1 PMG hierarchy: a pure application of the coarse solver), with 1 and 2 cycles and Chebyshev degrees
    1-4 (MGAMD_AMG_SMOOTHER_DEGREE: the odd degrees start in the other buffer);
  * cg_with_amg, whole PMG V-cycles and the outer CG with "amg" x 2 on the coarse level;
  * FP32 levels (AmgCycle<float>) against the FP64 oracle;
  * "gmg_vcycle" without a nested multigrid.
Every output vector is filled with NaN before the call that must overwrite it."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

import amg_oracle as ao
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_CYCLE = 1e-11  # FP64 AMG application against the oracle
TOL_SOL = 1e-10
# FP32 levels against the FP64 oracle: the bound test_float_levels_mixed_precision uses for the V-cycle (measured on MI355X:
# one-level AMG 0.9-1.8e-7, PMG V-cycle with amg x 2 4.7e-7 at p = 2, 6.9e-7 at p = 4)
TOL_F32 = 5e-5


# ------------------------------------------------------------------ K7 against float64 numpy
def _csr_case(rng, row_lengths):
    """square CSR matrix with the given row lengths (random columns; a column may repeat within a row, which K7 sums like any
    other entry)"""
    n = len(row_lengths)
    ptr = np.concatenate([[0], np.cumsum(row_lengths)]).astype(np.uint32)
    return ptr, rng.integers(0, n, int(ptr[-1])).astype(np.uint32), rng.standard_normal(int(ptr[-1]))


def _spmv_matrices():
    rng = np.random.default_rng(7)
    mats = [("rows1", _csr_case(rng, [150]))]
    for n in (31, 33, 257):
        L = rng.integers(2, 40, n)
        L[[0, 3, n - 1]] = 0  # empty rows
        L[[1, n // 2]] = 1  # 1-entry rows
        L[[2, n - 2]] = [150, 300]  # longer than 4 x 32 lanes
        mats.append((f"rows{n}", _csr_case(rng, L)))
    # > 4096 blocks at 32 lanes (8 rows per block): the grid-stride loop of the launcher's 4096-block cap
    L = rng.integers(20, 40, 40000)
    L[::997] = 0
    L[5::1013] = 200
    mats.append(("rows40000", _csr_case(rng, L)))
    return mats


SPMV_MATRICES = _spmv_matrices()


@pytest.mark.parametrize("number_type", ["F64", "F32"])
@pytest.mark.parametrize("name,mat", SPMV_MATRICES, ids=[m[0] for m in SPMV_MATRICES])
def test_csr_spmv_kernel(mgamd, ctx, number_type, name, mat):
    nt = getattr(mgamd, number_type)
    dt = np.float64 if number_type == "F64" else np.float32
    eps = float(np.finfo(dt).eps)
    ptr, col, val = mat
    n_rows = n_cols = len(ptr) - 1
    rng = np.random.default_rng(n_rows)
    r = lambda n: rng.standard_normal(n).astype(dt).astype(np.float64)  # inputs exactly representable in the kernel's type
    val = val.astype(dt).astype(np.float64)
    x, b, xold, dinv, y0 = r(n_cols), r(n_rows), r(n_rows), 1.0 + rng.random(n_rows), r(n_rows)
    dinv = dinv.astype(dt).astype(np.float64)
    f1, f2 = float(dt(0.37)), float(dt(1.3))
    A = sp.csr_matrix((val, col.astype(np.int64), ptr.astype(np.int64)), shape=(n_rows, n_cols))
    Aabs = sp.csr_matrix((np.abs(val), col.astype(np.int64), ptr.astype(np.int64)), shape=(n_rows, n_cols))
    s, sabs = A @ x, Aabs @ np.abs(x)
    nan = np.full(n_rows, np.nan)
    avg = len(col) / n_rows
    auto = 4 if avg <= 6 else (8 if avg <= 24 else (16 if avg <= 64 else 32))
    xs = x[:n_rows]
    for lanes in (4, 8, 16, 32, 0):
        cases = [(mgamd.SPMV_PLAIN, nan, {}, s, sabs),
                 (mgamd.SPMV_ADD, y0, {}, y0 + s, np.abs(y0) + sabs),
                 (mgamd.SPMV_RESID, nan, dict(b=b), b - s, np.abs(b) + sabs)]
        cheb = lambda xo: xs + f1 * (xs - xo) + f2 * dinv * (b - s)
        bound = lambda xo: np.abs(xs) + abs(f1) * (np.abs(xs) + np.abs(xo)) + abs(f2) * dinv * (np.abs(b) + sabs)
        z = np.zeros(n_rows)
        cases += [(mgamd.SPMV_CHEB, nan, dict(b=b, dinv=dinv, f1=f1, f2=f2), cheb(z), bound(z)),
                  (mgamd.SPMV_CHEB, nan, dict(b=b, dinv=dinv, f1=f1, f2=f2, xold=xold), cheb(xold), bound(xold)),
                  # xold aliased to the output buffer (the Chebyshev recurrence of the AMG smoother)
                  (mgamd.SPMV_CHEB, xold, dict(b=b, dinv=dinv, f1=f1, f2=f2, xold_is_y=True), cheb(xold), bound(xold))]
        for mode, yin, kw, ref, mag in cases:
            y, used = mgamd.debug_csr_spmv(ctx, nt, mode, lanes, ptr, col, val, x, yin, **kw)
            assert used == (lanes or auto)
            err = np.abs(y - ref)
            assert np.isfinite(y).all() and (err <= 4 * eps * mag).all(), (mode, lanes, float(np.max(err / np.maximum(mag, 1e-300))))


# ------------------------------------------------------------------ the one-level AMG against the oracle
AMG_CASES = [("annulus", 6), ("annulus", 7), ("quadrant", 6), ("quadrant", 7)]


@pytest.fixture(scope="module")
def amg_oracles():
    """the oracle's hierarchy per mesh, on the matrix of the level the product's hierarchy built (its DoF numbering depends on
    the brick layout, so the matrix comes from that very level)"""
    cache = {}

    def get(h, geo, L):
        d = h.dofs[0]
        if (geo, L) not in cache:
            cache[(geo, L)] = (d.keys(), ao.SmoothedAggregation(d.matrix()))
        keys, o = cache[(geo, L)]
        assert np.array_equal(keys, d.keys())
        return d, o

    return get


def _one_level(mgamd, ctx, monkeypatch, geo, L, degree, n_cycles, coarse="amg", number_type=None):
    if degree != 2:
        monkeypatch.setenv("MGAMD_AMG_SMOOTHER_DEGREE", str(degree))  # read when AmgCycle is built
    kw = {} if number_type is None else dict(number_type=number_type)
    h = mgamd.Hierarchy(ctx, geo, L, 1, "PMG", coarse_solver=coarse, coarse_n_cycles=n_cycles, **kw)
    monkeypatch.delenv("MGAMD_AMG_SMOOTHER_DEGREE", raising=False)
    assert len(h.operators) == 1 and h.mg.coarse_solver_used() == coarse
    return h


def _rhs(d, rng, constrained):
    """random right-hand side; constrained=False: zero on the constrained DoFs (the last rows)"""
    r = rng.standard_normal(d.n_dofs)
    if not constrained:
        r[d.info.n_interior + d.info.n_tail:] = 0.0
    return r


def _apply(mgamd, ctx, mg, r):
    vr, vz = mgamd.Vector(ctx, len(r)).from_host(r), mgamd.Vector(ctx, len(r))
    vz.set(np.nan)
    mg.vmult(vz, vr)
    return vz.to_host()


@pytest.mark.parametrize("geo,L", AMG_CASES, ids=[f"{g}-{L}" for g, L in AMG_CASES])
def test_one_level_amg_equals_oracle(mgamd, ctx, amg_oracles, monkeypatch, geo, L):
    """"amg" with 1 and 2 cycles (CoarseSolverNCycles) on the p = 1 level, FP64, right-hand sides with and without non-zero
    constrained entries; quadrant L=7 (283 k rows) runs real data through the grid-stride loop of K7"""
    rng = np.random.default_rng(5)
    for n_cycles in (1, 2):
        h = _one_level(mgamd, ctx, monkeypatch, geo, L, 2, n_cycles)
        d, o = amg_oracles(h, geo, L)
        for constrained in (False, True):
            r = _rhs(d, rng, constrained)
            err = rel_err(_apply(mgamd, ctx, h.mg, r), o.apply(r, n_cycles))
            print(f"{geo} L={L} cycles={n_cycles} constrained rhs={constrained}: rel. error {err:.2e}")
            assert err <= TOL_CYCLE, (n_cycles, constrained, err)


@pytest.mark.parametrize("degree", [1, 3, 4])
@pytest.mark.parametrize("geo,L", [("annulus", 6), ("quadrant", 6)], ids=["annulus-6", "quadrant-6"])
def test_one_level_amg_smoother_degrees(mgamd, ctx, amg_oracles, monkeypatch, geo, L, degree):
    """MGAMD_AMG_SMOOTHER_DEGREE 1, 3 (odd: the zero-start smoother begins in the other buffer, the general-start one ends with a
    copy) and 4 against the oracle at the same degree; quadrant L=6 has three AMG levels"""
    rng = np.random.default_rng(6)
    for n_cycles in (1, 2):
        h = _one_level(mgamd, ctx, monkeypatch, geo, L, degree, n_cycles)
        d, o = amg_oracles(h, geo, L)
        od = copy.copy(o)
        od.degree = degree
        for constrained in (False, True):
            r = _rhs(d, rng, constrained)
            err = rel_err(_apply(mgamd, ctx, h.mg, r), od.apply(r, n_cycles))
            print(f"{geo} L={L} degree={degree} cycles={n_cycles} constrained rhs={constrained}: rel. error {err:.2e}")
            assert err <= TOL_CYCLE, (n_cycles, constrained, err)


def test_cg_with_amg_equals_oracle(mgamd, oracle, ctx, amg_oracles, monkeypatch):
    """the coarse CG of "cg_with_amg" (reltol 1e-4, one AMG cycle as preconditioner) and the CG preconditioned by "amg":
    the oracle's pcg with the restated AMG needs the same iterations and reaches the same solution"""
    h = _one_level(mgamd, ctx, monkeypatch, "annulus", 7, 2, 1, coarse="cg_with_amg")
    d, o = amg_oracles(h, "annulus", 7)
    A = ao.csr(*d.matrix())
    b = h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    bh = b.to_host()
    xref, itref, _ = oracle.pcg(A, bh, o.precondition(1), 1e-4)
    assert rel_err(_apply(mgamd, ctx, h.mg, bh), xref) <= TOL_SOL
    ha = _one_level(mgamd, ctx, monkeypatch, "annulus", 7, 2, 1)
    x = ha.fine_operator.initialize_dof_vector()
    it, _ = mgamd.solve_cg(ha.fine_operator, ha.mg, x, b, 1e-4)
    assert it == itref and rel_err(x.to_host(), xref) <= TOL_SOL, (it, itref)
    # two AMG cycles per application of the coarse CG's preconditioner (annulus L=6, 9 763 rows): the one coarse solver x cycle
    # count whose residual / correction scratch no other test reaches
    h2 = _one_level(mgamd, ctx, monkeypatch, "annulus", 6, 2, 2, coarse="cg_with_amg")
    d2, o2 = amg_oracles(h2, "annulus", 6)
    b2 = h2.fine_operator.initialize_dof_vector()
    h2.fine_operator.rhs(b2)
    xref2, itref2, _ = oracle.pcg(ao.csr(*d2.matrix()), b2.to_host(), o2.precondition(2), 1e-4)
    err2 = rel_err(_apply(mgamd, ctx, h2.mg, b2.to_host()), xref2)
    print(f"cg_with_amg x 2, annulus L=6: iterations {h2.mg.coarse_iterations()} (oracle {itref2}), rel. error {err2:.2e}")
    assert err2 <= TOL_SOL and h2.mg.coarse_iterations() == itref2, (err2, h2.mg.coarse_iterations(), itref2)


@pytest.fixture(scope="module")
def pmg_oracles(oracle):
    """oracle PMG hierarchies on annulus L=6, built once per degree for the FP64 and the FP32 test (p = 4: 510 k DoFs)"""
    cache = {}

    def get(h, p):
        keys = [d.keys() for d in h.dofs]
        if p not in cache:
            levels, P = oracle.build_hierarchy("annulus", 6, p, "PMG", numbering_keys=keys)
            mg = oracle.Multigrid(levels, P, 3, coarse=ao.SmoothedAggregation(h.dofs[0].matrix()).precondition(2))
            Lf = levels[-1]
            cache[p] = (keys, mg, oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4))
        assert all(np.array_equal(a, b) for a, b in zip(cache[p][0], keys))
        return cache[p][1:]

    return get


def _pmg_against_oracle(mgamd, ctx, pmg_oracles, p, number_type=None):
    kw = {} if number_type is None else dict(number_type=number_type)
    h = mgamd.Hierarchy(ctx, "annulus", 6, p, "PMG", coarse_solver="amg", coarse_n_cycles=2, **kw)
    assert h.mg.coarse_solver_used() == "amg"
    mg, (xref, itref, _) = pmg_oracles(h, p)
    r = np.random.default_rng(p).standard_normal(h.n_dofs)
    err_v = rel_err(_apply(mgamd, ctx, h.mg, r), mg.vcycle(r))
    print(f"PMG p={p} {'FP32' if number_type else 'FP64'}: V-cycle rel. error {err_v:.2e}", end="")
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, _ = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    print(f", CG iterations {it} (oracle {itref}), solution rel. error {rel_err(x.to_host(), xref):.2e}")
    return err_v, it, itref, rel_err(x.to_host(), xref)


@pytest.mark.parametrize("p", [2, 4])
def test_pmg_vcycle_with_amg_equals_oracle(mgamd, ctx, pmg_oracles, p):
    """whole PMG V-cycles p -> ... -> 1 with "amg" x 2 on the p = 1 level (BASELINE configs[4]'s coarse solver) against the
    oracle's Multigrid with the restated AMG as its coarse solver; the outer CG needs the same iterations"""
    err_v, it, itref, err_x = _pmg_against_oracle(mgamd, ctx, pmg_oracles, p)
    assert err_v <= TOL_CYCLE, err_v
    assert it == itref and err_x <= TOL_SOL, (it, itref, err_x)


# ------------------------------------------------------------------ FP32 levels: AmgCycle<float>
def test_one_level_amg_float(mgamd, ctx, amg_oracles, monkeypatch):
    rng = np.random.default_rng(8)
    for n_cycles in (1, 2):
        h = _one_level(mgamd, ctx, monkeypatch, "quadrant", 6, 2, n_cycles, number_type=mgamd.F32)
        d, o = amg_oracles(h, "quadrant", 6)
        for constrained in (False, True):
            r = _rhs(d, rng, constrained)
            err = rel_err(_apply(mgamd, ctx, h.mg, r), o.apply(r, n_cycles))
            print(f"FP32 cycles={n_cycles} constrained rhs={constrained}: rel. error {err:.2e}")
            assert err <= TOL_F32, (n_cycles, constrained, err)


@pytest.mark.parametrize("p", [2, 4])
def test_pmg_vcycle_with_amg_float(mgamd, ctx, pmg_oracles, p):
    err_v, it, itref, err_x = _pmg_against_oracle(mgamd, ctx, pmg_oracles, p, mgamd.F32)
    assert err_v <= TOL_F32, err_v
    assert abs(it - itref) <= 1, (it, itref)


# ------------------------------------------------------------------ "gmg_vcycle" without a nested multigrid
def test_gmg_vcycle_without_nested_multigrid(mgamd, oracle, ctx):
    """a level 0 of <= 4096 DoFs is solved exactly ("direct"); a larger one is refused when the multigrid is built"""
    h = mgamd.Hierarchy(ctx, "quadrant", 3, 2, "HMG-global", coarse_solver="gmg_vcycle")
    assert h.mg.coarse_solver_used() == "direct"
    levels, P = oracle.build_hierarchy("quadrant", 3, 2, numbering_keys=[d.keys() for d in h.dofs])
    r = np.random.default_rng(9).standard_normal(levels[-1].n)
    assert rel_err(_apply(mgamd, ctx, h.mg, r), oracle.Multigrid(levels, P, 3).vcycle(r)) <= TOL_CYCLE
    d = mgamd.DoFs(mgamd.Triangulation("annulus", 6), 1, 0)
    assert d.n_dofs > 4096
    op = mgamd.Operator(ctx, d)
    sm = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
    with pytest.raises(mgamd.MgamdError):
        mgamd.PreconditionMG(ctx, [op], [None], [sm], "gmg_vcycle")
