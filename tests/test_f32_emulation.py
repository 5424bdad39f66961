"""oracle/f32_emulation.py, the float32 restatement of the oracle's smoother and V-cycle that the FP32 GPU tolerances are
formed from, against mgoracle itself (CPU only).  In float64 it must BE mgoracle's arithmetic; in float32 every vector must
really be float32 (a float64 temporary would hide the rounding the emulation exists to measure), its distance from the
float64 result must be float32 rounding (neither zero nor large), and the preconditioned CG must not notice the difference."""
import numpy as np
import pytest

from conftest import rel_err

DEGREES = [1, 2, 3, 4, 5]
CASES = [("quadrant", 3, 4, "HMG-global"), ("quadrant", 3, 4, "PMG")]
# window for rel_err(float32 emulation, float64 oracle): 1.4e-7 .. 9.0e-7 over the six hierarchies x smoother degrees 1-5 for which
# the window was set (those below reach 6.7e-7), widened by about 10 downwards and about 2 upwards; the larger hierarchies that
# DESIGN.md (parity section) adds reach 1.5e-6.  It guards the emulation, not the product.
E_REF_WINDOW = (1e-8, 2e-6)


@pytest.fixture(scope="module")
def emu():
    import f32_emulation

    return f32_emulation


@pytest.fixture(scope="module")
def multigrids(oracle):
    cache = {}

    def get(geo, L, p, mg_type):
        if (geo, L, p, mg_type) not in cache:
            levels, P = oracle.build_hierarchy(geo, L, p, mg_type)
            cache[(geo, L, p, mg_type)] = oracle.Multigrid(levels, P, 3, coarse="direct")
        return cache[(geo, L, p, mg_type)]

    return get


def test_does_not_import_the_product(emu):
    src = open(emu.__file__).read()
    assert "dealii_multigrid_amd" not in src


@pytest.mark.parametrize("geo,L,p,mg_type", CASES)
@pytest.mark.parametrize("k", DEGREES)
def test_float64_is_the_oracle(oracle, emu, multigrids, geo, L, p, mg_type, k):
    mg = emu.with_degree(multigrids(geo, L, p, mg_type), k)
    rng = np.random.default_rng(7)
    r = rng.standard_normal(mg.levels[-1].n)
    assert rel_err(emu.vcycle(mg, r, np.float64), mg.vcycle(r)) <= 1e-14
    same = emu.with_max_evs(mg, [c.max_ev for c in mg.sm])  # (own estimates injected: the same cycle)
    assert same is not mg and np.array_equal(same.vcycle(r), mg.vcycle(r))
    for lv, c in zip(mg.levels, mg.sm):
        assert c.k == k
        fresh = oracle.Chebyshev(lv.A, lv.inv_diag, k)  # (with_degree only relabels: same smoother as a newly built one)
        assert (fresh.max_ev, fresh.delta, fresh.theta) == (c.max_ev, c.delta, c.theta)
        b, x0 = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
        assert rel_err(emu.chebyshev_vmult(c, b, np.float64), fresh.vmult(b)) <= 1e-14
        assert rel_err(emu.chebyshev_step(c, x0, b, np.float64), fresh.step(x0, b)) <= 1e-14
        assert emu.eigenvalue_estimate(lv.A, lv.inv_diag, np.float64) == pytest.approx(c.max_ev, rel=1e-14)
        # with_max_ev: mgoracle's own delta / theta from its own estimate, and the stated formula from another one
        same = emu.with_max_ev(c, c.max_ev)
        assert (same.delta, same.theta, same.k) == (c.delta, c.theta, k) and same is not c
        other = emu.with_max_ev(c, 2.0 * c.max_ev)
        assert other.theta == pytest.approx(0.5 * (2.0 * c.max_ev + 2.0 * c.max_ev / 20.0), rel=1e-15)
        assert other.delta == pytest.approx(0.5 * (2.0 * c.max_ev - 2.0 * c.max_ev / 20.0), rel=1e-15)
        assert c.theta == same.theta  # the original is untouched


@pytest.mark.parametrize("geo,L,p,mg_type", CASES)
@pytest.mark.parametrize("k", DEGREES)
def test_float32_is_float32_throughout_and_rounding_sized(oracle, emu, multigrids, geo, L, p, mg_type, k):
    mg = emu.with_degree(multigrids(geo, L, p, mg_type), k)
    rng = np.random.default_rng(7)
    r = rng.standard_normal(mg.levels[-1].n)
    z32 = emu.vcycle(mg, r, np.float32)
    assert z32.dtype == np.float32
    e_ref = rel_err(z32.astype(np.float64), mg.vcycle(r))
    print(f"{geo} {L} p={p} {mg_type} k={k}: e_ref = {e_ref:.2e}")
    assert E_REF_WINDOW[0] <= e_ref <= E_REF_WINDOW[1]
    for lv, c in zip(mg.levels[1:], mg.sm[1:]):
        b, x0 = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
        for got, ref in ((emu.chebyshev_vmult(c, b, np.float32), c.vmult(b)), (emu.chebyshev_step(c, x0, b, np.float32), c.step(x0, b))):
            assert got.dtype == np.float32
            assert E_REF_WINDOW[0] <= rel_err(got.astype(np.float64), ref) <= E_REF_WINDOW[1]
    # the intermediate vectors too: every operand the emulation hands to numpy is float32
    seen = []
    orig = emu._iterate

    def spy(c, A, dinv, x, xold, b, dtype):
        out = orig(c, A, dinv, x, xold, b, dtype)
        seen.extend([A.dtype, dinv.dtype, x.dtype, xold.dtype, b.dtype, out.dtype])
        return out

    emu._iterate = spy
    try:
        emu.vcycle(mg, r, np.float32)
    finally:
        emu._iterate = orig
    assert seen and all(d == np.float32 for d in seen)


@pytest.mark.parametrize("geo,L,p,mg_type", CASES)
def test_float32_eigenvalue_estimate(emu, multigrids, geo, L, p, mg_type):
    """float32 vectors, double dots: within 2e-6 of the float64 estimate (measured: at most 1.05e-6 over 18 levels)"""
    mg = multigrids(geo, L, p, mg_type)
    for lv, c in zip(mg.levels, mg.sm):
        ev = emu.eigenvalue_estimate(lv.A, lv.inv_diag, np.float32)
        assert ev == pytest.approx(c.max_ev, rel=2e-6)


@pytest.mark.parametrize("geo,L,p,mg_type", CASES)
@pytest.mark.parametrize("k", DEGREES)
def test_float32_cycle_keeps_the_cg_iteration_count(oracle, emu, multigrids, geo, L, p, mg_type, k):
    mg = emu.with_degree(multigrids(geo, L, p, mg_type), k)
    Lf = mg.levels[-1]
    x64, it64, _ = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    x32, it32, _ = oracle.pcg(Lf.A, Lf.rhs_constant, lambda r: emu.vcycle(mg, r, np.float32).astype(np.float64), 1e-4)
    assert it32 == it64
    assert rel_err(x32, x64) < 1e-3


# ------------------------------------------------------------------ local smoothing (HMG-local, HPMG-local)
LS_CASES = [("quadrant", 3, 1), ("quadrant", 3, 3), ("quadrant", 3, 4), ("quadrant", 4, 2), ("circle", 5, 2), ("quadrant", 3, 5)]
PLS_CASES = [("quadrant", 3, 4)]
LS_DEGREES = [1, 2, 3]
UNIT_ROUNDOFF, MARGIN, CAP = 2.0 ** -24, 16, 5e-5  # tests/test_gpu_float_levels.py


@pytest.fixture(scope="module")
def local_smoothings():
    import ls_oracle

    cache = {}

    def get(geo, L, p, composed=False):
        if (geo, L, p, composed) not in cache:
            cache[(geo, L, p, composed)] = (ls_oracle.PolynomialOverLocalSmoothing if composed else ls_oracle.LocalSmoothing)(geo, L, p)
        return cache[(geo, L, p, composed)]

    return get


def ls_input(ref):
    r = np.random.default_rng(42).standard_normal(ref.G.n)
    r[ref.G.constrained] = 0.0
    return r


def check_e_ref(e_ref):
    """a condition on the case, not on the product: float32 rounding, and so small that 16 e_ref stays under half the cap"""
    assert UNIT_ROUNDOFF < e_ref <= CAP / 2


@pytest.mark.parametrize("geo,L,p", LS_CASES)
@pytest.mark.parametrize("k", LS_DEGREES)
def test_local_smoothing_cycle(oracle, emu, local_smoothings, geo, L, p, k):
    ls = emu.ls_with_degree(local_smoothings(geo, L, p), k)
    assert ls is not local_smoothings(geo, L, p) and all(c.k == k for c in ls.sm) and all(c.k == 3 for c in local_smoothings(geo, L, p).sm)
    r = ls_input(ls)
    z64 = ls.vcycle(r)
    assert np.array_equal(emu.ls_vcycle(ls, r, np.float64), z64)
    same = emu.ls_with_max_evs(ls, [c.max_ev for c in ls.sm])
    assert same is not ls and np.array_equal(same.vcycle(r), z64)
    other = emu.ls_with_max_evs(ls, [2.0 * c.max_ev for c in ls.sm])
    assert [c.theta for c in other.sm] == pytest.approx([2.0 * c.theta for c in ls.sm], rel=1e-15) and all(c.k == k for c in other.sm)
    z32 = emu.ls_vcycle(ls, r, np.float32)
    assert z32.dtype == np.float32
    e_ref = rel_err(z32.astype(np.float64), z64)
    print(f"local smoothing {geo} {L} p={p} k={k}: e_ref = {e_ref:.2e}")
    check_e_ref(e_ref)
    # every operand of the smoother is float32 (the level matrix, D^-1, the defect after the edge subtraction, the iterates)
    seen = []
    orig = emu._iterate

    def spy(c, A, dinv, x, xold, b, dtype):
        out = orig(c, A, dinv, x, xold, b, dtype)
        seen.extend([A.dtype, dinv.dtype, x.dtype, xold.dtype, b.dtype, out.dtype])
        return out

    emu._iterate = spy
    try:
        emu.ls_vcycle(ls, r, np.float32)
    finally:
        emu._iterate = orig
    assert seen and all(d == np.float32 for d in seen)
    # the preconditioned CG does not notice the difference
    x64, it64, _ = oracle.pcg(ls.G.A, ls.G.rhs_constant, ls.vcycle, 1e-4)
    x32, it32, _ = oracle.pcg(ls.G.A, ls.G.rhs_constant, lambda v: emu.ls_vcycle(ls, v, np.float32).astype(np.float64), 1e-4)
    assert it32 == it64
    assert rel_err(x32, x64) < 1e-3


def wrong_variant(ls, which):
    """ls with every level's A_down := A (a residual without the refinement-edge rows) or A_edge_in := 0 (no edge-in correction)"""
    import copy

    ls = copy.copy(ls)
    ls.levels = [copy.copy(Lv) for Lv in ls.levels]
    for Lv in ls.levels:
        Lv.__dict__.pop("_rounded", None)
        if which == "A_down := A":
            Lv.A_down = Lv.A
        else:
            Lv.A_edge_in = Lv.A_edge_in * 0.0
    return ls


@pytest.mark.parametrize("geo,L,p", LS_CASES)
@pytest.mark.parametrize("k", LS_DEGREES)
@pytest.mark.parametrize("which", ["A_down := A", "A_edge_in := 0"])
def test_a_wrong_local_smoothing_cycle_is_far_outside_the_bound(emu, local_smoothings, geo, L, p, k, which):
    """what a bound of 16 e_ref tells apart: a cycle without the edge rows in the residual, or without the edge-in correction"""
    ls = emu.ls_with_degree(local_smoothings(geo, L, p), k)
    r = ls_input(ls)
    z64 = ls.vcycle(r)
    e_ref = rel_err(emu.ls_vcycle(ls, r, np.float32).astype(np.float64), z64)
    wrong = wrong_variant(ls, which)
    for dtype in (np.float64, np.float32):
        dist = rel_err(emu.ls_vcycle(wrong, r, dtype).astype(np.float64), z64)
        print(f"local smoothing {geo} {L} p={p} k={k} {which} in {np.dtype(dtype).name}: {dist:.2e} = {dist / e_ref:.1e} e_ref")
        assert dist >= 1000 * MARGIN * e_ref
    assert np.array_equal(ls.vcycle(r), z64)  # the original is untouched


@pytest.mark.parametrize("geo,L,p", PLS_CASES)
@pytest.mark.parametrize("k", LS_DEGREES)
def test_polynomial_over_local_smoothing_cycle(oracle, emu, local_smoothings, geo, L, p, k):
    ref = local_smoothings(geo, L, p, composed=True)
    pls = emu.pls_with_degree(ref, k)
    assert all(c.k == k for c in pls.mg.sm + pls.ls.sm) and all(c.k == 3 for c in ref.mg.sm + ref.ls.sm)
    r = ls_input(pls)
    z64 = pls.vcycle(r)
    assert np.array_equal(z64, oracle.Multigrid.vcycle(pls.mg, r))
    assert np.array_equal(emu.pls_vcycle(pls, r, np.float64), z64)
    same = emu.pls_with_max_evs(pls, [c.max_ev for c in pls.mg.sm], [c.max_ev for c in pls.ls.sm])
    assert same is not pls and same.ls is not pls.ls and np.array_equal(same.vcycle(r), z64)
    other = emu.pls_with_max_evs(pls, [c.max_ev for c in pls.mg.sm], [2.0 * c.max_ev for c in pls.ls.sm])
    assert not np.array_equal(other.vcycle(r), z64)  # the coarse solve of the copy is the copy's local-smoothing cycle
    z32 = emu.pls_vcycle(pls, r, np.float32)
    assert z32.dtype == np.float32
    e_ref = rel_err(z32.astype(np.float64), z64)
    print(f"HPMG-local {geo} {L} p={p} k={k}: e_ref = {e_ref:.2e}")
    check_e_ref(e_ref)
    x64, it64, _ = oracle.pcg(pls.G.A, pls.G.rhs_constant, pls.vcycle, 1e-4)
    x32, it32, _ = oracle.pcg(pls.G.A, pls.G.rhs_constant, lambda v: emu.pls_vcycle(pls, v, np.float32).astype(np.float64), 1e-4)
    assert it32 == it64
    assert rel_err(x32, x64) < 1e-3
