"""Local smoothing (`HMG-local`, ref:multigrid_throughput.cc:1670-1873, ref:include/operator.h:49-120,152-226): operators
on the refinement levels with refinement-edge DoFs, the edge matrix, MGTransferMatrixFree between refinement levels,
copy_to_mg/copy_from_mg and the resulting preconditioner -- every piece against the independent textbook oracle
(oracle/ls_oracle.py: assembled level matrices, explicit edge index sets / edge matrices / transfer matrices), matched
through the geometric DoF keys."""
import numpy as np
import pytest

import support as su
from conftest import rel_err
from support import emu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

CASES = [("quadrant", 3, 1), ("quadrant", 4, 1), ("quadrant", 4, 2), ("quadrant", 3, 4), ("annulus", 5, 1), ("annulus", 5, 2), ("quadrant", 5, 1),
         ("hypercube", 3, 2),
         # circle: point refinement at the origin, entirely in the interior.  The refinement levels above 3 are patches that never touch
         # the boundary: their whole surface is refinement edge, the Dirichlet block of [I | T | E | D] is empty, and the patch repeats
         # with identical size level after level (125 DoFs of which 98 edge at p = 1)
         ("circle", 5, 1), ("circle", 5, 2), ("circle", 6, 1), ("circle", 6, 2),
         # several bricks per level: the finest level is 33^3 DoFs = eight 17-point bricks whose shared faces carry refinement-edge DoFs
         # (2977 of them, in the tail segment of [I | T | E | D]); the level below mixes bricks with smaller slots
         ("quadrant", 4, 4), ("quadrant", 5, 2)]
EIGHT_BRICKS = {("quadrant", 4, 4): 1657, ("quadrant", 5, 2): 1141}  # edge DoFs of the level below the finest


@pytest.fixture(scope="module")
def ls_hierarchies(mgamd, ctx):
    cache = {}

    def get(geo, L, p):
        if (geo, L, p) not in cache:
            h = mgamd.Hierarchy(ctx, geo, L, p, "HMG-local", coarse_solver="amg", max_brick=0)
            cache[(geo, L, p)] = (h, su.local_smoothing_oracle(h, geo, L, p))  # (shared with test_gpu_local_smoothing_float.py)
        return cache[(geo, L, p)]

    return get


@pytest.mark.parametrize("geo,L,p", CASES)
def test_level_operators_edge_matrices_and_transfers(mgamd, ctx, ls_hierarchies, geo, L, p):
    h, ref = ls_hierarchies(geo, L, p)
    rng = np.random.default_rng(41)
    assert len(h.operators) == len(ref.levels)
    if (geo, L, p) in EIGHT_BRICKS:
        assert sum(n for B, n in h.dofs[-1].groups()) == 8 and all(B * p + 1 == 17 for B, n in h.dofs[-1].groups() if n)
        assert (h.dofs[-1].n_dofs, h.dofs[-1].info.n_edge, h.dofs[-1].info.n_tail > 0) == (33 ** 3, 2977, True)
        assert h.dofs[-2].info.n_edge == EIGHT_BRICKS[(geo, L, p)] and len({B for B, n in h.dofs[-2].groups() if n}) > 1
    for l, (op, Lv) in enumerate(zip(h.operators, ref.levels)):
        info = h.dofs[l].info
        first_edge = info.n_interior + info.n_tail
        assert h.dofs[l].n_dofs == Lv.n and info.n_edge == Lv.edge.sum() and info.n_hanging == 0
        assert Lv.edge[first_edge:first_edge + info.n_edge].all() and Lv.edge.sum() == info.n_edge  # [I | T | E | D]
        if geo == "circle" and l > 3:  # an interior patch: edge DoFs and no Dirichlet DoF
            assert info.n_edge > 0 and info.n_dirichlet == 0 and first_edge + info.n_edge == Lv.n and not Lv.dirichlet.any()
            assert (Lv.n, info.n_edge) == {(5, 1): (125, 98), (5, 2): (729, 386), (6, 1): (425, 290), (6, 2): (2673, 1154)}[(L, p)]
        x = rng.standard_normal(Lv.n)
        src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector()
        op.vmult(dst, src)  # edge DoFs: zero input, identity rows (ref:include/operator.h:152-183)
        assert rel_err(dst.to_host(), Lv.A @ x) < 1e-13
        assert np.array_equal(src.to_host(), x)
        diag = op.initialize_dof_vector()
        op.compute_inverse_diagonal(diag)
        assert rel_err(diag.to_host(), Lv.inv_diag) < 1e-13
        op.vmult_interface_up(dst, src)  # ref:include/operator.h:203-226
        t = Lv.A_edge_in @ x
        assert np.abs(dst.to_host() - t).max() <= 1e-13 * max(np.abs(t).max(), 1.0)
        op.vmult_interface_down(dst, src)  # ref:include/operator.h:191-201: the matrix of Multigrid's residual step
        assert rel_err(dst.to_host(), Lv.A_down @ x) < 1e-13
        if l > 0:
            xc, xf0 = rng.standard_normal(ref.levels[l - 1].n), rng.standard_normal(Lv.n)
            vc, vf = h.operators[l - 1].initialize_dof_vector().from_host(xc), op.initialize_dof_vector().from_host(xf0)
            h.transfers[l].prolongate_and_add(vf, vc)
            assert rel_err(vf.to_host(), xf0 + ref.P[l] @ xc) < 1e-13
            rf, dc0 = rng.standard_normal(Lv.n), rng.standard_normal(ref.levels[l - 1].n)
            vr, vd = op.initialize_dof_vector().from_host(rf), h.operators[l - 1].initialize_dof_vector().from_host(dc0)
            h.transfers[l].restrict_and_add(vd, vr)
            assert rel_err(vd.to_host(), dc0 + ref.P[l].T @ rf) < 1e-13
        assert h.smoothers[l].eigenvalue_estimates()[1] == pytest.approx(ref.sm[l].max_ev, rel=1e-9)


@pytest.mark.parametrize("geo,L,p", CASES)
def test_local_smoothing_vcycle_and_solve(mgamd, oracle, ctx, ls_hierarchies, geo, L, p):
    h, ref = ls_hierarchies(geo, L, p)
    n = ref.G.n
    assert h.n_dofs == n and h.mg.coarse_solver_used() == "direct"
    r = np.random.default_rng(42).standard_normal(n)
    r[ref.G.constrained] = 0.0
    vr, vz = mgamd.Vector(ctx, n).from_host(r), mgamd.Vector(ctx, n)
    h.mg.vmult(vz, vr)
    zref = ref.vcycle(r)
    assert rel_err(vz.to_host(), zref) < 1e-11
    u = np.random.default_rng(43).standard_normal(n)
    u[ref.G.constrained] = 0.0
    vu, vw = mgamd.Vector(ctx, n).from_host(u), mgamd.Vector(ctx, n)
    h.mg.vmult(vw, vu)
    assert abs(u @ vz.to_host() - r @ vw.to_host()) < 1e-10 * abs(u @ vz.to_host())  # a symmetric preconditioner
    xref, itref, hist = ref.solve(1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    assert it == itref and rel_err(x.to_host(), xref) < 1e-10
    # edge prolongation is a stage of the cycle (time_edge_pro, ref:multigrid_throughput.cc:1189-1190,1391)
    h.mg.stage_timing(True)
    h.mg.vmult(vz, vr)
    ms = h.mg.stage_times()
    h.mg.stage_timing(False)
    has_edges = any(d.info.n_edge for d in h.dofs)
    assert ms[5].sum() > 0 and ms[7].sum() > 0 and ms[8].sum() > 0
    if not has_edges:
        assert ms[5].sum() < 0.2 * ms.sum()  # empty stage: only the event pairs


def test_float_levels_local_smoothing(mgamd, oracle, emu, ctx):
    """MGNumberType float (the reference's default) under the FP64 outer CG: the iteration count of the float32 emulation of the
    cycle (oracle/f32_emulation.py), which is the FP64 oracle's; tests/test_gpu_local_smoothing_float.py holds the kernels"""
    h = mgamd.Hierarchy(ctx, "quadrant", 4, 2, "HMG-local", coarse_solver="amg", number_type=mgamd.F32, max_brick=0)
    ref = su.local_smoothing_oracle(h, "quadrant", 4, 2)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    xref, it64, _ = ref.solve(1e-4)
    x32, it32, _ = oracle.pcg(ref.G.A, ref.G.rhs_constant, lambda r: emu.ls_vcycle(ref, r, np.float32).astype(np.float64), 1e-4)
    err = rel_err(x.to_host(), xref)
    print(f"FP32 local smoothing CG: iterations gpu {it}, float32 emulation {it32}, FP64 oracle {it64}, rel.err {err:.2e}")
    assert it == it32 and it32 == it64
    assert err < 1e-3


@pytest.mark.parametrize("geo,L,p", [("quadrant", 3, 4), ("annulus", 5, 2), ("quadrant", 4, 2), ("circle", 5, 2)])
def test_hpmg_local(mgamd, ctx, geo, L, p):
    """`HPMG-local` (ref:multigrid_throughput.cc:1685-1695,1846-1860): p-multigrid on the active mesh over ONE local-smoothing
    V-cycle at the lowest degree, against the composed oracle"""
    import ls_oracle

    h = mgamd.Hierarchy(ctx, geo, L, p, "HPMG-local", coarse_solver="amg", max_brick=0)
    assert h.mg.coarse_solver_used() == "gmg_vcycle" and h.degrees[-1] == p and h.degrees[0] == 1
    ref = ls_oracle.PolynomialOverLocalSmoothing(geo, L, p, numbering_keys_p=[d.keys() for d in h.dofs],
                                                 numbering_keys_levels=[d.keys() for d in h.ls["dofs"]])
    n = ref.G.n
    r = np.random.default_rng(44).standard_normal(n)
    r[ref.G.constrained] = 0.0
    vr, vz = mgamd.Vector(ctx, n).from_host(r), mgamd.Vector(ctx, n)
    h.mg.vmult(vz, vr)
    assert rel_err(vz.to_host(), ref.vcycle(r)) < 1e-11
    xref, itref, hist = ref.solve(1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    assert it == itref and rel_err(x.to_host(), xref) < 1e-10
