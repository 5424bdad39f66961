"""The ticket schedule of the persistent 17-point brick kernels (kernels_common.hpp TicketSchedule) against the numpy oracle.

A workgroup takes its first brick statically and every further one by a ticket of its XCD's counter; the counters reset themselves.
A lost or doubled brick is an O(1) error of the result, a counter that did not return to zero shows from the second pass on.
MGAMD_PERSISTENT_GRID caps the grid, so that the small meshes below draw several tickets per workgroup, with uneven shares:

  hypercube 4, p = 4    64 bricks of 4^3 cells: 7, 5 and 3 tickets per counter at the caps 8, 24 and 40
  hypercube 6, p = 1    64 bricks of 16^3 cells, the same counts in the p = 1 instantiations
  quadrant 5, p = 4     27 bricks (no multiple of 8) next to families and cells, fused transfers: 19 tickets at cap 8, three
                        counters with one ticket and five with none at cap 24, no ticket at cap 40 (27 workgroups)
  quadrant 7, p = 1     27 plain and 37 constrained 16^3 bricks in one launch of the pair kernel, whose two halves draw from two
                        sets of counters (the uniform p = 1 mesh has no constrained bricks, so it never reaches that kernel)

  quadrant 5, p = 4,    a local-smoothing level: 64 bricks with refinement-edge DoFs on three inner faces, in the three edge modes
  refinement level 5    (identity edge rows, edge DoFs as ordinary rows, edge columns alone): 7 and 5 tickets per counter at the caps 8, 24

and without a cap every one of them has fewer bricks than resident workgroups: the branch that draws no ticket.

Passes: the operator (mode 0), the zero-start Chebyshev sweep (modes 4, 5, 2) and one Chebyshev step (mode 2) on the finest level;
the residual (mode 1, fused mode 6) and the prolongating smoother pass (fused mode 7) run inside the V-cycle, which is the only
caller the residual pass has.  Tolerances: those of tests/support.py for the same quantities; FP32 levels as in
tests/test_gpu_float_levels.py (16 e_ref of the float32 emulation, cap 5e-5).

The references are the numpy oracle's, built once per mesh and shared by every case: about one to two minutes of CPU time per
mesh at these sizes (the sizes are what the schedule needs: 64 bricks for 40 workgroups); the device part takes seconds."""
import os

import numpy as np
import pytest

import support as su
from _degree_cases import float_cycle_reference
from conftest import rel_err
from support import emu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

HYPERCUBE_P4 = ("hypercube", 4, 4, "HMG-global")
HYPERCUBE_P1 = ("hypercube", 6, 1, "HMG-global")
OCTANT_P4 = ("quadrant", 5, 4, "HMG-global")
PAIR_P1 = ("quadrant", 7, 1, "HMG-global")
SHAPES = [HYPERCUBE_P4, HYPERCUBE_P1, OCTANT_P4]
CAPS = [8, 24, 40, None]
MARGIN_F32, CAP_F32 = 16, 5e-5  # tests/test_gpu_float_levels.py
case_id = lambda c: "-".join(map(str, c))  # noqa: E731
cap_id = lambda c: "uncapped" if c is None else f"cap{c}"  # noqa: E731


def capped_hierarchy(mgamd, ctx, case, cap, **kw):
    """the product's hierarchy with the persistent grid capped while its level operators are built"""
    before = os.environ.get("MGAMD_PERSISTENT_GRID")
    try:
        if cap is None:
            os.environ.pop("MGAMD_PERSISTENT_GRID", None)
        else:
            os.environ["MGAMD_PERSISTENT_GRID"] = str(cap)
        return su.hierarchy(mgamd, ctx, case, max_brick=0, **kw)
    finally:
        if before is None:
            os.environ.pop("MGAMD_PERSISTENT_GRID", None)
        else:
            os.environ["MGAMD_PERSISTENT_GRID"] = before


@pytest.fixture(scope="module")
def hierarchies(mgamd, ctx):
    cache = {}

    def get(case, cap, **kw):
        key = (case, cap, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = capped_hierarchy(mgamd, ctx, case, cap, **kw)
        return cache[key]

    return get


@pytest.fixture(scope="module")
def references():
    """per mesh: the oracle's finest level, or its whole hierarchy, in the numbering of the product's tables (which does not depend
    on the cap: asserted through the keys)"""
    fine, full, keys = {}, {}, {}

    def same_numbering(case, h):
        k = keys.setdefault(case, [d.keys() for d in h.dofs])
        assert all(np.array_equal(a, d.keys()) for a, d in zip(k, h.dofs))

    def finest(case, h):
        same_numbering(case, h)
        if case in full:
            return full[case][0][-1]
        if case not in fine:
            fine[case] = su.oracle_level(h.dofs[-1], *case[:3])
        return fine[case]

    def whole(case, h):
        same_numbering(case, h)
        if case not in full:
            full[case] = su.oracle_hierarchy(h.dofs, case)
        return full[case]

    finest.whole = whole
    return finest


def check_finest_level(mgamd, oracle, ctx, h, lv, tag):
    """operator, zero-start Chebyshev sweep and Chebyshev step on the finest level, twice (the second pass meets the counters
    the first one left)"""
    op = h.fine_operator
    rng = np.random.default_rng(3)
    ch = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
    cref = oracle.Chebyshev(lv.A, lv.inv_diag, 3, 20.0, 20)
    assert ch.eigenvalue_estimates()[1] == pytest.approx(cref.max_ev, rel=1e-10)
    for trial in range(2):
        x, b = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
        ea = rel_err(su.apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x)
        ev = rel_err(su.apply_nan(mgamd, ctx, ch.vmult, b), cref.vmult(b))
        vx, vb = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector().from_host(b)
        ch.step(vx, vb)
        es = rel_err(vx.to_host(), cref.step(x, b))
        print(f"{tag} pass {trial}: vmult {ea:.2e}, Chebyshev vmult {ev:.2e}, step {es:.2e}")
        assert ea < su.TOL_OP
        assert ev < su.TOL_CHEB and es < su.TOL_CHEB


@pytest.mark.parametrize("cap", CAPS, ids=cap_id)
@pytest.mark.parametrize("case", SHAPES, ids=case_id)
def test_operator_passes(mgamd, oracle, emu, ctx, hierarchies, references, case, cap):
    h = hierarchies(case, cap)
    n_bricks = max(n for B, n in h.dofs[-1].groups() if B * case[2] + 1 == 17)
    assert n_bricks == (27 if case == OCTANT_P4 else 64)
    if case == OCTANT_P4:
        assert n_bricks % 8 != 0 and sum(t.n_fused_bricks() for t in h.transfers[1:]) > 0
        assert all(n > 0 for B, n in h.dofs[-1].groups())  # families and cells next to the bricks
    levels, P = references.whole(case, h)
    tag = f"{case_id(case)} {cap_id(cap)}"
    check_finest_level(mgamd, oracle, ctx, h, levels[-1], tag)
    # the V-cycle: residual and fused transfer passes
    mg = su.injected(emu, oracle, levels, P, h)
    r = np.random.default_rng(7).standard_normal(levels[-1].n)
    ez = rel_err(su.apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r))
    print(f"{tag}: V-cycle {ez:.2e}")
    assert ez < su.TOL_CYCLE


@pytest.mark.parametrize("cap", [8, 24], ids=cap_id)
def test_pair_kernel_halves_draw_from_their_own_counters(mgamd, oracle, ctx, hierarchies, references, cap):
    h = hierarchies(PAIR_P1, cap)
    assert [n for B, n in h.dofs[-1].groups() if B == 16] == [27, 37]  # plain, constrained: more than the cap each
    check_finest_level(mgamd, oracle, ctx, h, references(PAIR_P1, h), f"{case_id(PAIR_P1)} {cap_id(cap)}")


@pytest.mark.parametrize("case", SHAPES, ids=case_id)
def test_counters_return_to_zero(mgamd, oracle, emu, ctx, hierarchies, references, case):
    """five operator applications in a row, a V-cycle, the operator again: every result against the oracle"""
    h = hierarchies(case, 24)
    levels, P = references.whole(case, h)
    mg = su.injected(emu, oracle, levels, P, h)
    lv = levels[-1]
    rng = np.random.default_rng(11)
    x = rng.standard_normal(lv.n)
    want = lv.A @ x
    for i in range(5):
        e = rel_err(su.apply_nan(mgamd, ctx, h.fine_operator.vmult, x), want)
        print(f"{case_id(case)} vmult {i}: {e:.2e}")
        assert e < su.TOL_OP
    r = rng.standard_normal(lv.n)
    ez = rel_err(su.apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r))
    e = rel_err(su.apply_nan(mgamd, ctx, h.fine_operator.vmult, x), want)
    print(f"{case_id(case)}: V-cycle {ez:.2e}, vmult after it {e:.2e}")
    assert ez < su.TOL_CYCLE and e < su.TOL_OP


def test_graph_replay(mgamd, oracle, emu, ctx, hierarchies, references):
    """three replays of the captured cycle: no host code runs between the launches that share a set of counters"""
    h = hierarchies(OCTANT_P4, 24)
    levels, P = references.whole(OCTANT_P4, h)
    mg = su.injected(emu, oracle, levels, P, h)
    n = levels[-1].n
    r = np.random.default_rng(7).standard_normal(n)
    eager = su.apply_nan(mgamd, ctx, h.mg.vmult, r)
    vz, vr = mgamd.Vector(ctx, n).from_host(np.full(n, np.nan)), mgamd.Vector(ctx, n).from_host(r)
    ms = h.mg.time_vcycles(vz, vr, 3, True)
    z = vz.to_host()
    assert ms > 0 and np.isfinite(z).all()
    e_eager, e_ref = rel_err(z, eager), rel_err(z, mg.vcycle(r))
    print(f"graph replay: against the eager cycle {e_eager:.2e}, against the oracle {e_ref:.2e}")
    assert e_eager < su.TOL_CYCLE and e_ref < su.TOL_CYCLE
    assert rel_err(su.apply_nan(mgamd, ctx, h.mg.vmult, r), eager) < su.TOL_CYCLE  # and the eager cycle after the replays


def test_float_levels(mgamd, oracle, emu, ctx, hierarchies, references):
    """FP32 levels under FP64 outer vectors: the last pass writes wide (out_wide)"""
    h64 = hierarchies(OCTANT_P4, 24)
    h = hierarchies(OCTANT_P4, 24, number_type=mgamd.F32)
    levels, P = references.whole(OCTANT_P4, h64)
    assert all(np.array_equal(a.keys(), b.keys()) for a, b in zip(h.dofs, h64.dofs))
    mg = oracle.Multigrid(levels, P, 3, coarse="direct")
    n = levels[-1].n
    r = np.random.default_rng(7).standard_normal(n)
    mgp, ref, e_ref = float_cycle_reference(emu, mg, [s.eigenvalue_estimates()[1] for s in h.smoothers], r)
    for trial in range(2):
        z = su.apply_nan(mgamd, ctx, h.mg.vmult, r)
        err = rel_err(z, ref)
        print(f"FP32 V-cycle {trial}: rel.err {err:.2e}, e_ref {e_ref:.2e}, ratio {err / e_ref:.2f}")
        assert err <= MARGIN_F32 * e_ref
        assert err < CAP_F32


@pytest.fixture(scope="module")
def edge_level():
    """ls_oracle.LSLevel of refinement level 5 of quadrant 5 at p = 4, assembled once for both caps"""
    import ls_oracle

    kept = {}

    def get(d):
        if not kept:
            kept["keys"] = d.keys()
            kept["level"] = ls_oracle.LSLevel(ls_oracle.level_meshes(su.mesh("quadrant", 5))[5], 4, kept["keys"])
        assert np.array_equal(kept["keys"], d.keys())  # the numbering does not depend on the cap
        return kept["level"]

    return get


@pytest.mark.parametrize("cap", [8, 24], ids=cap_id)
def test_tickets_in_the_edge_modes(mgamd, oracle, ctx, edge_level, cap):
    """A local-smoothing level operator on 64 bricks: refinement level 5 of quadrant 5 at p = 4, 16^3 cells whose three inner faces
    are refinement edge, the smallest mesh on which a refinement edge meets more bricks than the smallest cap.  Identity edge rows
    (vmult, the Chebyshev passes), the edge DoFs as ordinary rows (vmult_interface_down) and the edge columns alone
    (vmult_interface_up) all draw tickets; each twice, then vmult again."""
    before = os.environ.get("MGAMD_PERSISTENT_GRID")
    os.environ["MGAMD_PERSISTENT_GRID"] = str(cap)
    try:
        d = mgamd.DoFs(mgamd.Triangulation("quadrant", 5).level_mesh(5), 4, 0, local_smoothing_level=True)
        op = mgamd.Operator(ctx, d, mgamd.F64)
    finally:
        if before is None:
            os.environ.pop("MGAMD_PERSISTENT_GRID", None)
        else:
            os.environ["MGAMD_PERSISTENT_GRID"] = before
    assert sum(n for B, n in d.groups() if B * 4 + 1 == 17) == 64 and sum(n for B, n in d.groups()) == 64
    assert (d.n_dofs, d.info.n_edge, d.info.n_dirichlet) == (274625, 12097, 12481)
    lv = edge_level(d)
    assert lv.n == d.n_dofs and lv.edge.sum() == d.info.n_edge
    ch = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
    cref = oracle.Chebyshev(lv.A, lv.inv_diag, 3, 20.0, 20)
    assert ch.eigenvalue_estimates()[1] == pytest.approx(cref.max_ev, rel=1e-10)
    rng = np.random.default_rng(3)
    tag = f"quadrant-5-4 level 5 {cap_id(cap)}"
    for trial in range(2):
        x, b = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
        ea = rel_err(su.apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x)
        ed = rel_err(su.apply_nan(mgamd, ctx, op.vmult_interface_down, x), lv.A_down @ x)
        t = lv.A_edge_in @ x
        eu = np.abs(su.apply_nan(mgamd, ctx, op.vmult_interface_up, x) - t).max() / max(np.abs(t).max(), 1.0)
        ev = rel_err(su.apply_nan(mgamd, ctx, ch.vmult, b), cref.vmult(b))
        vx, vb = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector().from_host(b)
        ch.step(vx, vb)
        es = rel_err(vx.to_host(), cref.step(x, b))
        print(f"{tag} pass {trial}: vmult {ea:.2e}, interface down {ed:.2e}, interface up (max norm) {eu:.2e}, Chebyshev vmult {ev:.2e}, "
              f"step {es:.2e}")
        assert ea < su.TOL_OP and ed < su.TOL_OP and eu <= su.TOL_OP
        assert ev < su.TOL_CHEB and es < su.TOL_CHEB
    ea = rel_err(su.apply_nan(mgamd, ctx, op.vmult, x), lv.A @ x)
    print(f"{tag}: vmult after them {ea:.2e}")
    assert ea < su.TOL_OP
