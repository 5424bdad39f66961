"""Smoother degrees 1, 2, 4 and 5 on FP64 levels (every other GPU test runs degree 3), against the numpy oracle.

The degree decides the buffer logic of the cycle (runtime.hip): which of the two smoother buffers the outer z stands in for
when outer vectors and levels have one number type (odd: the second, even: the first), whether the final copy runs, the
"x1 on the fly" start passes (degree >= 2) against the plain scaled product (degree 1), the fused prolongation inside the
first post-smoothing pass followed by degree - 1 plain passes, and, on float levels under double outer vectors, the result
written wide inside the last pass (degree >= 2) or cast afterwards (degree 1).

Bounds are those of test_gpu_parity.py: estimates 1e-9, V-cycle 1e-11, CG counts equal, solution 1e-10.  Rows with an FP32
number type use the bound of test_gpu_float_levels.py, 16 * e_ref under the 5e-5 cap.

Hierarchies (_degree_cases.py): quadrant 3 p=4 HMG-global (hanging nodes), hypercube 4 p=2 HMG-global (17-point bricks, fused
transfers), quadrant 3 p=4 PMG, and quadrant 5 p=2 HMG-global, the mixed FUSED_CASES hierarchy whose numpy oracle builds
fastest (11.3 s on the CPU; quadrant 6 p=1 12.9 s, quadrant 4 p=4 30.8 s).  Each oracle hierarchy is built once."""
import threading

import numpy as np
import pytest

from _degree_cases import (HIER_CASES, HYPERCUBE_HMG, QUADRANT_HMG, float_cycle_reference, n_fused, oracle_levels, oracle_multigrid,
                           round32)
from conftest import rel_err

pytestmark = pytest.mark.gpu

DEGREES = [1, 2, 4, 5]
TOL_VCYCLE = 1e-11
TOL_SOL = 1e-10
FLOAT_MARGIN = 16  # test_gpu_float_levels.py says where it comes from
FLOAT_CAP = 5e-5


@pytest.fixture(scope="module")
def hierarchies(mgamd, ctx):
    cache = {}

    def get(case, k, number_type=None):
        number_type = mgamd.F64 if number_type is None else number_type
        if (case, k, number_type) not in cache:
            geo, L, p, mg_type = case
            cache[(case, k, number_type)] = mgamd.Hierarchy(ctx, geo, L, p, mg_type, smoother_degree=k, coarse_solver="amg",
                                                            number_type=number_type, max_brick=0)
        return cache[(case, k, number_type)]

    return get


def nan_vector(mgamd, ctx, n, number_type=None):
    v = mgamd.Vector(ctx, n) if number_type is None else mgamd.Vector(ctx, n, number_type)
    return v.from_host(np.full(n, np.nan))  # an entry that the cycle does not store stays NaN


def same_vector(a, b):
    return np.array_equal(a, b) or rel_err(a, b) < 1e-14  # (atomic summation order)


@pytest.mark.parametrize("case", HIER_CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("k", DEGREES)
def test_vcycle(mgamd, oracle, ctx, hierarchies, case, k):
    h = hierarchies(case, k)
    levels, P = oracle_levels(oracle, case, h)
    mg = oracle_multigrid(oracle, case, h, k)
    if case == HYPERCUBE_HMG:
        assert n_fused(h) > 0
    for l, s in enumerate(h.smoothers):
        assert s.eigenvalue_estimates()[1] == pytest.approx(mg.sm[l].max_ev, rel=1e-9)
    n = levels[-1].n
    r = np.random.default_rng(7).standard_normal(n)
    ref = mg.vcycle(r)
    vr, vz = mgamd.Vector(ctx, n).from_host(r), nan_vector(mgamd, ctx, n)
    h.mg.vmult(vz, vr)
    z = vz.to_host()
    assert np.isfinite(z).all()
    err = rel_err(z, ref)
    print(f"V-cycle {case} k={k}: rel.err {err:.2e}")
    assert err < TOL_VCYCLE
    assert np.array_equal(vr.to_host(), r)  # the right-hand side is read only
    h.mg.vmult(vz, vr)
    assert same_vector(vz.to_host(), z)  # no state left in the smoother buffers
    # graph replay
    vz.from_host(np.full(n, np.nan))
    ms = h.mg.time_vcycles(vz, vr, 2, True)
    assert ms > 0 and rel_err(vz.to_host(), ref) < TOL_VCYCLE and rel_err(vz.to_host(), z) < 1e-13
    # stage callbacks: the separate stages of the reference instead of the fused passes
    events = []
    h.mg.connect_stages(lambda s, start, lv: events.append((s, start, lv)))
    vz.from_host(np.full(n, np.nan))
    h.mg.vmult(vz, vr)
    h.mg.connect_stages(None)
    nl = len(levels)
    assert events[0] == (7, True, nl - 1) and events[-1] == (8, False, nl - 1)
    assert rel_err(vz.to_host(), ref) < TOL_VCYCLE and rel_err(vz.to_host(), z) < 1e-13
    assert np.array_equal(vr.to_host(), r)


@pytest.mark.parametrize("case", HIER_CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("k", DEGREES)
def test_cg_iteration_counts_and_solution(mgamd, oracle, ctx, hierarchies, case, k):
    h = hierarchies(case, k)
    levels, P = oracle_levels(oracle, case, h)
    mg = oracle_multigrid(oracle, case, h, k)
    Lf = levels[-1]
    xref, itref, hist = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    err = rel_err(x.to_host(), xref)
    print(f"CG {case} k={k}: iterations gpu {it} oracle {itref}, rel.err {err:.2e}")
    assert it == itref
    assert res == pytest.approx(hist[-1], rel=1e-6)
    assert err < TOL_SOL


@pytest.mark.parametrize("k", [1, 2])
def test_separate_transfer_kernels(mgamd, oracle, ctx, hierarchies, k, monkeypatch):
    """MGAMD_NO_FUSED_TRANSFER=1 on the brick hierarchy: prolongation as a kernel of its own before the post-smoother"""
    case = HYPERCUBE_HMG
    geo, L, p, mg_type = case
    h = hierarchies(case, k)
    monkeypatch.setenv("MGAMD_NO_FUSED_TRANSFER", "1")
    h0 = mgamd.Hierarchy(ctx, geo, L, p, mg_type, smoother_degree=k, coarse_solver="amg", max_brick=0)
    monkeypatch.delenv("MGAMD_NO_FUSED_TRANSFER")
    assert n_fused(h) > 0 and n_fused(h0) == 0
    mg = oracle_multigrid(oracle, case, h, k)
    n = h.n_dofs
    r = np.random.default_rng(11).standard_normal(n)
    vr, vz, vz0 = mgamd.Vector(ctx, n).from_host(r), nan_vector(mgamd, ctx, n), nan_vector(mgamd, ctx, n)
    h.mg.vmult(vz, vr)
    h0.mg.vmult(vz0, vr)
    err, err0 = rel_err(vz.to_host(), mg.vcycle(r)), rel_err(vz0.to_host(), mg.vcycle(r))
    print(f"separate transfers k={k}: fused {err:.2e} separate {err0:.2e}")
    assert err < TOL_VCYCLE and err0 < TOL_VCYCLE
    assert rel_err(vz.to_host(), vz0.to_host()) < 1e-13


@pytest.mark.parametrize("k", [1, 2])
def test_no_collapsed_levels(mgamd, oracle, ctx, hierarchies, k, monkeypatch):
    """MGAMD_COLLAPSE_MAX_DOFS=0: every level below the finest runs its degree-k smoother kernel by kernel (by default the
    levels up to 2048 DoFs are one precomputed dense matrix and never run a smoother)"""
    case = QUADRANT_HMG
    geo, L, p, mg_type = case
    h = hierarchies(case, k)
    monkeypatch.setenv("MGAMD_COLLAPSE_MAX_DOFS", "0")
    h0 = mgamd.Hierarchy(ctx, geo, L, p, mg_type, smoother_degree=k, coarse_solver="amg", max_brick=0)
    monkeypatch.delenv("MGAMD_COLLAPSE_MAX_DOFS")
    levels, P = oracle_levels(oracle, case, h)
    mg = oracle_multigrid(oracle, case, h, k)
    n = h.n_dofs
    r = np.random.default_rng(9).standard_normal(n)
    vr, vz0 = mgamd.Vector(ctx, n).from_host(r), nan_vector(mgamd, ctx, n)
    h0.mg.vmult(vz0, vr)
    z0 = vz0.to_host()
    err = rel_err(z0, mg.vcycle(r))
    print(f"no collapsed levels k={k}: rel.err {err:.2e}")
    assert np.isfinite(z0).all() and err < TOL_VCYCLE
    h0.mg.vmult(vz0, vr)
    assert same_vector(vz0.to_host(), z0)
    Lf = levels[-1]
    xref, itref, hist = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h0.fine_operator.initialize_dof_vector(), h0.fine_operator.initialize_dof_vector()
    h0.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h0.fine_operator, h0.mg, x, b, 1e-4)
    assert it == itref and rel_err(x.to_host(), xref) < TOL_SOL


@pytest.mark.parametrize("k", [1, 2])
def test_auto_slot_policy(mgamd, ctx, k, monkeypatch):
    """max_brick=-1 against max_brick=0 through the DoF keys (as test_gpu_parity.test_auto_slot_policy_same_vcycle)"""
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")
    geo, L, p = "quadrant", 4, 2
    ha = mgamd.Hierarchy(ctx, geo, L, p, "HMG-global", smoother_degree=k, coarse_solver="amg", max_brick=-1)
    hb = mgamd.Hierarchy(ctx, geo, L, p, "HMG-global", smoother_degree=k, coarse_solver="amg", max_brick=0)
    ka, kb = ha.dofs[-1].keys(), hb.dofs[-1].keys()
    pos = {tuple(key): i for i, key in enumerate(kb.tolist())}
    perm = np.array([pos[tuple(key)] for key in ka.tolist()])
    rb = np.random.default_rng(5).standard_normal(len(kb))
    za, zb = nan_vector(mgamd, ctx, len(ka)), nan_vector(mgamd, ctx, len(kb))
    ha.mg.vmult(za, mgamd.Vector(ctx, len(ka)).from_host(rb[perm]))
    hb.mg.vmult(zb, mgamd.Vector(ctx, len(kb)).from_host(rb))
    err = rel_err(za.to_host(), zb.to_host()[perm])
    print(f"slot policies k={k}: rel.err {err:.2e}")
    assert np.isfinite(za.to_host()).all() and err < TOL_VCYCLE


@pytest.mark.parametrize("k", [1, 2])
def test_local_smoothing(mgamd, ctx, k):
    import ls_oracle

    geo, L, p = "quadrant", 3, 2
    h = mgamd.Hierarchy(ctx, geo, L, p, "HMG-local", smoother_degree=k, coarse_solver="amg", max_brick=0)
    ref = ls_oracle.LocalSmoothing(geo, L, p, smoother_degree=k, numbering_keys_global=h.active_dofs.keys(),
                                   numbering_keys_levels=[d.keys() for d in h.dofs])
    for l, s in enumerate(h.smoothers):
        assert s.eigenvalue_estimates()[1] == pytest.approx(ref.sm[l].max_ev, rel=1e-9)
    n = ref.G.n
    r = np.random.default_rng(42).standard_normal(n)
    r[ref.G.constrained] = 0.0
    vr, vz = mgamd.Vector(ctx, n).from_host(r), nan_vector(mgamd, ctx, n)
    h.mg.vmult(vz, vr)
    z = vz.to_host()
    err = rel_err(z, ref.vcycle(r))
    print(f"local smoothing k={k}: rel.err {err:.2e}")
    assert np.isfinite(z).all() and err < TOL_VCYCLE
    xref, itref, hist = ref.solve(1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    assert it == itref and rel_err(x.to_host(), xref) < TOL_SOL


def run_ranks(n_ranks, fn):
    out, err = [None] * n_ranks, [None] * n_ranks

    def work(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # noqa
            err[r] = e

    th = [threading.Thread(target=work, args=(r,)) for r in range(n_ranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not any(t.is_alive() for t in th), "a simulated rank did not finish"
    for e in err:
        if e is not None:
            raise e
    return out


def key_vector(keys, seed):
    """deterministic pseudo-random value per geometric DoF key: the same GLOBAL vector on every rank and in the oracle"""
    k = np.asarray(keys, dtype=np.int64)
    h = (k[:, 0] * 73856093) ^ (k[:, 1] * 19349663) ^ (k[:, 2] * 83492791) ^ (k[:, 3] * 2654435761) ^ (k[:, 4] * 97) ^ seed
    return np.sin(h.astype(np.float64) * 1e-3) + 0.25 * np.cos(h.astype(np.float64) * 7e-5)


@pytest.fixture(scope="module")
def sharded_oracle_levels(oracle):
    return oracle.build_hierarchy("quadrant", 4, 2, "HMG-global")


@pytest.mark.parametrize("k", [2, 5])
def test_two_ranks(mgamd, oracle, sharded_oracle_levels, k, monkeypatch):
    """two simulated ranks against the numpy oracle with the key-hash start vector (pattern and bounds of
    test_gpu_distributed_sim.test_sharded_hierarchy_matches_numpy_oracle)"""
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")
    geo, L, p, n_ranks = "quadrant", 4, 2, 2
    levels, P = sharded_oracle_levels
    omg = oracle.Multigrid(levels, P, k, coarse="direct", start_vectors=[oracle.key_hash_start_vector(lv) for lv in levels])
    Lf = levels[-1]
    kf = {tuple(int(v) for v in key): i for i, key in enumerate(Lf.keys)}
    r = key_vector(Lf.keys, 2)
    r[Lf.constrained] = 0.0
    zref = omg.vcycle(r)
    xref, itref, hist = oracle.pcg(Lf.A, Lf.rhs_constant, omg.vcycle, 1e-4)
    group = mgamd.SimGroup(n_ranks)

    def rank_main(rk):
        ctx = mgamd.Context(0)
        h = mgamd.DistributedHierarchy(ctx, group.comm(rk), geo, L, p, smoother_degree=k, coarse_solver="amg", max_brick=0,
                                       min_root_dofs=0)
        idx = np.array([kf[tuple(int(v) for v in key)] for key in h.dofs[-1].keys()])
        op = h.fine_operator
        vr, vz = op.initialize_dof_vector().from_host(r[idx]), op.initialize_dof_vector().from_host(np.full(len(idx), np.nan))
        h.mg.vmult(vz, vr)
        b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
        op.rhs(b)
        it, res = mgamd.solve_cg(op, h.mg, x, b, 1e-4)
        return dict(idx=idx, z=vz.to_host(), x=x.to_host(), it=it, n_dofs=h.n_dofs, dist=list(h.distributed), peers=h.dofs[-1].info.n_peers)

    for o in run_ranks(n_ranks, rank_main):
        assert o["n_dofs"] == Lf.n and o["peers"] >= 1 and o["dist"][-1]
        err = rel_err(o["z"], zref[o["idx"]])
        print(f"two ranks k={k}: V-cycle rel.err {err:.2e}, iterations {o['it']} (oracle {itref})")
        assert np.isfinite(o["z"]).all() and err < TOL_VCYCLE
        assert o["it"] == itref
        assert rel_err(o["x"], xref[o["idx"]]) < TOL_SOL


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("levels_type,outer_type", [("F64", "F64"), ("F32", "F64"), ("F32", "F32"), ("F64", "F32")])
def test_number_types_of_levels_and_outer_vectors(mgamd, oracle, ctx, hierarchies, levels_type, outer_type, k):
    """(F32, F32) is the aliasing path (z stands in for a smoother buffer) in float; (F32, F64) writes z wide inside the last
    pass for k >= 2 and casts after it for k = 1; (F64, F32) copies in and out.  An FP32 outer r is rounded first and the
    rounded r goes to the reference."""
    import f32_emulation as emu

    case = QUADRANT_HMG
    lt, ot = getattr(mgamd, levels_type), getattr(mgamd, outer_type)
    h = hierarchies(case, k, lt)
    mg = oracle_multigrid(oracle, case, hierarchies(case, k), k)
    n = h.n_dofs
    r = np.random.default_rng(7).standard_normal(n)
    if ot == mgamd.F32:
        r = round32(r)
    vr, vz = mgamd.Vector(ctx, n, ot).from_host(r), nan_vector(mgamd, ctx, n, ot)
    h.mg.vmult(vz, vr)
    z = vz.to_host()
    assert np.isfinite(z).all()
    assert np.array_equal(vr.to_host(), r)
    if (lt, ot) == (mgamd.F64, mgamd.F64):
        err = rel_err(z, mg.vcycle(r))
        print(f"levels {levels_type} outer {outer_type} k={k}: rel.err {err:.2e}")
        assert err < TOL_VCYCLE
    else:
        mgp, ref, e_ref = float_cycle_reference(emu, mg, [s.eigenvalue_estimates()[1] for s in h.smoothers], r)
        err = rel_err(z, ref)
        print(f"levels {levels_type} outer {outer_type} k={k}: rel.err {err:.2e}, e_ref {e_ref:.2e}, ratio {err / e_ref:.2f}")
        assert err <= FLOAT_MARGIN * e_ref
        assert rel_err(z, mg.vcycle(r)) < FLOAT_CAP
    # a second cycle; graph replay and stage callbacks, which take other copy paths for the outer vectors (callbacks the
    # cast-after path).  In float the atomic summation order moves the result by float32 rounding: the bound again, not equality
    def check_again(what):
        if (lt, ot) == (mgamd.F64, mgamd.F64):
            assert rel_err(vz.to_host(), z) < 1e-13
        else:
            again = rel_err(vz.to_host(), ref)
            print(f"  {what}: rel.err {again:.2e}, ratio {again / e_ref:.2f}")
            assert np.isfinite(vz.to_host()).all() and again <= FLOAT_MARGIN * e_ref

    vz.from_host(np.full(n, np.nan))
    h.mg.vmult(vz, vr)
    check_again("second cycle")
    vz.from_host(np.full(n, np.nan))
    h.mg.time_vcycles(vz, vr, 2, True)
    check_again("graph replay")
    h.mg.connect_stages(lambda s, start, lv: None)
    vz.from_host(np.full(n, np.nan))
    h.mg.vmult(vz, vr)
    h.mg.connect_stages(None)
    check_again("stage callbacks")
