"""The AMG coarse solvers on a SHARDED coarse level (csrc/amg_shard.hpp, runtime.hip AmgCycle in its sharded set-up, the ranged
entry point of K7 and the level-0 gather / scatter kernels of kernels_amg.hpp) on simulated ranks: n ranks run as host threads over the in-process communicator
(as in test_gpu_distributed_sim.py); partition, shard plans, ghost imports, partial restrictions + all-reduce and the level-0
exchange are the production code.  Compared, through the geometric DoF keys, with the independent numpy restatement
oracle/amg_oracle.py on the GLOBAL matrix and with the one-rank Hierarchy.  Tolerances: test_gpu_amg.py's own."""
import copy
import os
import threading

import numpy as np
import pytest

import amg_oracle as ao
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_CYCLE = 1e-11  # test_gpu_amg.py
TOL_SOL = 1e-10
TOL_F32 = 5e-5


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
    for e in err:
        if e is not None:
            raise e
    return out


def keyset(keys):
    return [tuple(int(v) for v in k) for k in keys]


@pytest.fixture(autouse=True)
def key_based_chebyshev_start_vector():
    os.environ["MGAMD_CHEB_KEY_INIT"] = "1"
    yield
    del os.environ["MGAMD_CHEB_KEY_INIT"]


@pytest.fixture(scope="module")
def one_rank(mgamd):
    """per mesh: the global p = 1 DoFs (the numbering every rank's setup uses), their key -> row map, the oracle's hierarchy on
    their matrix and the rows of the AMG's second level"""
    cache = {}

    def get(geo, L):
        if (geo, L) not in cache:
            d = mgamd.DoFs(mgamd.Triangulation(geo, L), 1, 0)
            kf = {k: i for i, k in enumerate(keyset(d.keys()))}
            sizes = d.amg_setup_info()
            cache[(geo, L)] = (d, kf, ao.SmoothedAggregation(d.matrix()), sizes[1][0])
        return cache[(geo, L)]

    return get


def _apply(mgamd, ctx, mg, r):
    vr, vz = mgamd.Vector(ctx, len(r)).from_host(r), mgamd.Vector(ctx, len(r))
    vz.set(np.nan)
    mg.vmult(vz, vr)
    return vz.to_host()


def _rhs_pair(d, seed):
    rng = np.random.default_rng(seed)
    r0, r1 = rng.standard_normal(d.n_dofs), rng.standard_normal(d.n_dofs)
    r0[d.info.n_interior + d.info.n_tail:] = 0.0  # without / with non-zero constrained entries
    return r0, r1


def _check_copies_identical(out, field, n):
    """copies of shared DoFs are bitwise identical across ranks; every global DoF is held by some rank"""
    ref, seen = np.zeros(n), np.zeros(n, bool)
    for o in out:
        idx, v = o["idx"], o[field]
        m = seen[idx]
        assert np.array_equal(ref[idx][m], v[m])
        ref[idx], seen[idx] = v, True
    assert seen.all()


def _sharded_one_level(mgamd, group, rk, geo, L, n_cycles, min_rows, kf, rhs, coarse="amg", number_type=None, sharded_amg=True):
    ctx = mgamd.Context(0)
    kw = {} if number_type is None else dict(number_type=number_type)
    h = mgamd.DistributedHierarchy(ctx, group.comm(rk), geo, L, 1, coarse_solver=coarse, max_brick=0, min_root_dofs=0, mg_type="PMG",
                                   coarse_n_cycles=n_cycles, sharded_amg=sharded_amg, amg_min_sharded_rows=min_rows, **kw)
    assert len(h.operators) == 1
    idx = np.array([kf[k] for k in keyset(h.dofs[0].keys())])
    return dict(idx=idx, z=[_apply(mgamd, ctx, h.mg, r[idx]) for r in rhs], used=h.mg.coarse_solver_used(), layout=h.mg.amg_layout(),
                its=h.mg.coarse_iterations(), dist=h.distributed[0])


AMG_CASES = [("annulus", 7), ("quadrant", 6)]


@pytest.mark.parametrize("n_ranks", [2, 3, 4, 8])
@pytest.mark.parametrize("geo,L", AMG_CASES, ids=[f"{g}-{L}" for g, L in AMG_CASES])
def test_sharded_amg_equals_oracle_and_one_rank(mgamd, ctx, one_rank, geo, L, n_ranks):
    """the p = 1 "PMG" hierarchy is one level: a pure application of the coarse solver.  "amg" x 1 and x 2, every level above the
    dense one sharded (min_sharded_rows 0) and level 0 only, right-hand sides without and with non-zero constrained entries"""
    d, kf, o, rows1 = one_rank(geo, L)
    rhs = _rhs_pair(d, 5)
    for n_cycles in (1, 2):
        h1 = mgamd.Hierarchy(ctx, geo, L, 1, "PMG", coarse_solver="amg", coarse_n_cycles=n_cycles, max_brick=0)
        assert np.array_equal(h1.dofs[0].keys(), d.keys())
        z1 = [_apply(mgamd, ctx, h1.mg, r) for r in rhs]
        zo = [o.apply(r, n_cycles) for r in rhs]
        for min_rows in (0, rows1):
            group = mgamd.SimGroup(n_ranks)
            out = run_ranks(n_ranks, lambda rk: _sharded_one_level(mgamd, group, rk, geo, L, n_cycles, min_rows, kf, rhs))
            for o_r in out:
                assert o_r["used"] == "amg" and o_r["dist"]
                lay = o_r["layout"]
                assert not lay[0]["replicated"] and lay[-1]["replicated"] and lay[0]["global_rows"] == d.n_dofs
                if min_rows:
                    assert all(lv["replicated"] for lv in lay[1:])
                for k in range(2):
                    e_o, e_1 = rel_err(o_r["z"][k], zo[k][o_r["idx"]]), rel_err(o_r["z"][k], z1[k][o_r["idx"]])
                    print(f"{geo} L={L} ranks={n_ranks} cycles={n_cycles} min_rows={min_rows} constrained rhs={bool(k)}: "
                          f"vs oracle {e_o:.2e}, vs one rank {e_1:.2e}")
                    assert e_o <= TOL_CYCLE and e_1 <= TOL_CYCLE, (n_cycles, min_rows, k, e_o, e_1)
            for k in range(2):
                _check_copies_identical([dict(idx=o_r["idx"], z=o_r["z"][k]) for o_r in out], "z", d.n_dofs)
            # the layout query: every row of a sharded level is owned once, ghosts travel
            for l, lv0 in enumerate(out[0]["layout"]):
                if not lv0["replicated"]:
                    assert sum(o_r["layout"][l]["owned_rows"] for o_r in out) == lv0["global_rows"]
                    assert all(o_r["layout"][l]["ghosts"] > 0 and o_r["layout"][l]["peers"] > 0 for o_r in out)
            if geo == "quadrant" and min_rows == 0:
                assert sum(not lv["replicated"] for lv in out[0]["layout"]) >= 2  # three AMG levels, two of them sharded


@pytest.mark.parametrize("degree", [1, 3])
def test_sharded_amg_smoother_degrees(mgamd, one_rank, degree):
    """MGAMD_AMG_SMOOTHER_DEGREE 1 and 3 (odd: the zero-start smoother begins in the other buffer): fresh ghosts before every
    Chebyshev product"""
    geo, L, n_ranks = "quadrant", 6, 3
    d, kf, o, _ = one_rank(geo, L)
    od = copy.copy(o)
    od.degree = degree
    rhs = _rhs_pair(d, 6)
    os.environ["MGAMD_AMG_SMOOTHER_DEGREE"] = str(degree)  # read when the cycle is built
    try:
        group = mgamd.SimGroup(n_ranks)
        out = run_ranks(n_ranks, lambda rk: _sharded_one_level(mgamd, group, rk, geo, L, 1, 0, kf, rhs))
    finally:
        del os.environ["MGAMD_AMG_SMOOTHER_DEGREE"]
    for o_r in out:
        for k in range(2):
            err = rel_err(o_r["z"][k], od.apply(rhs[k], 1)[o_r["idx"]])
            print(f"degree={degree} constrained rhs={bool(k)}: rel. error {err:.2e}")
            assert err <= TOL_CYCLE, (degree, k, err)


def test_sharded_amg_without_halo_overlap(mgamd, one_rank, monkeypatch):
    """MGAMD_NO_HALO_OVERLAP=1: import, then ONE launch over all rows -- the same numbers"""
    geo, L, n_ranks = "quadrant", 6, 4
    d, kf, o, _ = one_rank(geo, L)
    rhs = _rhs_pair(d, 7)
    monkeypatch.setenv("MGAMD_NO_HALO_OVERLAP", "1")
    group = mgamd.SimGroup(n_ranks)
    out = run_ranks(n_ranks, lambda rk: _sharded_one_level(mgamd, group, rk, geo, L, 2, 0, kf, rhs))
    for o_r in out:
        for k in range(2):
            assert rel_err(o_r["z"][k], o.apply(rhs[k], 2)[o_r["idx"]]) <= TOL_CYCLE


def test_one_rank_communicator_equals_unsharded_amg(mgamd, ctx, one_rank):
    geo, L = "quadrant", 6
    d, kf, o, _ = one_rank(geo, L)
    rhs = _rhs_pair(d, 8)
    h1 = mgamd.Hierarchy(ctx, geo, L, 1, "PMG", coarse_solver="amg", coarse_n_cycles=2, max_brick=0)
    group = mgamd.SimGroup(1)
    (o_r,) = run_ranks(1, lambda rk: _sharded_one_level(mgamd, group, rk, geo, L, 2, 0, kf, rhs))
    assert o_r["used"] == "amg" and all(lv["replicated"] and lv["ghosts"] == 0 for lv in o_r["layout"])
    for k in range(2):
        assert rel_err(o_r["z"][k], _apply(mgamd, ctx, h1.mg, rhs[k])[o_r["idx"]]) <= 1e-13


def test_default_is_still_the_geometric_stand_in(mgamd, one_rank):
    geo, L, n_ranks = "annulus", 6, 2
    d, kf, o, _ = one_rank(geo, L)
    rhs = _rhs_pair(d, 9)
    group = mgamd.SimGroup(n_ranks)
    out = run_ranks(n_ranks, lambda rk: _sharded_one_level(mgamd, group, rk, geo, L, 1, 0, kf, rhs, sharded_amg=False))
    assert all(o_r["used"] == "gmg_vcycle" for o_r in out)


def test_sharded_amg_float(mgamd, one_rank):
    geo, L, n_ranks = "quadrant", 6, 2
    d, kf, o, _ = one_rank(geo, L)
    rhs = _rhs_pair(d, 10)
    group = mgamd.SimGroup(n_ranks)
    out = run_ranks(n_ranks, lambda rk: _sharded_one_level(mgamd, group, rk, geo, L, 2, 0, kf, rhs, number_type=mgamd.F32))
    for o_r in out:
        for k in range(2):
            err = rel_err(o_r["z"][k], o.apply(rhs[k], 2)[o_r["idx"]])
            print(f"FP32 constrained rhs={bool(k)}: rel. error {err:.2e}")
            assert err <= TOL_F32


def test_cg_with_amg_on_two_ranks_equals_one_rank(mgamd, ctx, one_rank):
    """the distributed coarse CG preconditioned by the sharded cycle: as many iterations as on one rank, the same solution"""
    geo, L, n_ranks = "annulus", 7, 2
    d, kf, o, _ = one_rank(geo, L)
    b = d.rhs_constant()
    h1 = mgamd.Hierarchy(ctx, geo, L, 1, "PMG", coarse_solver="cg_with_amg", max_brick=0)
    x1 = _apply(mgamd, ctx, h1.mg, b)
    it1 = h1.mg.coarse_iterations()
    group = mgamd.SimGroup(n_ranks)
    out = run_ranks(n_ranks, lambda rk: _sharded_one_level(mgamd, group, rk, geo, L, 1, 0, kf, [b], coarse="cg_with_amg"))
    assert it1 > 0
    for o_r in out:
        assert o_r["used"] == "cg_with_amg" and o_r["its"] == it1
        assert rel_err(o_r["z"][0], x1[o_r["idx"]]) <= TOL_SOL


# ------------------------------------------------------------------ whole PMG hierarchies
@pytest.fixture(scope="module")
def pmg_oracles(mgamd, oracle):
    """oracle PMG hierarchy on annulus L=6 with the restated AMG x 2 as coarse solver, built once per degree"""
    cache = {}

    def get(p):
        if p not in cache:
            levels, P = oracle.build_hierarchy("annulus", 6, p, "PMG")
            d0 = mgamd.DoFs(mgamd.Triangulation("annulus", 6), 1, 0)
            # the restated AMG acts on the product's global numbering of the p = 1 space: permute through the keys
            k0 = {k: i for i, k in enumerate(keyset(levels[0].keys))}
            perm = np.array([k0[k] for k in keyset(d0.keys())])  # product row -> oracle row
            amg = ao.SmoothedAggregation(d0.matrix()).precondition(2)

            def coarse(r):
                z = np.empty_like(r)
                z[perm] = amg(r[perm])
                return z

            mg = oracle.Multigrid(levels, P, 3, coarse=coarse, start_vectors=[oracle.key_hash_start_vector(lv) for lv in levels])
            Lf = levels[-1]
            cache[p] = (Lf, mg, oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4))
        return cache[p]

    return get


def _pmg_rank(mgamd, group, rk, p, kf, r, number_type=None):
    ctx = mgamd.Context(0)
    kw = {} if number_type is None else dict(number_type=number_type)
    h = mgamd.DistributedHierarchy(ctx, group.comm(rk), "annulus", 6, p, coarse_solver="amg", max_brick=0, min_root_dofs=0, mg_type="PMG",
                                   coarse_n_cycles=2, sharded_amg=True, amg_min_sharded_rows=0, **kw)
    idx = np.array([kf[k] for k in keyset(h.dofs[-1].keys())])
    op = h.fine_operator
    vr, vz = op.initialize_dof_vector().from_host(r[idx]), op.initialize_dof_vector()
    h.mg.vmult(vz, vr)
    b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
    op.rhs(b)
    it, _ = mgamd.solve_cg(op, h.mg, x, b, 1e-4)
    return dict(idx=idx, z=vz.to_host(), x=x.to_host(), it=it, used=h.mg.coarse_solver_used(), dist=list(h.distributed))


@pytest.mark.parametrize("n_ranks", [2, 4])
@pytest.mark.parametrize("p", [2, 4])
def test_sharded_pmg_with_amg_equals_oracle(mgamd, pmg_oracles, p, n_ranks):
    """annulus L=6 PMG p -> ... -> 1 with "amg" x 2 on the sharded p = 1 level (BASELINE configs[4]'s coarse solver at test size)
    against the oracle's Multigrid with the restated AMG: V-cycle, outer CG count, solution"""
    Lf, mg, (xref, itref, _) = pmg_oracles(p)
    kf = {k: i for i, k in enumerate(keyset(Lf.keys))}
    r = np.random.default_rng(p).standard_normal(Lf.n)
    r[Lf.constrained] = 0.0
    zref = mg.vcycle(r)
    group = mgamd.SimGroup(n_ranks)
    out = run_ranks(n_ranks, lambda rk: _pmg_rank(mgamd, group, rk, p, kf, r))
    for o in out:
        e_v, e_x = rel_err(o["z"], zref[o["idx"]]), rel_err(o["x"], xref[o["idx"]])
        print(f"PMG p={p} ranks={n_ranks}: V-cycle {e_v:.2e}, CG iterations {o['it']} (oracle {itref}), solution {e_x:.2e}")
        assert o["used"] == "amg" and all(o["dist"])
        assert e_v <= TOL_CYCLE and o["it"] == itref and e_x <= TOL_SOL, (e_v, o["it"], itref, e_x)
    _check_copies_identical(out, "x", Lf.n)


def test_sharded_pmg_with_amg_float(mgamd, pmg_oracles):
    """FP32 levels once: test_gpu_amg.py's bounds for them (V-cycle <= TOL_F32, outer CG within one iteration)"""
    p, n_ranks = 2, 2
    Lf, mg, (xref, itref, _) = pmg_oracles(p)
    kf = {k: i for i, k in enumerate(keyset(Lf.keys))}
    r = np.random.default_rng(p).standard_normal(Lf.n)
    r[Lf.constrained] = 0.0
    zref = mg.vcycle(r)
    group = mgamd.SimGroup(n_ranks)
    out = run_ranks(n_ranks, lambda rk: _pmg_rank(mgamd, group, rk, p, kf, r, mgamd.F32))
    for o in out:
        assert o["used"] == "amg"
        assert rel_err(o["z"], zref[o["idx"]]) <= TOL_F32
        assert abs(o["it"] - itref) <= 1, (o["it"], itref)


def test_sharded_amg_error_paths(mgamd, ctx):
    """asked for on something it cannot run on: a clear error, never a silent substitution"""
    d = mgamd.DoFs(mgamd.Triangulation("annulus", 6), 1, 0)
    op = mgamd.Operator(ctx, d)
    sm = mgamd.PreconditionChebyshev(op, 3, 20.0, 20)
    with pytest.raises(mgamd.MgamdError, match="AMG coarse solvers"):
        mgamd.PreconditionMG(ctx, [op], [None], [sm], "cg", sharded_amg=d)
    d2 = mgamd.DoFs(mgamd.Triangulation("annulus", 6), 2, 0)
    with pytest.raises(mgamd.MgamdError, match="degree"):
        mgamd.PreconditionMG(ctx, [op], [None], [sm], "amg", sharded_amg=d2)
