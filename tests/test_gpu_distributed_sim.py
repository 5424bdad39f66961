"""Sharded path on ONE GPU: n ranks run as host threads over the in-process simulator communicator (device-to-device
copies instead of RCCL send/recv); everything else -- partition, local numbering, halo plans, pack/combine kernels,
distributed transfer, all-reduce onto the replicated levels, global dots -- is the production code.  Results are
compared with the single-rank solve (CG iterates within the FP64 tolerance, iteration counts equal)."""
import os
import threading

import numpy as np
import pytest

from conftest import rel_err
from support import key_vector, keyset, run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def key_based_chebyshev_start_vector():
    # the sharded path has no global DoF index: its Chebyshev start vector hashes the geometric DoF key; use the same
    # start vector for the single-rank reference (and the replicated levels) so that the comparison is arithmetic-exact
    os.environ["MGAMD_CHEB_KEY_INIT"] = "1"
    yield
    del os.environ["MGAMD_CHEB_KEY_INIT"]


# (geometry, NRefGlobal, degree, Type, coarse solver, ranks): vs the INDEPENDENT numpy oracle through the DoF keys
ORACLE_CASES = [("quadrant", 5, 1, "HMG-global", "amg", 2), ("quadrant", 4, 4, "HMG-global", "amg", 2), ("quadrant", 5, 2, "HMG-global", "amg", 3),
                ("annulus", 6, 1, "HMG-global", "amg", 4), ("hypercube", 4, 2, "HMG-global", "amg", 2),
                ("annulus", 5, 4, "PMG", "cg_with_chebyshev", 2),  # BASELINE.json configs[4] at test size
                ("quadrant", 4, 4, "PMG", "cg", 3), ("annulus", 5, 2, "HPMG", "amg", 3),
                ("annulus", 6, 2, "PMG", "amg", 2)]  # AMG on a 9,763-DoF coarse level: sharded geometric stand-in = HPMG


@pytest.mark.parametrize("geo,L,p,mg_type,coarse,n_ranks", ORACLE_CASES)
def test_sharded_hierarchy_matches_numpy_oracle(mgamd, oracle, geo, L, p, mg_type, coarse, n_ranks):
    """operator, V-cycle and preconditioned solve of the SHARDED hierarchy (partition, local numbering, halo exchange,
    rank-local transfers, all-reduce onto replicated levels, distributed coarse CG, global dots) against the independent
    numpy oracle, matched through the geometric DoF keys; copies of shared DoFs identical on all sharers."""
    stand_in = mg_type == "PMG" and coarse == "amg"
    levels, P = oracle.build_hierarchy(geo, L, p, "HPMG" if stand_in else mg_type)
    omg = oracle.Multigrid(levels, P, 3, coarse="direct" if coarse == "amg" else coarse,
                           start_vectors=[oracle.key_hash_start_vector(lv) for lv in levels])
    Lf = levels[-1]
    kf = {tuple(int(v) for v in k): i for i, k in enumerate(Lf.keys)}
    u = key_vector(Lf.keys, 1)
    r = key_vector(Lf.keys, 2)
    r[Lf.constrained] = 0.0
    Au, zref = Lf.A @ u, omg.vcycle(r)
    xref, itref, hist = oracle.pcg(Lf.A, Lf.rhs_constant, omg.vcycle, 1e-4)
    group = mgamd.SimGroup(n_ranks)

    def rank_main(rk):
        ctx = mgamd.Context(0)
        h = mgamd.DistributedHierarchy(ctx, group.comm(rk), geo, L, p, coarse_solver=coarse, max_brick=0, min_root_dofs=0, mg_type=mg_type)
        keys = keyset(h.dofs[-1].keys())
        idx = np.array([kf[k] for k in keys])
        op = h.fine_operator
        vu, vA = op.initialize_dof_vector().from_host(u[idx]), op.initialize_dof_vector()
        op.vmult(vA, vu)
        vr, vz = op.initialize_dof_vector().from_host(r[idx]), op.initialize_dof_vector()
        h.mg.vmult(vz, vr)
        b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
        op.rhs(b)
        it, res = mgamd.solve_cg(op, h.mg, x, b, 1e-4)
        return dict(idx=idx, Au=vA.to_host(), z=vz.to_host(), x=x.to_host(), b=b.to_host(), it=it, res=res, n_dofs=h.n_dofs,
                    dist=list(h.distributed), used=h.mg.coarse_solver_used(), peers=h.dofs[-1].info.n_peers)

    out = run_ranks(n_ranks, rank_main)
    tol_v, tol_x = (1e-11, 1e-10) if coarse == "amg" else (1e-4, 1e-5)  # an inner CG stops on a tolerance
    for o in out:
        assert o["n_dofs"] == Lf.n and o["peers"] >= 1 and o["dist"][-1]
        assert o["used"] == ("gmg_vcycle" if stand_in else ("direct" if coarse == "amg" else coarse))
        assert rel_err(o["Au"], Au[o["idx"]]) < 1e-13
        assert np.abs(o["b"] - Lf.rhs_constant[o["idx"]]).max() < 1e-14
        assert rel_err(o["z"], zref[o["idx"]]) < tol_v
        assert o["it"] == itref
        assert rel_err(o["x"], xref[o["idx"]]) < tol_x
    if mg_type == "PMG":
        assert all(out[0]["dist"])  # the p-levels live on the finest mesh: all distributed
    if mg_type == "HPMG":
        assert out[0]["dist"][-2] and not out[0]["dist"][0]
    # copies of shared DoFs agree across ranks (bitwise: ascending-rank combination order)
    seen = {}
    for o in out:
        for i, v in zip(o["idx"], o["x"]):
            if i in seen:
                assert seen[i] == v
            seen[i] = v
    assert len(seen) == Lf.n


def test_eight_ranks_balanced_and_consistent(mgamd):
    """octant L=6 p=4 (2.3 M DoFs) on 8 simulated ranks: weights (hanging-node cells x 2, CellWeightPolicy-2.0) balanced to
    10 %, result equal to the single-rank solve."""
    geo, L, p, n_ranks = "quadrant", 6, 4, 8
    ctx0 = mgamd.Context(0)
    h0 = mgamd.Hierarchy(ctx0, geo, L, p, "HMG-global", coarse_solver="amg", max_brick=0)
    b0, x0 = h0.fine_operator.initialize_dof_vector(), h0.fine_operator.initialize_dof_vector()
    h0.fine_operator.rhs(b0)
    it0, res0 = mgamd.solve_cg(h0.fine_operator, h0.mg, x0, b0, 1e-4)
    ref = dict(zip(keyset(h0.dofs[-1].keys()), x0.to_host()))
    trias = h0.trias
    part = mgamd.Partition(trias, n_ranks, 2.0, 0)
    owner = part.owner(len(trias) - 1)
    _, _, _, _, mask = trias[-1].cells()
    w = np.where((mask >> 3) != 0, 2.0, 1.0)
    load = np.array([w[owner == rk].sum() for rk in range(n_ranks)])
    assert load.max() / load.mean() < 1.10
    group = mgamd.SimGroup(n_ranks)

    def rank_main(rk):
        ctx = mgamd.Context(0)
        h = mgamd.DistributedHierarchy(ctx, group.comm(rk), geo, L, p, coarse_solver="amg", max_brick=0, min_root_dofs=0)
        b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
        h.fine_operator.rhs(b)
        it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
        return dict(it=it, keys=keyset(h.dofs[-1].keys()), x=x.to_host(), n_dofs=h.n_dofs, peers=h.dofs[-1].info.n_peers)

    out = run_ranks(n_ranks, rank_main)
    for o in out:
        assert o["n_dofs"] == h0.n_dofs and o["it"] == it0 and 1 <= o["peers"] <= 7
        assert rel_err(o["x"], np.array([ref[k] for k in o["keys"]])) < 1e-10


@pytest.mark.parametrize("geo,L,p,n_ranks", [("quadrant", 5, 1, 2), ("quadrant", 4, 4, 2), ("quadrant", 5, 2, 3), ("annulus", 6, 1, 4),
                                             ("hypercube", 4, 2, 2), ("quadrant", 5, 4, 4)])
def test_sharded_solve_matches_single_rank(mgamd, geo, L, p, n_ranks):
    # single-rank reference on the same GPU, with the numbering-independent Chebyshev start vector of the sharded path
    ctx0 = mgamd.Context(0)
    h0 = mgamd.Hierarchy(ctx0, geo, L, p, "HMG-global", coarse_solver="amg", max_brick=0)
    b0, x0 = h0.fine_operator.initialize_dof_vector(), h0.fine_operator.initialize_dof_vector()
    h0.fine_operator.rhs(b0)
    it0, res0 = mgamd.solve_cg(h0.fine_operator, h0.mg, x0, b0, 1e-4)
    ref = dict(zip(keyset(h0.dofs[-1].keys()), x0.to_host()))
    rng = np.random.default_rng(31)
    u0 = rng.standard_normal(h0.n_dofs)
    vu, vAu = h0.fine_operator.initialize_dof_vector().from_host(u0), h0.fine_operator.initialize_dof_vector()
    h0.fine_operator.vmult(vAu, vu)
    uref, Auref = dict(zip(keyset(h0.dofs[-1].keys()), u0)), dict(zip(keyset(h0.dofs[-1].keys()), vAu.to_host()))

    group = mgamd.SimGroup(n_ranks)

    def rank_main(r):
        ctx = mgamd.Context(0)
        comm = group.comm(r)
        h = mgamd.DistributedHierarchy(ctx, comm, geo, L, p, coarse_solver="amg", max_brick=0, min_root_dofs=0)
        keys = keyset(h.dofs[-1].keys())
        # operator application on consistent copies of a global vector
        u = h.fine_operator.initialize_dof_vector().from_host(np.array([uref[k] for k in keys]))
        Au = h.fine_operator.initialize_dof_vector()
        h.fine_operator.vmult(Au, u)
        err_A = max(abs(a - Auref[k]) for a, k in zip(Au.to_host(), keys)) / max(abs(v) for v in Auref.values())
        b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
        h.fine_operator.rhs(b)
        it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
        info = h.dofs[-1].info
        return dict(it=it, res=res, keys=keys, x=x.to_host(), n_dofs=h.n_dofs, err_A=err_A, root=h.partition.root_level, peers=info.n_peers,
                    send=info.n_halo_send, n_local=h.n_local)

    out = run_ranks(n_ranks, rank_main)
    assert all(o["n_dofs"] == h0.n_dofs for o in out)  # every DoF owned exactly once
    assert all(o["peers"] >= 1 and o["send"] > 0 for o in out)
    assert sum(o["n_local"] for o in out) > h0.n_dofs  # shared copies exist
    for o in out:
        assert o["err_A"] < 1e-13
        assert o["it"] == it0
        assert o["res"] == pytest.approx(res0, rel=1e-7)
        xr = np.array([ref[k] for k in o["keys"]])
        assert rel_err(o["x"], xr) < 1e-10
    # copies of shared DoFs agree across ranks
    seen = {}
    for o in out:
        for k, v in zip(o["keys"], o["x"]):
            if k in seen:
                assert abs(seen[k] - v) <= 1e-12 * max(1.0, abs(v))
            seen[k] = v
    assert len(seen) == h0.n_dofs


@pytest.mark.parametrize("geo,L,p,mg_type,n_ranks,group", [("quadrant", 5, 2, "HMG-global", 8, 4), ("quadrant", 6, 1, "HMG-global", 8, 2),
                                                           ("annulus", 6, 1, "HMG-global", 4, 2), ("quadrant", 4, 4, "HPMG", 4, 2)])
def test_two_tier_hierarchy_matches_numpy_oracle(mgamd, oracle, geo, L, p, mg_type, n_ranks, group):
    """Partition tiers (round 3): the finest levels cut into n_ranks chunks, the levels below into n_ranks / group parts that a group
    of ranks holds together (SubsetComm: halo exchange between parts, sums over the parts, group sum after the restriction from the
    finer tier), the rest replicated -- V-cycle, solve and iteration count against the independent numpy oracle."""
    levels, P = oracle.build_hierarchy(geo, L, p, mg_type)
    omg = oracle.Multigrid(levels, P, 3, coarse="direct", start_vectors=[oracle.key_hash_start_vector(lv) for lv in levels])
    Lf = levels[-1]
    kf = {tuple(int(v) for v in k): i for i, k in enumerate(Lf.keys)}
    r = key_vector(Lf.keys, 2)
    r[Lf.constrained] = 0.0
    zref = omg.vcycle(r)
    xref, itref, hist = oracle.pcg(Lf.A, Lf.rhs_constant, omg.vcycle, 1e-4)
    sim = mgamd.SimGroup(n_ranks)
    # tiers by size: the two finest meshes on all ranks, the two below them on the parts
    seq = mgamd.create_geometric_coarsening_sequence(mgamd.Triangulation(geo, L))
    n_cells = [t.n_cells for t in seq]
    p_low = min(lv.p for lv in levels)

    def rank_main(rk):
        ctx = mgamd.Context(0)
        h = mgamd.DistributedHierarchy(ctx, sim.comm(rk), geo, L, p, coarse_solver="amg", max_brick=0, mg_type=mg_type, subset_group=group,
                                       min_root_dofs=n_cells[-2] * p_low ** 3, min_subset_dofs=n_cells[-4] * p_low ** 3)
        keys = keyset(h.dofs[-1].keys())
        idx = np.array([kf[k] for k in keys])
        op = h.fine_operator
        vr, vz = op.initialize_dof_vector().from_host(r[idx]), op.initialize_dof_vector()
        h.mg.vmult(vz, vr)
        b, x = op.initialize_dof_vector(), op.initialize_dof_vector()
        op.rhs(b)
        it, res = mgamd.solve_cg(op, h.mg, x, b, 1e-4)
        return dict(idx=idx, z=vz.to_host(), x=x.to_host(), it=it, n_dofs=h.n_dofs, layout=h.layout(), level_dofs=h.global_level_dofs(ctx),
                    group=h.partition.group)

    out = run_ranks(n_ranks, rank_main)
    for o in out:
        assert o["group"] == group and n_ranks // group in o["layout"] and o["layout"][0] == 1 and o["layout"][-1] == n_ranks
        assert o["level_dofs"] == [lv.n for lv in levels]  # every DoF of every level owned exactly once
        assert rel_err(o["z"], zref[o["idx"]]) < 1e-11
        assert o["it"] == itref
        assert rel_err(o["x"], xref[o["idx"]]) < 1e-10
