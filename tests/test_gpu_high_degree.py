"""FE degrees 5, 6 and 7 on the device: every path that degrees 1-4 have, against the numpy oracle built at run time.

The largest brick at these degrees is 2^3 cells (11-, 13- and 15-point lattices), so a level runs the 2^3-brick + single-cell
launch, the 2^3-brick kernel, the wave-scoped single cells, the diagonal kernel and the tail kernel; the transfers add the
h-patches (p, 2p + 1) = 511 / 613 / 715, the p-patches 206 and 308 of the bisection sequences 5->2->1, 6->3->1, 7->3->1 and
the 2^3 brick transfers.  Tolerances are those of test_gpu_parity.py (FP64 rounding level, equal CG iteration counts), of
test_float_levels_mixed_precision for the FP32 levels and of test_gpu_distributed_sim.py for the sharded path.

Meshes: quadrant NRefGlobal 2 (hanging faces and edges, Dirichlet boundary: 2530 / 4171 / 6400 DoFs) and hypercube
NRefGlobal 2 (64 cells = eight 2^3 bricks sharing faces, edges and one vertex) are the smallest on which every slot kind,
the constrained-family path and brick-to-brick shell accumulation occur."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from conftest import ROOT, oracle_level, rel_err

pytestmark = pytest.mark.gpu

TOL_OP = 1e-13
TOL_CHEB = 1e-12
TOL_VCYCLE = 1e-11
TOL_SOL = 1e-10

DEGREES = [5, 6, 7]
N_DOFS_QUADRANT_2 = {5: 2530, 6: 4171, 7: 6400}
# max_brick 0: 2^3 bricks + single cells in one launch;  max_brick 1: single cells only (the wave-scoped kernel)
OP_CASES = [(geo, 2, p, mb) for p in DEGREES for geo in ("quadrant", "hypercube") for mb in (0, 1)]


class RenumberedLevel:
    """an oracle level in the numbering of another DoF handler of the same space (matched through the geometric DoF keys)"""

    def __init__(self, lv, keys):
        pos = {tuple(int(v) for v in k): i for i, k in enumerate(lv.keys)}
        perm = np.array([pos[tuple(int(v) for v in k)] for k in keys])
        assert len(perm) == lv.n and len(set(perm.tolist())) == lv.n
        self.n, self.A, self.inv_diag = lv.n, lv.A[perm][:, perm], lv.inv_diag[perm]


@pytest.fixture(scope="module")
def levels(mgamd, oracle, ctx):
    """(DoFs, Operator, oracle level); the oracle level of a (mesh, degree) is assembled once and renumbered for the second
    slot policy"""
    cache, meshes, assembled = {}, {}, {}

    def get(geo, L, p, max_brick):
        key = (geo, L, p, max_brick)
        if key not in cache:
            if (geo, L) not in meshes:
                meshes[(geo, L)] = oracle.create_mesh(geo, L)
            t = mgamd.Triangulation(geo, L)
            d = mgamd.DoFs(t, p, max_brick)
            if (geo, L, p) not in assembled:
                assembled[(geo, L, p)] = oracle_level(oracle, d, geo, L, p, mesh=meshes[(geo, L)])
                lv = assembled[(geo, L, p)]
            else:
                lv = RenumberedLevel(assembled[(geo, L, p)], d.keys())
            cache[key] = (d, mgamd.Operator(ctx, d), lv)
        return cache[key]

    return get


@pytest.mark.parametrize("geo,L,p,max_brick", OP_CASES)
def test_vmult(mgamd, ctx, levels, geo, L, p, max_brick):
    d, op, lv = levels(geo, L, p, max_brick)
    assert op.m() == lv.n
    if geo == "quadrant":
        assert lv.n == N_DOFS_QUADRANT_2[p]
    sizes = {B for B, n in d.groups() if n}
    assert sizes == ({1} if max_brick == 1 else ({1, 2} if geo == "quadrant" else {2}))
    rng = np.random.default_rng(3)
    for trial in range(2):  # (twice: the tail accumulator must be clean after a pass)
        x = rng.standard_normal(lv.n)
        src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector()
        dst.set(7.0)  # vmult must overwrite
        op.vmult(dst, src)
        err = rel_err(dst.to_host(), lv.A @ x)
        print(f"vmult {geo} L={L} p={p} max_brick={max_brick}: rel.err {err:.2e}")
        assert err < TOL_OP
        assert np.array_equal(src.to_host(), x)  # src untouched


@pytest.mark.parametrize("geo,L,p,max_brick", OP_CASES)
def test_inverse_diagonal(mgamd, ctx, levels, geo, L, p, max_brick):
    d, op, lv = levels(geo, L, p, max_brick)
    diag = op.initialize_dof_vector()
    op.compute_inverse_diagonal(diag)
    err = rel_err(diag.to_host(), lv.inv_diag)
    print(f"inverse diagonal {geo} L={L} p={p} max_brick={max_brick}: rel.err {err:.2e}")
    assert err < TOL_OP


@pytest.mark.parametrize("p", DEGREES)
@pytest.mark.parametrize("max_brick", [0, 1])
@pytest.mark.parametrize("degree", [1, 3])
def test_chebyshev(mgamd, oracle, ctx, levels, p, max_brick, degree):
    """vmult (zero start: the first two passes form c0 dinv b on the fly) and step: with the operator's vmult and the
    residual of the V-cycle tests these are all five operator modes"""
    d, op, lv = levels("quadrant", 2, p, max_brick)
    ch = mgamd.PreconditionChebyshev(op, degree, 20.0, 20)
    ref = oracle.Chebyshev(lv.A, lv.inv_diag, degree, 20.0, 20)
    lo, hi = ch.eigenvalue_estimates()
    assert hi == pytest.approx(ref.max_ev, rel=1e-10)
    rng = np.random.default_rng(5)
    b, x0 = rng.standard_normal(lv.n), rng.standard_normal(lv.n)
    vb, vx = op.initialize_dof_vector().from_host(b), op.initialize_dof_vector()
    ch.vmult(vx, vb)
    e1 = rel_err(vx.to_host(), ref.vmult(b))
    vx.from_host(x0)
    ch.step(vx, vb)
    e2 = rel_err(vx.to_host(), ref.step(x0, b))
    print(f"chebyshev p={p} max_brick={max_brick} degree={degree}: vmult {e1:.2e} step {e2:.2e}")
    assert e1 < TOL_CHEB and e2 < TOL_CHEB


# p = 5 on quadrant NRefGlobal 3, p = 6 and 7 on NRefGlobal 2 (the numpy oracle needs 3-13 s per solve at NRefGlobal 3 there)
HIER_CASES = [("quadrant", 3 if p == 5 else 2, p, t) for p in DEGREES for t in ("HMG-global", "PMG", "HPMG")]


@pytest.fixture(scope="module")
def hierarchies(mgamd, oracle, ctx):
    cache = {}

    def get(geo, L, p, mg_type):
        key = (geo, L, p, mg_type)
        if key not in cache:
            h = mgamd.Hierarchy(ctx, geo, L, p, mg_type, coarse_solver="amg", max_brick=0)
            lv, P = oracle.build_hierarchy(geo, L, p, mg_type, numbering_keys=[d.keys() for d in h.dofs])
            cache[key] = (h, lv, P)
        return cache[key]

    return get


@pytest.fixture(scope="module")
def oracle_solves(oracle, hierarchies):
    """the oracle's multigrid and preconditioned solve of a hierarchy, computed once"""
    cache = {}

    def get(geo, L, p, mg_type):
        key = (geo, L, p, mg_type)
        if key not in cache:
            h, lv, P = hierarchies(geo, L, p, mg_type)
            mg = oracle.Multigrid(lv, P, 3, coarse="direct")
            cache[key] = (mg,) + tuple(oracle.pcg(lv[-1].A, lv[-1].rhs_constant, mg.vcycle, 1e-4))
        return cache[key]

    return get


@pytest.mark.parametrize("geo,L,p,mg_type", HIER_CASES)
def test_transfer(mgamd, ctx, hierarchies, geo, L, p, mg_type):
    h, lv, P = hierarchies(geo, L, p, mg_type)
    if mg_type != "HMG-global":
        assert [l.p for l in lv][-3:] == {5: [1, 2, 5], 6: [1, 3, 6], 7: [1, 3, 7]}[p]
    rng = np.random.default_rng(6)
    for l in range(1, len(lv)):
        xc, xf0 = rng.standard_normal(lv[l - 1].n), rng.standard_normal(lv[l].n)
        vc, vf = h.operators[l - 1].initialize_dof_vector().from_host(xc), h.operators[l].initialize_dof_vector().from_host(xf0)
        h.transfers[l].prolongate_and_add(vf, vc)
        e1 = rel_err(vf.to_host(), xf0 + P[l] @ xc)
        rf, dc0 = rng.standard_normal(lv[l].n), rng.standard_normal(lv[l - 1].n)
        vr, vd = h.operators[l].initialize_dof_vector().from_host(rf), h.operators[l - 1].initialize_dof_vector().from_host(dc0)
        h.transfers[l].restrict_and_add(vd, vr)
        e2 = rel_err(vd.to_host(), dc0 + P[l].T @ rf)
        print(f"transfer {geo} L={L} p={p} {mg_type} level {l} (p {lv[l - 1].p} -> {lv[l].p}): prolongate {e1:.2e} restrict {e2:.2e}")
        assert e1 < TOL_OP and e2 < TOL_OP


@pytest.mark.parametrize("geo,L,p,mg_type", HIER_CASES)
def test_vcycle(mgamd, oracle, ctx, hierarchies, oracle_solves, geo, L, p, mg_type):
    h, lv, P = hierarchies(geo, L, p, mg_type)
    mg = oracle_solves(geo, L, p, mg_type)[0]
    for l, s in enumerate(h.smoothers):
        assert s.eigenvalue_estimates()[1] == pytest.approx(mg.sm[l].max_ev, rel=1e-9)
    r = np.random.default_rng(7).standard_normal(lv[-1].n)
    vr, vz = mgamd.Vector(ctx, lv[-1].n).from_host(r), mgamd.Vector(ctx, lv[-1].n)
    h.mg.vmult(vz, vr)
    ref = mg.vcycle(r)
    err = rel_err(vz.to_host(), ref)
    print(f"V-cycle {geo} L={L} p={p} {mg_type}: rel.err {err:.2e}")
    assert err < TOL_VCYCLE
    # graph replay gives the same vector
    ms = h.mg.time_vcycles(vz, vr, 2, True)
    assert ms > 0 and rel_err(vz.to_host(), ref) < TOL_VCYCLE


@pytest.mark.parametrize("geo,L,p,mg_type", HIER_CASES)
def test_cg_solve_iteration_counts_and_solution(mgamd, oracle, ctx, hierarchies, oracle_solves, geo, L, p, mg_type):
    h, lv, P = hierarchies(geo, L, p, mg_type)
    mg, xref, itref, hist = oracle_solves(geo, L, p, mg_type)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    err = rel_err(x.to_host(), xref)
    print(f"CG {geo} L={L} p={p} {mg_type}: iterations gpu {it} oracle {itref}, rel.err {err:.2e}")
    assert it == itref
    assert res == pytest.approx(hist[-1], rel=1e-6)
    assert err < TOL_SOL


@pytest.mark.parametrize("mg_type", ["HMG-global", "PMG"])
def test_float_levels_mixed_precision(mgamd, oracle, ctx, mg_type):
    """MGNumberType float at p = 6: FP32 V-cycle under the FP64 outer CG (bounds of test_gpu_parity.py's test of that name)"""
    geo, L, p = "quadrant", 2, 6
    h = mgamd.Hierarchy(ctx, geo, L, p, mg_type, coarse_solver="amg", number_type=mgamd.F32, max_brick=0)
    lv, P = oracle.build_hierarchy(geo, L, p, mg_type, numbering_keys=[d.keys() for d in h.dofs])
    rng = np.random.default_rng(21)
    for l, op in enumerate(h.operators):
        x = rng.standard_normal(lv[l].n)
        src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector()
        op.vmult(dst, src)
        assert rel_err(dst.to_host(), lv[l].A @ x) < 2e-6
        if l > 0:
            xc = rng.standard_normal(lv[l - 1].n)
            vc, vf = h.operators[l - 1].initialize_dof_vector().from_host(xc), h.operators[l].initialize_dof_vector()
            h.transfers[l].prolongate_and_add(vf, vc)
            assert rel_err(vf.to_host(), P[l] @ xc) < 2e-6
    mg = oracle.Multigrid(lv, P, 3)
    r = rng.standard_normal(lv[-1].n)
    vr, vz = mgamd.Vector(ctx, lv[-1].n).from_host(r), mgamd.Vector(ctx, lv[-1].n)
    vz.from_host(np.full(lv[-1].n, np.nan))  # an entry of z that the cycle does not store stays NaN
    h.mg.vmult(vz, vr)  # double in, float V-cycle, double out
    z = vz.to_host()
    assert np.isfinite(z).all()
    assert rel_err(z, mg.vcycle(r)) < 5e-5
    Lf = lv[-1]
    xref, itref, hist = oracle.pcg(Lf.A, Lf.rhs_constant, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    assert abs(it - itref) <= 1
    assert rel_err(x.to_host(), xref) < 1e-3


def test_local_smoothing(mgamd, ctx):
    """`HMG-local` at p = 5 on the smallest mesh of test_gpu_local_smoothing.py: level operators with refinement-edge DoFs, edge
    matrices, transfers between refinement levels, V-cycle and solve against the textbook oracle (ls_oracle)"""
    import ls_oracle

    geo, L, p = "quadrant", 3, 5
    h = mgamd.Hierarchy(ctx, geo, L, p, "HMG-local", coarse_solver="amg", max_brick=0)
    ref = ls_oracle.LocalSmoothing(geo, L, p, numbering_keys_global=h.active_dofs.keys(), numbering_keys_levels=[d.keys() for d in h.dofs])
    rng = np.random.default_rng(41)
    assert len(h.operators) == len(ref.levels)
    for l, (op, Lv) in enumerate(zip(h.operators, ref.levels)):
        info = h.dofs[l].info
        assert h.dofs[l].n_dofs == Lv.n and info.n_edge == Lv.edge.sum() and info.n_hanging == 0
        x = rng.standard_normal(Lv.n)
        src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector()
        op.vmult(dst, src)
        assert rel_err(dst.to_host(), Lv.A @ x) < 1e-13
        diag = op.initialize_dof_vector()
        op.compute_inverse_diagonal(diag)
        assert rel_err(diag.to_host(), Lv.inv_diag) < 1e-13
        op.vmult_interface_up(dst, src)
        t = Lv.A_edge_in @ x
        assert np.abs(dst.to_host() - t).max() <= 1e-13 * max(np.abs(t).max(), 1.0)
        op.vmult_interface_down(dst, src)
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
    n = ref.G.n
    assert h.n_dofs == n
    r = np.random.default_rng(42).standard_normal(n)
    r[ref.G.constrained] = 0.0
    vr, vz = mgamd.Vector(ctx, n).from_host(r), mgamd.Vector(ctx, n)
    h.mg.vmult(vz, vr)
    assert rel_err(vz.to_host(), ref.vcycle(r)) < 1e-11
    xref, itref, hist = ref.solve(1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    assert it == itref and rel_err(x.to_host(), xref) < 1e-10


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


def test_sharded_solve_matches_single_rank(mgamd, monkeypatch):
    """two simulated ranks, p = 5, quadrant NRefGlobal 3, `HMG-global`: sharded vmult and CG solve against the one-rank run
    (bounds of test_gpu_distributed_sim.py's test of that name)"""
    # the sharded path has no global DoF index: both runs use the key-hash Chebyshev start vector
    monkeypatch.setenv("MGAMD_CHEB_KEY_INIT", "1")
    geo, L, p, n_ranks = "quadrant", 3, 5, 2
    ctx0 = mgamd.Context(0)
    h0 = mgamd.Hierarchy(ctx0, geo, L, p, "HMG-global", coarse_solver="amg", max_brick=0)
    b0, x0 = h0.fine_operator.initialize_dof_vector(), h0.fine_operator.initialize_dof_vector()
    h0.fine_operator.rhs(b0)
    it0, res0 = mgamd.solve_cg(h0.fine_operator, h0.mg, x0, b0, 1e-4)
    keys0 = keyset(h0.dofs[-1].keys())
    ref = dict(zip(keys0, x0.to_host()))
    u0 = np.random.default_rng(31).standard_normal(h0.n_dofs)
    vu, vAu = h0.fine_operator.initialize_dof_vector().from_host(u0), h0.fine_operator.initialize_dof_vector()
    h0.fine_operator.vmult(vAu, vu)
    uref, Auref = dict(zip(keys0, u0)), dict(zip(keys0, vAu.to_host()))
    group = mgamd.SimGroup(n_ranks)

    def rank_main(r):
        ctx = mgamd.Context(0)
        h = mgamd.DistributedHierarchy(ctx, group.comm(r), geo, L, p, coarse_solver="amg", max_brick=0, min_root_dofs=0)
        keys = keyset(h.dofs[-1].keys())
        u = h.fine_operator.initialize_dof_vector().from_host(np.array([uref[k] for k in keys]))
        Au = h.fine_operator.initialize_dof_vector()
        h.fine_operator.vmult(Au, u)
        err_A = max(abs(a - Auref[k]) for a, k in zip(Au.to_host(), keys)) / max(abs(v) for v in Auref.values())
        b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
        h.fine_operator.rhs(b)
        it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
        info = h.dofs[-1].info
        return dict(it=it, res=res, keys=keys, x=x.to_host(), n_dofs=h.n_dofs, err_A=err_A, peers=info.n_peers, send=info.n_halo_send)

    out = run_ranks(n_ranks, rank_main)
    assert all(o["n_dofs"] == h0.n_dofs for o in out)
    assert all(o["peers"] >= 1 and o["send"] > 0 for o in out)
    for o in out:
        print(f"sharded p=5: vmult err {o['err_A']:.2e}, iterations {o['it']} (one rank {it0})")
        assert o["err_A"] < 1e-13
        assert o["it"] == it0
        assert o["res"] == pytest.approx(res0, rel=1e-7)
        assert rel_err(o["x"], np.array([ref[k] for k in o["keys"]])) < 1e-10


def test_harness_degree_six(oracle, tmp_path):
    """the JSON-driven harness binary on "Degree": 6 (quadrant, NRefGlobal 2, double levels): DoF count and CG iteration count of
    the oracle (written like test_harness_gpu.py)"""
    binary = os.path.join(ROOT, "dealii_multigrid_amd", "bin", "multigrid_throughput")
    base = json.load(open(os.path.join(ROOT, "tests", "golden", "input_0003.json")))
    cfg = dict(base, Type="HMG-global", GeometryType="quadrant", NRefGlobal=2, Degree=6, MGNumberType="double", Verbosity=False)
    f = str(tmp_path / "degree6.json")
    json.dump(cfg, open(f, "w"))
    r = subprocess.run([binary, f], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.rstrip().split("\n")
    start = max(i for i, l in enumerate(lines) if l.startswith("dim "))
    row = dict(zip(lines[start].split(), lines[start + 1].split()))
    lv, P = oracle.build_hierarchy("quadrant", 2, 6, "HMG-global")
    mg = oracle.Multigrid(lv, P, 3, coarse="direct")
    itref = oracle.pcg(lv[-1].A, lv[-1].rhs_constant, mg.vcycle, 1e-4)[1]
    assert int(row["degree"]) == 6 and int(row["n_dofs"]) == lv[-1].n == N_DOFS_QUADRANT_2[6]
    assert int(row["n_iterations"]) == itref
