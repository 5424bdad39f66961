"""Local smoothing (`HMG-local`, `HPMG-local`) with FP32 levels (MGNumberType float, the reference's default), and the cycle driver's
other paths (FP32 outer vectors, graph replay, stage callbacks) in both number types, against oracle/ls_oracle.py.

Local smoothing runs the kernels of global coarsening with other gather / scatter limits (identity edge rows, the residual matrix
with the edge rows, the edge-in matrix), its own indexed copies between the active mesh and the levels and its own cycle driver.
The tolerances are those of tests/test_gpu_float_levels.py:

  one kernel (operator, inverse diagonal, both edge matrices, both transfer directions)   rel.err < 2e-6 against the FP64 oracle
  chained kernels (the V-cycle)      rel.err <= 16 e_ref and < 5e-5,   e_ref = rel_err(float32 emulation, float64 oracle)

with e_ref from f32_emulation.ls_vcycle / pls_vcycle for that mesh, smoother degree and input, the product's eigenvalue estimates
injected.  tests/test_f32_emulation.py holds the emulation itself: bitwise the oracle in float64, e_ref <= 2.5e-5 on these meshes,
and a cycle without the edge rows in the residual or without the edge-in correction 0.06 to 0.6 away.

Smoother degrees 1, 2, 3: step_raw returns another buffer by parity, and copy_from_mg reads sol[l] of every level.
Every case prints its error and, for chained kernels, its ratio to e_ref; DESIGN.md (parity section) holds the table."""
import json
import os

import numpy as np
import pytest

import support as su
from _degree_cases import round32
from conftest import rel_err
from support import emu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

TOL_F32, MARGIN, CAP = su.TOL_F32, 16, 5e-5  # tests/test_gpu_float_levels.py
UNIT_ROUNDOFF = 2.0 ** -24

# p = 1, 3, 4, 5 on the smallest mesh with refinement edges; one 17-point brick per level (quadrant 4, p = 2); interior patches whose
# whole surface is refinement edge and which have no Dirichlet DoF (circle 5)
VCYCLE_CASES = [("quadrant", 3, 1), ("quadrant", 3, 3), ("quadrant", 3, 4), ("quadrant", 3, 5), ("quadrant", 4, 2), ("circle", 5, 2)]
EIGHT_BRICKS = ("quadrant", 4, 4)  # eight 17-point bricks on the finest level: edge DoFs on the faces the bricks share
KERNEL_CASES = VCYCLE_CASES + [EIGHT_BRICKS]
DEGREES = [1, 2, 3]
NUMBER_TYPES = [("F32", "F64"), ("F32", "F32"), ("F64", "F32")]  # (levels, outer vectors)
DRIVER_CASE = ("quadrant", 3, 4)  # second cycle, graph replay, stage callbacks
HPMG_CASES = [("quadrant", 3, 4), ("circle", 5, 2)]
case_id = lambda c: "-".join(map(str, c))  # noqa: E731


@pytest.fixture(scope="module")
def hierarchies(mgamd, ctx):
    """(product hierarchy, oracle) per (mesh, degree, smoother degree, number type of the levels); one oracle per (mesh, degree)"""
    cache = {}

    def get(case, k, levels_type):
        if (case, k, levels_type) not in cache:
            h = mgamd.Hierarchy(ctx, *case, "HMG-local", smoother_degree=k, coarse_solver="amg", number_type=getattr(mgamd, levels_type),
                                max_brick=0)
            assert h.mg.coarse_solver_used() == "direct"
            cache[(case, k, levels_type)] = (h, su.local_smoothing_oracle(h, *case))
        return cache[(case, k, levels_type)]

    return get


def seeded_input(ref, outer_type="F64"):
    r = np.random.default_rng(42).standard_normal(ref.G.n)
    r[ref.G.constrained] = 0.0
    return round32(r) if outer_type == "F32" else r


def nan_vector(mgamd, ctx, n, outer_type="F64"):
    return mgamd.Vector(ctx, n, getattr(mgamd, outer_type)).from_host(np.full(n, np.nan))


def injected(emu, ref, h, k):
    """the oracle with smoother degree k and the product's eigenvalue estimates: the comparison is about the kernels alone"""
    return emu.ls_with_max_evs(emu.ls_with_degree(ref, k), [s.eigenvalue_estimates()[1] for s in h.smoothers])


def float_reference(emu, ls, r):
    """the float64 cycle of r and e_ref, the distance of the float32 emulation from it"""
    z64 = ls.vcycle(r)
    z32 = emu.ls_vcycle(ls, r, np.float32)
    assert z32.dtype == np.float32
    return z64, rel_err(z32.astype(np.float64), z64)


@pytest.mark.parametrize("case", KERNEL_CASES, ids=case_id)
def test_float_level_kernels(mgamd, oracle, emu, ctx, hierarchies, case):
    """every FP32 kernel of every local-smoothing level on its own, twice (the tail accumulator must be clean after a pass)"""
    h, ref = hierarchies(case, 3, "F32")
    geo, L, p = case
    assert len(h.operators) == len(ref.levels) and any(Lv.edge.any() for Lv in ref.levels)
    if case == EIGHT_BRICKS:
        assert sum(n for B, n in h.dofs[-1].groups()) == 8 and all(B * p + 1 == 17 for B, n in h.dofs[-1].groups() if n)
    rng = np.random.default_rng(41)
    for l, (op, Lv) in enumerate(zip(h.operators, ref.levels)):
        assert op.m() == Lv.n and h.dofs[l].info.n_edge == Lv.edge.sum()
        if geo == "circle" and l > 3:
            assert Lv.edge.any() and not Lv.dirichlet.any()
        tag = f"FP32 local smoothing {case_id(case)} level {l} ({Lv.n} DoFs, {Lv.edge.sum()} edge)"
        for trial in range(2):
            x = round32(rng.standard_normal(Lv.n))
            src, dst = op.initialize_dof_vector().from_host(x), op.initialize_dof_vector()
            dst.set(7.0)  # every pass must overwrite
            op.vmult(dst, src)  # identity edge rows
            e_a = rel_err(dst.to_host(), Lv.A @ x)
            diag = op.initialize_dof_vector()
            diag.set(7.0)
            op.compute_inverse_diagonal(diag)  # D^-1 of the edge rows: 1
            e_d = rel_err(diag.to_host(), Lv.inv_diag)
            dst.set(7.0)
            op.vmult_interface_down(dst, src)  # the residual matrix: edge DoFs as ordinary rows and columns
            e_down = rel_err(dst.to_host(), Lv.A_down @ x)
            dst.set(7.0)
            op.vmult_interface_up(dst, src)  # the edge-in matrix: edge columns only
            t = Lv.A_edge_in @ x
            e_up = np.abs(dst.to_host() - t).max() / max(np.abs(t).max(), 1.0)
            print(f"{tag} pass {trial}: vmult {e_a:.2e}, inverse diagonal {e_d:.2e}, interface down {e_down:.2e}, interface up (max norm) {e_up:.2e}")
            assert e_a < TOL_F32
            assert e_d < TOL_F32
            assert e_down < TOL_F32
            assert e_up <= TOL_F32
            assert np.array_equal(src.to_host(), x)  # src untouched
        if l > 0:
            nc = ref.levels[l - 1].n
            xc, xf0 = round32(rng.standard_normal(nc)), round32(rng.standard_normal(Lv.n))
            vc, vf = h.operators[l - 1].initialize_dof_vector().from_host(xc), op.initialize_dof_vector().from_host(xf0)
            h.transfers[l].prolongate_and_add(vf, vc)
            e1 = rel_err(vf.to_host(), xf0 + ref.P[l] @ xc)
            rf, dc0 = round32(rng.standard_normal(Lv.n)), round32(rng.standard_normal(nc))
            vr, vd = op.initialize_dof_vector().from_host(rf), h.operators[l - 1].initialize_dof_vector().from_host(dc0)
            h.transfers[l].restrict_and_add(vd, vr)
            e2 = rel_err(vd.to_host(), dc0 + ref.P[l].T @ rf)
            print(f"{tag}: prolongate {e1:.2e}, restrict {e2:.2e}")
            assert e1 < TOL_F32 and e2 < TOL_F32
            assert np.array_equal(vc.to_host(), xc) and np.array_equal(vr.to_host(), rf)
        # the eigenvalue estimate: the bound of test_gpu_float_levels.test_chebyshev
        want = ref.sm[l].max_ev
        dev_ref = abs(emu.eigenvalue_estimate(Lv.A, Lv.inv_diag, np.float32) - want) / want
        dev = abs(h.smoothers[l].eigenvalue_estimates()[1] - want) / want
        print(f"{tag}: eigenvalue estimate dev {dev:.1e} (emulation {dev_ref:.1e})")
        assert dev <= max(MARGIN * dev_ref, MARGIN * UNIT_ROUNDOFF), (dev, dev_ref)


@pytest.mark.parametrize("levels_type,outer_type", NUMBER_TYPES)
@pytest.mark.parametrize("k", DEGREES)
@pytest.mark.parametrize("case", VCYCLE_CASES, ids=case_id)
def test_vcycle(mgamd, emu, ctx, hierarchies, case, k, levels_type, outer_type):
    """(F32, F64): indexed copies double -> float and back; (F32, F32): the cycle driver in float throughout; (F64, F32): float
    outer vectors on double levels.  An FP32 outer r is rounded first and the rounded r goes to the reference."""
    h, ref = hierarchies(case, k, levels_type)
    n = ref.G.n
    assert h.n_dofs == n
    ls = injected(emu, ref, h, k)
    r = seeded_input(ref, outer_type)
    z64, e_ref = float_reference(emu, ls, r)
    vr, vz = mgamd.Vector(ctx, n, getattr(mgamd, outer_type)).from_host(r), nan_vector(mgamd, ctx, n, outer_type)
    tag = f"local smoothing V-cycle {case_id(case)} k={k} levels {levels_type} outer {outer_type}"

    def check(what):
        z = vz.to_host()
        assert np.isfinite(z).all()
        err = rel_err(z, z64)
        print(f"{tag} {what}: rel.err {err:.2e}, e_ref {e_ref:.2e}, ratio {err / e_ref:.2f}")
        assert err <= MARGIN * e_ref
        assert err < CAP
        assert np.array_equal(vr.to_host(), r)

    h.mg.vmult(vz, vr)
    check("first cycle")
    if case != DRIVER_CASE:
        return
    vz.from_host(np.full(n, np.nan))
    h.mg.vmult(vz, vr)
    check("second cycle")
    vz.from_host(np.full(n, np.nan))
    assert h.mg.time_vcycles(vz, vr, 2, True) > 0
    check("graph replay")
    h.mg.connect_stages(lambda s, start, lv: None)
    vz.from_host(np.full(n, np.nan))
    h.mg.vmult(vz, vr)
    h.mg.connect_stages(None)
    check("stage callbacks")


@pytest.mark.parametrize("case", [("quadrant", 3, 4), ("circle", 5, 2)], ids=case_id)
def test_double_levels_graph_replay_and_stage_callbacks(mgamd, emu, ctx, hierarchies, case):
    """the captured cycle holds the two memsets and the indexed copies of every level; callbacks synchronise between the stages"""
    h, ref = hierarchies(case, 3, "F64")
    n = ref.G.n
    for l, s in enumerate(h.smoothers):
        assert s.eigenvalue_estimates()[1] == pytest.approx(ref.sm[l].max_ev, rel=1e-9)
    ls = injected(emu, ref, h, 3)
    r = seeded_input(ref)
    z64 = ls.vcycle(r)
    eager = su.apply_nan(mgamd, ctx, h.mg.vmult, r)
    vr, vz = mgamd.Vector(ctx, n).from_host(r), nan_vector(mgamd, ctx, n)
    tag = f"local smoothing {case_id(case)} FP64"

    def check(what):
        z = vz.to_host()
        assert np.isfinite(z).all()
        e_oracle, e_eager = rel_err(z, z64), rel_err(z, eager)
        print(f"{tag} {what}: against the oracle {e_oracle:.2e}, against the eager cycle {e_eager:.2e}")
        assert e_oracle < su.TOL_CYCLE
        assert e_eager < 1e-13
        assert np.array_equal(vr.to_host(), r)

    assert rel_err(eager, z64) < su.TOL_CYCLE
    assert h.mg.time_vcycles(vz, vr, 3, True) > 0
    check("graph replay")
    vz.from_host(np.full(n, np.nan))
    h.mg.vmult(vz, vr)
    check("eager cycle after the replays")
    stages = []
    h.mg.connect_stages(lambda s, start, lv: stages.append((s, start, lv)))
    vz.from_host(np.full(n, np.nan))
    h.mg.vmult(vz, vr)
    h.mg.connect_stages(None)
    check("stage callbacks")
    assert {s for s, _, _ in stages} == set(range(9)) and len(stages) % 2 == 0
    vz.from_host(np.full(n, np.nan))
    h.mg.vmult(vz, vr)
    check("eager cycle after the callbacks")


@pytest.mark.parametrize("k", DEGREES)
@pytest.mark.parametrize("case", VCYCLE_CASES, ids=case_id)
def test_cg_iteration_count_of_the_emulated_cycle(mgamd, oracle, emu, ctx, hierarchies, case, k):
    h, ref = hierarchies(case, k, "F32")
    ls = injected(emu, ref, h, k)
    G = ref.G
    xref, it64, _ = oracle.pcg(G.A, G.rhs_constant, ls.vcycle, 1e-4)
    x32, it32, _ = oracle.pcg(G.A, G.rhs_constant, lambda r: emu.ls_vcycle(ls, r, np.float32).astype(np.float64), 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    err = rel_err(x.to_host(), xref)
    print(f"FP32 local smoothing CG {case_id(case)} k={k}: iterations gpu {it}, float32 emulation {it32}, FP64 oracle {it64}, rel.err {err:.2e}")
    assert it == it32
    assert err < 1e-3


@pytest.fixture(scope="module")
def hpmg_local(mgamd, ctx):
    """`HPMG-local` with FP32 levels: the p-levels and the local-smoothing levels underneath, and the composed oracle"""
    import ls_oracle

    cache = {}

    def get(case):
        if case not in cache:
            h = mgamd.Hierarchy(ctx, *case, "HPMG-local", coarse_solver="amg", number_type=mgamd.F32, max_brick=0)
            assert h.mg.coarse_solver_used() == "gmg_vcycle" and h.degrees[-1] == case[2] and h.degrees[0] == 1
            ref = ls_oracle.PolynomialOverLocalSmoothing(*case, numbering_keys_p=[d.keys() for d in h.dofs],
                                                         numbering_keys_levels=[d.keys() for d in h.ls["dofs"]])
            cache[case] = (h, ref)
        return cache[case]

    return get


@pytest.mark.parametrize("case", HPMG_CASES, ids=case_id)
def test_hpmg_local_float_levels(mgamd, oracle, emu, ctx, hpmg_local, case):
    """the float p-level 0 hands its defect to the local-smoothing cycle in float (vcycle_ls_raw<float>) and takes its result"""
    h, ref = hpmg_local(case)
    pls = emu.pls_with_max_evs(ref, [s.eigenvalue_estimates()[1] for s in h.smoothers],
                               [s.eigenvalue_estimates()[1] for s in h.ls["smoothers"]])
    n = ref.G.n
    r = seeded_input(ref)
    z64 = pls.vcycle(r)
    z32 = emu.pls_vcycle(pls, r, np.float32)
    assert z32.dtype == np.float32
    e_ref = rel_err(z32.astype(np.float64), z64)
    for trial in range(2):
        z = su.apply_nan(mgamd, ctx, h.mg.vmult, r)
        err = rel_err(z, z64)
        print(f"FP32 HPMG-local V-cycle {case_id(case)} cycle {trial}: rel.err {err:.2e}, e_ref {e_ref:.2e}, ratio {err / e_ref:.2f}")
        assert err <= MARGIN * e_ref
        assert err < CAP
    G = ref.G
    xref, it64, _ = oracle.pcg(G.A, G.rhs_constant, pls.vcycle, 1e-4)
    x32, it32, _ = oracle.pcg(G.A, G.rhs_constant, lambda v: emu.pls_vcycle(pls, v, np.float32).astype(np.float64), 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b)
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    err = rel_err(x.to_host(), xref)
    print(f"FP32 HPMG-local CG {case_id(case)}: iterations gpu {it}, float32 emulation {it32}, FP64 oracle {it64}, rel.err {err:.2e}")
    assert it == it32
    assert err < 1e-3


def test_hpmg_local_harness_input_with_float_levels(hpmg_local, tmp_path):
    """input_0003.json with Type HPMG-local and MGNumberType at its float default (iterations: +-1, the harness convention for
    float levels)"""
    cfg = dict(json.load(open(os.path.join(su.GOLDEN, "input_0003.json"))), Type="HPMG-local")
    assert cfg["MGNumberType"] == "float"
    f = str(tmp_path / "hpls_float.json")
    json.dump(cfg, open(f, "w"))
    rc, out, err = su.run_harness(f)
    assert rc == 0, err
    header, rows = su.final_table(out)
    r = rows[0]
    assert (int(r["n_dofs"]), int(r["n_levels"]), r["coarse_solver"]) == (9295, 3, "gmg_vcycle")
    itref = hpmg_local(("quadrant", 3, 4))[1].solve(1e-4)[1]  # (the module's oracle of the input's mesh and degree)
    print(f"HPMG-local harness run, float levels: iterations {r['n_iterations']} (oracle {itref})")
    assert abs(int(r["n_iterations"]) - itref) <= 1
