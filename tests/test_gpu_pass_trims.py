"""The trimmed brick passes against the oracles.

  * The fused residual pass (MODE_RESIDUAL_RESTRICT) runs its tail epilogue only over the rows a slot outside the fused bricks
    touches (TransferTables::residual_tail_runs, tail_runs_kernel): an accumulator entry left non-zero, or a row of t that is
    needed and not written, shows in the operator applications and in the second V-cycle after a first one.
  * The Chebyshev passes of the persistent 17-point brick kernel (zero-start MODE_CHEB_FIRST / MODE_CHEB_SECOND, plain MODE_CHEB)
    on levels with and without a D^-1 code table, with several bricks per workgroup, and on a brick whose shell carries D^-1
    values outside the level's 255-entry table.  Three trims of these passes were built and measured with this file (DESIGN.md
    section 4, "pass trims"); none of them won, the kernels are the parent's, and the cases stay as the pin for the next attempt.

References.  ("quadrant", 4, 4): the numpy oracle (mgoracle), as tests/test_gpu_parity.py.  ("quadrant", 6, 4), 2.1 M DoFs, 343 fused
bricks on the finest level: the numpy oracle needs more than ten minutes for its matrices, so the operator of every level and the
V-cycle come from the C++ CPU oracle (oracle/cpu_oracle.py, as tests/test_gpu_vs_cpu_oracle.py) and the Chebyshev iteration is
mgoracle.Chebyshev on that operator; bounds as in those tests: operator 1e-13, Chebyshev 1e-12, V-cycle 1e-11."""
import os
import subprocess
import sys

import numpy as np
import pytest

import physics_oracle as po
import support as su
from conftest import rel_err

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("quadrant", 4, 4, "HMG-global"), ("quadrant", 6, 4, "HMG-global")]
TOL_OP, TOL_CHEB, TOL_CYCLE = 1e-13, 1e-12, 1e-11


class Reference:
    """operator and inverse diagonal of every level and the V-cycle, from the numpy oracle or from the C++ CPU oracle"""

    class _Matrix:  # what mgoracle.Chebyshev needs of a matrix, on the CPU oracle's operator
        def __init__(self, level):
            self.level, self.shape = level, (level.n, level.n)

        def __matmul__(self, x):
            return self.level.vmult(x)

    def __init__(self, mgamd, oracle, h, geo, L, p, mg_type):
        if L <= 4:
            levels, P = oracle.build_hierarchy(geo, L, p, mg_type, numbering_keys=[d.keys() for d in h.dofs])
            self.A = [lv.A for lv in levels]
            self.inv_diag = [lv.inv_diag for lv in levels]
            self.mg = oracle.Multigrid(levels, P, 3, coarse="direct")
            self.max_ev = [s.max_ev for s in self.mg.sm]
        else:
            import cpu_oracle

            levels, transfers, self.mg = cpu_oracle.build_from_dofs(h.dofs, mgamd.transfer_tables, coarse="amg")
            self.keep = (levels, transfers)
            self.A = [self._Matrix(lv) for lv in levels]
            self.inv_diag = [lv.inverse_diagonal() for lv in levels]
            self.max_ev = [self.mg.max_eigenvalue(l) for l in range(len(levels))]


@pytest.fixture(scope="module")
def hierarchies(mgamd, oracle, ctx):
    cache = {}

    def get(case):
        if case not in cache:
            geo, L, p, mg_type = case
            h = mgamd.Hierarchy(ctx, geo, L, p, mg_type, coarse_solver="amg", max_brick=0)
            assert sum(t.n_fused_bricks() for t in h.transfers[1:]) > 0
            cache[case] = (h, Reference(mgamd, oracle, h, geo, L, p, mg_type))
        return cache[case]

    return get


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_accumulator_left_clean(mgamd, ctx, hierarchies, case):
    h, ref = hierarchies(case)
    n = h.n_dofs
    r = np.random.default_rng(7).standard_normal(n)
    z1 = su.apply_nan(mgamd, ctx, h.mg.vmult, r)
    rng = np.random.default_rng(3)
    for l, op in enumerate(h.operators):  # an accumulator entry the residual pass left behind is added to A x here
        x = rng.standard_normal(h.dofs[l].n_dofs)
        err = rel_err(su.apply_nan(mgamd, ctx, op.vmult, x), ref.A[l] @ x)
        print(f"{case} level {l}: vmult after a V-cycle rel.err {err:.2e}")
        assert err <= TOL_OP
    z2 = su.apply_nan(mgamd, ctx, h.mg.vmult, r)
    err = rel_err(z2, z1)
    print(f"{case}: second V-cycle against the first {err:.2e}")
    assert err <= 1e-14


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_cycle_unchanged(mgamd, oracle, ctx, hierarchies, case):
    h, ref = hierarchies(case)
    for l, s in enumerate(h.smoothers):
        assert s.eigenvalue_estimates()[1] == pytest.approx(ref.max_ev[l], rel=1e-9)
    n = h.n_dofs
    r = np.random.default_rng(7).standard_normal(n)
    err = rel_err(su.apply_nan(mgamd, ctx, h.mg.vmult, r), ref.mg.vcycle(r))
    print(f"{case}: V-cycle rel.err {err:.2e}")
    assert err <= TOL_CYCLE
    # zero-start vmult (MODE_CHEB_FIRST, MODE_CHEB_SECOND, MODE_CHEB) and step, on the finest level (code table) and on the
    # coarsest level that still has a 17-point brick (quadrant L = 4: 10528 tail DoFs; below 4096 a level has no codes)
    rng = np.random.default_rng(5)
    for l in sorted({len(h.operators) - 1, next(i for i, d in enumerate(h.dofs) if any(4 * B + 1 == 17 and ns > 0 for B, ns in d.groups()))}):
        op, nl = h.operators[l], h.dofs[l].n_dofs
        for degree in (2, 3):
            ch = mgamd.PreconditionChebyshev(op, degree, 20.0, 20)
            cref = oracle.Chebyshev(ref.A[l], ref.inv_diag[l], degree, 20.0, 20)
            assert ch.eigenvalue_estimates()[1] == pytest.approx(cref.max_ev, rel=1e-10)
            b, x0 = rng.standard_normal(nl), rng.standard_normal(nl)
            ev = rel_err(su.apply_nan(mgamd, ctx, ch.vmult, b), cref.vmult(b))
            vx, vb = op.initialize_dof_vector().from_host(x0), op.initialize_dof_vector().from_host(b)
            ch.step(vx, vb)
            es = rel_err(vx.to_host(), cref.step(x0, b))
            print(f"{case} level {l} degree {degree}: Chebyshev vmult {ev:.2e}, step {es:.2e}")
            assert ev <= TOL_CHEB and es <= TOL_CHEB


def _dump(tmp_path, name, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    out = str(tmp_path / name)
    subprocess.run([sys.executable, os.path.join(HERE, "_vcycle_dump.py"), "quadrant", "7", "4", out], check=True, env=env, timeout=400)
    return np.load(out)


def test_several_bricks_per_persistent_workgroup(tmp_path):
    """quadrant L=7 p=4: 3375 bricks on 512 persistent workgroups, the slot loop (and the hand-over of the prefetched operands
    from one brick to the next) runs several times.  Default against separate transfer kernels (whole tail epilogue) and against
    the vector read of D^-1 (no code table)."""
    ref = _dump(tmp_path, "default.npz", {})
    assert any(B == 4 and ns > 512 for B, ns in ref["groups"])
    for switch in ("MGAMD_NO_FUSED_TRANSFER", "MGAMD_NO_DINV_CODES"):
        alt = _dump(tmp_path, switch + ".npz", {switch: "1"})
        for key in ("ax", "step", "vcycle"):
            err = np.linalg.norm(ref[key] - alt[key]) / np.linalg.norm(ref[key])
            print(f"{switch} {key}: {err:.2e}")
            assert err <= 1e-12, (switch, key)


def test_code_255_on_the_shell_of_a_brick(mgamd, oracle, ctx):
    """quadrant L=4 p=4 with a coefficient that is 2 on the cells of the one 17-point brick and differs from cell to cell around it
    (physics_oracle.per_cell): the shell entries of the brick carry more than 255 distinct D^-1 values (278 measured), so
    whatever the 255 table entries of the level are, some of the brick's shell DoFs have code 255 and whoever reads D^-1 through
    the codes -- tail_kernel today -- reads the vector for them.  V-cycle against oracle/physics_oracle.py."""
    import f32_emulation as emu

    case = ("quadrant", 4, 4, "HMG-global")
    plain = mgamd.DoFs(mgamd.Triangulation("quadrant", 4), 4, 0)
    grp, _ = plain.cell_slots()
    B = list(plain.info.group_B)
    t = mgamd.Triangulation("quadrant", 4)
    cells = po.product_cells(t)
    in_brick = {c for c, g in zip(cells, grp) if B[int(g)] == 4}
    assert len(in_brick) == 64

    def field(cell):
        return 2.0 if tuple(cell) in in_brick else po.per_cell(cell)

    t.set_coefficient(po.product_values(t, po.field_on(cells, field)))
    h = mgamd.Hierarchy(ctx, t, 4, 4, "HMG-global", coarse_solver="amg", max_brick=0)
    d = h.dofs[-1]
    assert (4, 1) in [tuple(g) for g in d.groups()]  # the brick survived the field
    assert d.n_dofs - d.info.n_interior >= 4096      # the level has a code table
    # distinct D^-1 values on the brick's shell, from the product's own diagonal (differences above 1e-9 relative only)
    diag = h.fine_operator.initialize_dof_vector()
    h.fine_operator.compute_inverse_diagonal(diag)
    dv = diag.to_host()
    grp2, _ = d.cell_slots()
    B2 = list(d.info.group_B)
    cd = d.cell_dofs()
    shell = np.unique(np.concatenate([cd[c] for c in range(len(grp2)) if B2[int(grp2[c])] == 4]))
    shell = shell[(shell >= d.info.n_interior) & (shell < d.info.n_interior + d.info.n_tail)]
    n_distinct = len(np.unique(np.round(np.log(dv[shell]) * 1e9)))
    print(f"{len(shell)} tail DoFs on the brick's shell with {n_distinct} distinct D^-1 values")
    assert n_distinct > 255
    levels, P = su.oracle_hierarchy(h.dofs, case, po.Problem(0.0, field))
    mg = su.injected(emu, oracle, levels, P, h)
    r = np.random.default_rng(7).standard_normal(levels[-1].n)
    err = rel_err(su.apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r))
    print(f"V-cycle rel.err {err:.2e}")
    assert err <= TOL_CYCLE
