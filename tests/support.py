"""What the test files share, defined once.  Not a test module and not a conftest.

  * one session cache of the numpy oracle's spaces (one constraint search per (mesh, degree)) and of their mask-0 transfers, in the
    oracle's own numbering, keyed by the leaves themselves: named geometries, caller-built leaves and the random octrees cannot
    collide;
  * oracle_level / oracle_hierarchy: the levels of a physics_oracle.Problem in the numbering of the product's tables -- always
    renumber the cached space, then form the level;
  * tria / hierarchy: the product's mesh and multigrid hierarchy for the same Problem, with the propagation assertions;
  * the checks, tolerances, case lists and helpers that several test files use.

Problem.coefficient may here also be the NAME of one of physics_oracle.FIELDS or a function of the cell; it is evaluated on the
(finest) mesh."""
import dataclasses
import os
import subprocess
import threading

import numpy as np
import pytest

import mgoracle
import physics_oracle as po
import time_stepping_oracle as ts
from conftest import ROOT, rel_err
from physics_oracle import Problem

TOL_OP, TOL_CHEB, TOL_CYCLE, TOL_SOL, TOL_F32 = 1e-13, 1e-12, 1e-11, 1e-10, 2e-6

# operator shapes, the smallest that reach each kernel: families, single cells with hanging faces and edges, p = 1 clusters;
# wave-scoped cells only; constrained rim bricks; one 17-point brick (persistent kernel, closed-form D^-1) at p = 4, 2, 1; eight 17^3
# bricks sharing faces, edges and a vertex; the 11- and 15-point lattices
OP_CASES = ([("quadrant", 3, p, 0) for p in (1, 2, 3, 4)] + [("quadrant", 3, 4, 1), ("quadrant", 4, 1, 0), ("hypercube", 2, 4, 0),
            ("hypercube", 3, 2, 0), ("hypercube", 4, 1, 0), ("hypercube", 3, 4, 0), ("quadrant", 2, 5, 0), ("quadrant", 2, 7, 0)])


@pytest.fixture(scope="module")
def emu():
    """oracle/f32_emulation.py; a test module takes it with `from support import emu`"""
    import f32_emulation

    return f32_emulation


# ------------------------------------------------------------------ the numpy oracle's spaces, cached
_meshes, _spaces, _transfers = {}, {}, {}


def mesh(geo, L, n_ref_local=0):
    """mgoracle.create_mesh, once per session"""
    tag = (geo, L, n_ref_local)
    if tag not in _meshes:
        _meshes[tag] = mgoracle.create_mesh(geo, L, n_ref_local)
    return _meshes[tag]


def space(leaves, p):
    tag = (frozenset(leaves), p)
    if tag not in _spaces:
        _spaces[tag] = po.Space(leaves, p)
    return _spaces[tag]


def natural_transfers(meshes, degs):
    """the mask-0 transfers between the cached spaces, coarse -> fine"""
    P0 = [None]
    for l in range(1, len(meshes)):
        tag = (frozenset(meshes[l]), degs[l], frozenset(meshes[l - 1]), degs[l - 1])
        if tag not in _transfers:
            _transfers[tag] = po.natural_transfer(space(meshes[l], degs[l]), space(meshes[l - 1], degs[l - 1]))
        P0.append(_transfers[tag])
    return P0


def _keys(d):
    return d.keys() if hasattr(d, "keys") else d


def _on(problem, leaves):
    """the problem with its coefficient as {cell: a} on the leaves"""
    c = problem.coefficient
    if isinstance(c, str):
        c = po.FIELDS[c]
    return dataclasses.replace(problem, coefficient=po.field_on(leaves, c)) if callable(c) else problem


def oracle_level_on(d, leaves, p, problem=Problem()):
    """the level of the problem on the leaves, numbered like the product's tables d (DoFs or an array of keys; None: the oracle's
    own numbering)"""
    s = space(leaves, p)
    return po.Level(s if d is None else s.renumbered(_keys(d))[0], _on(problem, leaves))


def oracle_level(d, geo, L, p, problem=Problem()):
    return oracle_level_on(d, mesh(geo, L), p, problem)


def oracle_hierarchy_on(dofs, meshes, degs, problem=Problem(), restrict=None):
    """(levels, P) on (meshes, degrees) coarse -> fine in the numbering of the product's level tables `dofs` (None: the oracle's
    own); the coefficient is the problem's on the finest mesh and restrict (default physics_oracle.restrict_field) of it below"""
    spaces, P0 = [space(m, p) for m, p in zip(meshes, degs)], natural_transfers(meshes, degs)
    if dofs is not None:
        spaces, Q = zip(*[s.renumbered(_keys(d)) for s, d in zip(spaces, dofs)])
        P0 = [None] + [(Q[l] @ P0[l] @ Q[l - 1].T).tocsr() for l in range(1, len(spaces))]
    return po.hierarchy(list(spaces), P0, _on(problem, meshes[-1]), restrict)


def oracle_hierarchy(dofs, case, problem=Problem(), restrict=None):
    """the same for case = (geometry, NRefGlobal, degree, Type)"""
    return oracle_hierarchy_on(dofs, *po.level_plan_on(mesh(*case[:2]), *case[2:]), problem, restrict)


_local_smoothings = {}


def local_smoothing_oracle(h, geo, L, p):
    """ls_oracle.LocalSmoothing(geo, L, p) in the numbering of the product's `HMG-local` hierarchy h, assembled once per session.
    The numbering at max_brick=0 depends on neither the number type nor the smoother degree: asserted through the keys of every
    hierarchy that asks."""
    import ls_oracle

    keys = [h.active_dofs.keys()] + [d.keys() for d in h.dofs]
    if (geo, L, p) not in _local_smoothings:
        ref = ls_oracle.LocalSmoothing(geo, L, p, numbering_keys_global=keys[0], numbering_keys_levels=keys[1:])
        _local_smoothings[(geo, L, p)] = (keys, ref)
    kept, ref = _local_smoothings[(geo, L, p)]
    assert len(kept) == len(keys) and all(np.array_equal(a, b) for a, b in zip(kept, keys))
    return ref


# ------------------------------------------------------------------ the product's side of a Problem
def set_problem(mgamd, t, problem):
    """mask, Robin coefficients and coefficient of the problem on the product's mesh t"""
    t.set_dirichlet_faces(problem.dirichlet_faces)
    if any(problem.robin):
        t.set_robin_coefficients(problem.robin)
    if problem.coefficient is not None:
        cells = po.product_cells(t)
        t.set_coefficient(po.product_values(t, _on(problem, cells).coefficient))
    return t


def tria(mgamd, geo, L, problem=Problem()):
    return set_problem(mgamd, mgamd.Triangulation(geo, L), problem)


def tria_of(mgamd, leaves, problem=Problem()):
    """the product's mesh on a caller's leaves"""
    arr = np.array(sorted(leaves), dtype=np.int64)
    t = mgamd.Triangulation.from_leaves(arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3])
    assert t.n_cells == len(leaves)
    return set_problem(mgamd, t, problem)


def hierarchy(mgamd, ctx, case, problem=Problem(), **kw):
    """mgamd.Hierarchy of the problem on case = (geometry, NRefGlobal, degree, Type); the coefficient is given by name (the
    product evaluates physics_oracle.XYZ[name] on its own leaves).  Every level carries what the finest mesh was given."""
    geo, L, p, mg_type = case
    kw.setdefault("coarse_solver", "amg")
    if problem.coefficient is not None:
        kw["coefficient"] = po.XYZ[problem.coefficient]
    if any(problem.robin):
        kw["robin"] = problem.robin
    if problem.dirichlet_faces != po.ALL:
        kw["dirichlet_faces"] = problem.dirichlet_faces
    h = mgamd.Hierarchy(ctx, geo, L, p, mg_type, mass_coefficient=problem.sigma, **kw)
    assert all(d.dirichlet_faces() == problem.dirichlet_faces for d in h.dofs)
    assert all(t.dirichlet_faces() == problem.dirichlet_faces for t in h.trias)
    assert all(np.array_equal(d.robin_coefficients(), problem.robin) for d in h.dofs)
    assert all(np.array_equal(t.robin_coefficients(), problem.robin) for t in h.trias)
    return h


def assert_level_coefficients(h, levels):
    """what the product's meshes carry is what the oracle restated from the finest field"""
    for t, lv in zip(h.trias, levels):
        ref = po.product_values(t, lv.coefficient)
        assert np.abs(t.coefficient() / ref - 1.0).max() <= 1e-15
    for d, t in zip(h.dofs, h.trias):
        assert d.coefficient_range() == (t.coefficient().min(), t.coefficient().max())


# ------------------------------------------------------------------ slots of the product's tables
def slot_groups(d, t):
    """[(B, [(a, cell level, has a hanging face) of slot 0, 1, ...])] for every slot group of the tables d on the mesh t that holds
    slots, from cell_slots(), info.group_B, the mesh's coefficient and its constraint masks"""
    grp, slot = d.cell_slots()
    B, a = list(d.info.group_B), t.coefficient()
    lev, _, _, _, mask = t.cells()
    hanging = ((mask >> 3) & 7) != 0  # octree.hpp MASK_FACE_SHIFT: a face of the cell lies on a coarser neighbour
    out = {}
    for c in range(len(grp)):
        v = out.setdefault(int(grp[c]), {}).setdefault(int(slot[c]), [a[c], int(lev[c]), False])
        assert v[0] == a[c] and v[1] == lev[c]  # one value, one level per slot
        v[2] |= bool(hanging[c])
    return [(B[g], [tuple(sl[s]) for s in range(len(sl))]) for g, sl in sorted(out.items())]


def slots_of(groups, B):
    """the slots of brick size B in slot order, group after group"""
    return [v for b, sl in groups if b == B for v in sl]


def consecutive(slots, what):
    """pairs of consecutive slots that differ in entry `what` (0: a, 1: cell level)"""
    return sum(slots[s][what] != slots[s + 1][what] for s in range(len(slots) - 1))


def atomic_contributions(d):
    """per DoF, how many partial sums the operator kernels add into it with floating-point atomics: one per slot (brick, family
    or single cell) that has the DoF on its shell, counted from the cell -> slot and cell -> DoF tables; 0 for slot-interior DoFs,
    which one thread completes, and for constrained DoFs (identity rows)"""
    grp, slot = d.cell_slots()
    cd = d.cell_dofs()
    pairs = set()
    for c in range(len(grp)):
        for g in cd[c]:
            if g != 0xFFFFFFFF:
                pairs.add((int(g), int(grp[c]), int(slot[c])))
    cnt = np.zeros(d.n_dofs, np.int64)
    for g, _, _ in pairs:
        cnt[g] += 1
    cnt[:d.info.n_interior] = 0
    cnt[d.info.n_interior + d.info.n_tail:] = 0
    return cnt


# ------------------------------------------------------------------ device checks
def apply_nan(mgamd, ctx, fn, x):
    """fn(dst, src) into a NaN-prefilled destination; the source must come back untouched"""
    src, dst = mgamd.Vector(ctx, len(x)).from_host(x), mgamd.Vector(ctx, len(x)).from_host(np.full(len(x), np.nan))
    fn(dst, src)
    assert np.array_equal(src.to_host(), x)
    out = dst.to_host()
    assert np.isfinite(out).all()
    return out


def injected(emu, oracle, levels, P, h, coarse="direct"):
    """oracle.Multigrid with the product's eigenvalue estimates injected (asserted first), so that the comparison is about the
    kernels alone"""
    mg = oracle.Multigrid(levels, P, 3, coarse=coarse)
    evs = [s.eigenvalue_estimates()[1] for s in h.smoothers]
    for l, ev in enumerate(evs):
        assert ev == pytest.approx(mg.sm[l].max_ev, rel=1e-9)
    return emu.with_max_evs(mg, evs)


def check_transfers(h, levels, P, tag):
    rng = np.random.default_rng(6)
    for l in range(1, len(levels)):
        xc, xf0 = rng.standard_normal(levels[l - 1].n), rng.standard_normal(levels[l].n)
        vc, vf = h.operators[l - 1].initialize_dof_vector().from_host(xc), h.operators[l].initialize_dof_vector().from_host(xf0)
        h.transfers[l].prolongate_and_add(vf, vc)
        e1 = rel_err(vf.to_host(), xf0 + P[l] @ xc)
        rf, dc0 = rng.standard_normal(levels[l].n), rng.standard_normal(levels[l - 1].n)
        vr, vd = h.operators[l].initialize_dof_vector().from_host(rf), h.operators[l - 1].initialize_dof_vector().from_host(dc0)
        h.transfers[l].restrict_and_add(vd, vr)
        e2 = rel_err(vd.to_host(), dc0 + P[l].T @ rf)
        print(f"{tag} transfer {l - 1} <-> {l}: prolongate {e1:.2e} restrict {e2:.2e}")
        assert e1 < TOL_OP and e2 < TOL_OP


def vcycle_and_solve(mgamd, oracle, emu, ctx, h, levels, P, tag, rhs_kind=0, coarse="direct"):
    """one V-cycle on a seeded vector, the right-hand side of rhs_kind (0: f == 1, 1: the Gaussian) and the CG solve against the
    oracle's Multigrid (coarse solver `coarse`) and pcg; returns (oracle multigrid, product iterate, oracle iterate)"""
    mg = injected(emu, oracle, levels, P, h, coarse)
    Lf = levels[-1]
    r = np.random.default_rng(7).standard_normal(Lf.n)
    ez = rel_err(apply_nan(mgamd, ctx, h.mg.vmult, r), mg.vcycle(r))
    bref = Lf.rhs_constant if rhs_kind == 0 else Lf.rhs_function(po.gaussian_load(Lf.mass_coefficient), oracle.gaussian_solution)
    xref, itref, hist = oracle.pcg(Lf.A, bref, mg.vcycle, 1e-4)
    b, x = h.fine_operator.initialize_dof_vector(), h.fine_operator.initialize_dof_vector()
    h.fine_operator.rhs(b, rhs_kind)
    eb = np.abs(b.to_host() - bref).max() / np.abs(bref).max()
    it, res = mgamd.solve_cg(h.fine_operator, h.mg, x, b, 1e-4)
    ex = rel_err(x.to_host(), xref)
    print(f"{tag}: V-cycle {ez:.2e}, rhs {eb:.2e}, CG iterations {it} (oracle {itref}), iterate {ex:.2e}")
    assert ez < TOL_CYCLE
    assert eb < 1e-12
    assert it == itref
    assert ex < TOL_SOL
    return mg, x, xref


def layers(x, planes, values):
    """values[k] where x lies between planes[k - 1] and planes[k]: a coefficient constant in layers normal to x"""
    return np.asarray(values)[np.sum(np.asarray(x)[..., None] > np.asarray(planes), axis=-1)]


# ------------------------------------------------------------------ the theta time stepper
def vec(op, a):
    return op.initialize_dof_vector().from_host(np.ascontiguousarray(a, dtype=np.float64))


def run_steps(mgamd, h, stepper, u0, n_steps, reltol, source=None):
    """n steps on the GPU; source(n) -> nodal values of f at t_n.  Returns the iterate and the CG iterations per step"""
    op = h.fine_operator
    u, its = vec(op, u0), []
    for n in range(n_steps):
        if source is None:
            it, _ = stepper.step(u, reltol=reltol)
        else:
            it, _ = stepper.step(u, vec(op, source(n)), vec(op, source(n + 1)), reltol=reltol)
        its.append(it)
    assert stepper.n_steps() == n_steps
    return u.to_host(), its


def oracle_steps(oracle, lv, precond, u0, theta, dt, n_steps, reltol, source=None):
    Mh, solve = ts.mass_matrix(lv), ts.pcg_solver(oracle, lv, precond, reltol)
    u, its = u0.copy(), []
    for n in range(n_steps):
        u, it = ts.theta_step(lv, u, None if source is None else source(n), None if source is None else source(n + 1), theta, dt, solve, Mh)
        its.append(it)
    return u, its


def linear_source(n_dofs, dt):
    f0 = np.sin(0.37 * np.arange(n_dofs)) + 0.25
    return lambda n: (1.0 + n * dt) * f0


# ------------------------------------------------------------------ random octrees
def random_mesh(oracle, seed, n_global, rounds, fraction):
    rng = np.random.default_rng(seed)
    leaves = oracle.refine_global({(0, 0, 0, 0)}, n_global)
    for _ in range(rounds):
        cells = sorted(leaves)
        # a random blob (cells near a random point) plus a sprinkle of single cells
        c = rng.random(3)
        centre = lambda cell: (np.array(cell[1:]) + 0.5) / (1 << cell[0])
        near = [cell for cell in cells if np.linalg.norm(centre(cell) - c) < 0.3 and rng.random() < 0.7]
        single = [cells[t] for t in rng.choice(len(cells), max(1, int(fraction * len(cells))), replace=False)]
        leaves = oracle.refine(leaves, list(set(near) | set(single)))
    return leaves


# ------------------------------------------------------------------ simulated ranks
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


def key_vector(keys, seed):
    """deterministic pseudo-random value per geometric DoF key: the same GLOBAL vector on every rank and in the oracle"""
    k = np.asarray(keys, dtype=np.int64)
    h = (k[:, 0] * 73856093) ^ (k[:, 1] * 19349663) ^ (k[:, 2] * 83492791) ^ (k[:, 3] * 2654435761) ^ (k[:, 4] * 97) ^ seed
    return np.sin(h.astype(np.float64) * 1e-3) + 0.25 * np.cos(h.astype(np.float64) * 7e-5)


# ------------------------------------------------------------------ the harness binary
BIN = os.path.join(ROOT, "dealii_multigrid_amd", "bin", "multigrid_throughput")
GOLDEN = os.path.join(ROOT, "tests", "golden")
# ref:multigrid_throughput.cc:2328-2335 (dim..n_dofs), :1488 (sub_comm_size), :1278-1283 (n_levels..throughput),
# :1381-1394 (stage times), :1396-1401 (transfer times); this project's additions come after them
REFERENCE_COLUMNS = ["dim", "n_cells", "n_cells_hn", "n_cells_n", "degree", "n_ref_global", "n_ref_local", "n_dofs", "sub_comm_size",
                     "n_levels", "n_iterations", "time", "time_cg", "throughput", "time_pre", "time_residuum", "time_res", "time_cs",
                     "time_pro", "time_edge_pro", "time_post", "time_to_mg", "time_to_global"]


def run_harness(*files):
    r = subprocess.run([BIN, *files], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def final_table(stdout):
    lines = stdout.rstrip().split("\n")
    start = max(i for i, l in enumerate(lines) if l.startswith("dim "))
    header = lines[start].split()
    return header, [dict(zip(header, l.split())) for l in lines[start + 1:] if l.strip()]


# ------------------------------------------------------------------ recorded vectors of the numpy oracle
def assert_recorded(lv, name, p=1):
    """A x, inv_diag and rhs_constant of the level lv (quadrant L=2, the oracle's own numbering) against problem `name` of
    tests/golden/physics_oracle_quadrant2.npz, recorded from levels that were built directly (tests/golden/README.md)"""
    g = np.load(os.path.join(GOLDEN, "physics_oracle_quadrant2.npz"))
    for what, v in (("Ax", lv.A @ g[f"p{p}/x"]), ("inv_diag", lv.inv_diag), ("rhs_constant", lv.rhs_constant)):
        ref = g[f"p{p}/{name}/{what}"]
        assert np.abs(v - ref).max() <= 1e-14 * np.abs(ref).max(), (name, what)
