"""Shared by test_random_meshes_host.py and test_gpu_random_meshes_physics.py: the random octrees, the product's meshes with a
per-brick coefficient field on them, and the numpy hierarchies of A = K_a + sigma M on the same leaves.  Not a test module.

Meshes (test_gpu_random_meshes.random_mesh arguments: seed, global refinements, rounds, sprinkle fraction):
  S  (8, 1, 2, 0.1)     50 cells, levels 1-3    degrees 5, 6, 7
  M  (5, 2, 2, 0.05)   344 cells, levels 2-4    degrees 1 ... 4
  B  (8, 3, 1, 0.02)   757 cells, levels 3-4    degrees 1, 2, 3; four 4^3 bricks survive at p = 2 (seed 2 leaves one)
  R  (41, 4, 1, 0.004) 16^3 base; two whole octants stay unrefined (seed 4 leaves one): at p = 1 two plain 8^3 bricks with different
     a share a workgroup of the 9-point lattice kernel and its per-slot D^-1 table.  Plus ONE aligned 4^3 block of level-4 cells refined as a whole (rim_block): its 512 children are
     an 8^3 brick of level-5 cells with whole hanging faces, a CONSTRAINED brick at p = 1.  random_mesh alone cannot give one: its
     blob takes each cell with probability 0.7, so no 4^3 block is refined completely, whatever the seed.

Every numpy level is built ONCE per (mesh, degree), at sigma = 0 without a coefficient and in the oracle's own numbering (the
constraint search is what costs); a case permutes it into the numbering of the product's tables, which changes with the field
because the slots do (helmholtz_oracle.renumber), puts its coefficient in (coefficient_oracle.with_coefficient) and shifts.
test_random_meshes_host.py holds that shortcut against a level built directly."""
import numpy as np

import coefficient_oracle as co
import helmholtz_oracle as ho
from test_gpu_random_meshes import random_mesh

MESHES = dict(S=(8, 1, 2, 0.1), M=(5, 2, 2, 0.05), B=(8, 3, 1, 0.02), R=(41, 4, 1, 0.004))

_leaves, _levels, _transfers = {}, {}, {}


def rim_block(leaves, level=4):
    """the 64 cells of the first aligned 4^3 block of `level` (blocks in descending order) that is unrefined together with the
    layer of cells around it: refined as a whole, its children form one brick whose hanging entities are whole faces and edges"""
    n = 1 << level
    for b in [(x, y, z) for x in range(n // 4 - 1, -1, -1) for y in range(n // 4 - 1, -1, -1) for z in range(n // 4 - 1, -1, -1)]:
        hood = [(level, 4 * b[0] + x, 4 * b[1] + y, 4 * b[2] + z) for x in range(-1, 5) for y in range(-1, 5) for z in range(-1, 5)]
        if all(c in leaves for c in hood if all(0 <= v < n for v in c[1:])):
            return [(level, 4 * b[0] + x, 4 * b[1] + y, 4 * b[2] + z) for x in range(4) for y in range(4) for z in range(4)]
    raise ValueError("no unrefined 4^3 block")


def leaves_of(oracle, name):
    if name not in _leaves:
        leaves = random_mesh(oracle, *MESHES[name])
        if name == "R":
            leaves = oracle.refine(leaves, rim_block(leaves))
        _leaves[name] = leaves
    return _leaves[name]


def tria_of(mgamd, leaves, field=None):
    """the product's mesh on the leaves, with the field FIELDS[field] set on it if one is named"""
    arr = np.array(sorted(leaves), dtype=np.int64)
    t = mgamd.Triangulation.from_leaves(arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3])
    assert t.n_cells == len(leaves)
    if field is not None:
        t.set_coefficient(co.product_values(t, co.field_on(co.product_cells(t), co.FIELDS[field])))
    return t


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


def describe(groups):
    return " | ".join(f"B={b}: {len(sl)} slots, {len(set(v[0] for v in sl))} a, consecutive pairs with another a {consecutive(sl, 0)}, "
                      f"another level {consecutive(sl, 1)}" for b, sl in groups)


def assert_slots_differ(mgamd, name, degree, field, d, t):
    """the tables d (max_brick 0) of the finest mesh t of mesh `name` under `field` hold what the case is there for: slots that share
    a workgroup and differ in a and in h.  Computed from the tables, printed, asserted.

    Two conditions are stated for the tables as they are, not as one might expect them:
      * p = 1: LevelTables::build leaves the 2^3 and 4^3 bricks to the single-cell cluster kernel, so there is no B = 2 or B = 4
        group on any mesh; the slots that share a workgroup there (pair and cluster launches) are the single cells, and the
        per_family conditions are asked of the B = 1 group.
      * a field that splits bricks (per_cell), like max_brick = 1, leaves single cells only: "B = 1 and B = 2 slots" is asked of
        the mesh's plain tables at p >= 2."""
    groups = slot_groups(d, t)
    print(f"{name} p={degree} {field}: n_hanging {d.info.n_hanging}; {describe(groups)}")
    assert d.info.n_hanging > 0
    if degree >= 2:
        plain_t = tria_of(mgamd, set(co.product_cells(t)))
        plain = slot_groups(mgamd.DoFs(plain_t, degree, 0), plain_t)
        assert slots_of(plain, 1) and slots_of(plain, 2)
    if field == "per_family":
        sl = slots_of(groups, 2 if degree >= 2 else 1)
        if name == "S":
            assert len(sl) >= 3 and len(set(v[0] for v in sl)) >= 3 and len(set(v[1] for v in sl)) >= 2
        else:
            assert len(sl) >= 20 and len(set(v[0] for v in sl)) >= 10 and consecutive(sl, 0) >= 1 and consecutive(sl, 1) >= 1
    if field == "per_block4" and degree >= 2:
        assert len(set(v[0] for v in slots_of(groups, 4))) >= 2
    if name == "R" and field in ("uniform", "octants") and degree == 1:
        big = [v for b, sl in groups if b >= 8 for v in sl]
        assert any(v[0] != 1.0 and v[2] for v in big), big  # a constrained rim brick with a != 1
        if field == "octants":  # two plain bricks of ONE group (one launch, several slots per workgroup) with different a
            assert any(b >= 8 and len(set(v[0] for v in sl)) >= 2 for b, sl in groups)
    return groups


# ------------------------------------------------------------------ numpy hierarchies
def level_plan(oracle, name, degree, mg_type):
    return ho.level_plan_on(oracle, leaves_of(oracle, name), degree, mg_type)


def base_hierarchy(oracle, name, degree, mg_type):
    """(levels, P, meshes) at sigma = 0 without a coefficient in the oracle's own numbering; levels and transfers are shared
    between the hierarchy types through (mesh, degree)"""
    meshes, degs = level_plan(oracle, name, degree, mg_type)
    cls = ho.level_class(oracle, 0.0)
    levels = []
    for m, p in zip(meshes, degs):
        tag = (name, len(m), p)
        if tag not in _levels:
            _levels[tag] = cls(m, p)
        levels.append(_levels[tag])
    P = [None]
    for l in range(1, len(levels)):
        tag = (name, len(meshes[l]), degs[l], len(meshes[l - 1]), degs[l - 1])
        if tag not in _transfers:
            _transfers[tag] = oracle.build_transfer(levels[l], levels[l - 1])
        P.append(_transfers[tag])
    return levels, P, meshes


def level_coefficients(oracle, name, field, meshes):
    """{cell: a} per mesh: the field on the finest mesh, restrict_field of it on every other; None without a field"""
    if field is None:
        return [None] * len(meshes)
    finest = co.field_on(leaves_of(oracle, name), co.FIELDS[field])
    return [finest if len(m) == len(finest) else co.restrict_field(finest, m) for m in meshes]


def oracle_level(oracle, name, degree, field, sigma, keys):
    """the finest level alone, numbered by keys = dofs.keys()"""
    lv = ho.renumber(base_hierarchy(oracle, name, degree, "PMG" if degree == 1 else "HMG-global")[0][-1], keys)
    c = level_coefficients(oracle, name, field, [leaves_of(oracle, name)])[0]
    return ho.reshift(lv, sigma) if c is None else co.with_coefficient(lv, c, sigma)


def oracle_hierarchy(oracle, name, degree, mg_type, field, sigma, keys):
    """(levels, P) of K_a + sigma M numbered like the product's level tables, keys[l] = dofs[l].keys()"""
    base, P, meshes = base_hierarchy(oracle, name, degree, mg_type)
    levels, P = ho.renumber_hierarchy(base, P, keys)
    coeffs = level_coefficients(oracle, name, field, meshes)
    return [ho.reshift(lv, sigma) if c is None else co.with_coefficient(lv, c, sigma) for lv, c in zip(levels, coeffs)], P
