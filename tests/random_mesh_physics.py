"""What is specific to the random octrees of test_random_meshes_host.py, test_gpu_random_meshes_physics.py and the random-octree cases
of the boundary, Robin and geometry tests: the four meshes and the check that a coefficient field gives their tables slots that
differ.  Not a test module.

Meshes (support.random_mesh arguments: seed, global refinements, rounds, sprinkle fraction):
  S  (8, 1, 2, 0.1)     50 cells, levels 1-3    degrees 5, 6, 7
  M  (5, 2, 2, 0.05)   344 cells, levels 2-4    degrees 1 ... 4
  B  (8, 3, 1, 0.02)   757 cells, levels 3-4    degrees 1, 2, 3; four 4^3 bricks survive at p = 2 (seed 2 leaves one)
  R  (41, 4, 1, 0.004) 16^3 base; two whole octants stay unrefined (seed 4 leaves one): at p = 1 two plain 8^3 bricks with different
     a share a workgroup of the 9-point lattice kernel and its per-slot D^-1 table.  Plus ONE aligned 4^3 block of level-4 cells refined as a whole (rim_block): its 512 children are
     an 8^3 brick of level-5 cells with whole hanging faces, a CONSTRAINED brick at p = 1.  random_mesh alone cannot give one: its
     blob takes each cell with probability 0.7, so no 4^3 block is refined completely, whatever the seed.

The numpy levels on these leaves come from support.oracle_level_on / oracle_hierarchy_on like every other: one constraint search
per (mesh, degree) in the oracle's own numbering, permuted into the numbering of the product's tables (which changes with the
field because the slots do), then formed.  test_random_meshes_host.py holds that against a space built directly."""
import physics_oracle as po
from support import consecutive, random_mesh, slot_groups, slots_of, tria_of

MESHES = dict(S=(8, 1, 2, 0.1), M=(5, 2, 2, 0.05), B=(8, 3, 1, 0.02), R=(41, 4, 1, 0.004))

_leaves = {}


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
        plain_t = tria_of(mgamd, set(po.product_cells(t)))
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


def level_plan(oracle, name, degree, mg_type):
    return po.level_plan_on(leaves_of(oracle, name), degree, mg_type)
