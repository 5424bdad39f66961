"""Flagged refinement (Triangulation.refine, mgamd_tria_refine), the face-neighbour table of the error indicator and the marking
helper, on the host: against mgoracle.refine / mgoracle._find_leaf as cell sets."""
import ctypes as C

import numpy as np
import pytest

import physics_oracle as po
import random_mesh_physics as rm
from support import mesh, tria_of


def flagged(cells, flags):
    return [c for c, f in zip(cells, flags) if f]


def check_refine(mgamd, oracle, t, flags):
    """t.refine(flags) against mgoracle.refine: the cell set, the parent map, no old leaf split twice; returns the new mesh"""
    old = po.product_cells(t)
    fine, parent = t.refine(flags, return_parent=True)
    new = po.product_cells(fine)
    assert set(new) == oracle.refine(set(old), flagged(old, flags)) and len(new) == len(set(new)) == fine.n_cells
    assert parent.shape == (fine.n_cells,)
    splits = np.zeros(len(old), np.int64)
    for (l, i, j, k), par in zip(new, parent):
        ol, oi, oj, ok = old[par]
        s = l - ol
        assert 0 <= s <= 1, "an old leaf was split more than once"
        assert (i >> s, j >> s, k >> s) == (oi, oj, ok)
        splits[par] += 1
    assert set(np.unique(splits)) <= {1, 8}
    assert all(splits[t] == 8 for t in np.flatnonzero(flags))  # every flagged leaf is refined, by exactly one level
    return fine


def test_no_flag_and_all_flags(mgamd, oracle):
    t = mgamd.Triangulation("quadrant", 3)
    same = check_refine(mgamd, oracle, t, np.zeros(t.n_cells, np.uint8))
    assert po.product_cells(same) == po.product_cells(t)
    every = check_refine(mgamd, oracle, t, np.ones(t.n_cells, np.uint8))
    assert set(po.product_cells(every)) == oracle.refine_global(mesh("quadrant", 3), 1)
    u = mgamd.Triangulation("hypercube", 1)
    assert po.product_cells(check_refine(mgamd, oracle, u, np.ones(8))) == po.product_cells(mgamd.Triangulation("hypercube", 2))


def test_corner_cell_four_times_ripples(mgamd, oracle):
    t = mgamd.Triangulation("hypercube", 2)
    counts = [t.n_cells]
    for step in range(4):
        cells = po.product_cells(t)
        # the cell at the origin, then the corner cell of the deepest family that points away from the origin: its neighbours are
        # one level coarser, so every further step ripples
        corner = cells.index((2, 0, 0, 0)) if step == 0 else max(range(len(cells)), key=lambda c: cells[c])
        flags = np.zeros(t.n_cells, np.uint8)
        flags[corner] = 1
        t = check_refine(mgamd, oracle, t, flags)
        counts.append(t.n_cells)
    print("corner refinement, cells per step:", counts)
    assert t.n_levels == 7 and counts[2] - counts[1] > 7  # the ripple splits more than the flagged cell


@pytest.mark.parametrize("name", ["S", "M", "B", "R"])
def test_random_flags_on_random_octrees(mgamd, oracle, name):
    t = tria_of(mgamd, rm.leaves_of(oracle, name))
    rng = np.random.default_rng(17)
    check_refine(mgamd, oracle, t, rng.random(t.n_cells) < (0.02 if name == "R" else 0.15))


def test_coefficient_mask_and_robin_are_carried(mgamd, oracle):
    t = mgamd.Triangulation("quadrant", 3)
    assert not t.refine(np.zeros(t.n_cells)).has_coefficient()
    a = 0.5 + np.arange(t.n_cells) / 7.0
    t.set_coefficient(a)
    t.set_dirichlet_faces(0b111101)
    t.set_robin_coefficients({1: 2.5})
    rng = np.random.default_rng(3)
    fine, parent = t.refine(rng.random(t.n_cells) < 0.2, return_parent=True)
    assert fine.n_cells > t.n_cells and fine.has_coefficient()
    assert np.array_equal(fine.coefficient(), a[parent])
    assert fine.dirichlet_faces() == 0b111101 and np.array_equal(fine.robin_coefficients(), [0, 2.5, 0, 0, 0, 0])
    mgamd.DoFs(fine, 2)  # the refined mesh is one the level tables accept


def test_refusals(mgamd):
    t = mgamd.Triangulation("hypercube", 1)
    with pytest.raises(mgamd.MgamdError, match="flags is null"):
        t.refine(None)
    with pytest.raises(ValueError, match="flags for 8 cells"):
        t.refine(np.ones(7))
    # one corner refined down to the deepest level of the keys: a flag there is refused by name
    while t.n_levels < 15:
        lev, i, j, k, _ = t.cells()
        t = t.refine((lev == lev.max()) & (i == 0) & (j == 0) & (k == 0))
    lev = t.cells()[0]
    assert lev.max() == 14
    with pytest.raises(mgamd.MgamdError, match=r"flagged leaf \d+ \(level 14, 0, 0, 0\) is at the deepest level"):
        t.refine(lev == 14)
    lib = C.CDLL(mgamd._LIB_PATH)
    out = C.c_void_p()
    assert lib.mgamd_tria_refine(t._h, None, C.byref(out), None) == 3  # MGAMD_ERR_INVALID


@pytest.mark.parametrize("name", ["S", "M", "B", "R", "quadrant3", "hypercube0"])
def test_neighbour_table_agrees_with_find_leaf(mgamd, oracle, name):
    leaves = {"quadrant3": mesh("quadrant", 3), "hypercube0": mesh("hypercube", 0)}.get(name) or rm.leaves_of(oracle, name)
    t = tria_of(mgamd, leaves)
    cells = po.product_cells(t)
    code, nbr = t._face_neighbours()
    seen = set()
    for c, (l, i, j, k) in enumerate(cells):
        ijk = (i, j, k)
        for f in range(6):
            d, side = f >> 1, f & 1
            u, v = (1 if d == 0 else 0), (1 if d == 2 else 2)
            n = list(ijk)
            n[d] += 1 if side else -1
            seen.add(int(code[c, f]))
            if not 0 <= n[d] < (1 << l):
                assert code[c, f] == 0
                continue
            nb = oracle._find_leaf(leaves, l, *n)
            if nb is None:
                assert code[c, f] == 6
                for s in range(4):
                    m = [0, 0, 0]
                    m[d], m[u], m[v] = 2 * n[d] + (0 if side else 1), 2 * ijk[u] + (s & 1), 2 * ijk[v] + (s >> 1)
                    assert cells[nbr[c, f, s]] == oracle._find_leaf(leaves, l + 1, *m) == (l + 1, *m)
            else:
                assert cells[nbr[c, f, 0]] == nb
                assert code[c, f] == (1 if nb[0] == l else 2 + (ijk[u] & 1) + 2 * (ijk[v] & 1))
    if name in ("M", "B", "R", "quadrant3"):
        assert seen == set(range(7))  # every code occurs


def test_mark_maximum(mgamd):
    assert mgamd.mark_maximum(np.zeros(5), 0.5).tolist() == [0] * 5  # nothing to refine: nothing flagged
    assert mgamd.mark_maximum([], 0.5).tolist() == []
    eta = np.array([1.0, 4.0, 2.0, 4.0, 1.9999999999999998, 0.0])
    assert mgamd.mark_maximum(eta, 0.5).tolist() == [0, 1, 1, 1, 0, 0]  # the ties stay together; >= includes the threshold itself
    assert mgamd.mark_maximum(eta, 1.0).tolist() == [0, 1, 0, 1, 0, 0]
    assert mgamd.mark_maximum(eta, 0.0).tolist() == [1] * 6
    assert mgamd.mark_maximum(eta, 0.5).dtype == np.uint8
    assert mgamd.mark_maximum([1.0, np.nan, 3.0], 0.5).tolist() == [0, 0, 0]  # an eta that is not a number marks nothing
