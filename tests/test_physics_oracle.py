"""oracle/physics_oracle.py on the CPU: the one statement of -div(a grad u) + sigma u with per-face conditions against
  * vectors recorded from the layered modules it replaced (tests/golden/physics_oracle_quadrant2.npz, see tests/golden/README.md):
    every vector to <= 1e-14 relative in the maximum norm, the project's figure for "the same up to rounding";
  * mgoracle.Level itself for the default problem: no difference at all;
  * itself under a change of ONE field of the problem on a level with convective faces: the other terms stay in A (the layered
    shortcuts lost the face term there: |dA| / |A| of 0.125, 0.125 and 0.024 on quadrant L=2 p=2 R1);
  * itself under a seeded renumbering: Q A Q^T to <= 1e-15 |A|.
Quadrant L=2: 15 cells; p = 1: 46 DoFs, 12 hanging, 2 of them on the convective face x = -1 of R1; p = 2: 235 DoFs, 54 and 6."""
import dataclasses
import os

import numpy as np
import pytest

import physics_oracle as po
from conftest import ROOT

Q = (1.0, -2.0, 3.0, 0.0, 0.5, 0.0)
PROBLEMS = dict(  # name -> (sigma, field, mask, beta)
    default=(0.0, None, po.ALL, (0.0,) * 6),
    sigma=(7.5, None, po.ALL, (0.0,) * 6),
    octants_sigma=(7.5, "octants", po.ALL, (0.0,) * 6),
    per_cell=(0.0, "per_cell", po.ALL, (0.0,) * 6),
    M1=(0.0, None, po.M1, (0.0,) * 6),
    M2=(0.0, None, po.M2, (0.0,) * 6),
    M0_sigma=(7.5, None, po.M0, (0.0,) * 6),
    R1=(0.0, None, *po.R1),
    R2=(0.0, None, *po.R2),
    R1_sigma_octants=(7.5, "octants", *po.R1),
)
CASES = [(1, name) for name in PROBLEMS] + [(2, "R1_sigma_octants")]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "physics_oracle_quadrant2.npz"))


@pytest.fixture(scope="module")
def spaces(oracle):
    mesh = oracle.create_mesh("quadrant", 2)
    return {p: po.Space(mesh, p) for p in (1, 2)}


def problem(name, mesh):
    sigma, field, mask, beta = PROBLEMS[name]
    return po.Problem(sigma, None if field is None else po.field_on(mesh, po.FIELDS[field]), mask, beta)


def same(a, ref):
    return np.abs(a - ref).max() <= 1e-14 * np.abs(ref).max()


@pytest.mark.parametrize("p,name", CASES)
def test_recorded_vectors(oracle, golden, spaces, p, name):
    space = spaces[p]
    lv = po.Level(space, problem(name, space.leaves))
    x, g, t = golden[f"p{p}/x"], golden[f"p{p}/g"], f"p{p}/{name}/"
    assert (lv.n, int(lv.hanging.sum()), len(lv.cells)) == {1: (46, 12, 15), 2: (235, 54, 15)}[p]
    got = dict(Ax=lv.A @ x, inv_diag=lv.inv_diag, rhs_constant=lv.rhs_constant,
               rhs_gaussian=lv.rhs_function(po.gaussian_load(lv.mass_coefficient), oracle.gaussian_solution),
               Mhx=lv.C.T @ (lv.Mraw @ (lv.C @ x)), flux_load=po.flux_load(lv, Q), lift_mass=po.lift(lv, g, True),
               lift_no_mass=po.lift(lv, g, False), distribute_values=po.distribute_values(lv, x, g))
    for what, v in got.items():
        ref = golden[t + what]
        assert ref.shape == v.shape, what  # (a recorded zero vector, as the flux load under ALL, has to be met exactly)
        assert same(v, ref), (what, np.abs(v - ref).max() / np.abs(ref).max())


def test_convective_face_of_R1_carries_hanging_nodes(spaces):
    for p, n in ((1, 2), (2, 6)):
        lv = po.Level(spaces[p], po.Problem(0.0, None, *po.R1))
        on_face = np.array([k[0] == 0 for k in lv.keys])
        assert int((lv.hanging & on_face).sum()) == n and abs(lv.Braw[lv.hanging & on_face]).sum() > 0


@pytest.mark.parametrize("name", ["default", "M1"])
def test_recorded_transfer(oracle, golden, name):
    meshes = oracle.coarsening_sequence(oracle.create_mesh("quadrant", 2))
    assert [len(m) for m in meshes[-2:]] == [8, 15]
    levels, P = po.build_hierarchy_on(problem(name, None), meshes[-2:], [1, 1])
    t = f"transfer/{name}/"
    assert same(P[1] @ golden[t + "xc"], golden[t + "P_xc"]) and same(P[1].T @ golden[t + "xf"], golden[t + "PT_xf"])


@pytest.mark.parametrize("p", [1, 2])
def test_default_problem_is_mgoracle_level(oracle, spaces, p):
    lv, ref = po.Level(spaces[p]), oracle.Level(spaces[p].leaves, p)
    assert abs(lv.A - ref.A).max() == 0
    assert np.abs(lv.inv_diag - ref.inv_diag).max() == 0 and np.abs(lv.rhs_constant - ref.rhs_constant).max() == 0
    assert abs(lv.C - ref.C).max() == 0 and np.array_equal(lv.constrained, ref.constrained) and lv.Braw.nnz == 0


def test_one_field_changes_one_term(spaces):
    """on the R1 level of p = 2: another sigma adds (sigma2 - sigma1) C^T Mraw C and nothing else; another coefficient or another
    mask compatible with beta leaves C^T Braw C inside A"""
    space = spaces[2]
    r1 = po.Problem(1.25, None, *po.R1)
    lv = po.Level(space, r1)
    face = lambda l: l.C.T @ l.Braw @ l.C  # noqa: E731
    assert abs(face(lv)).max() > 0.01 * abs(lv.A).max()
    s2 = po.Level(space, dataclasses.replace(r1, sigma=7.5))
    assert abs(s2.A - lv.A - (7.5 - 1.25) * (lv.C.T @ lv.Mraw @ lv.C)).max() <= 1e-14 * abs(lv.A).max()
    co = po.Level(space, dataclasses.replace(r1, coefficient=po.field_on(space.leaves, po.octants)))
    plain = po.Level(space, dataclasses.replace(r1, coefficient=co.coefficient, robin=(0.0,) * 6))
    assert abs(co.A - plain.A - face(co)).max() <= 1e-14 * abs(co.A).max() and abs(face(co) - face(lv)).max() == 0
    assert abs(co.A - lv.A).max() > 0.01 * abs(lv.A).max()
    mk = po.Level(space, dataclasses.replace(r1, dirichlet_faces=0b100010))  # z = +1 as well: no beta there
    plain = po.Level(space, dataclasses.replace(r1, dirichlet_faces=0b100010, robin=(0.0,) * 6))
    assert mk.dirichlet.sum() > lv.dirichlet.sum()
    assert abs(mk.A - plain.A - face(mk)).max() <= 1e-14 * abs(mk.A).max() and abs(face(mk)).max() > 0.01 * abs(mk.A).max()
    with pytest.raises(AssertionError):
        dataclasses.replace(r1, dirichlet_faces=po.M1)  # beta > 0 on a Dirichlet face


@pytest.mark.parametrize("p", [1, 2])
def test_renumbered_space(spaces, p):
    space = spaces[p]
    order = np.random.default_rng(17).permutation(space.n)
    keys = [space.keys[o] for o in order]
    other, Qm = space.renumbered(keys)
    assert other.keys == keys and np.array_equal(other.cell_dofs, np.argsort(order)[space.cell_dofs])
    direct = po.Space(space.leaves, p, numbering_keys=keys)
    for name in PROBLEMS:
        pr = problem(name, space.leaves)
        a, b, c = po.Level(space, pr), po.Level(other, pr), po.Level(direct, pr)
        assert abs(b.A - Qm @ a.A @ Qm.T).max() <= 1e-15 * abs(a.A).max()
        assert abs(b.A - c.A).max() <= 1e-15 * abs(a.A).max()
        assert np.array_equal(b.constrained, Qm @ a.constrained) and np.array_equal(b.constrained, c.constrained)
        assert same(b.rhs_constant, Qm @ a.rhs_constant) and same(b.inv_diag, Qm @ a.inv_diag)
