"""Test-side oracle of the shifted operator A = K + sigma M (weak form of -Laplace u + sigma u): pure numpy/scipy, built from
the PUBLIC pieces of oracle/mgoracle.py, which is not edited.  Not a test module.

level_class(oracle, sigma) subclasses mgoracle.Level: after the parent's assembly it forms the mass matrix
M = sum over cells of h^3 kron(fe.M, fe.M, fe.M) on cell_dofs and sets  Kraw <- Kraw + sigma M,  A <- C^T Kraw C + I on the
constrained rows,  inv_diag with the 1e-10 guard.  Everything else of a Level (rhs_function's lifting through Kraw, distribute,
the constraints) follows.  Numbering goes through the DoF keys, as in conftest.oracle_level.

build_hierarchy mirrors mgoracle.build_hierarchy (create_mesh, coarsening_sequence, build_transfer) with that class; transfers do
not depend on sigma.  patched(monkeypatch, oracle, sigma) substitutes the class inside mgoracle for the duration of one test, for
code that calls mgoracle.build_hierarchy itself; mgoracle.Level is never assigned globally.

reshift(level, sigma) gives the same level for another sigma without repeating the constraint search (a shallow copy whose
matrices are formed anew); reshift_hierarchy does it for a list of levels.
"""
import copy

import numpy as np
import scipy.sparse as sp


def level_class(oracle, sigma):
    class HelmholtzLevel(oracle.Level):
        mass_coefficient = float(sigma)

        def _assemble(self):
            super()._assemble()
            fe, nloc = self.fe, (self.p + 1) ** 3
            Mc = np.kron(np.kron(fe.M, fe.M), fe.M)
            rows = np.repeat(self.cell_dofs, nloc, axis=1).ravel()
            cols = np.tile(self.cell_dofs, (1, nloc)).ravel()
            hs = np.array([2.0 / (1 << c[0]) for c in self.cells])
            vals = ((hs ** 3)[:, None] * Mc.ravel()[None, :]).ravel()
            self.Mraw = sp.coo_matrix((vals, (rows, cols)), shape=(self.n, self.n)).tocsr()
            self.K0raw = self.Kraw
            _shift(self, self.mass_coefficient)

    return HelmholtzLevel


def _shift(lv, sigma):
    lv.mass_coefficient = float(sigma)
    lv.Kraw = (lv.K0raw + lv.mass_coefficient * lv.Mraw).tocsr()
    A = (lv.C.T @ lv.Kraw @ lv.C).tocsr()
    lv.A = (A + sp.diags(lv.constrained.astype(float))).tocsr()
    d = lv.A.diagonal().copy()
    lv.inv_diag = np.where(np.abs(d) > 1e-10, 1.0 / d, 1.0)


def reshift(lv, sigma):
    """the level lv (a HelmholtzLevel) for another sigma; lv itself is left unchanged"""
    out = copy.copy(lv)
    out.__dict__.pop("_rounded", None)
    _shift(out, sigma)
    return out


def reshift_hierarchy(levels, sigma):
    return [reshift(lv, sigma) for lv in levels]


def _renumber(lv, keys):
    ext = {tuple(int(v) for v in k): i for i, k in enumerate(keys)}
    assert len(ext) == lv.n, (len(ext), lv.n)
    perm = np.array([ext[tuple(int(v) for v in k)] for k in lv.keys], dtype=np.int64)  # old -> new
    inv = np.argsort(perm)
    Q = sp.csr_matrix((np.ones(lv.n), (perm, np.arange(lv.n))), shape=(lv.n, lv.n))
    out = copy.copy(lv)
    out.__dict__.pop("_rounded", None)
    out.cell_dofs = perm[lv.cell_dofs]
    out.keys = [lv.keys[o] for o in inv]
    out.key_to_dof = {k: i for i, k in enumerate(out.keys)}
    for name in ("dirichlet", "hanging", "constrained", "rhs_constant", "inv_diag"):
        setattr(out, name, getattr(lv, name)[inv])
    for name in ("Ch", "C", "Kraw", "K0raw", "Mraw", "A"):
        setattr(out, name, (Q @ getattr(lv, name) @ Q.T).tocsr())
    return out, Q


def renumber(lv, keys):
    """the level lv (a HelmholtzLevel) in another numbering of the same space, `keys` being the DoF keys in the new order: what
    level_class(...)(mesh, p, numbering_keys=keys) builds, without repeating the constraint search.  Every table of the level
    (cell_dofs, keys, the masks, C, Ch, the raw matrices, A, inv_diag, rhs_constant) is permuted; lv itself is left unchanged"""
    return _renumber(lv, keys)[0]


def renumber_hierarchy(levels, P, keys):
    """renumber for every level, keys[l] the new order of level l, and the transfers between them permuted to match"""
    new, Q = zip(*[_renumber(lv, k) for lv, k in zip(levels, keys)])
    return list(new), [None] + [(Q[l] @ P[l] @ Q[l - 1].T).tocsr() for l in range(1, len(new))]


def level(oracle, sigma, dofs, geometry, n_ref, degree, mesh=None):
    """one Level of K + sigma M numbered like the product's `dofs`"""
    if mesh is None:
        mesh = oracle.create_mesh(geometry, n_ref)
    return level_class(oracle, sigma)(mesh, degree, numbering_keys=dofs.keys())


def level_plan(oracle, geometry, n_ref_global, degree, mg_type):
    """(meshes, degrees) coarse -> fine, as mgoracle.build_hierarchy chooses them"""
    return level_plan_on(oracle, oracle.create_mesh(geometry, n_ref_global), degree, mg_type)


def level_plan_on(oracle, fine, degree, mg_type):
    """the same for a caller's set of leaves (level, i, j, k) as the finest mesh"""
    pseq = [degree]
    while pseq[-1] > 1:
        pseq.append(max(pseq[-1] // 2, 1))
    pseq = pseq[::-1]
    if mg_type == "HMG-global":
        meshes = oracle.coarsening_sequence(fine)
        return meshes, [degree] * len(meshes)
    if mg_type == "PMG":
        return [fine] * len(pseq), pseq
    if mg_type == "HPMG":
        hm = oracle.coarsening_sequence(fine)
        return hm + [fine] * (len(pseq) - 1), [pseq[0]] * len(hm) + pseq[1:]
    raise ValueError(mg_type)


def build_hierarchy(oracle, sigma, geometry, n_ref_global, degree, mg_type="HMG-global", numbering_keys=None):
    """levels (coarse -> fine) of K + sigma M and the transfers between them"""
    cls = level_class(oracle, sigma)
    meshes, degs = level_plan(oracle, geometry, n_ref_global, degree, mg_type)
    levels = [cls(m, p, numbering_keys[l] if numbering_keys is not None else None) for l, (m, p) in enumerate(zip(meshes, degs))]
    P = [None] + [oracle.build_transfer(levels[l], levels[l - 1]) for l in range(1, len(levels))]
    return levels, P


def patched(monkeypatch, oracle, sigma):
    """mgoracle.build_hierarchy builds HelmholtzLevel objects until the test's monkeypatch is undone"""
    monkeypatch.setattr(oracle, "Level", level_class(oracle, sigma))


def gaussian_load(oracle, sigma):
    """f of the manufactured Gaussian solution: -Laplace u_g + sigma u_g"""
    return lambda x, y, z: oracle.gaussian_rhs(x, y, z) + sigma * oracle.gaussian_solution(x, y, z)
