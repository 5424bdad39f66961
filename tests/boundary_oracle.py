"""Test-side oracle of per-face boundary conditions: pure numpy/scipy on top of tests/helmholtz_oracle.py, tests/coefficient_oracle.py
and the PUBLIC pieces of oracle/mgoracle.py, none of which is edited.  Not a test module.

Faces of the cube [-1, 1]^3 are numbered f = 2 axis + side (0: x = -1, 1: x = +1, ... 5: z = +1); bit f of a mask set means face f
is Dirichlet, clear means natural.  A DoF is Dirichlet iff it lies on at least one Dirichlet face.

level_class(oracle, sigma, mask, coeff=None) subclasses the sigma / coefficient level and overrides _constraints: the parent's search
first (mgoracle.Level._constraints: Dirichlet on the whole boundary, the hanging-node search), then dirichlet, constrained and C are
re-masked by face.  _assemble follows with the re-masked C.

remask(level, mask) gives an existing level (a HelmholtzLevel or CoefficientLevel in any numbering) another mask without repeating
the constraint search, in the manner of helmholtz_oracle.reshift: a shallow copy whose dirichlet, constrained, C, A, inv_diag and
rhs_constant are formed anew.  The transfers depend on the mask (build_transfer reads fine.constrained and coarse.C): transfers()
builds them for a list of re-masked levels.

flux_load(level, q) is the boundary load of one constant flux per face, written independently of the product: per boundary cell
face q h^2 m (x) m on the face nodes, then C^T, then constrained rows 0.
"""
import copy

import numpy as np
import scipy.sparse as sp

import coefficient_oracle as co
import helmholtz_oracle as ho

ALL = 0x3F
M1 = 0b000001  # only x = -1 is Dirichlet
M2 = 0b101010  # the three "+" faces are Dirichlet
M0 = 0         # no Dirichlet face (with sigma > 0)


def dirichlet_by_face(oracle, keys, p, mask):
    """bool per DoF: the key lies on a face whose bit is set in mask"""
    top = p << oracle.LMAX
    out = np.zeros(len(keys), dtype=bool)
    for d, key in enumerate(keys):
        out[d] = any((key[t] == 0 and (mask >> (2 * t)) & 1) or (key[t] == top and (mask >> (2 * t + 1)) & 1) for t in range(3))
    return out


def _apply_mask(oracle, lv, mask):
    lv.dirichlet_faces = int(mask)
    lv.dirichlet = dirichlet_by_face(oracle, lv.keys, lv.p, mask)
    lv.constrained = lv.dirichlet | lv.hanging
    lv.C = (lv.Ch @ sp.diags((~lv.dirichlet).astype(float))).tocsr()


def level_class(oracle, sigma, mask, coeff=None):
    base = ho.level_class(oracle, sigma) if coeff is None else co.level_class(oracle, sigma, coeff)

    class BoundaryLevel(base):
        def _constraints(self):
            super()._constraints()
            _apply_mask(oracle, self, mask)

    return BoundaryLevel


def raw_load(lv):
    """sum over cells of h^3 m (x) m (x) m on cell_dofs: the load of f == 1 before any constraint"""
    mc = np.kron(np.kron(lv.fe.m, lv.fe.m), lv.fe.m)
    hs = np.array([2.0 / (1 << c[0]) for c in lv.cells])
    b = np.zeros(lv.n)
    np.add.at(b, lv.cell_dofs.ravel(), ((hs ** 3)[:, None] * mc[None, :]).ravel())
    return b


def remask(oracle, lv, mask, sigma=None):
    """the level lv for another mask (and sigma, default lv's); lv itself is left unchanged"""
    out = copy.copy(lv)
    out.__dict__.pop("_rounded", None)
    _apply_mask(oracle, out, mask)
    ho._shift(out, lv.mass_coefficient if sigma is None else sigma)
    b = out.C.T @ raw_load(out)
    b[out.constrained] = 0.0
    out.rhs_constant = b
    return out


def remask_hierarchy(oracle, levels, mask, sigma=None):
    levels = [remask(oracle, lv, mask, sigma) for lv in levels]
    return levels, transfers(oracle, levels)


def transfers(oracle, levels):
    return [None] + [oracle.build_transfer(levels[l], levels[l - 1]) for l in range(1, len(levels))]


def natural_transfers(oracle, levels):
    """the transfers of the levels under mask 0 (no Dirichlet DoF), from which mask_transfers derives those of every mask; the
    levels' matrices are not formed"""
    nat = []
    for lv in levels:
        out = copy.copy(lv)
        _apply_mask(oracle, out, 0)
        nat.append(out)
    return transfers(oracle, nat)


def mask_transfers(P0, levels):
    """the transfers of re-masked levels from those of mask 0, without walking the cells again.  build_transfer returns
    diag(w) Praw C_c with w = 0 on constrained fine rows and 1 / touch elsewhere, and C_c = Ch_c diag(not dirichlet_c).  Under mask
    0 constrained means hanging, so  P0 = diag(w0) Praw Ch_c;  a mask adds the Dirichlet DoFs to both sets:
    P = diag(not dirichlet_f) P0 diag(not dirichlet_c), products with 0 and 1 only.  test_boundary_host.py holds it against
    build_transfer on re-masked levels."""
    return [None] + [(sp.diags((~levels[l].dirichlet).astype(float)) @ P0[l] @ sp.diags((~levels[l - 1].dirichlet).astype(float))).tocsr()
                     for l in range(1, len(levels))]


def flux_load(lv, q):
    """b_i = sum_f q[f] int_{face f} phi_i through the hanging-node constraints; constrained rows 0"""
    p, n1, m = lv.p, lv.p + 1, lv.fe.m
    stride = (1, n1, n1 * n1)  # cell_dofs: x fastest
    F = np.zeros(lv.n)
    for ci, (l, i, j, k) in enumerate(lv.cells):
        h, ijk, last = 2.0 / (1 << l), (i, j, k), (1 << l) - 1
        for f in range(6):
            d, side = f >> 1, f & 1
            if q[f] == 0.0 or ijk[d] != (last if side else 0):
                continue
            e, g = (d + 1) % 3, (d + 2) % 3
            for ae in range(n1):
                for ag in range(n1):
                    F[lv.cell_dofs[ci, side * p * stride[d] + ae * stride[e] + ag * stride[g]]] += q[f] * h * h * m[ae] * m[ag]
    b = lv.C.T @ F
    b[lv.constrained] = 0.0
    return b
