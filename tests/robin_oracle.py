"""Test-side oracle of convective (Robin) faces  a grad u . n + beta_f (u - u_ext) = 0:  pure numpy/scipy on top of
tests/boundary_oracle.py (and through it helmholtz_oracle.py, coefficient_oracle.py and the PUBLIC pieces of oracle/mgoracle.py), none
of which is edited.  Not a test module.

The operator is  A = A_mask + U C^T B C U,  B = sum_f beta_f B_f the surface mass matrices of the convective faces and U the
projector on the unconstrained DoFs.  face_matrix(level, beta) assembles B from the level's own cell_dofs and the 1D mass matrix
fe.M, entry by entry over the boundary cell faces, in the manner of boundary_oracle.flux_load and independently of the product:
per boundary cell face  beta h^2 M (x) M  on the face nodes.

robin(level, beta) gives an existing level (re-masked, shifted, with or without a coefficient, in any numbering) the face term: a
shallow copy whose Kraw, A and inv_diag are formed anew; the level itself is left unchanged.  The transfers do not depend on beta.

The two setups of the tests:  R1 = only x = +1 is Dirichlet, beta = 2.5 on x = -1 (on quadrant the refined corner touches it: a
convective face with hanging nodes) and 0.75 on y = +1 (none);  R2 = no Dirichlet face, sigma = 0, beta = 1.5 on y = -1 and 4 on
z = +1: regular only because of the convective faces.
"""
import copy

import numpy as np
import scipy.sparse as sp

import boundary_oracle as bo

R1 = (0b000010, (2.5, 0.0, 0.0, 0.75, 0.0, 0.0))
R2 = (0, (0.0, 0.0, 1.5, 0.0, 0.0, 4.0))


def face_matrix(lv, beta):
    """B = sum_f beta[f] int_{face f} phi_i phi_j over ALL DoFs of the level's cells (before any constraint), sparse"""
    p, n1, M = lv.p, lv.p + 1, np.asarray(lv.fe.M)
    stride = (1, n1, n1 * n1)  # cell_dofs: x fastest
    rows, cols, vals = [], [], []
    for ci, (l, i, j, k) in enumerate(lv.cells):
        h, ijk, last = 2.0 / (1 << l), (i, j, k), (1 << l) - 1
        for f in range(6):
            d, side = f >> 1, f & 1
            if beta[f] == 0.0 or ijk[d] != (last if side else 0):
                continue
            e, g = (d + 1) % 3, (d + 2) % 3
            for ae in range(n1):
                for ag in range(n1):
                    r = lv.cell_dofs[ci, side * p * stride[d] + ae * stride[e] + ag * stride[g]]
                    for be in range(n1):
                        for bg in range(n1):
                            rows.append(r)
                            cols.append(lv.cell_dofs[ci, side * p * stride[d] + be * stride[e] + bg * stride[g]])
                            vals.append(beta[f] * h * h * M[ae, be] * M[ag, bg])
    return sp.coo_matrix((vals, (rows, cols)), shape=(lv.n, lv.n)).tocsr()


def robin(lv, beta):
    """the level lv with the face term of the Robin coefficients beta (six values); lv itself is left unchanged"""
    beta = tuple(float(b) for b in beta)
    mask = getattr(lv, "dirichlet_faces", bo.ALL)
    assert all(b >= 0.0 for b in beta) and not any(b > 0.0 and (mask >> f) & 1 for f, b in enumerate(beta))
    out = copy.copy(lv)
    out.__dict__.pop("_rounded", None)
    out.robin = beta
    out.Braw = face_matrix(lv, beta)
    U = sp.diags((~lv.constrained).astype(float))
    out.Kraw = (lv.Kraw + out.Braw).tocsr()
    out.A = (lv.A + U @ (lv.C.T @ out.Braw @ lv.C) @ U).tocsr()
    d = out.A.diagonal().copy()
    out.inv_diag = np.where(np.abs(d) > 1e-10, 1.0 / d, 1.0)
    return out


def robin_hierarchy(levels, beta):
    return [robin(lv, beta) for lv in levels]
