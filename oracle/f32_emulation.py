"""The oracle's Chebyshev smoother and V-cycle restated with the number type of the level vectors as a parameter.

mgoracle computes everything in float64.  The product also runs its multigrid levels in float32 (MGNumberType float, the
reference's default), and a float64 reference alone cannot say how far a correct float32 cycle may sit from it.  The
functions here redo mgoracle.Chebyshev.vmult / step and mgoracle.Multigrid.vcycle on an existing mgoracle object with
  * matrices, transfers, the inverse diagonal, the recurrence factors f1, f2 and 1/theta rounded to `dtype`,
  * every vector in `dtype` (no float64 temporary: scalars are cast before they meet an array),
  * theta, delta and the recurrence scalars computed in double and the "direct" coarse solve done in double and cast back,
    as the product's runtime does.
With dtype=float64 they are mgoracle's own arithmetic; with float32 their distance from the float64 result is the rounding
error a float32 implementation of the SAME algorithm makes, which is the yardstick for the product's float32 tolerances.
ls_vcycle and pls_vcycle do the same for ls_oracle's local-smoothing cycle (`HMG-local`) and for the p-multigrid over it
(`HPMG-local`); the objects are passed in, ls_oracle is not imported.
numpy/scipy only; the product is never imported."""
import copy

import numpy as np

import mgoracle


def _rounded(owner, dtype, make):
    """make() once per (owner, dtype), kept on the owner: a Chebyshev holds its matrix and inverse diagonal rounded to dtype, a
    Multigrid its transfers.  with_max_ev / with_max_evs / with_degree copy shallowly, so the copies of every smoother degree
    share the rounded operands of the object they were made from."""
    kept = owner.__dict__.setdefault("_rounded", {})
    if dtype not in kept:
        kept[dtype] = make()
    return kept[dtype]


def _dot(a, b):
    return float(np.dot(a.astype(np.float64), b.astype(np.float64)))


def _iterate(c, A, dinv, x, xold, b, dtype):
    if c.k < 2 or abs(c.delta) < 1e-40:
        return x
    rhok, sigma = c.delta / c.theta, c.theta / c.delta
    for _ in range(c.k - 1):
        rhokp = 1.0 / (2.0 * sigma - rhok)
        f1, f2 = dtype(rhokp * rhok), dtype(2.0 * rhokp / c.delta)
        rhok = rhokp
        xn = x + f1 * (x - xold) + f2 * dinv * (b - A @ x)
        xold, x = x, xn
    return x


def _operands(c, dtype):
    dtype = np.dtype(dtype).type
    if dtype is np.float64:
        return dtype, c.A, c.dinv
    return (dtype,) + _rounded(c, dtype, lambda: (c.A.astype(dtype), np.asarray(c.dinv).astype(dtype)))


def chebyshev_vmult(c, b, dtype):
    """mgoracle.Chebyshev.vmult (zero initial guess) in `dtype`"""
    dtype, A, dinv = _operands(c, dtype)
    b = np.asarray(b, dtype=dtype)
    x1 = dtype(1.0 / c.theta) * dinv * b
    return _iterate(c, A, dinv, x1, np.zeros_like(b), b, dtype)


def chebyshev_step(c, x0, b, dtype):
    """mgoracle.Chebyshev.step (general initial guess) in `dtype`"""
    dtype, A, dinv = _operands(c, dtype)
    x0, b = np.asarray(x0, dtype=dtype), np.asarray(b, dtype=dtype)
    x1 = x0 + dtype(1.0 / c.theta) * dinv * (b - A @ x0)
    return _iterate(c, A, dinv, x1, x0, b, dtype)


def vcycle(mg, r, dtype):
    """mgoracle.Multigrid.vcycle with level vectors, matrices and transfers in `dtype`; the coarse solve in double"""
    dtype = np.dtype(dtype).type
    nl = len(mg.levels)
    if dtype is np.float64:
        P, R = mg.P, [None] + [mg.P[l].T for l in range(1, nl)]
    else:
        P, R = _rounded(mg, dtype, lambda: ([None] + [mg.P[l].astype(dtype) for l in range(1, nl)],
                                            [None] + [mg.P[l].T.tocsr().astype(dtype) for l in range(1, nl)]))
    defect = [np.zeros(L.n, dtype=dtype) for L in mg.levels]
    sol = [None] * nl
    defect[-1] = np.array(r, dtype=dtype)
    for l in range(nl - 1, 0, -1):
        sol[l] = chebyshev_vmult(mg.sm[l], defect[l], dtype)
        t = defect[l] - _operands(mg.sm[l], dtype)[1] @ sol[l]
        defect[l - 1] += R[l] @ t
    sol[0] = mg.coarse_solve(defect[0].astype(np.float64)).astype(dtype)
    for l in range(1, nl):
        sol[l] = sol[l] + P[l] @ sol[l - 1]
        sol[l] = chebyshev_step(mg.sm[l], sol[l], defect[l], dtype)
    return sol[-1]


def _ls_operands(ls, dtype):
    """per level A_down and A_edge_in, and P, P^T of the ls_oracle.LocalSmoothing ls in `dtype`: its own objects in float64,
    rounded once per level / per ls otherwise"""
    nl = len(ls.levels)
    if dtype is np.float64:
        return ([L.A_down for L in ls.levels], [L.A_edge_in for L in ls.levels], ls.P, [None] + [ls.P[l].T for l in range(1, nl)])
    down, edge_in = zip(*[_rounded(L, dtype, lambda L=L: (L.A_down.astype(dtype), L.A_edge_in.astype(dtype))) for L in ls.levels])
    P, R = _rounded(ls, dtype, lambda: ([None] + [ls.P[l].astype(dtype) for l in range(1, nl)],
                                        [None] + [ls.P[l].T.tocsr().astype(dtype) for l in range(1, nl)]))
    return down, edge_in, P, R


def ls_vcycle(ls, r, dtype):
    """ls_oracle.LocalSmoothing.vcycle with the level vectors, the copies to and from the levels, the level matrices, both
    edge matrices and the transfers in `dtype`; the level-0 solve in double"""
    dtype = np.dtype(dtype).type
    nl = len(ls.levels)
    A_down, A_edge_in, P, R = _ls_operands(ls, dtype)
    r = np.asarray(r, dtype=dtype)
    defect = [np.zeros(L.n, dtype=dtype) for L in ls.levels]
    for l, (g, li) in enumerate(ls.copy):
        defect[l][li] = r[g]
    sol, x = [None] * nl, [None] * nl
    for l in range(nl - 1, 0, -1):
        x[l] = chebyshev_vmult(ls.sm[l], defect[l], dtype)
        t = defect[l] - A_down[l] @ x[l]  # the residual carries the refinement-edge rows
        defect[l - 1] += R[l] @ t
    sol[0] = ls.A0.solve(defect[0].astype(np.float64)).astype(dtype)
    for l in range(1, nl):
        xl = x[l] + P[l] @ sol[l - 1]
        if ls.levels[l].edge.any():
            defect[l] -= A_edge_in[l] @ xl
        sol[l] = chebyshev_step(ls.sm[l], xl, defect[l], dtype)
    z = np.zeros(ls.G.n, dtype=dtype)
    for l, (g, li) in enumerate(ls.copy):
        z[g] = sol[l][li]
    return z


def ls_with_max_evs(ls, max_evs, smoothing_range=20.0):
    """a copy of the ls_oracle.LocalSmoothing ls (levels, transfers, copy indices and factorisation shared) whose smoothers
    take the given estimates, one per level"""
    ls = copy.copy(ls)
    ls.sm = [with_max_ev(c, ev, smoothing_range) for c, ev in zip(ls.sm, max_evs)]
    return ls


def ls_with_degree(ls, degree):
    """a copy of ls whose smoothers have another degree"""
    ls = copy.copy(ls)
    ls.sm = [copy.copy(c) for c in ls.sm]
    for c in ls.sm:
        c.k = degree
    return ls


def _pls_over(pls, mg, ls):
    """a copy of the ls_oracle.PolynomialOverLocalSmoothing pls on the p-multigrid mg whose coarse solve is ls's V-cycle"""
    pls = copy.copy(pls)
    pls.ls, pls.mg = ls, copy.copy(mg)
    pls.mg.coarse = ls.vcycle
    return pls


def pls_with_max_evs(pls, max_evs_p, max_evs_ls, smoothing_range=20.0):
    """a copy of pls whose p-level smoothers and whose local-smoothing smoothers take the given estimates"""
    return _pls_over(pls, with_max_evs(pls.mg, max_evs_p, smoothing_range), ls_with_max_evs(pls.ls, max_evs_ls, smoothing_range))


def pls_with_degree(pls, degree):
    return _pls_over(pls, with_degree(pls.mg, degree), ls_with_degree(pls.ls, degree))


def pls_vcycle(pls, r, dtype):
    """PolynomialOverLocalSmoothing.vcycle in `dtype`: vcycle() of its p-multigrid with ls_vcycle of its ls as the coarse solve
    (vcycle() hands the coarse defect over through float64, which is exact for float32 data)"""
    dtype = np.dtype(dtype).type
    pls.mg.__dict__.setdefault("_rounded", {})  # (kept on pls.mg: the copy below shares it)
    mg = copy.copy(pls.mg)
    mg.coarse = lambda d: ls_vcycle(pls.ls, d, dtype).astype(np.float64)
    return vcycle(mg, r, dtype)


def eigenvalue_estimate(A, inv_diag, dtype, start=None, eig_cg_n_iterations=20):
    """The smoother's estimate of the largest eigenvalue of D^-1 A (mgoracle.Chebyshev.__init__): vectors and matrix in
    `dtype`, dot products and the CG scalars in double, the Lanczos matrix through mgoracle.lanczos_from_cg, times 1.2."""
    dtype = np.dtype(dtype).type
    n = A.shape[0]
    A, dinv = A.astype(dtype), np.asarray(inv_diag).astype(dtype)
    if start is None:
        i11 = np.arange(n) % 11
        r = i11.astype(dtype) - dtype(i11.astype(np.float64).mean())
    else:
        r = np.array(start, dtype=dtype)
    alphas, betas = [], []
    if np.sqrt(_dot(r, r)) > 0:
        z = dinv * r
        d = z.copy()
        rz = _dot(r, z)
        for it in range(eig_cg_n_iterations):
            Ad = A @ d
            dAd = _dot(d, Ad)
            if not dAd > 0:  # (runtime.hip's estimate stops here too; mgoracle's positive definite levels never do)
                break
            alpha = rz / dAd
            r = r - dtype(alpha) * Ad
            alphas.append(alpha)
            if np.sqrt(_dot(r, r)) <= 1e-10:
                break
            z = dinv * r
            rz_new = _dot(r, z)
            beta = rz_new / rz
            betas.append(beta)
            rz = rz_new
            d = z + dtype(beta) * d
    if not alphas:  # (zero start vector: mgoracle and runtime.hip take 1.0 for the raw estimate)
        return 1.2
    T = mgoracle.lanczos_from_cg(alphas, betas[: len(alphas) - 1] + [0.0])
    return 1.2 * np.linalg.eigvalsh(T)[-1]


def with_max_ev(c, max_ev, smoothing_range=20.0):
    """a copy of the mgoracle.Chebyshev c whose delta and theta follow from the given (1.2-scaled) eigenvalue estimate"""
    c = copy.copy(c)
    c.max_ev = float(max_ev)
    alpha = c.max_ev / smoothing_range if smoothing_range > 1.0 else min(0.9 * c.max_ev, c.min_ev)
    c.delta = 0.5 * (c.max_ev - alpha)
    c.theta = 0.5 * (c.max_ev + alpha)
    return c


def with_max_evs(mg, max_evs, smoothing_range=20.0):
    """a copy of the mgoracle.Multigrid mg (levels, transfers and coarse factorisation shared) whose smoothers take the
    given estimates, one per level"""
    mg = copy.copy(mg)
    mg.sm = [with_max_ev(c, ev, smoothing_range) for c, ev in zip(mg.sm, max_evs)]
    return mg


def with_degree(mg, degree):
    """a copy of mg whose smoothers have another degree (the eigenvalue estimates do not depend on it)"""
    mg = copy.copy(mg)
    mg.sm = [copy.copy(c) for c in mg.sm]
    for c in mg.sm:
        c.k = degree
    return mg
