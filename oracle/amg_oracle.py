"""Independent numpy/scipy restatement of the smoothed-aggregation AMG behind the coarse solvers "amg", "cg_with_amg" and
"amg_petsc" (DESIGN.md section 9), written from its specification, not from the C++ (csrc/amg.hpp, runtime.hip AmgCycle):

  strength     j != i strongly coupled to i:  a_ij != 0  and  |a_ij| >= theta sqrt(|a_ii a_jj|),  theta = 1e-4
  aggregates   three greedy passes in row order over the rows with at least one strong connection (the others, the identity
               rows of constrained DoFs, stay out): (1) a row whose whole strong neighbourhood is free roots an aggregate of
               itself and that neighbourhood; (2) each row left over joins the pass-1 aggregate of its strongest (largest |a_ij|)
               aggregated neighbour, the first in column order on ties; (3) each row still free roots a new aggregate of itself
               and its still free strong neighbours
  prolongator  P = (I - omega D^-1 A) P_t,  P_t = 1/sqrt(|aggregate|) on the aggregate's rows,  omega = 4 / (3 lambda)
  lambda       1.1 x the 20-step power iteration of D^-1 A from v_i = 1 + 0.25 ((i 2654435761 mod 2^32) >> 16 mod 7)
  coarse       A_c = P^T A P, until <= 1000 rows or 12 levels; the coarsest level is solved exactly
  cycle        Chebyshev of degree d in D^-1 A on [lambda / 20, lambda], zero start before the coarse correction, general start
               after it; residual, restriction by P^T, recursion, prolongation added

Sparsity patterns are symbolic (what a sparse product produces before any cancellation), so they can be compared entry by
entry with the product's, which keeps the zeros that cancellation leaves."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

THETA = 1e-4
MAX_COARSE = 1000
MAX_LEVELS = 12
POWER_ITERATIONS = 20
CHEBYSHEV_RANGE = 20.0


def csr(ptr, col, val, shape=None):
    """a scipy CSR matrix from a (row_ptr, col, val) triple, explicit zeros kept"""
    n = len(ptr) - 1
    return sp.csr_matrix((np.asarray(val, np.float64), np.asarray(col, np.int64), np.asarray(ptr, np.int64)),
                         shape=shape or (n, n))


def _ones(M):
    return sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)


def _on_pattern(pattern, M):
    """the values of M on the (sorted) pattern of `pattern`, zero where M stores nothing"""
    pattern.sort_indices()
    M = M.tocsr()
    M.sort_indices()
    keys = lambda X: np.repeat(np.arange(X.shape[0], dtype=np.int64), np.diff(X.indptr)) * X.shape[1] + X.indices
    kp, km = keys(pattern), keys(M)
    val = np.zeros(len(kp))
    if len(km):
        pos = np.minimum(np.searchsorted(km, kp), len(km) - 1)
        hit = km[pos] == kp
        val[hit] = M.data[pos[hit]]
    return sp.csr_matrix((val, pattern.indices.copy(), pattern.indptr.copy()), shape=pattern.shape)


def product(A, B):
    """A B on the symbolic pattern of the product"""
    return _on_pattern(_ones(abs(A)) @ _ones(abs(B)), A @ B)


def diagonal_inverse(A):
    d = A.diagonal()
    return np.where(d != 0, 1.0 / np.where(d != 0, d, 1.0), 1.0)


def strength(A, theta=THETA):
    """strong off-diagonal couplings as a CSR matrix holding |a_ij| (explicit zeros removed)"""
    C = A.tocoo()
    d = np.abs(A.diagonal())
    keep = (C.row != C.col) & (C.data != 0) & (np.abs(C.data) >= theta * np.sqrt(d[C.row] * d[C.col]))
    S = sp.csr_matrix((np.abs(C.data[keep]), (C.row[keep], C.col[keep])), shape=A.shape)
    S.sort_indices()
    return S


def aggregate(A, theta=THETA):
    """aggregate index per row (-1: no strong connection), number of aggregates"""
    S = strength(A, theta)
    n = A.shape[0]
    ptr, nb, w = S.indptr.tolist(), S.indices.tolist(), S.data.tolist()
    coupled = np.diff(S.indptr) > 0
    agg = [-1] * n
    na = 0
    for i in range(n):  # pass 1
        if not coupled[i] or agg[i] >= 0:
            continue
        nbs = nb[ptr[i]:ptr[i + 1]]
        if any(agg[j] >= 0 for j in nbs):
            continue
        agg[i] = na
        for j in nbs:
            agg[j] = na
        na += 1
    agg1 = list(agg)
    for i in range(n):  # pass 2
        if not coupled[i] or agg1[i] >= 0:
            continue
        best, to = 0.0, -1
        for k in range(ptr[i], ptr[i + 1]):
            if agg1[nb[k]] >= 0 and w[k] > best:
                best, to = w[k], agg1[nb[k]]
        agg[i] = to
    for i in range(n):  # pass 3
        if not coupled[i] or agg[i] >= 0:
            continue
        agg[i] = na
        for j in nb[ptr[i]:ptr[i + 1]]:
            if agg[j] < 0:
                agg[j] = na
        na += 1
    return np.array(agg, np.int64), na


def power_lambda(A, dinv, iterations=POWER_ITERATIONS):
    n = A.shape[0]
    i = np.arange(n, dtype=np.uint64)
    v = 1.0 + 0.25 * ((((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)) % np.uint64(7)).astype(np.float64)
    lam = 1.0
    # norms as sums in index order (np.cumsum), so that lambda, omega and hence the coarse matrices come out to the last bit
    # wherever the product sums in the same order: the pass-2 choice of the strongest neighbour on a coarse level breaks ties of
    # equal couplings, which a rounding difference of one ulp would flip
    for _ in range(iterations):
        w = dinv * (A @ v)
        nw, nv = np.cumsum(w * w)[-1], np.cumsum(v * v)[-1]
        lam = np.sqrt(nw / nv)
        v = w * (1.0 / np.sqrt(nw))
    return 1.1 * lam


class Level:
    def __init__(self, A):
        self.A = A
        self.n = A.shape[0]
        self.dinv = diagonal_inverse(A)
        self.lambda_max = power_lambda(A, self.dinv)
        self.P = self.agg = None
        self.n_aggregates = 0


class SmoothedAggregation:
    """the hierarchy on an assembled matrix (scipy CSR, or a (row_ptr, col, val) triple) and its V-cycle with a Chebyshev
    smoother of degree `degree`"""

    def __init__(self, A, degree=2, max_coarse=MAX_COARSE, max_levels=MAX_LEVELS, theta=THETA):
        if isinstance(A, tuple):
            A = csr(*A)
        self.degree = degree
        self.levels = [Level(A.tocsr())]
        while True:
            L = self.levels[-1]
            if L.n <= max_coarse or len(self.levels) >= max_levels:
                break
            agg, na = aggregate(L.A, theta)
            if na == 0 or na >= L.n:
                break
            rows = np.flatnonzero(agg >= 0)
            size = np.bincount(agg[rows], minlength=na)
            Pt = sp.csr_matrix((1.0 / np.sqrt(size[agg[rows]]), (rows, agg[rows])), shape=(L.n, na))
            omega = 4.0 / (3.0 * L.lambda_max)
            AP = product(L.A, Pt)
            P = _on_pattern(_ones(AP) + _ones(Pt), Pt - sp.diags(omega * L.dinv) @ AP)
            L.P, L.agg, L.n_aggregates = P, agg, na
            self.levels.append(Level(product(P.T.tocsr(), product(L.A, P))))
        self.coarse_lu = sla.lu_factor(self.levels[-1].A.toarray())

    # Chebyshev in D^-1 A on [lambda / range, lambda] (Saad, Iterative Methods, Alg. 12.1)
    def _chebyshev(self, L, b, x0):
        lmax = L.lambda_max
        theta, delta = 0.5 * (lmax + lmax / CHEBYSHEV_RANGE), 0.5 * (lmax - lmax / CHEBYSHEV_RANGE)
        sigma = theta / delta
        rho = 1.0 / sigma
        xold = np.zeros_like(b) if x0 is None else x0
        x = (xold if x0 is not None else 0.0) + L.dinv * (b - (L.A @ x0 if x0 is not None else 0.0)) / theta
        for _ in range(self.degree - 1):
            rho_new = 1.0 / (2.0 * sigma - rho)
            x, xold = x + rho_new * rho * (x - xold) + 2.0 * rho_new / delta * L.dinv * (b - L.A @ x), x
            rho = rho_new
        return x

    def _cycle(self, l, b):
        L = self.levels[l]
        if l + 1 == len(self.levels):
            return sla.lu_solve(self.coarse_lu, b)
        x = self._chebyshev(L, b, None)
        xc = self._cycle(l + 1, L.P.T @ (b - L.A @ x))
        return self._chebyshev(L, b, x + L.P @ xc)

    def vcycle(self, r):
        """one V-cycle from a zero initial guess (the `coarse=` callable of mgoracle.Multigrid)"""
        return self._cycle(0, np.asarray(r, np.float64))

    def apply(self, r, n_cycles=1):
        """x = V(r), then n_cycles - 1 corrections x += V(r - A x)"""
        x = self.vcycle(r)
        for _ in range(1, n_cycles):
            x = x + self.vcycle(r - self.levels[0].A @ x)
        return x

    def precondition(self, n_cycles=1):
        """the coarse solver as a preconditioner (mgoracle.pcg) or a `coarse=` callable: n_cycles V-cycles"""
        return lambda r: self.apply(r, n_cycles)


def true_lambda_max(A):
    """the largest eigenvalue of D^-1 A (A symmetric positive definite), by scipy's Lanczos on D^-1/2 A D^-1/2"""
    import scipy.sparse.linalg as spla

    s = np.sqrt(np.abs(diagonal_inverse(A)))
    B = (sp.diags(s) @ A @ sp.diags(s)).tocsr()
    if B.shape[0] <= 2000:
        return float(np.linalg.eigvalsh(B.toarray())[-1])
    return float(spla.eigsh(B, k=1, which="LA", tol=1e-10, return_eigenvectors=False)[0])
