"""Shard plans of the sharded algebraic multigrid (csrc/amg_shard.hpp: replicated setup, sharded cycle), host only: ownership,
ghost lists, exchange lists and the local matrices of every rank, checked against the global hierarchy of the one-rank AMG
(mgamd_debug_amg_host_level_get) in numpy.  No GPU: the plans are host code (mgamd_dev.h, mgamd_debug_amg_shard_*).

The local rows keep the entries of the global rows in their order, and scipy adds a CSR row up in storage order, so the products
of the local matrices equal the rows of the global products to the last bit; 1e-15 leaves room for the one place where the order
differs, the sum of the ranks' partial restrictions onto a replicated level."""
import numpy as np
import pytest
import scipy.sparse as sp

from support import random_mesh

INVALID = 0xFFFFFFFF
TOL = 1e-15

# (geometry, NRefGlobal) or ("random", random_mesh's (seed, global refinements, rounds, fraction)), all at p = 1
# (quadrant L=6 is the one with three AMG levels: a sharded level below a sharded level)
MESHES = [("annulus", 5), ("annulus", 6), ("quadrant", 5), ("random", (4, 4, 1, 0.004)), ("quadrant", 6)]
MESH_IDS = [f"{g}-{L}" if g != "random" else f"random-seed{L[0]}" for g, L in MESHES]
RANKS = [2, 3, 4, 8]


def _csr(t, n_cols):
    ptr, col, val = t
    return sp.csr_matrix((val, col.astype(np.int64), ptr.astype(np.int64)), shape=(len(ptr) - 1, n_cols))


@pytest.fixture(scope="module")
def hierarchies(mgamd, oracle):
    cache = {}

    def get(geo, L):
        key = (geo, str(L))
        if key not in cache:
            if geo == "random":
                arr = np.array(sorted(random_mesh(oracle, *L)), dtype=np.int64)
                fine = mgamd.Triangulation.from_leaves(arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3])
            else:
                fine = mgamd.Triangulation(geo, L)
            trias = mgamd.create_geometric_coarsening_sequence(fine)
            H = mgamd.DoFs(fine, 1, -1).amg_hierarchy()
            lv = [H.level(l) for l in range(H.n_levels)]
            G = []
            for l, d in enumerate(lv):
                n = len(d["A"][0]) - 1
                A = _csr(d["A"], n)
                P = _csr(d["P"], d["n_cols_P"]) if d["P"] is not None else None
                G.append(dict(n=n, A=A, P=P, R=P.T.tocsr() if P is not None else None))
                if P is not None:
                    G[-1]["R"].sort_indices()
            cache[key] = (trias, G)
        return cache[key]

    return get


def _plans(mgamd, trias, n_ranks, min_rows):
    part = mgamd.Partition(trias, n_ranks, 2.0, 0)
    S = mgamd.AmgShardPlans(part, len(trias) - 1, 1, -1, min_rows)
    return S, [[S.level(r, l) for l in range(S.n_levels)] for r in range(n_ranks)]


def _local_vector(x, lv):
    """[x_owned-and-mirror | x_ghost]; the padding of the receive buffer is NaN: nothing may read it"""
    g = lv["ghost"].astype(np.int64)
    xg = np.full(len(g), np.nan)
    xg[g != INVALID] = x[g[g != INVALID]]
    return np.concatenate([x[lv["rows"].astype(np.int64)], xg])


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("only_level0", [False, True], ids=["min_rows_0", "level0_only"])
@pytest.mark.parametrize("n_ranks", RANKS)
@pytest.mark.parametrize("geo,L", MESHES, ids=MESH_IDS)
def test_shard_plans(mgamd, hierarchies, geo, L, n_ranks, only_level0):
    trias, G = hierarchies(geo, L)
    assert len(G) >= 2  # (annulus L=5 has one level above the dense coarsest one: both settings shard level 0 only)
    min_rows = G[1]["n"] if only_level0 else 0  # level 1 and everything below replicated / only the coarsest replicated
    S, plans = _plans(mgamd, trias, n_ranks, min_rows)
    assert S.n_levels == len(G)
    assert S.n_sharded_levels == (1 if only_level0 else len(G) - 1)
    ns = S.n_sharded_levels
    rng = np.random.default_rng(7)
    owner = []
    for l in range(len(G)):
        n = G[l]["n"]
        if l >= ns:
            for r in range(n_ranks):
                assert plans[r][l]["replicated"] and plans[r][l]["n_rows"] == n
            continue
        A = G[l]["A"]
        # ---- every row is owned exactly once, the owned counts sum to the global rows; mirrors are isolated identity rows
        own = np.full(n, -1)
        for r in range(n_ranks):
            p = plans[r][l]
            assert not p["replicated"] and p["n_global"] == n and len(p["rows"]) == p["n_rows"]
            rows = p["rows"].astype(np.int64)
            owned = rows[p["n_mirror"]:]
            assert np.all(own[owned] == -1), "a row is owned twice"
            own[owned] = r
            assert len(np.unique(rows)) == len(rows)
            if l > 0:
                assert p["n_mirror"] == 0
            for g in rows[:p["n_mirror"]]:
                assert A.indptr[g + 1] - A.indptr[g] == 1 and A.indices[A.indptr[g]] == g and A.data[A.indptr[g]] == 1.0
        assert np.all(own >= 0), "a row without owner"
        assert sum(plans[r][l]["n_rows"] - plans[r][l]["n_mirror"] for r in range(n_ranks)) == n
        for r in range(n_ranks):  # a mirror is owned by another rank
            m = plans[r][l]["rows"][:plans[r][l]["n_mirror"]].astype(np.int64)
            assert np.all(own[m] != r)
        owner.append(own)
    for l in range(ns):
        n, A, P, R = G[l]["n"], G[l]["A"], G[l]["P"], G[l]["R"]
        x = rng.standard_normal(n)
        xc = rng.standard_normal(P.shape[1])
        Ax, Px, Rx = A @ x, P @ xc, R @ x
        partial = np.zeros(P.shape[1])
        for r in range(n_ranks):
            p = plans[r][l]
            rows = p["rows"].astype(np.int64)
            nloc, nm, ni = p["n_rows"], p["n_mirror"], p["n_interior"]
            owned = rows[nm:]
            is_local = np.zeros(n, bool)
            is_local[rows] = True
            # ---- the ghost list is exactly the set of non-owned columns the owned rows of A, P (of the finer level) and R reference
            expect = set(A[owned].indices[~is_local[A[owned].indices]].tolist())
            if l + 1 < ns:
                oc = plans[r][l + 1]["rows"].astype(np.int64)
                expect |= set(R[oc].indices[~is_local[R[oc].indices]].tolist())
            if l > 0:
                of = plans[r][l - 1]["rows"].astype(np.int64)[plans[r][l - 1]["n_mirror"]:]
                cols = G[l - 1]["P"][of].indices
                expect |= set(cols[~is_local[cols]].tolist())
            ghost = p["ghost"].astype(np.int64)
            real = ghost[ghost != INVALID]
            assert len(real) == p["n_ghost"] == len(set(real.tolist())) and set(real.tolist()) == expect
            assert not np.any(is_local[real]) and len(ghost) == p["n_recv"] == p["peer_offset"][-1]
            # grouped by peer (ascending rank), every ghost owned by the peer it comes from
            assert np.all(np.diff(p["peers"]) > 0) and r not in p["peers"]
            for j, q in enumerate(p["peers"]):
                seg = ghost[p["peer_offset"][j]:p["peer_offset"][j + 1]]
                assert np.all(seg[:p["recv_count"][j]] != INVALID) and np.all(seg[p["recv_count"][j]:] == INVALID)
                assert np.all(owner[l][seg[:p["recv_count"][j]]] == q)
                # ---- what q sends to r is what r expects from q, in the same order; the pair's segments have one (padded) size
                pq = plans[q][l]
                k = list(pq["peers"]).index(r)
                assert pq["peer_offset"][k + 1] - pq["peer_offset"][k] == len(seg)
                sidx = pq["send_idx"][pq["peer_offset"][k]:pq["peer_offset"][k + 1]].astype(np.int64)
                assert pq["send_count"][k] == p["recv_count"][j]
                assert np.all(sidx[pq["send_count"][k]:] == INVALID)
                sent = pq["rows"].astype(np.int64)[sidx[:pq["send_count"][k]]]
                assert np.all(sidx[:pq["send_count"][k]] >= pq["n_mirror"])  # only owned rows travel
                assert np.array_equal(sent, seg[:p["recv_count"][j]])
            # ---- interior rows (and mirrors) reference no ghost, in any product that writes them
            Al = _csr(p["A"], nloc + p["n_recv"])
            Pl_cols = (plans[r][l + 1]["n_rows"] + plans[r][l + 1]["n_recv"]) if l + 1 < ns else P.shape[1]
            Pl = _csr(p["P"], Pl_cols)
            assert Al.shape[0] == nloc and Pl.shape[0] == nloc
            assert Al[:nm + ni].indices.max(initial=-1) < nloc
            if l + 1 < ns:
                assert Pl[:nm + ni].indices.max(initial=-1) < plans[r][l + 1]["n_rows"]
            if l > 0:
                Rf = _csr(plans[r][l - 1]["R"], plans[r][l - 1]["n_rows"] + plans[r][l - 1]["n_recv"])
                assert Rf.shape[0] == nloc and Rf[:ni].indices.max(initial=-1) < plans[r][l - 1]["n_rows"]
            if n_ranks > 1 and len(owned):
                b = Al[nm + ni:]
                assert np.all(np.diff(b.indptr) > 0) or b.shape[0] == 0
            # ---- numpy emulation of the sharded products
            xl = _local_vector(x, p)
            assert _rel(Al @ xl, Ax[rows]) <= TOL
            if l + 1 < ns:
                pc = plans[r][l + 1]
                assert _rel(Pl @ _local_vector(xc, pc), Px[rows]) <= TOL
                Rl = _csr(p["R"], nloc + p["n_recv"])
                assert Rl.shape[0] == pc["n_rows"]
                assert _rel(Rl @ xl, Rx[pc["rows"].astype(np.int64)]) <= TOL
            else:
                assert _rel(Pl @ xc, Px[rows]) <= TOL
                Rl = _csr(p["R"], nloc + p["n_recv"])
                assert Rl.shape[0] == P.shape[1]
                assert Rl.indices.max(initial=-1) < nloc, "the partial restriction reads owned columns only"
                partial += Rl @ np.nan_to_num(xl)
        if l + 1 == ns:
            assert _rel(partial, Rx) <= TOL  # partial sums + all-reduce onto the replicated level


def test_aggregates_follow_the_majority_of_their_members(mgamd, hierarchies):
    """level k+1: an aggregate belongs to the rank that owns most of its member rows, ties to the lowest rank"""
    trias, G = hierarchies("annulus", 6)
    fine = trias[-1]
    H = mgamd.DoFs(fine, 1, -1).amg_hierarchy()
    for n_ranks in (3, 8):
        S, plans = _plans(mgamd, trias, n_ranks, 0)
        for l in range(S.n_sharded_levels - 1):
            agg = H.level(l)["agg"]
            own = np.full(G[l]["n"], -1)
            own_c = np.full(G[l + 1]["n"], -1)
            for r in range(n_ranks):
                own[plans[r][l]["rows"].astype(np.int64)[plans[r][l]["n_mirror"]:]] = r
                own_c[plans[r][l + 1]["rows"].astype(np.int64)] = r
            votes = np.zeros((G[l + 1]["n"], n_ranks), np.int64)
            np.add.at(votes, (agg[agg >= 0], own[agg >= 0]), 1)
            assert np.array_equal(own_c, votes.argmax(axis=1))  # argmax: the first (lowest) rank among equals


def test_one_rank_has_no_sharded_level(mgamd, hierarchies):
    trias, G = hierarchies("annulus", 5)
    part = mgamd.Partition(trias, 1, 2.0, 0)
    S = mgamd.AmgShardPlans(part, len(trias) - 1, 1, -1, 0)
    assert S.n_sharded_levels == 0 and all(S.level(0, l)["replicated"] for l in range(S.n_levels))


# ------------------------------------------------------------------ the whole sharded cycle, emulated on the plans
def _emulated_sharded_vcycle(plans, G, o, r, n_ranks, ns):
    """the device cycle restated on the ranks' local matrices: vectors [local rows | receive buffer], a ghost import copies what the
    peers' send lists name into the receive segments (padding included, as the padded exchange does), the restriction onto the first
    replicated level is the sum of the ranks' partial products; Chebyshev coefficients from the oracle's levels"""
    import amg_oracle as ao

    def imp(l, vs):
        for rk in range(n_ranks):
            p = plans[rk][l]
            for j, q in enumerate(p["peers"]):
                pq = plans[q][l]
                k = list(pq["peers"]).index(rk)
                sidx = pq["send_idx"][pq["peer_offset"][k]:pq["peer_offset"][k + 1]].astype(np.int64)
                seg = np.where(sidx == INVALID, 0.0, vs[q][np.where(sidx == INVALID, 0, sidx)])
                vs[rk][p["n_rows"] + p["peer_offset"][j]:p["n_rows"] + p["peer_offset"][j + 1]] = seg

    def mats(l):
        out = []
        for rk in range(n_ranks):
            p = plans[rk][l]
            nc = p["n_rows"] + p["n_recv"]
            pc = (plans[rk][l + 1]["n_rows"] + plans[rk][l + 1]["n_recv"]) if l + 1 < ns else G[l]["P"].shape[1]
            out.append((_csr(p["A"], nc), _csr(p["P"], pc), _csr(p["R"], nc), p["rows"].astype(np.int64), p["n_recv"]))
        return out

    def cheb(l, M, b, x0):
        L = o.levels[l]
        lmax = L.lambda_max
        theta, delta = 0.5 * (lmax + lmax / ao.CHEBYSHEV_RANGE), 0.5 * (lmax - lmax / ao.CHEBYSHEV_RANGE)
        sigma = theta / delta
        rho = 1.0 / sigma
        dinv = [L.dinv[m[3]] for m in M]
        pad = lambda v, m: np.concatenate([v, np.full(m[4], np.nan)])  # noqa: E731
        if x0 is None:
            xold = [np.zeros(len(m[3])) for m in M]
            x = [pad(dinv[k] * b[k] / theta, M[k]) for k in range(n_ranks)]
        else:
            imp(l, x0)
            xold = [v[:len(m[3])] for v, m in zip(x0, M)]
            x = [pad(xold[k] + dinv[k] * (b[k] - M[k][0] @ x0[k]) / theta, M[k]) for k in range(n_ranks)]
        for _ in range(o.degree - 1):
            rho_new = 1.0 / (2.0 * sigma - rho)
            imp(l, x)
            xn = [pad(x[k][:len(M[k][3])] + rho_new * rho * (x[k][:len(M[k][3])] - xold[k]) + 2.0 * rho_new / delta * dinv[k] *
                      (b[k] - M[k][0] @ x[k]), M[k]) for k in range(n_ranks)]
            xold, x, rho = [v[:len(m[3])] for v, m in zip(x, M)], xn, rho_new
        return x

    def cycle(l, b):
        if l >= ns:  # replicated from here on: the one-rank cycle
            return o._cycle(l, b)
        M = mats(l)
        x = cheb(l, M, b, None)
        imp(l, x)
        res = [np.concatenate([b[k] - M[k][0] @ x[k], np.full(M[k][4], np.nan)]) for k in range(n_ranks)]
        if l + 1 < ns:
            imp(l, res)
            xc = cycle(l + 1, [M[k][2] @ res[k] for k in range(n_ranks)])
            imp(l + 1, xc)
            x = [np.concatenate([x[k][:len(M[k][3])] + M[k][1] @ xc[k], np.full(M[k][4], np.nan)]) for k in range(n_ranks)]
        else:
            bc = sum(M[k][2] @ np.nan_to_num(res[k]) for k in range(n_ranks))  # partial sums + all-reduce
            xc = cycle(l + 1, bc)
            x = [np.concatenate([x[k][:len(M[k][3])] + M[k][1] @ xc, np.full(M[k][4], np.nan)]) for k in range(n_ranks)]
        return cheb(l, M, b, x)

    x = cycle(0, [r[plans[rk][0]["rows"].astype(np.int64)] for rk in range(n_ranks)])
    z = np.full(len(r), np.nan)
    for rk in range(n_ranks):
        p = plans[rk][0]
        rows = p["rows"].astype(np.int64)
        z[rows[p["n_mirror"]:]] = x[rk][p["n_mirror"]:p["n_rows"]]
    for rk in range(n_ranks):  # a mirror row carries the value its owner computed
        p = plans[rk][0]
        assert np.array_equal(z[p["rows"].astype(np.int64)[:p["n_mirror"]]], x[rk][:p["n_mirror"]])
    return z


@pytest.mark.parametrize("only_level0", [False, True], ids=["min_rows_0", "level0_only"])
@pytest.mark.parametrize("n_ranks", [2, 3, 8])
def test_emulated_sharded_cycle_equals_the_oracle(mgamd, hierarchies, n_ranks, only_level0):
    """quadrant L=6 (three AMG levels): the cycle run on the ranks' local matrices, vectors and exchange lists equals the oracle's
    cycle on the global matrix, for right-hand sides without and with non-zero constrained entries"""
    import amg_oracle as ao

    trias, G = hierarchies("quadrant", 6)
    d = mgamd.DoFs(trias[-1], 1, -1)
    o = ao.SmoothedAggregation(d.matrix())
    assert len(o.levels) == len(G) == 3
    S, plans = _plans(mgamd, trias, n_ranks, G[1]["n"] if only_level0 else 0)
    rng = np.random.default_rng(11)
    for constrained in (False, True):
        r = rng.standard_normal(d.n_dofs)
        if not constrained:
            r[d.info.n_interior + d.info.n_tail:] = 0.0
        z = _emulated_sharded_vcycle(plans, G, o, r, n_ranks, S.n_sharded_levels)
        assert np.isfinite(z).all() and _rel(z, o.vcycle(r)) <= 1e-13
