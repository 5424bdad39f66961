"""Micro-benchmark behind the lane choice of the assembled operator (csr_spmv_lanes_long): the
wavefront-per-row kernel K8 (64 lanes) against K7 at 32 lanes and at its own choice, on the assembled matrix of one level, in
the plain, Chebyshev and dot modes.  Bytes: 12 B per stored entry (value + column), the floor of one pass over the matrix.

  python tools/spmv_bench.py quadrant 5 1 2 3 4        # geometry, NRefGlobal, degrees"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dealii_multigrid_amd as m

HBM = 8e12  # B/s, the figure README and DESIGN quote shares of

geo, L, degrees = sys.argv[1], int(sys.argv[2]), [int(p) for p in sys.argv[3:]]
ctx = m.Context(0)
modes = [("plain", m.SPMV_PLAIN), ("cheb", m.SPMV_CHEB), ("dot", m.SPMV_DOT)]
print(f"# {geo} L={L}: ms per launch (share of 8 TB/s at 12 B x nnz); two alternating rounds per cell")
print(f"{'p':>2} {'rows':>9} {'nnz':>11} {'mean row':>8} {'K7':>3} {'mode':>5} | {'K7 choice':>24} | {'K7, 32 lanes':>24} | {'K8, 64 lanes':>24} | K8 / K7@32")
for p in degrees:
    A = m.SparseMatrix(ctx, m.DoFs(m.Triangulation(geo, L), p, -1))
    avg = A.nnz / A.n_rows
    k7 = 4 if avg <= 6 else (8 if avg <= 24 else (16 if avg <= 64 else 32))
    reps = max(20, min(400, int(2e9 / (12 * A.nnz))))
    for name, mode in modes:
        t = {}
        for _ in range(2):  # alternate the candidates, keep both rounds
            for lanes in (k7, 32, 64):
                t.setdefault(lanes, []).append(A.time_spmv(mode, lanes, reps))
        cell = lambda l: " / ".join(f"{v:.4f}" for v in t[l]) + f" ({12 * A.nnz / (min(t[l]) * 1e-3) / HBM:5.1%})"  # noqa: E731
        print(f"{p:>2} {A.n_rows:>9} {A.nnz:>11} {avg:>8.1f} {k7:>3} {name:>5} | {cell(k7):>24} | {cell(32):>24} | {cell(64):>24} | {min(t[64]) / min(t[32]):.3f}",
              flush=True)
    del A
