"""In-kernel phase timeline of the dominant lattice kernel (development tool; MGAMD_STAMPS must be set)."""
import sys, os, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dealii_multigrid_amd as m

geo, L, p = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
mode = int(os.environ["MGAMD_STAMPS"])
ctx = m.Context(0)
d = m.DoFs(m.Triangulation(geo, L), p, int(sys.argv[4]) if len(sys.argv) > 4 else 0)
op = m.Operator(ctx, d)
n = d.n_dofs
x, y, b = (op.initialize_dof_vector() for _ in range(3))
x.from_host(np.random.default_rng(0).standard_normal(n)); b.from_host(np.random.default_rng(1).standard_normal(n))
if mode == 0:
    for _ in range(3): op.vmult(y, x)
elif mode in (4, 5):  # zero-start passes
    ch = m.PreconditionChebyshev(op, 3, 20.0, 2)
    for _ in range(3): ch.vmult(y, b)
else:
    ch = m.PreconditionChebyshev(op, 3, 20.0, 2)
    for _ in range(3): ch.step(y, b)
ctx.synchronize()
buf = np.zeros(8 * 70000, np.uint64); cnt = C.c_uint64()
m._chk(m._lib.mgamd_level_op_debug_stamps(op._h, buf.ctypes.data_as(C.c_void_p), C.c_uint64(buf.size), C.byref(cnt)))
st = buf[: cnt.value].reshape(-1, 8).astype(np.int64)
vpos = np.nonzero(st[:, 0] > 0)[0]  # row = position v of the brick in the walk of the persistent kernel
st = st[st[:, 0] > 0]
t0 = st[:, 0].min()
tick = 0.01  # us per tick (100 MHz)
dur = (st[:, 4] - st[:, 0]) * tick
print(f"{geo} L={L} p={p} mode={mode}: {len(st)} workgroups, kernel span {(st[:,4].max()-t0)*tick:.1f} us")
print(f"  per-WG total   : median {np.median(dur):6.2f} us  p10 {np.percentile(dur,10):6.2f}  p90 {np.percentile(dur,90):6.2f}")
for k, name in enumerate(["gather (issue+wait+LDS)", "sweeps (+epilogue operand issue)", "interior epilogue", "shell atomics + drain"]):
    ph = (st[:, k + 1] - st[:, k]) * tick
    print(f"  {name:34s}: median {np.median(ph):6.2f} us  p10 {np.percentile(ph,10):6.2f}  p90 {np.percentile(ph,90):6.2f}")
if (st[:, 5] > 0).all() and (st[:, 6] > 0).all():  # the one-shot body also stamps the constraint passes
    for name, a, b in [("  of which: interpolation passes", 1, 5), ("            sweeps", 5, 6), ("            transposed passes", 6, 2)]:
        ph = (st[:, b] - st[:, a]) * tick
        print(f"  {name:34s}: median {np.median(ph):6.2f} us  p10 {np.percentile(ph,10):6.2f}  p90 {np.percentile(ph,90):6.2f}")
starts = np.sort(st[:, 0] - t0) * tick
print("  WG start times (us) quantiles:", [round(float(np.percentile(starts, q)), 1) for q in (0, 5, 25, 50, 75, 95, 100)])
# concurrency: average number of WGs alive
ends = (st[:, 4] - t0) * tick
span = ends.max()
print(f"  avg concurrent WGs: {dur.sum()/span:.1f}  (256 CUs)")

# ---- the schedule of the persistent kernel, workgroup by workgroup (bricks grouped by the workgroup that ran them) ----
# Stamp 7 of a brick, where the build writes it, is 1 + the id of the workgroup that ran it (ticket schedule); without it the
# bricks of workgroup w are v = w, w + grid, ... (static walk).  MGAMD_STAMPS_GRID: the grid of the launch (default: two
# workgroups on each of 256 CUs, or the cap MGAMD_PERSISTENT_GRID).
grid = int(os.environ.get("MGAMD_STAMPS_GRID", os.environ.get("MGAMD_PERSISTENT_GRID", "512")))
n_bricks = int(vpos.max()) + 1
if (st[:, 5] == 0).all() and n_bricks > grid:
    owner = st[:, 7] - 1 if (st[:, 7] > 0).all() else vpos % grid
    order = np.lexsort((st[:, 0], owner))
    o, s0, s4 = owner[order], st[order, 0], st[order, 4]
    first = np.r_[True, o[1:] != o[:-1]]
    last = np.r_[first[1:], True]
    wg_start, wg_end = s0[first], s4[last]
    n_per_wg = np.diff(np.r_[np.nonzero(first)[0], len(o)])
    gaps = np.where(first[1:], 0, s0[1:] - s4[:-1])  # stamp 4 of one brick -> stamp 0 of the workgroup's next
    gap_sum = np.add.reduceat(np.r_[0, gaps], np.nonzero(first)[0]) * tick
    k_start, k_end = wg_start.min(), wg_end.max()
    q = lambda a: "min %7.2f  median %7.2f  p95 %7.2f  max %7.2f" % (a.min(), np.median(a), np.percentile(a, 95), a.max())
    late, early = (wg_start - k_start) * tick, (k_end - wg_end) * tick
    n_wg = len(wg_start)
    print(f"  schedule: {n_wg} workgroups ({'stamped owner' if (st[:, 7] > 0).all() else 'v mod %d' % grid}), "
          f"bricks per workgroup min {n_per_wg.min()} median {int(np.median(n_per_wg))} max {n_per_wg.max()}")
    print(f"  first stamp 0 after the earliest (us): {q(late)}")
    print(f"  last stamp 4 before the latest (us)  : {q(early)}")
    print(f"  gaps stamp 4 -> next stamp 0, summed per workgroup (us): {q(gap_sum)}")
    span_s = (k_end - k_start) * tick
    print(f"  idle share: start {late.sum() / (n_wg * span_s) * 100:5.2f} %  end {early.sum() / (n_wg * span_s) * 100:5.2f} %  "
          f"total {(late.sum() + early.sum()) / (n_wg * span_s) * 100:5.2f} % of {n_wg} x {span_s:.1f} us;  "
          f"gaps {gap_sum.sum() / (n_wg * span_s) * 100:5.2f} %;  mean brick lifetime {dur.mean():.2f} us")
