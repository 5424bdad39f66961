/* mgamd_dev.h -- development and measurement entry points of libmgamd.so that are NOT part of the drop-in boundary
 * (include/mgamd.h): in-kernel phase stamps of debug builds and the HIP-event profile of the dominant kernel that bench.py turns
 * into `roofline.achieved`.  Nothing here replaces an interface of the reference. */
#ifndef MGAMD_DEV_H
#define MGAMD_DEV_H

#include "mgamd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* development aid: with MGAMD_STAMPS=<mode> in the environment the largest slot group's kernel of that mode
 * records 8 wall-clock stamps (10 ns ticks) per workgroup at its phase boundaries; returns them */
int mgamd_level_op_debug_stamps(mgamd_level_op *op, unsigned long long *out, uint64_t max_count, uint64_t *count);

/* per-kernel device time of the dominant kernel (cell operator) accumulated since the last reset,
 * measured with HIP events when profiling is enabled (bench.py roofline.achieved) */
int mgamd_ctx_kernel_profile(mgamd_ctx *ctx, int enable);
/* which launches are measured: brick_size = 0 (default) the slot group with the most work on every level;
 * brick_size = B only groups of B^3-cell bricks, i.e. the launches of ONE kernel symbol (what rocprofv3 averages) */
int mgamd_ctx_kernel_profile_brick(mgamd_ctx *ctx, int brick_size);
int mgamd_ctx_kernel_profile_read(mgamd_ctx *ctx, double *total_ms, uint64_t *n_launches, double *algorithmic_bytes);
/* the bytes the measured launches are written to move themselves (the slot-interior D^-1 is evaluated in closed form by the
 * p = 1 and the persistent 17-point lattice kernels, one word less than SURVEY 8(d)'s figure in `algorithmic_bytes`) */
int mgamd_ctx_kernel_profile_bytes_moved(mgamd_ctx *ctx, double *bytes_moved);

/* the coarse solver a multigrid runs when asked for `name` on a level 0 of n_level0_dofs DoFs (sharded or not), with or without a
 * nested multigrid / the global DoFs of the sharded AMG: what mgamd_mg_coarse_solver_used() will report, or the error
 * mgamd_mg_create* will return for it (the checks of the objects themselves aside).  Host only, no GPU. */
int mgamd_debug_coarse_resolve(const char *name, uint64_t n_level0_dofs, int level0_sharded, int has_nested, int has_amg_global,
                               char used[32]);

/* ---- the algebraic multigrid of the "amg" coarse solvers, for tests against an independent restatement ----
 * host hierarchy (amg.hpp) of the smoothed aggregation built on the level's assembled matrix (mgamd_dofs_matrix); level 0 finest */
typedef struct mgamd_amg_host mgamd_amg_host;
int mgamd_debug_amg_host_create(const mgamd_dofs *d, mgamd_amg_host **out);
int mgamd_debug_amg_host_destroy(mgamd_amg_host *h);
int mgamd_debug_amg_host_n_levels(const mgamd_amg_host *h, uint32_t *n_levels);
/* sizes of level l: rows of A, non-zeros of A, columns and non-zeros of P (0 on the coarsest level), aggregates, lambda_max (the
 * upper end of the Chebyshev interval of that level's smoother) */
int mgamd_debug_amg_host_level_info(const mgamd_amg_host *h, uint32_t level, uint32_t *n_rows, uint64_t *nnz_A, uint32_t *n_cols_P,
                                    uint64_t *nnz_P, uint32_t *n_aggregates, double *lambda_max);
/* the arrays of level l (any pointer may be null): A and P as CSR with sorted columns, the aggregate of each row (-1: decoupled row;
 * n_rows entries, none on the coarsest level) */
int mgamd_debug_amg_host_level_get(const mgamd_amg_host *h, uint32_t level, uint32_t *A_ptr, uint32_t *A_col, double *A_val,
                                   uint32_t *P_ptr, uint32_t *P_col, double *P_val, int32_t *agg);

/* ---- the shard plans of the sharded AMG (amg_shard.hpp), host only, no GPU: what every rank of `partition` would hold for the AMG
 * on multigrid level `level` (a mesh index of the partition) at `degree`.  Built as on the device path: global tables
 * (mgamd_dofs_create), the one-rank hierarchy, owners of level 0 from every rank's local tables (checked: every row exactly once),
 * aggregates to the rank owning most members. */
typedef struct mgamd_amg_shard mgamd_amg_shard;
int mgamd_debug_amg_shard_create(const mgamd_partition *partition, unsigned level, int degree, int max_brick, uint32_t min_sharded_rows,
                                 mgamd_amg_shard **out);
int mgamd_debug_amg_shard_destroy(mgamd_amg_shard *h);
/* the first step of every shard plan, on its own: the global row of every DoF of `local` in `global` (rows[n_dofs of local], may be
 * null).  MGAMD_ERR_INVALID if the two are not the same space: another degree, or another mass coefficient. */
int mgamd_debug_amg_shard_match_rows(const mgamd_dofs *global, const mgamd_dofs *local, uint32_t *rows);
int mgamd_debug_amg_shard_n_levels(const mgamd_amg_shard *h, uint32_t *n_levels, uint32_t *n_sharded_levels);
/* info[12] of one rank's level: replicated, global rows, local rows, mirror rows (identity rows of constrained DoFs computed here
 * but owned elsewhere; local rows are [mirror | owned interior | owned boundary]), owned interior rows, ghosts, length of the padded
 * send / receive buffers, peers, non-zeros of the local A, P, R, rows of the local R.  Replicated levels hold the global matrices
 * (mgamd_debug_amg_host_level_get) and report zero sizes for the local ones. */
int mgamd_debug_amg_shard_level_info(const mgamd_amg_shard *h, unsigned rank, uint32_t level, uint32_t info[12]);
/* the arrays (any pointer may be null): rows = global row of every local row; ghost = global row behind every receive slot
 * (0xFFFFFFFF: padding); peers, peer_offset (peers + 1, padded), send_count / recv_count (true counts per peer); send_idx = local row
 * packed into every send slot (0xFFFFFFFF: padding); A, P, R = local CSR, columns numbered [local rows | receive slots] of the
 * level they read (P: of the next level, or global if that one is replicated) */
int mgamd_debug_amg_shard_level_get(const mgamd_amg_shard *h, unsigned rank, uint32_t level, uint32_t *rows, uint32_t *ghost, int32_t *peers,
                                    uint32_t *peer_offset, uint32_t *send_count, uint32_t *recv_count, uint32_t *send_idx, uint32_t *A_ptr,
                                    uint32_t *A_col, double *A_val, uint32_t *P_ptr, uint32_t *P_col, double *P_val, uint32_t *R_ptr,
                                    uint32_t *R_col, double *R_val);

/* one launch of the AMG cycle's CSR kernel (K7, kernels_amg.hpp) through the production launcher on host data converted to
 * number_type: mode 0 y = A x, 1 y += A x, 2 y = b - A x, 3 y = x + f1 (x - xold) + f2 dinv (b - A x) (n_cols == n_rows).
 * lanes 4/8/16/32, or 0 for the production choice from the average row length (returned in *lanes_used).  y (n_rows) is uploaded
 * before and downloaded after the launch; b, xold, dinv may be null where the mode does not read them; xold_is_y: xold is the
 * device buffer of y itself (how the Chebyshev recurrence calls the kernel) */
int mgamd_debug_csr_spmv(mgamd_ctx *ctx, int number_type, int mode, int lanes, uint32_t n_rows, uint32_t n_cols, const uint32_t *ptr,
                         const uint32_t *col, const double *val, const double *x, double *y, const double *b, const double *xold,
                         int xold_is_y, const double *dinv, double f1, double f2, int *lanes_used);

/* the same with what the assembled operator (mgamd_matrix_create) adds: lanes 64 (K8: one wavefront per row, FP64 only) and mode 4,
 * y = A x with x . y in the same pass (FP64, n_cols == n_rows; at K7's lane counts too), the sum finished as the solver does and
 * returned in *dot.  max_blocks > 0 caps the grid below the launcher's own cap (a row's result must not depend on it); *blocks: the
 * grid launched.  lanes_used, blocks, dot may be null. */
int mgamd_debug_csr_spmv_ex(mgamd_ctx *ctx, int number_type, int mode, int lanes, uint32_t n_rows, uint32_t n_cols, const uint32_t *ptr,
                            const uint32_t *col, const double *val, const double *x, double *y, const double *b, const double *xold,
                            int xold_is_y, const double *dinv, double f1, double f2, int max_blocks, int *lanes_used, int *blocks,
                            double *dot);
/* the assembled operator's lane choice: 64 above its mean-row-length threshold, the coarse solver's choice below */
int mgamd_debug_csr_spmv_lanes_long(uint32_t n_rows, uint64_t nnz, int *lanes);
/* measurement (tools/spmv_bench.py): milliseconds per launch of A's product in mode 0 (plain), 3 (Chebyshev) or 4 (with the dot) at
 * `lanes` lanes per row (4-64), HIP events around `reps` launches after a warm-up launch, on scratch vectors */
int mgamd_debug_matrix_time_spmv(mgamd_matrix *A, int mode, int lanes, unsigned reps, double *ms_per_launch);
/* the row pointers assemble_level_matrix builds from its per-row entry counts (accumulated in 64 bits): MGAMD_ERR, with the count
 * in mgamd_last_error(), when the matrix needs more than 2^32 - 1 entries; ptr has n_rows + 1 entries.  No GPU needed. */
int mgamd_debug_csr_row_pointers(uint32_t n_rows, const uint64_t *row_counts, uint32_t *ptr);

/* ---- the jump error indicator (mgamd_level_op_estimate_error) ----
 * the face-neighbour table its second kernel walks, host only: code[n_cells][6] and nbr[n_cells][6][4] (either may be null), face
 * f = 2 axis + side.  code 0: boundary face; 1: one neighbour of the same level, nbr[0]; 2 + (c1 | c2 << 1): one neighbour one level
 * coarser, nbr[0], (c1, c2) the position of the cell's face inside the neighbour's along the lower and the higher in-face axis;
 * 6: four neighbours one level finer, nbr[c1 | c2 << 1] on the quarter (c1, c2) */
int mgamd_debug_tria_face_neighbours(const mgamd_tria *t, uint8_t *code, uint32_t *nbr);
/* measurement: bytes of the indicator's device tables and scratch, host time of their build, and the device time of the two kernels
 * of the last call (HIP events); all 0 before the operator's first estimate.  Any pointer may be null. */
int mgamd_debug_level_op_estimator_info(const mgamd_level_op *op, uint64_t *bytes, double *build_ms, double *kernel_ms);

/* ---- the error norms (mgamd_level_op_integrate_difference) ----
 * measurement: bytes of the device arrays the norms use (the gather table shared with the indicator, the leaves' corners, the result),
 * the device time of the kernel of the last call (HIP events), and whether the indicator's neighbour table has been built (1) or not
 * (0: a norm-only operator never builds it).  bytes and kernel_ms are 0 before the operator's first norm.  Any pointer may be null. */
int mgamd_debug_level_op_error_norm_info(const mgamd_level_op *op, uint64_t *bytes, double *kernel_ms, int *neighbours_built);

/* ---- cell evaluate and integrate (mgamd_level_op_evaluate, mgamd_level_op_integrate) ----
 * measurement: bytes of the device arrays the two calls use (the gather table shared with the indicator and the norms; they hold
 * nothing else), and the device times of the last evaluate and of the last integrate (its memset included) by HIP events; the call
 * waits for those events.  All 0 before the operator's first evaluate or integrate.  Any pointer may be null. */
int mgamd_debug_level_op_cell_values_info(const mgamd_level_op *op, uint64_t *bytes, double *evaluate_ms, double *integrate_ms);

/* ---- point sets (mgamd_level_op_point_set_create, mgamd_point_set_evaluate, mgamd_point_set_integrate) ----
 * measurement.  Of the operator op (may be null): operator_bytes, the device arrays only its point sets use (sorted leaf keys and
 * corners), 0 before its first non-empty point set; gather_bytes, the gather table shared with the indicator, the norms and the
 * cell values, 0 until some call has built it (a point set does at its first evaluate or integrate).  Of the set ps (may be
 * null): its device bytes, the host time of its build (the binning by leaf), and the device times by HIP events of its locate
 * kernel and of its last evaluate and last integrate (memsets included), each 0 before the first such call; the call waits
 * for those events.  Not both of op and ps null; any output pointer may be null. */
int mgamd_debug_point_set_info(const mgamd_level_op *op, const mgamd_point_set *ps, uint64_t *operator_bytes,
                               uint64_t *gather_bytes, uint64_t *set_bytes, double *build_ms, double *locate_ms,
                               double *evaluate_ms, double *integrate_ms);

#ifdef __cplusplus
}
#endif
#endif /* MGAMD_DEV_H */
