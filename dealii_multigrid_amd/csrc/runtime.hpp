// Device runtime: HIP stream + device vectors + the objects behind the C ABI.
// Class and method names follow deal.II's plugin surface as the reference uses it
// (SURVEY.md section 8b): LevelOperator <-> Operator<3,1,Number> (ref:include/operator.h),
// Chebyshev <-> PreconditionChebyshev, Transfer2 <-> MGTwoLevelTransfer,
// Multigrid <-> Multigrid + PreconditionMG + MGTransferGlobalCoarsening, solve_cg <-> SolverCG.
#pragma once
#include "api_common.hpp"
#include "comm.hpp"

#include <hip/hip_runtime.h>

#include <functional>
#include <map>
#include <sstream>

namespace mgamd
{
#define HIP_CHECK(expr)                                                                                       \
  do                                                                                                          \
    {                                                                                                         \
      hipError_t e_ = (expr);                                                                                 \
      if (e_ != hipSuccess)                                                                                   \
        {                                                                                                     \
          std::ostringstream os_;                                                                             \
          os_ << "HIP error " << hipGetErrorString(e_) << " at " << __FILE__ << ":" << __LINE__ << ": " #expr; \
          throw std::runtime_error(os_.str());                                                                \
        }                                                                                                     \
    }                                                                                                         \
  while (0)

  struct Ctx
  {
    int         device = 0;
    hipStream_t stream = nullptr;
    int         n_cu   = 256;     // compute units (grid of the persistent-workgroup kernels)
    double     *d_partial = nullptr; // 1024 block partials
    double     *d_result  = nullptr; // 8 scalars
    double     *h_result  = nullptr; // pinned
    double     *d_cg      = nullptr; // 8 scalars of the device-resident CG (kernels.hpp)
    // dominant-kernel profiling (HIP events around the largest lattice_apply launches)
    bool                                           profile = false;
    int                                            prof_brick = 0; // 0: the dominant group of each level; B: groups of B^3 bricks only
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    size_t                                         prof_used  = 0;
    double                                         prof_bytes = 0.0;       // SURVEY 8(d) figure: the algorithm's words
    double                                         prof_bytes_moved = 0.0; // what the kernels are written to move (closed-form D^-1)
    double                                         prof_ms_accum = 0.0; // already harvested
    uint64_t                                       prof_n_accum  = 0;

    // second queue of the pipelined operator pass (small-slot kernels and tail stages overlap with the brick chunks) and a
    // ring of timing-free events for the cross-queue ordering
    hipStream_t             side = nullptr;
    std::vector<hipEvent_t> sync_events;
    size_t                  sync_next = 0;

    explicit Ctx(int dev);
    ~Ctx();
    void
    sync()
    {
      HIP_CHECK(hipStreamSynchronize(stream));
    }
    // `to` waits for everything enqueued on `from` so far
    void
    order_after(hipStream_t to, hipStream_t from)
    {
      hipEvent_t e = sync_events[sync_next];
      sync_next    = (sync_next + 1) % sync_events.size();
      HIP_CHECK(hipEventRecord(e, from));
      HIP_CHECK(hipStreamWaitEvent(to, e, 0));
    }
    void
    harvest_profile();
  };

  template <typename T>
  struct DBuf
  {
    T     *p = nullptr;
    size_t n = 0;
    DBuf() = default;
    DBuf(const DBuf &) = delete;
    DBuf &
    operator=(const DBuf &) = delete;
    ~DBuf()
    {
      if (p)
        (void)hipFree(p);
    }
    void
    alloc(size_t count)
    {
      if (p)
        (void)hipFree(p);
      p = nullptr;
      n = count;
      if (count)
        HIP_CHECK(hipMalloc((void **)&p, count * sizeof(T)));
    }
    void
    upload(const std::vector<T> &h)
    {
      alloc(h.size());
      if (n)
        HIP_CHECK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
    }
    void
    zero(hipStream_t s)
    {
      if (n)
        HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(T), s));
    }
  };
} // namespace mgamd

// ---- opaque handles -------------------------------------------------------------------------
struct mgamd_ctx
{
  std::unique_ptr<mgamd::Ctx> ctx;
};

struct mgamd_vec
{
  mgamd::Ctx *ctx  = nullptr;
  size_t      n    = 0;
  int         type = MGAMD_F64;
  void       *data = nullptr;
  ~mgamd_vec();
  template <typename T>
  T *
  as()
  {
    check<T>();
    return static_cast<T *>(data);
  }
  template <typename T>
  const T *
  as() const
  {
    check<T>();
    return static_cast<const T *>(data);
  }
  template <typename T>
  void
  check() const
  {
    if ((int)sizeof(T) != type)
      throw std::invalid_argument("vector number type does not match the operator's");
  }
};

namespace mgamd
{
  mgamd_vec *
  vec_create(Ctx *ctx, size_t n, int type);

  // launch helpers on type-erased vectors
  void
  vec_set(mgamd_vec &v, double value);
  void
  vec_copy(mgamd_vec &dst, const mgamd_vec &src);
  void
  vec_sadd(mgamd_vec &y, double s, double a, const mgamd_vec &x);
  double
  vec_dot(const mgamd_vec &x, const mgamd_vec &y);

  struct LevelOperatorBase;
  // A located point set of one operator (LevelOperatorBase::point_set_create); device vectors in the operator's number type.
  // evaluate: values [n] and/or gradients [3][n] in the caller's point order, exactly 0 where a point was not found; either output
  // may be null.  integrate: b is OVERWRITTEN with sum_k (w_k phi_i(x_k) + W_k . grad phi_i(x_k)) through C^T, constrained rows 0;
  // either input may be null, not both.  Stream-ordered, nothing is copied to the host.
  struct PointSetBase
  {
    LevelOperatorBase *op = nullptr;
    uint64_t           n = 0, n_found = 0;
    virtual ~PointSetBase() = default;
    virtual void
    get(int32_t *cell, double *ref) const = 0; // leaf (-1: not found) and reference coordinate [n][3] per point; either may be null
    virtual void
    evaluate(const mgamd_vec *u, mgamd_vec *values, mgamd_vec *gradients) = 0;
    virtual void
    integrate(const mgamd_vec *values, const mgamd_vec *gradients, mgamd_vec *b) = 0;
    // measurement: device bytes of the set, host time of its build (the binning by leaf), device times of its locate kernel and of
    // the last evaluate and the last integrate (HIP events; waits for them), 0 before the first
    virtual void
    info(uint64_t &bytes, double &build_ms, double &locate_ms, double &evaluate_ms, double &integrate_ms) const = 0;
  };

  struct LevelOperatorBase
  {
    Ctx                         *ctx  = nullptr;
    int                          type = MGAMD_F64;
    std::shared_ptr<LevelTables> tables;
    std::shared_ptr<Tria>        tria;
    std::shared_ptr<Comm>        comm; // sharded runs: set when this level is distributed
    std::shared_ptr<HaloPlan>    halo_plan;
    // mass coefficient of K + sigma M: the operator's OWN copy of tables->sigma, taken at construction (a time-stepping caller
    // changes it on the tables and builds new operators)
    double sigma = 0.0;
    // no Dirichlet face, sigma == 0 (the operator's own) and no convective face: the constants are in the kernel.  The operator, its mass product,
    // inverse diagonal and Chebyshev stay available; every solver built on it refuses through this (DESIGN.md "Boundary conditions")
    void
    refuse_singular(const char *who) const
    {
      if (tables->dirichlet_faces == 0 && sigma == 0.0 && !tables->has_robin())
        throw std::invalid_argument(std::string(who) + ": refused, the operator is singular: dirichlet_faces mask 0 (no Dirichlet face) with "
                                    "mass coefficient sigma = 0 and no convective face has the constants in its kernel, and no mean-value "
                                    "projection is built");
    }
    virtual ~LevelOperatorBase() = default;
    // inner product counting every DoF once across ranks (copies of DoFs owned by other ranks are skipped)
    virtual double
    dot(const mgamd_vec &x, const mgamd_vec &y) = 0;
    // sum over the sharing ranks of the tail entries of a vector (in place); no-op on one rank
    virtual void
    exchange_add_tail(mgamd_vec &v) = 0;
    uint64_t
    n_dofs_owned() const
    {
      return (uint64_t)tables->n_interior + tables->n_tail_owned + tables->n_dirichlet_owned + tables->n_hanging_owned;
    }
    uint32_t
    n_dofs() const
    {
      return tables->n_dofs;
    }
    // length of this rank's part of an inner product over the GLOBAL vector.  Sharded: the owned prefix [interior | owned tail],
    // which counts every DoF exactly once over the ranks (constrained entries are zero in every vector of the sharded solver
    // path: homogeneous data).  One rank: the whole vector, constrained rows included.
    size_t
    n_dot() const
    {
      return comm ? (size_t)tables->n_interior + tables->n_tail_owned : (size_t)n_dofs();
    }
    virtual void
    vmult(mgamd_vec &dst, const mgamd_vec &src) = 0;
    // dst = C^T M C src: the mass matrix of the level's space; rows and columns of constrained DoFs are zero (not on the
    // operator of a local-smoothing level)
    virtual void
    vmult_mass(mgamd_vec &dst, const mgamd_vec &src) = 0;
    virtual void
    compute_inverse_diagonal(mgamd_vec &d) = 0;
    virtual void
    vmult_interface_up(mgamd_vec &dst, const mgamd_vec &src) = 0; // local-smoothing levels: the edge matrix
    virtual void
    vmult_interface_down(mgamd_vec &dst, const mgamd_vec &src) = 0; // the level matrix of Multigrid's residual step
    virtual size_t
    read_debug_stamps(unsigned long long *out, size_t max_count) = 0;
    void
    rhs(mgamd_vec &b, int kind = 0);
    // b = the boundary load of the constant fluxes q[6] (LevelTables::compute_rhs_boundary_flux), completed over the ranks as rhs
    void
    rhs_boundary_flux(mgamd_vec &b, const double q[6]);
    void
    distribute(mgamd_vec &x, int kind);
    // Non-zero Dirichlet data (level_tables.hpp, DirichletCells): rhs = -[C^T (K_a + [include_mass] sigma M) C g^] on free rows, 0
    // on constrained rows, g^ = g on Dirichlet DoFs and 0 elsewhere; stream-ordered, completed over the ranks
    virtual void
    rhs_dirichlet(mgamd_vec &rhs, const mgamd_vec &g, bool include_mass) = 0;
    // x: Dirichlet DoFs from g, then hanging DoFs from their parents; free DoFs untouched; stream-ordered
    virtual void
    distribute_values(mgamd_vec &x, const mgamd_vec &g) = 0;
    // The jump error indicator eta_K of u per leaf, in the order of the mesh's cells, to the host array eta (kernels_estimator.hpp);
    // q: the six boundary fluxes of rhs_boundary_flux, or null for no boundary term.  Stream-ordered behind whatever the stream
    // holds for u; returns after the copy to the host.  The tables and the scratch are built by the first call.
    virtual void
    estimate_error(const mgamd_vec &u, const double *q, double *eta) = 0;
    // measurement: bytes of the indicator's device tables and scratch, host time of their build, device time of the two kernels
    // of the last call (HIP events); all 0 before the first call
    virtual void
    estimator_info(uint64_t &bytes, double &build_ms, double &kernel_ms) const = 0;
    // The error norms per leaf (kernels_error_norm.hpp), in the order of the mesh's cells, to the host array out.  kind 0, 1: the
    // built-in w (values and gradients null); kind -1: caller data at the quadrature points.  n_q: 0 for p + 2.  norm: MGAMD_NORM_*.
    // Stream-ordered behind whatever the stream holds for u; returns after the copy to the host.  The gather table is the
    // indicator's, built by whichever of the two comes first.
    virtual void
    integrate_difference(const mgamd_vec &u, int kind, const mgamd_vec *values, const mgamd_vec *gradients, int n_q, int norm, double *out) = 0;
    // measurement: bytes of the device arrays the error norms use (the shared gather table, the corners, the result), device time
    // of the kernel of the last call (HIP events), and whether the indicator's neighbour table is built; 0 before the first call
    virtual void
    error_norm_info(uint64_t &bytes, double &kernel_ms, int &neighbours_built) const = 0;
    // Cell evaluate and integrate (kernels_cell_values.hpp), device vectors in the operator's number type at the points of
    // LevelTables::quadrature_points(n_q), n_q: 0 for p + 2.  evaluate: values [cell][qz][qy][qx] and/or gradients
    // [cell][component][qz][qy][qx] of the level's Q_p function of u; either output may be null.  integrate: b is OVERWRITTEN with
    // sum_K sum_q w_q h_K^3 (v_q phi_i + V_q . grad phi_i) through C^T, constrained rows 0; either input may be null, not both.
    // Stream-ordered, nothing is copied to the host.  The gather table is the indicator's and the norms', built by whichever call
    // comes first.
    virtual void
    evaluate(const mgamd_vec *u, int n_q, mgamd_vec *values, mgamd_vec *gradients) = 0;
    virtual void
    integrate(const mgamd_vec *values, const mgamd_vec *gradients, int n_q, mgamd_vec *b) = 0;
    // measurement: bytes of the device arrays the two calls use (the shared gather table; they hold nothing else) and the device
    // times of the last evaluate and the last integrate (HIP events; waits for them); 0 before the first call
    virtual void
    cell_values_info(uint64_t &bytes, double &evaluate_ms, double &integrate_ms) const = 0;
    // Point evaluation and point sources (kernels_point_values.hpp).  A point set is n caller points (xyz[3k...], always double)
    // located on the device and binned by leaf once, then used for many vectors.  It belongs to this operator: its device arrays
    // are freed with the operator at the latest (a handle that outlives the operator refuses every call), point_set_destroy frees
    // them earlier.  The sorted Morton keys of the leaves are uploaded by the first point set,
    // the gather table (the indicator's, the norms' and the cell values') by the first evaluate or integrate.
    virtual std::shared_ptr<PointSetBase>
    point_set_create(uint64_t n, const double *xyz) = 0;
    virtual void
    point_set_destroy(PointSetBase *ps) = 0;
    // measurement: bytes of the operator's device arrays that only the point sets use (the keys and corners of the leaves), 0
    // before the first point set; and of the shared gather table, 0 until some call has built it
    virtual void
    point_tables_bytes(uint64_t &locator, uint64_t &gather) const = 0;

  private:
    // distribute_values without its refusals (sizes, local-smoothing levels): distribute(x, kind) runs on every level
    virtual void
    distribute_values_core(mgamd_vec &x, const mgamd_vec &g) = 0;
    void
    upload_load(mgamd_vec &b, const std::vector<double> &h);
  };

  struct ChebyshevBase
  {
    virtual ~ChebyshevBase() = default;
    LevelOperatorBase *op = nullptr;
    unsigned           degree = 3;
    double             min_eig = 0, max_eig = 0, theta = 1, delta = 0;
    virtual void
    vmult(mgamd_vec &dst, const mgamd_vec &src) = 0;
    virtual void
    step(mgamd_vec &dst, const mgamd_vec &src) = 0;
  };

  struct Transfer2Base
  {
    virtual ~Transfer2Base() = default;
    LevelOperatorBase *fine = nullptr, *coarse = nullptr;
    virtual void
    prolongate_and_add(mgamd_vec &dst_fine, const mgamd_vec &src_coarse) = 0;
    virtual void
    restrict_and_add(mgamd_vec &dst_coarse, const mgamd_vec &src_fine) = 0;
    // bricks of the fine level whose part of this transfer can run inside the level operator's passes (0: none)
    virtual uint64_t
    n_fused_bricks_total() const = 0;
  };

  struct MultigridBase
  {
    virtual ~MultigridBase() = default;
    Ctx                 *ctx = nullptr;
    mgamd_stage_callback cb  = nullptr;
    void                *cb_user = nullptr;
    virtual void
    vcycle(mgamd_vec &z, const mgamd_vec &r) = 0; // PreconditionMG::vmult
    virtual double
    time_vcycles(mgamd_vec &z, const mgamd_vec &r, unsigned n, bool use_graph) = 0;
    virtual unsigned
    n_levels() const = 0;
    // turn this hierarchy (levels built with mgamd_dofs_create_level) into a local-smoothing preconditioner of the problem on
    // the active mesh `active`
    virtual void
    setup_local_smoothing(const LevelTables &active) = 0;
    // switch the tabulated (collapsed) coarse levels on/off at run time; returns the collapse level (0: none)
    virtual unsigned
    set_collapse(bool on) = 0;
    // the coarse solver actually in use ("direct", "cg", "cg_with_chebyshev", "gmg_vcycle")
    std::string coarse_used;
    int         number_type = MGAMD_F64;
    virtual LevelOperatorBase *
    finest_operator() const = 0;
    // tables of the vectors vcycle() acts on: the finest level's, or the active mesh's for local smoothing
    virtual const LevelTables *
    outer_tables() const = 0;
    // z = V-cycle(r) on raw device pointers of the LEVEL number type (nested use)
    virtual void
    vcycle_level_raw(void *z, const void *r) = 0;
    // the algebraic coarse solver's levels, 5 numbers each: global rows, owned rows, ghosts, peers, replicated (empty: no AMG)
    virtual void
    amg_layout(std::vector<uint32_t> &out) const = 0;
    // inner CG iterations of the coarse solvers cg, cg_with_chebyshev, cg_with_amg, accumulated since construction
    virtual uint64_t
    coarse_cg_iterations() const = 0;

    // Stage times without host synchronisation: a HIP event pair is recorded on the stream around every stage of the
    // UNCHANGED cycle (same code path as an un-instrumented cycle, collapsed coarse levels included) and resolved when read.
    struct StageRecord
    {
      int        stage;
      unsigned   level;
      hipEvent_t e0, e1;
    };
    bool                     stage_timing = false;
    std::vector<StageRecord> stage_records;
    size_t                   stage_used = 0;
    void
    set_stage_timing(bool on)
    {
      ctx->sync();
      stage_timing = on;
      stage_used   = 0;
    }
    // ms[stage * n_levels + level] += elapsed; returns the number of records consumed
    size_t
    read_stage_times(double *ms)
    {
      ctx->sync();
      for (size_t i = 0; i < stage_used; ++i)
        {
          float t = 0;
          HIP_CHECK(hipEventElapsedTime(&t, stage_records[i].e0, stage_records[i].e1));
          ms[(size_t)stage_records[i].stage * n_levels() + stage_records[i].level] += t;
        }
      const size_t n = stage_used;
      stage_used     = 0;
      return n;
    }
    void
    release_stage_records()
    {
      for (auto &r : stage_records)
        {
          (void)hipEventDestroy(r.e0);
          (void)hipEventDestroy(r.e1);
        }
      stage_records.clear();
    }
  };

  LevelOperatorBase *
  make_level_operator(Ctx *ctx, const mgamd_dofs *dofs, int type, std::shared_ptr<Comm> comm = nullptr);
  ChebyshevBase *
  make_chebyshev(LevelOperatorBase *op, unsigned degree, double smoothing_range, unsigned eig_cg_n_iterations);
  Transfer2Base *
  make_transfer2(LevelOperatorBase *fine, LevelOperatorBase *coarse);
  // amg_global != nullptr (the global tables of level 0's space): the AMG coarse solvers run on a sharded level 0 (amg_shard.hpp),
  // levels of at most amg_min_sharded_rows rows replicated
  // nested != nullptr: the coarse problem is handed to `n_cycles` V-cycles of another multigrid whose finest level is
  // levels[0] (the geometric stand-in for the reference's Trilinos/PETSc AMG coarse solvers on large coarse levels)
  MultigridBase *
  make_multigrid(Ctx *ctx, unsigned n_levels, LevelOperatorBase *const *levels, Transfer2Base *const *transfers,
                 ChebyshevBase *const *smoothers, const std::string &coarse_solver, MultigridBase *nested = nullptr,
                 unsigned n_cycles = 1, const LevelTables *amg_global = nullptr, uint32_t amg_min_sharded_rows = 0);
  void
  solve_cg(LevelOperatorBase &A, MultigridBase *M, mgamd_vec &x, const mgamd_vec &b, double reltol, double abstol, unsigned maxiter,
           unsigned &n_iterations, double &residual);
  // theta-scheme for  M u' + K u = M f  (homogeneous Dirichlet data, constraints eliminated) with constant step dt on the
  // operator A = K + sigma M, sigma = 1 / (theta dt), and its multigrid.  One step, written for the increment delta = u_new - u:
  //     w = theta f_new + (1 - theta) f_old + sigma u;   t = M w (vmult_mass);   r = t - A u (residual pass), 0 on constrained rows;
  //     A delta = r / theta by solve_cg's device PCG from delta = 0 (reltol acts on the increment's residual);   u += delta
  // Work vectors are allocated once, here; every launch goes to the context's stream; the host read-backs are the PCG's.
  struct ThetaStepperBase
  {
    virtual ~ThetaStepperBase() = default;
    double   theta = 1, dt = 0, t = 0;
    uint64_t n_steps = 0;
    // f_old, f_new: nodal source values at t and t + dt, both null for f = 0.  u is advanced in place; its constrained entries
    // are not read and are 0 on return
    virtual void
    step(mgamd_vec &u, const mgamd_vec *f_old, const mgamd_vec *f_new, double reltol, double abstol, unsigned maxiter, unsigned &n_iterations,
         double &residual) = 0;
    // The same step with non-zero Dirichlet data and a boundary load.  g_old, g_new: Dirichlet values at t and t + dt (only their
    // entries at Dirichlet DoFs are read), both null for homogeneous data; load: l = theta l_new + (1 - theta) l_old (a flux,
    // beta u_ext), may be null.  On the free rows
    //     A delta = (M w + l - A u - K_ID g_old) / theta - A_ID (g_new - g_old),   u += delta
    // with two launches of the lifting kernel.  All three null: the launches of step, in its order.
    virtual void
    step_data(mgamd_vec &u, const mgamd_vec *f_old, const mgamd_vec *f_new, const mgamd_vec *g_old, const mgamd_vec *g_new, const mgamd_vec *load,
              double reltol, double abstol, unsigned maxiter, unsigned &n_iterations, double &residual) = 0;
  };
  ThetaStepperBase *
  make_theta_stepper(LevelOperatorBase &A, MultigridBase *M, double theta, double dt);
  // K7 (kernels_amg.hpp) as the AMG cycle launches it: lanes per row from the average row length, a grid of at most 4096 blocks
  // (grid-stride above); mode: SpmvMode; lanes 0 = csr_spmv_lanes
  int
  csr_spmv_lanes(uint32_t n_rows, size_t nnz);
  // K8 (one wave64 per row, lanes = 64) above this mean row length, K7's choice below: the assembled operator and its AMG only
  // (between the measured 102, where K8 loses, and 185, where it wins: profiles/amg_solver_spmv.txt; MGAMD_SPMV_WAVE_MIN_MEAN_ROW
  // in the environment replaces it: development and tests)
  constexpr double CSR_SPMV_WAVE_MIN_MEAN_ROW = 144.0;
  int
  csr_spmv_lanes_long(uint32_t n_rows, size_t nnz);
  // returns the blocks launched; mode SPMV_DOT: one partial of x . y per block in `partial` (at most 1024); max_blocks > 0: a
  // lower cap on the grid
  template <typename T>
  int
  launch_csr_spmv(hipStream_t stream, int mode, int lanes, uint32_t n_rows, const uint32_t *ptr, const uint32_t *col, const T *val, const T *x,
                  T *y, const T *b, const T *xold, const T *dinv, double f1, double f2, double *partial = nullptr, int max_blocks = 0);

  // ---- CG on the assembled matrix with the AMG preconditioner: the reference's Type "AMG" / "AMGPETSc", solve_with_amg
  // (ref:multigrid_throughput.cc:1877-1966).  FP64, one rank, global-coarsening levels.
  // Operator::get_trilinos_system_matrix (ref:include/operator.h:244-287) on the device: vmult is a plain CSR product
  struct AssembledMatrixBase
  {
    virtual ~AssembledMatrixBase() = default;
    Ctx     *ctx    = nullptr;
    uint32_t n_rows = 0;
    uint64_t nnz    = 0;
    int      lanes  = 0; // lanes per row of its products (csr_spmv_lanes_long)
    virtual void
    vmult(mgamd_vec &dst, const mgamd_vec &src) = 0;
    // measurement (tools/spmv_bench.py): milliseconds per launch of the product in `mode` at `lanes` lanes per row, HIP events
    // around `reps` launches after one warm-up launch, on scratch vectors
    virtual double
    time_spmv(int mode, int lanes, unsigned reps) = 0;
  };
  // TrilinosWrappers::PreconditionAMG on that matrix (ref:multigrid_throughput.cc:1907-1909): n_cycles V-cycles of the library's
  // smoothed-aggregation AMG (amg.hpp); level 0 works on the operator's device matrix, which it keeps alive
  struct AmgPreconditionerBase
  {
    virtual ~AmgPreconditionerBase() = default;
    virtual void
    vmult(mgamd_vec &z, const mgamd_vec &r) = 0;
    virtual void
    layout(std::vector<uint32_t> &rows_per_level) const = 0;
  };
  std::shared_ptr<AssembledMatrixBase>
  make_assembled_matrix(Ctx *ctx, const mgamd_dofs *dofs);
  AmgPreconditionerBase *
  make_amg_preconditioner(const std::shared_ptr<AssembledMatrixBase> &A, unsigned n_cycles);
  // SolverCG on the matrix (ref:multigrid_throughput.cc:1911-1915); M null: no preconditioner.  A p and p . A p come from one
  // SPMV_DOT launch (MGAMD_NO_FUSED_DOT=1 in the environment: the product, then the inner product, as the other solvers do)
  void
  solve_cg_matrix(AssembledMatrixBase &A, AmgPreconditionerBase *M, mgamd_vec &x, const mgamd_vec &b, double reltol, double abstol,
                  unsigned maxiter, unsigned &n_iterations, double &residual);
} // namespace mgamd

struct mgamd_level_op
{
  std::unique_ptr<mgamd::LevelOperatorBase> op;
};
struct mgamd_point_set
{
  std::shared_ptr<mgamd::PointSetBase> ps;
};
struct mgamd_cheb
{
  std::unique_ptr<mgamd::ChebyshevBase> c;
};
struct mgamd_transfer2
{
  std::unique_ptr<mgamd::Transfer2Base> t;
};
struct mgamd_mg
{
  std::unique_ptr<mgamd::MultigridBase> mg;
};
struct mgamd_time_stepper
{
  std::unique_ptr<mgamd::ThetaStepperBase> ts;
};
struct mgamd_matrix
{
  std::shared_ptr<mgamd::AssembledMatrixBase> A;
};
struct mgamd_amg
{
  std::unique_ptr<mgamd::AmgPreconditionerBase> P;
};
