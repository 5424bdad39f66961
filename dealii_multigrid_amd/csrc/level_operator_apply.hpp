// LevelOperator<T>::apply_P: the launch logic of one operator application.  Included by apply_inst.hip only (see
// level_operator.hpp): every (number type, degree, mode) instantiation pulls in the kernels of kernels.hpp for its slot groups.
#pragma once
#include "level_operator.hpp"

namespace mgamd
{
  template <typename T>
  template <int P, int MODE>
  void
  LevelOperator<T>::apply_P(const T *src, const Epilogue<T> &epi, bool diag, double words, int edge_mode, const FusedTransferHost<T> *fused)
  {
    ApplyArgs<T, P> a;
    const uint32_t  first_edge = tables->n_interior + tables->n_tail;
    a.gather_limit  = first_edge + (edge_mode == EDGE_IN ? tables->n_edge : 0);
    a.scatter_limit = first_edge + (edge_mode != EDGE_OUT ? tables->n_edge : 0);
    const uint32_t tail_end = tables->n_tail + (edge_mode != EDGE_OUT ? tables->n_edge : 0);
    a.m          = mats<P>();
    a.src        = src;
    a.tail_acc   = tail_acc.p;
    a.n_interior = tables->n_interior;
    a.ablate     = ablate;
    a.stamps     = nullptr;
    a.epi        = epi;
    a.sigma      = sigma;
    // Sharded level: the slots that touch shared DoFs first, then the halo exchange on the side queue UNDERNEATH the remaining
    // slots (ref: MatrixFree::cell_loop overlaps its ghost exchange with the interior cell ranges, ref:include/operator.h:166-167).
    if (!diag && !plan.interior_slots.empty())
      {
        for (const LaunchStep &s : plan.halo_slots)
          launch_step<P, MODE>(ctx->stream, a, s, false, fused);
        ctx->order_after(ctx->side, ctx->stream); // the side queue waits for the halo slots only
        // the exchange is enqueued BEFORE the interior slots: their persistent workgroups fill every CU's LDS until the
        // launch ends, so RCCL's send/recv kernels must be resident first to run underneath them (the simulator's
        // exchange blocks the host instead: no overlap there, same results)
        exchange_add_raw(tail_acc.p, ctx->side);
        for (const LaunchStep &s : plan.interior_slots)
          launch_step<P, MODE>(ctx->stream, a, s, false, fused);
        ctx->order_after(ctx->stream, ctx->side);
        launch_tail<MODE>(ctx->stream, 0, tail_end, true, epi, diag);
        return;
      }
    const hipStream_t main = ctx->stream;
    auto prof_begin = [&](const GroupDev<T> &g) {
      const bool prof = ctx->profile && !diag && MODE == MODE_CHEB && !g.constrained && g.B == (ctx->prof_brick ? ctx->prof_brick : dominant_B);
      if (prof)
        {
          if (ctx->prof_used == ctx->prof_events.size())
            {
              hipEvent_t e0, e1;
              HIP_CHECK(hipEventCreate(&e0));
              HIP_CHECK(hipEventCreate(&e1));
              ctx->prof_events.push_back({e0, e1});
            }
          HIP_CHECK(hipEventRecord(ctx->prof_events[ctx->prof_used].first, main));
        }
      return prof;
    };
    auto prof_end = [&](const GroupDev<T> &g, size_t n_slots) {
      HIP_CHECK(hipEventRecord(ctx->prof_events[ctx->prof_used].second, main));
      ++ctx->prof_used;
      // algorithmic bytes of THIS kernel: `words` per slot-interior DoF (the fused epilogue is complete for them); for
      // the (N-1)^3 - (N-2)^3 shell DoFs a brick is responsible for, one gathered word and one partial sum (the other
      // words of their epilogue are tail_kernel's)
      // (D^-1 of slot-interior DoFs is evaluated in closed form, not read, by the p = 1 kernels and by the persistent
      // 17-point lattice kernels: one word less per interior DoF)
      // prof_bytes keeps SURVEY 8(d)'s per-unit figure (the algorithm's words); prof_bytes_moved is the kernel's own count
      const bool   closed_dinv = P == 1 || persistent_lattice(g.N);
      const double w_interior  = words - (closed_dinv ? 1.0 : 0.0);
      const double n1 = (double)(g.N - 1), n2 = (double)(g.N - 2);
      ctx->prof_bytes += sizeof(T) * (double)n_slots * (words * n2 * n2 * n2 + 2.0 * (n1 * n1 * n1 - n2 * n2 * n2));
      ctx->prof_bytes_moved += sizeof(T) * (double)n_slots * (w_interior * n2 * n2 * n2 + 2.0 * (n1 * n1 * n1 - n2 * n2 * n2));
    };
    for (const LaunchStep &s : diag ? plan.diagonal : plan.ordinary)
      {
        const bool prof = s.g && prof_begin(*s.g); // (the step of the convective faces has no slot group)
        launch_step<P, MODE>(main, a, s, diag, fused, !diag);
        if (prof)
          prof_end(*s.g, s.g->n_slots);
      }
    if (halo)
      exchange_add_raw(tail_acc.p); // complete the shared tail sums across ranks before the epilogue
    // The fused residual pass: the fused bricks write neither t nor the accumulator, so only the rows that a slot outside the
    // fused set touches are finished (they are the rows of t the un-fused patches restrict, and the accumulator entries to
    // re-zero), plus the constrained rows.  Measured on octant p=4, level 8: 18 % of the tail, 153 -> 41 us.
    // A sharded level keeps the whole tail: the exchange adds remote sums to entries outside that set.
    if constexpr (MODE == MODE_RESIDUAL_RESTRICT)
      if (!diag && !halo && !tables->n_edge && fused && fused->tail_chunks)
        return launch_tail_runs<MODE>(main, fused->tail_chunks, fused->n_tail_chunks, epi);
    launch_tail<MODE>(main, 0, tail_end, true, epi, diag);
  }

  template <typename T>
  template <int P>
  void
  LevelOperator<T>::lift_P(T *dst, const T *g, double mass_sigma, double alpha)
  {
    DirichletLiftArgs<T, P> a;
    a.idx     = dirichlet->idx.p;
    a.mask    = dirichlet->mask.p;
    a.scale   = dirichlet->scale.p;
    a.n_cells = dirichlet->n_cells;
    for (int i = 0; i < (P + 1) * (P + 1); ++i)
      {
        a.K[i]  = tables->fe.K[i];
        a.M[i]  = tables->fe.M[i];
        a.I0[i] = tables->fe.I[0][i];
        a.I1[i] = tables->fe.I[1][i];
      }
    a.g               = g;
    a.dst             = dst;
    a.dirichlet_begin = tables->first_dirichlet();
    a.dirichlet_end   = tables->first_dirichlet() + tables->n_dirichlet;
    a.scatter_limit   = tables->first_constrained(); // the free rows; on a sharded level the copies of shared rows too (the exchange sums them)
    a.alpha           = (T)alpha;
    a.sigma           = (T)mass_sigma;
    // two groups of cells per workgroup where there are that many: the 1D matrices are staged in LDS once per workgroup
    const uint32_t n_groups = (a.n_cells + dirichlet_cells_per_workgroup<P>() - 1) / dirichlet_cells_per_workgroup<P>();
    const uint32_t grid     = std::min<uint32_t>(2048u, (n_groups + 1) / 2);
    hipLaunchKernelGGL((dirichlet_lift_kernel<T, P>), grid, 256, 0, ctx->stream, a);
    HIP_CHECK(hipGetLastError());
  }

  template <typename T>
  template <int P>
  void
  LevelOperator<T>::estimate_P(const T *u, const double *q)
  {
    constexpr int N = P + 1, N2 = N * N;
    EstimatorDev &e = *estimator;
    if (!e.n_cells)
      return;
    FaceFluxArgs<T, P> a;
    a.idx     = e.idx.p;
    a.mask    = e.mask.p;
    a.scale   = e.scale.p;
    a.code    = e.code.p;
    a.n_cells = e.n_cells;
    a.n_dofs  = n_dofs();
    a.u       = u;
    a.flux    = e.flux.p;
    FluxJumpArgs<T, P> b;
    b.flux    = e.flux.p;
    b.code    = e.code.p;
    b.nbr     = e.nbr.p;
    b.scale   = e.scale.p;
    b.n_cells = e.n_cells;
    b.eta     = e.eta.p;
    for (int i = 0; i < N; ++i)
      {
        a.D[i]     = tables->fe.D[0][i];
        a.D[N + i] = tables->fe.D[1][i];
      }
    for (int i = 0; i < N2; ++i)
      {
        a.I0[i] = b.I0[i] = tables->fe.I[0][i];
        a.I1[i] = b.I1[i] = tables->fe.I[1][i];
        b.M[i]  = tables->fe.M[i];
      }
    a.natural = 0;
    for (int f = 0; f < 6; ++f)
      {
        a.q[f]    = q ? q[f] : 0.0;
        a.beta[f] = tables->robin[f];
        if (q && !((tables->dirichlet_faces >> f) & 1))
          a.natural |= 1u << f;
      }
    // two groups of cells per workgroup where there are that many: the 1D matrices are staged in LDS once per workgroup
    const uint32_t groups_a = (e.n_cells + dirichlet_cells_per_workgroup<P>() - 1) / dirichlet_cells_per_workgroup<P>();
    const uint32_t groups_b = (e.n_cells + jump_cells_per_workgroup<P>() - 1) / jump_cells_per_workgroup<P>();
    hipLaunchKernelGGL((face_flux_kernel<T, P>), std::min<uint32_t>(4096u, (groups_a + 1) / 2), 256, 0, ctx->stream, a);
    hipLaunchKernelGGL((flux_jump_kernel<T, P>), std::min<uint32_t>(4096u, (groups_b + 1) / 2), 256, 0, ctx->stream, b);
    HIP_CHECK(hipGetLastError());
  }

  template <typename T>
  template <int P>
  void
  LevelOperator<T>::difference_norm_P(const T *u, int kind, const T *values, const T *gradients, int n_q, int norm)
  {
    constexpr int N = P + 1, N2 = N * N;
    EstimatorDev &e = *estimator;
    if (!e.n_cells)
      return;
    DifferenceNormArgs<T, P> a;
    static_assert(DifferenceNormArgs<T, P>::NQM <= FE1D::MAX_GAUSS_POINTS, "the rule generator is held to 10 points");
    if (n_q < N || n_q > DifferenceNormArgs<T, P>::NQM)
      throw std::invalid_argument("integrate_difference: n_q outside p + 1 ... p + 3"); // (resolve_n_q refused it already: the LDS bound)
    a.idx       = e.idx.p;
    a.mask      = e.mask.p;
    a.scale     = e.scale.p;
    a.origin    = e.origin.p;
    a.n_cells   = e.n_cells;
    a.n_dofs    = n_dofs();
    a.u         = u;
    a.values    = values;
    a.gradients = gradients;
    a.out       = e.norm_out.p;
    a.kind      = kind;
    a.norm      = norm;
    a.n_q       = n_q;
    a.sigma     = sigma; // the operator's own: what it was built with
    std::vector<double> xq, wq, S, G;
    tables->fe.shape_at_gauss(n_q, xq, wq, S, G);
    std::memset(a.S, 0, sizeof(a.S));
    std::memset(a.G, 0, sizeof(a.G));
    std::memset(a.xq, 0, sizeof(a.xq));
    std::memset(a.wq, 0, sizeof(a.wq));
    std::copy(S.begin(), S.end(), a.S);
    std::copy(G.begin(), G.end(), a.G);
    std::copy(xq.begin(), xq.end(), a.xq);
    std::copy(wq.begin(), wq.end(), a.wq);
    for (int i = 0; i < N2; ++i)
      {
        a.I0[i] = tables->fe.I[0][i];
        a.I1[i] = tables->fe.I[1][i];
      }
    // two groups of leaves per workgroup where there are that many: the 1D matrices are staged in LDS once per workgroup
    const uint32_t groups = (e.n_cells + dirichlet_cells_per_workgroup<P>() - 1) / dirichlet_cells_per_workgroup<P>();
    hipLaunchKernelGGL((difference_norm_kernel<T, P>), std::min<uint32_t>(4096u, (groups + 1) / 2), 256, 0, ctx->stream, a);
    HIP_CHECK(hipGetLastError());
  }

  // the 1D matrices of cell_evaluate_kernel and cell_integrate_kernel for the rule QGauss(n_q): the members both argument structs share
  template <typename Args>
  static void
  fill_cell_values_matrices(Args &a, const FE1D &fe, int n_q, std::vector<double> &wq)
  {
    const int n = fe.p + 1;
    static_assert(Args::NQM <= FE1D::MAX_GAUSS_POINTS, "the rule generator is held to 10 points");
    if (n_q < n || n_q > Args::NQM)
      throw std::invalid_argument("cell values: n_q outside p + 1 ... p + 3"); // (resolve_n_q refused it already: the LDS bound)
    std::vector<double> xq, S, G;
    fe.shape_at_gauss(n_q, xq, wq, S, G);
    std::memset(a.S, 0, sizeof(a.S));
    std::memset(a.G, 0, sizeof(a.G));
    std::copy(S.begin(), S.end(), a.S);
    std::copy(G.begin(), G.end(), a.G);
    for (int i = 0; i < n * n; ++i)
      {
        a.I0[i] = fe.I[0][i];
        a.I1[i] = fe.I[1][i];
      }
    a.n_q = n_q;
  }

  template <typename T>
  template <int P>
  void
  LevelOperator<T>::cell_evaluate_P(const T *u, int n_q, T *values, T *gradients)
  {
    EstimatorDev &e = *estimator;
    if (!e.n_cells)
      return;
    CellEvaluateArgs<T, P> a;
    std::vector<double>    wq;
    fill_cell_values_matrices(a, tables->fe, n_q, wq);
    a.idx       = e.idx.p;
    a.mask      = e.mask.p;
    a.scale     = e.scale.p;
    a.n_cells   = e.n_cells;
    a.n_dofs    = n_dofs();
    a.u         = u;
    a.values    = values;
    a.gradients = gradients;
    // two groups of leaves per workgroup where there are that many: the 1D matrices are staged in LDS once per workgroup
    const uint32_t groups = (e.n_cells + dirichlet_cells_per_workgroup<P>() - 1) / dirichlet_cells_per_workgroup<P>();
    hipLaunchKernelGGL((cell_evaluate_kernel<T, P>), std::min<uint32_t>(4096u, (groups + 1) / 2), 256, 0, ctx->stream, a);
    HIP_CHECK(hipGetLastError());
  }

  template <typename T>
  template <int P>
  void
  LevelOperator<T>::cell_integrate_P(const T *values, const T *gradients, int n_q, T *b)
  {
    EstimatorDev &e = *estimator;
    if (!e.n_cells)
      return;
    CellIntegrateArgs<T, P> a;
    std::vector<double>     wq;
    fill_cell_values_matrices(a, tables->fe, n_q, wq);
    std::memset(a.wq, 0, sizeof(a.wq));
    std::copy(wq.begin(), wq.end(), a.wq);
    a.idx           = e.idx.p;
    a.mask          = e.mask.p;
    a.scale         = e.scale.p;
    a.n_cells       = e.n_cells;
    a.scatter_limit = tables->first_constrained(); // the free rows
    a.values        = values;
    a.gradients     = gradients;
    a.dst           = b;
    const uint32_t groups = (e.n_cells + integrate_cells_per_workgroup<P>() - 1) / integrate_cells_per_workgroup<P>();
    hipLaunchKernelGGL((cell_integrate_kernel<T, P>), std::min<uint32_t>(4096u, (groups + 1) / 2), 256, 0, ctx->stream, a);
    HIP_CHECK(hipGetLastError());
  }

  // what point_evaluate_kernel and point_integrate_kernel share: the gather table, the set's CSR list and the 1D element
  template <int P, typename Estimator, typename Set>
  static void
  fill_point_walk(PointWalkArgs<P> &w, const Estimator &e, const Set &ps, const FE1D &fe)
  {
    const int n = P + 1;
    w.idx        = e.idx.p;
    w.mask       = e.mask.p;
    w.scale      = e.scale.p;
    w.leaf       = ps.leaf.p;
    w.ptr        = ps.ptr.p;
    w.perm       = ps.perm.p;
    w.occ        = ps.occ.p;
    w.ref        = ps.ref.p;
    w.n_occupied = ps.n_occupied;
    w.n_points   = (uint32_t)ps.n;
    for (int i = 0; i < n * n; ++i)
      {
        w.I0[i] = fe.I[0][i];
        w.I1[i] = fe.I[1][i];
      }
    for (int a = 0; a < n; ++a)
      {
        long double den = 1.0L;
        for (int b = 0; b < n; ++b)
          if (b != a)
            den *= (long double)fe.nodes[a] - fe.nodes[b];
        w.nodes[a]   = fe.nodes[a];
        w.inv_den[a] = (double)(1.0L / den);
      }
  }

  template <typename T>
  template <int P>
  void
  LevelOperator<T>::point_evaluate_P(const PointSetDev &ps, const T *u, T *values, T *gradients)
  {
    PointEvaluateArgs<T, P> a;
    fill_point_walk<P>(a.w, *estimator, ps, tables->fe);
    a.n_dofs    = n_dofs();
    a.u         = u;
    a.values    = values;
    a.gradients = gradients;
    const uint32_t groups = (ps.n_occupied + dirichlet_cells_per_workgroup<P>() - 1) / dirichlet_cells_per_workgroup<P>();
    hipLaunchKernelGGL((point_evaluate_kernel<T, P>), std::min<uint32_t>(4096u, groups), 256, 0, ctx->stream, a);
    HIP_CHECK(hipGetLastError());
  }

  template <typename T>
  template <int P>
  void
  LevelOperator<T>::point_integrate_P(const PointSetDev &ps, const T *values, const T *gradients, T *b)
  {
    PointIntegrateArgs<T, P> a;
    fill_point_walk<P>(a.w, *estimator, ps, tables->fe);
    a.scatter_limit = tables->first_constrained(); // the free rows
    a.values        = values;
    a.gradients     = gradients;
    a.dst           = b;
    const uint32_t groups = (ps.n_occupied + dirichlet_cells_per_workgroup<P>() - 1) / dirichlet_cells_per_workgroup<P>();
    hipLaunchKernelGGL((point_integrate_kernel<T, P>), std::min<uint32_t>(4096u, groups), 256, 0, ctx->stream, a);
    HIP_CHECK(hipGetLastError());
  }

} // namespace mgamd
