// The level operator (Operator<3,1,Number>, ref:include/operator.h:11-557) on the device: slot groups, tail accumulator,
// halo plan, and the launch logic of one operator application (apply_P).  Class template in a header so that the kernel
// instantiations behind apply_P<P, MODE> are compiled in their own translation units (apply_inst.hip, one per number type
// and degree, built in parallel); runtime.hip sees them through the explicit instantiation declarations at the end.
#pragma once
#include "runtime.hpp"
#include "kernels.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>
#include <unordered_map>

namespace mgamd
{
  inline int
  grid_for(size_t n)
  {
    size_t g = (n + 255) / 256;
    if (g > 2048)
      g = 2048;
    if (g < 1)
      g = 1;
    return (int)g;
  }

  template <typename T>
  inline double
  dot_raw(Ctx *ctx, const T *x, const T *y, size_t n)
  {
    if (!n)
      return 0.0;
    int g = grid_for(n);
    if (g > 1024)
      g = 1024;
    hipLaunchKernelGGL(vec_dot_kernel<T>, g, 256, 0, ctx->stream, x, y, n, ctx->d_partial);
    hipLaunchKernelGGL(vec_dot_final_kernel<>, 1, 256, 0, ctx->stream, ctx->d_partial, g, ctx->d_result);
    HIP_CHECK(hipMemcpyAsync(ctx->h_result, ctx->d_result, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    return ctx->h_result[0];
  }

  // ------------------------------------------------------------------------------------------
  // Level operator
  // ------------------------------------------------------------------------------------------
  // hipFuncAttributeMaxDynamicSharedMemorySize per (device, kernel), raised whenever a launch asks for more than the value
  // set so far; recorded only after the call has succeeded.  Callers may be concurrent host threads (SimComm).
  inline void
  ensure_dynamic_lds(Ctx *ctx, const void *kern, size_t lds)
  {
    static std::mutex                                      m;
    static std::map<std::pair<int, const void *>, size_t> done;
    std::lock_guard<std::mutex>                            lock(m);
    auto                                                   it = done.find({ctx->device, kern});
    if (it != done.end() && it->second >= lds)
      return;
    HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    done[{ctx->device, kern}] = lds;
  }

  // a launch with dynamic LDS above the default limit
  template <typename A>
  inline void
  launch_lds(Ctx *ctx, hipStream_t st, void (*kern)(A), int grid, int block, size_t lds, const A &args)
  {
    ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), lds);
    hipLaunchKernelGGL(kern, grid, block, lds, st, args);
  }

  // two 4-wave workgroups with a 17^3 lattice pair each fit one CU; a multiple of 8 keeps a workgroup in its XCD's range
  inline int
  resident_workgroups(const Ctx *ctx, int per_cu = 2)
  {
    return std::max(8, per_cu * ctx->n_cu / 8 * 8);
  }

  // a launch of PERSISTENT workgroups: at most the resident ones (per_cu on every CU), which walk the n_work items
  // grid_cap > 0: at most that many (LevelOperator::persistent_grid_cap, a development switch)
  inline int
  persistent_grid(const Ctx *ctx, int n_work, int per_cu, int grid_cap)
  {
    const int resident = resident_workgroups(ctx, per_cu);
    return std::min(n_work, grid_cap > 0 ? std::min(resident, grid_cap) : resident);
  }
  template <typename A>
  inline void
  launch_persistent(Ctx *ctx, hipStream_t st, void (*kern)(A), int n_work, int per_cu, int block, size_t lds, const A &args, int grid_cap = 0)
  {
    launch_lds(ctx, st, kern, persistent_grid(ctx, n_work, per_cu, grid_cap), block, lds, args);
  }

  // f(std::integral_constant<int, V>) for the V among Vs... that equals v; false if there is none
  template <int... Vs, typename F>
  inline bool
  dispatch_value(int v, F &&f)
  {
    return ((v == Vs && (f(std::integral_constant<int, Vs>()), true)) || ...);
  }
  // the instantiated degrees
  template <typename F>
  inline bool
  dispatch_degree(int p, F &&f)
  {
    return dispatch_value<1, 2, 3, 4, 5, 6, 7>(p, f);
  }
  // the brick sizes among Bs... whose lattice of degree P has at most 17 points
  template <int P, int... Bs, typename F>
  inline bool
  dispatch_brick_size(int B, F &&f)
  {
    return P * B + 1 <= 17 && dispatch_value<Bs...>(B, [&](auto b) {
             if constexpr (P * b() + 1 <= 17)
               f(b);
           });
  }

  // one slot group: its diagonal, or one operator application with the kernel of its lattice
  template <typename T, int P, int B, int MODE, bool CONSTR = false>
  inline void
  launch_lattice(Ctx *ctx, hipStream_t st, const ApplyArgs<T, P> &a, bool diag, int grid_cap = 0)
  {
    using G = Geo<P, B>;
    if (a.g.n_slots == 0)
      return;
    const int grid = (int)((a.g.n_slots + G::SPW - 1) / G::SPW);
    if (diag)
      launch_lds(ctx, st, lattice_diag_kernel<T, P, B, CONSTR>, grid, G::BLOCK, 3 * (size_t)G::SPW * G::N3 * sizeof(T), a);
    else if constexpr (B == 1 && P >= 2)
      { // single cells wave-scoped (kernels.hpp cell_waves_kernel)
        using GW = Geo<P, 1, 64>;
        const uint32_t n_w    = (uint32_t)((a.g.n_slots + GW::SPW - 1) / GW::SPW);
        const uint32_t grid_w = (n_w + CELL_WAVES - 1) / CELL_WAVES;
        constexpr size_t lds  = CELL_WAVES * cell_wave_lds<T, P>();
        static_assert(lds <= 64 * 1024, "above the default dynamic-LDS limit the launch has to go through launch_lds");
        hipLaunchKernelGGL((cell_waves_kernel<T, P, MODE>), grid_w, 64 * CELL_WAVES, lds, st, a);
      }
    else if constexpr (persistent_lattice(G::N))
      // one-slot-per-workgroup lattices (17^3): persistent workgroups with a software pipeline over their slots
      // (kernels.hpp, lattice_apply_persistent_body).  Two workgroups fit a CU (LDS); the grid is a multiple of 8 so
      // that a workgroup stays inside the Morton range of its XCD.
      // (the mass term is compiled in or out of these kernels: kernels.hpp, lattice_apply_persistent_body; the mass PASS has no
      // such term and one form)
      {
        void (*kern)(ApplyArgs<T, P>) = lattice_apply_persistent_kernel<T, P, B, MODE, CONSTR, false>;
        if constexpr (MODE != MODE_MASS)
          if (a.sigma != 0.0)
            kern = lattice_apply_persistent_kernel<T, P, B, MODE, CONSTR, true>;
        launch_persistent(ctx, st, kern, grid, persistent_wgs_per_cu<T, P>(), G::ABLOCK, apply_lds_bytes<T, P, B>(), a, grid_cap);
      }
    else
      launch_lds(ctx, st, lattice_apply_kernel<T, P, B, MODE, CONSTR>, grid, G::ABLOCK, apply_lds_bytes<T, P, B>(), a);
    HIP_CHECK(hipGetLastError());
  }

  template <typename T>
  struct GroupDev
  {
    int            B = 1, N = 2;
    bool           constrained = false; // the group of constrained bricks larger than a family
    size_t         n_halo      = 0;     // sharded levels: the first n_halo slots touch DoFs shared with other ranks
    size_t         n_slots = 0;
    DBuf<uint32_t> interior_base, shell_idx;
    DBuf<uint16_t> mask, shell_pos;
    // Per slot, with the slot's diffusion coefficient a (SlotGroup::a): the operator's scale a h, the mass term's factor
    // h^2 / a, and the cell size h itself for the mass pass (MODE_MASS; only held where some a != 1, otherwise it is `h`).
    DBuf<double>   h, q, h_cell;
    DBuf<uint32_t> fmask; // constrained 2^3 bricks, only if the group has any
    void
    upload_scales(const SlotGroup &g)
    {
      std::vector<double> ah(g.h.size()), ratio(g.h.size());
      bool                any = false;
      for (size_t s = 0; s < g.h.size(); ++s)
        {
          ah[s]    = g.a[s] * g.h[s];
          ratio[s] = g.h[s] * g.h[s] / g.a[s];
          any |= g.a[s] != 1.0;
        }
      h.upload(ah);
      q.upload(ratio);
      if (any)
        h_cell.upload(g.h);
    }
    // the scale of a pass: mass_pass = MODE_MASS, whose matrix does not depend on a
    const double *
    scale(bool mass_pass) const
    {
      return mass_pass && h_cell.p ? h_cell.p : h.p;
    }
    SlotGroupDev
    view(bool mass_pass) const
    {
      return SlotGroupDev{interior_base.p, shell_idx.p, mask.p, scale(mass_pass), shell_pos.p, (uint32_t)n_slots, fmask.p, q.p};
    }
    // slots [begin, end) only (sharded levels: halo slots first, then the rest)
    SlotGroupDev
    view(size_t begin, size_t end, bool mass_pass) const
    {
      const size_t n_shell = (size_t)N * N * N - (size_t)(N - 2) * (N - 2) * (N - 2);
      return SlotGroupDev{interior_base.p + begin, shell_idx.p + begin * n_shell, mask.p + begin, scale(mass_pass) + begin, shell_pos.p,
                          (uint32_t)(end - begin), fmask.p ? fmask.p + begin : nullptr, q.p + begin};
    }
    // single cells at p = 1: per-cluster distinct node lists for cell_cluster_apply_kernel
    DBuf<uint32_t> uniq_ptr, uniq_idx;
    DBuf<uint16_t> loc;
    uint32_t       max_uniq = 0;
    bool
    has_clusters() const
    {
      return uniq_ptr.p != nullptr;
    }
    CellClusterDev
    cluster_view(bool mass_pass) const
    {
      return CellClusterDev{uniq_ptr.p, uniq_idx.p, loc.p, mask.p, scale(mass_pass), (uint32_t)n_slots, max_uniq, q.p};
    }
    // dynamic LDS of the cluster kernel (cell_cluster_body): the values and the sums of a cluster's distinct nodes
    size_t
    cluster_lds_bytes() const
    {
      return 2 * (size_t)std::max<uint32_t>(max_uniq, 1) * sizeof(T);
    }
    void
    build_clusters(const SlotGroup &g)
    {
      const size_t          ns = g.n_slots(), ncl = (ns + CLUSTER_CELLS - 1) / CLUSTER_CELLS;
      std::vector<uint32_t> ptr(ncl + 1, 0), idx;
      std::vector<uint16_t> l(ns * 8, 0xFFFFu);
      std::vector<uint32_t> tmp;
      for (size_t c = 0; c < ncl; ++c)
        {
          const size_t s0 = c * CLUSTER_CELLS, s1 = std::min(ns, s0 + CLUSTER_CELLS);
          tmp.clear();
          for (size_t sl = s0; sl < s1; ++sl)
            for (int s = 0; s < 8; ++s)
              if (g.shell_idx[sl * 8 + s] != INVALID_DOF)
                tmp.push_back(g.shell_idx[sl * 8 + s]);
          std::sort(tmp.begin(), tmp.end());
          tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
          for (size_t sl = s0; sl < s1; ++sl)
            for (int s = 0; s < 8; ++s)
              {
                const uint32_t gi = g.shell_idx[sl * 8 + s];
                if (gi != INVALID_DOF)
                  l[sl * 8 + g.shell_pos[s]] = (uint16_t)(std::lower_bound(tmp.begin(), tmp.end(), gi) - tmp.begin());
              }
          idx.insert(idx.end(), tmp.begin(), tmp.end());
          ptr[c + 1] = (uint32_t)idx.size();
          max_uniq   = std::max<uint32_t>(max_uniq, (uint32_t)tmp.size());
        }
      if (idx.empty())
        idx.push_back(0);
      uniq_ptr.upload(ptr);
      uniq_idx.upload(idx);
      loc.upload(l);
    }
  };

  // Host view of the level transfers fused into the operator passes of the FINE level (Transfer2 owns the tables; kernels.hpp,
  // FusedTransferDev): the bricks of slot group `group` flagged in `flags` restrict / prolongate inside the persistent kernel.
  template <typename T>
  struct FusedTransferHost
  {
    int                 group = -1;
    const uint32_t     *flags = nullptr;      // [n_slots of the group][256]
    const uint32_t     *coarse_idx = nullptr; // [n_slots of the group][nc3]
    uint32_t            nc3 = 0;
    std::vector<double> E;                    // 1D h-embedding (2p+1) x (p+1)
    const uint8_t      *tail_flags = nullptr; // [n_tail]: the tail DoF is owned by a fused brick
    // the rows the fused residual pass finishes (TransferTables::residual_tail_runs and the constrained DoFs) in chunks of at
    // most TAIL_CHUNK rows for tail_runs_kernel: [begin, end) pairs; nullptr: the whole tail (sharded levels)
    const uint32_t     *tail_chunks   = nullptr;
    uint32_t            n_tail_chunks = 0;
    // per call
    T *coarse = nullptr, *scratch = nullptr, *x_inout = nullptr;
  };
  // degrees whose 17-point lattice kernel carries the fused modes (p = 3 has 13-point lattices, one workgroup per brick)
  constexpr bool
  fused_transfer_supported(int p)
  {
    return persistent_brick(p) != 0;
  }

  template <typename T>
  struct LevelOperator : LevelOperatorBase
  {
    int                                       p = 1;
    std::vector<std::unique_ptr<GroupDev<T>>> groups;
    DBuf<T>                                   tail_acc;
    // D^-1 codes of the tail / constrained DoFs for tail_kernel (kernels.hpp, Epilogue::dinv_code), valid for the vector dinv_coded
    DBuf<uint8_t>                             dinv_code;
    DBuf<T>                                   dinv_table;
    const T                                  *dinv_coded = nullptr;
    // brick size of the DOMINANT slot group, the one with the most lattice points: the group the launch plan keeps in a
    // launch of its own at p = 1, the one whose workgroups are stamped, and the default of the profiled brick size
    int                                       dominant_B = 0;
    uint32_t                                  ablate = 0; // debug: MGAMD_ABLATE
    DBuf<unsigned long long>                  stamps;     // debug: MGAMD_STAMPS=<mode>, 8 stamps per workgroup of the largest group
    int                                       stamp_mode = -1;
    bool                                      halo_overlap = true; // MGAMD_NO_HALO_OVERLAP=1: exchange after all slots, on the main queue
    // Ticket counters of the persistent kernels (kernels.hpp TicketSchedule): TICKETS_PER_STEP per step of the ordinary and of the
    // halo-overlap plan (8 for the step's bricks, 8 for the constrained partner of a pair launch), so no two launches that may be
    // in flight together share a set.  Zeroed here once; every launch leaves its counters at zero.
    static constexpr size_t                   TICKETS_PER_STEP = 16;
    DBuf<uint32_t>                            ticket_counters;
    int                                       persistent_grid_cap = 0; // development: MGAMD_PERSISTENT_GRID=<n> (at least 8), 0 = none

    // sharded runs: device image of the halo plan
    struct HaloDev
    {
      DBuf<uint32_t> pack_idx, sh_tail, sh_ptr;
      DBuf<int32_t>  sh_src, sh_owner_src;
      DBuf<T>        send, recv;
    };
    std::unique_ptr<HaloDev> halo;

    // device image of the table of convective faces (LevelTables::robin_faces); null where this rank's cells have none: such a
    // level has no face step in its launch plan and runs the launches it ran without the feature
    struct RobinDev
    {
      DBuf<uint32_t> idx;
      DBuf<uint8_t>  flags;
      DBuf<double>   scale;
      uint32_t       n_faces = 0;
    };
    std::unique_ptr<RobinDev> robin;

    // Non-zero Dirichlet data: device images of LevelTables::dirichlet_cells (the lifting) and LevelTables::hanging_rows
    // (distribute_values), uploaded by the first call that needs them: an operator that never sees such data allocates nothing
    struct DirichletDev
    {
      DBuf<uint32_t> idx;
      DBuf<uint16_t> mask;
      DBuf<double>   scale;
      uint32_t       n_cells = 0;
    };
    std::unique_ptr<DirichletDev> dirichlet;
    struct HangingDev
    {
      DBuf<uint32_t> ptr, col;
      DBuf<double>   val;
      uint32_t       n_rows = 0;
    };
    std::unique_ptr<HangingDev> hanging;
    // The jump error indicator and the error norms: device images of LevelTables::EstimatorCells, built by the first call that needs
    // them and freed with the operator.  An operator that is never asked allocates nothing and launches nothing.
    //   gather      idx, mask, scale: ONE copy, shared by estimate_error and integrate_difference, built by whichever comes first
    //   neighbours  code, nbr, the face-flux scratch [cell][6][(p+1)^2] and eta: the indicator's alone (ensure_estimator(true))
    //   norms       the leaves' corners (the built-in Gaussian) and the result: the error norms' alone
    // The indicator's share is, per cell, 4 (p+1)^3 + 48 (p+1)^2 + 128 bytes, the shared gather table included.
    struct EstimatorDev
    {
      DBuf<uint32_t> idx, nbr;
      DBuf<uint16_t> mask;
      DBuf<double>   scale, flux, eta;
      DBuf<uint8_t>  code;
      uint32_t       n_cells = 0;
      bool           neighbours = false;
      uint64_t       gather_bytes = 0, bytes = 0; // bytes: the indicator's share (0 until its first call)
      double         build_ms = 0.0, kernel_ms = 0.0;
      hipEvent_t     e0 = nullptr, e1 = nullptr;
      // the error norms
      DBuf<double> origin, norm_out;
      bool         norms = false;
      uint64_t     norm_bytes = 0; // corners and result
      double       norm_kernel_ms = 0.0;
      ~EstimatorDev()
      {
        if (e0)
          (void)hipEventDestroy(e0);
        if (e1)
          (void)hipEventDestroy(e1);
      }
    };
    std::unique_ptr<EstimatorDev> estimator;
    // the shared gather table and, with `neighbours`, the indicator's part; `who` names the caller in the refusals
    void
    ensure_estimator(bool neighbours, const char *who)
    {
      if (estimator && (estimator->neighbours || !neighbours))
        return;
      const auto                  t0 = std::chrono::steady_clock::now();
      LevelTables::EstimatorCells ec;
      if (!estimator)
        {
          tables->build_estimator_cells(ec, neighbours, who);
          auto dev = std::make_unique<EstimatorDev>();
          dev->idx.upload(ec.idx);
          dev->mask.upload(ec.mask);
          dev->scale.upload(ec.scale);
          dev->n_cells      = (uint32_t)ec.size();
          dev->gather_bytes = ec.idx.size() * 4 + ec.mask.size() * 2 + ec.scale.size() * 8;
          HIP_CHECK(hipEventCreate(&dev->e0));
          HIP_CHECK(hipEventCreate(&dev->e1));
          estimator = std::move(dev);
        }
      else
        {
          tables->refuse_estimate(who);
          tables->tria->face_neighbours(ec.code, ec.nbr);
        }
      if (neighbours)
        {
          EstimatorDev &dev = *estimator;
          const size_t  n2 = (size_t)(p + 1) * (p + 1), nc = dev.n_cells;
          dev.nbr.upload(ec.nbr);
          dev.code.upload(ec.code);
          dev.flux.alloc(nc * 6 * n2);
          dev.eta.alloc(nc);
          dev.neighbours = true;
          dev.bytes      = dev.gather_bytes + ec.nbr.size() * 4 + ec.code.size() + (nc * 6 * n2 + nc) * sizeof(double);
          dev.build_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
    }

    // The kernel launches of one operator application, planned once (build_launch_plan): one step per launch, in launch order.
    enum class LaunchKind
    {
      LATTICE,             // the plain bricks / cells of g with the kernel of their lattice (launch_lattice)
      LATTICE_CONSTRAINED, // the same for a group of constrained bricks (p = 1)
      BRICK_PAIR,          // the plain bricks g + the constrained bricks `partner` of the same size (p = 1, launch_pair)
      BRICKS_AND_CELLS,    // the 2^3 bricks g + the single cells `partner` (p >= 2, lattice_apply_small_kernel)
      BRICKS_AND_CLUSTERS, // the 8^3 bricks g + the cell clusters `partner` (p = 1, lattice_cluster_kernel)
      CLUSTERS,            // the cell clusters of g (p = 1, cell_cluster_apply_kernel)
      ROBIN_FACES          // the convective faces of the level (robin_face_kernel); g is null, [begin, end) the face entries
    };
    struct LaunchStep
    {
      LaunchKind   kind;
      GroupDev<T> *g, *partner;
      size_t       begin, end; // slots of g (the whole group except in the halo-overlap pass)
      uint32_t    *tickets = nullptr; // this step's ticket counters in ticket_counters (persistent kernels, TicketSchedule)
    };
    struct LaunchPlan
    {
      std::vector<LaunchStep> ordinary, diagonal;
      // halo-overlap pass of a sharded level: the slots that touch shared DoFs, then (under the exchange) the others; both
      // empty where the pass does not apply (the ordinary steps are launched instead)
      std::vector<LaunchStep> halo_slots, interior_slots;
    } plan;

    LevelOperator(Ctx *c, const mgamd_dofs *dofs, std::shared_ptr<Comm> cm)
    {
      ctx    = c;
      type   = (int)sizeof(T);
      tables = dofs->tables;
      tria   = dofs->tria;
      p      = tables->p;
      sigma  = tables->sigma;
      if (tables->ls_level && sigma != 0.0)
        throw std::invalid_argument("level operator: mass coefficient " + std::to_string(sigma) +
                                    " on a local-smoothing level: not implemented (refinement-edge matrices have no mass term)");
      if (cm && dofs->halo)
        {
          comm      = cm;
          halo_plan = dofs->halo;
          halo      = std::make_unique<HaloDev>();
          halo->pack_idx.upload(halo_plan->pack_idx);
          halo->sh_tail.upload(halo_plan->sh_tail);
          halo->sh_ptr.upload(halo_plan->sh_ptr);
          halo->sh_src.upload(halo_plan->sh_src);
          halo->sh_owner_src.upload(halo_plan->sh_owner_src);
          halo->send.alloc(std::max<size_t>(halo_plan->pack_idx.size(), 1));
          halo->recv.alloc(std::max<size_t>(halo_plan->pack_idx.size(), 1));
        }
      size_t best = 0;
      for (const SlotGroup &g : tables->groups)
        {
          auto d     = std::make_unique<GroupDev<T>>();
          d->B           = g.B;
          d->N           = g.N;
          d->constrained = g.constrained_group;
          d->n_halo      = g.n_halo_slots;
          d->n_slots = g.n_slots();
          if (d->n_slots)
            {
              d->interior_base.upload(g.interior_base);
              d->shell_idx.upload(g.shell_idx);
              d->mask.upload(g.mask);
              d->upload_scales(g);
              d->shell_pos.upload(g.shell_pos);
              if (std::any_of(g.fmask.begin(), g.fmask.end(), [](uint32_t m) { return m != 0; }))
                d->fmask.upload(g.fmask);
              if (p == 1 && g.B == 1 && !tables->ls_level)
                d->build_clusters(g); // (the cluster tables bake in which nodes are constrained: not on local-smoothing levels)
            }
          const size_t work = d->n_slots * (size_t)g.N * g.N * g.N;
          if (work > best)
            {
              best       = work;
              dominant_B = g.B;
            }
          groups.push_back(std::move(d));
        }
      if (const char *e = getenv("MGAMD_ABLATE"))
        ablate = (uint32_t)atoi(e);
      // debug: stamp the group of this brick size instead of the dominant one.  It REPLACES dominant_B, so it also decides
      // whether the p = 1 launch plan merges the 8^3 bricks with the cell clusters (build_launch_plan).
      if (const char *e = getenv("MGAMD_STAMP_B"))
        dominant_B = atoi(e);
      halo_overlap = getenv("MGAMD_NO_HALO_OVERLAP") == nullptr;
      if (const char *e = getenv("MGAMD_STAMPS"))
        {
          stamp_mode = atoi(e);
          size_t nwg = 0;
          for (auto &g : groups)
            if (g->B == dominant_B)
              nwg = g->n_slots; // >= number of workgroups
          stamps.alloc(nwg * 8 + 8);
          stamps.zero(ctx->stream);
        }
      tail_acc.alloc(std::max<uint32_t>(tables->n_tail + tables->n_edge, 1));
      tail_acc.zero(ctx->stream);
      if (tables->robin_faces.size())
        {
          robin = std::make_unique<RobinDev>();
          robin->idx.upload(tables->robin_faces.idx);
          robin->flags.upload(tables->robin_faces.flags);
          robin->scale.upload(tables->robin_faces.scale);
          robin->n_faces = (uint32_t)tables->robin_faces.size();
        }
      // development: fewer persistent workgroups than the resident ones, so that small meshes draw many tickets per workgroup.
      // At least 8: the ticket schedule needs a workgroup for every one of the 8 item ranges.
      if (const char *e = getenv("MGAMD_PERSISTENT_GRID"))
        persistent_grid_cap = std::max(8, atoi(e));
      build_launch_plan();
      ticket_counters.alloc(TICKETS_PER_STEP * (plan.ordinary.size() + plan.halo_slots.size() + plan.interior_slots.size()));
      ticket_counters.zero(ctx->stream);
      uint32_t *next_set = ticket_counters.p;
      for (std::vector<LaunchStep> *steps : {&plan.ordinary, &plan.halo_slots, &plan.interior_slots})
        for (LaunchStep &s : *steps)
          {
            s.tickets = next_set;
            next_set += TICKETS_PER_STEP;
          }
    }

    // Which kernel runs which slot group, and with whom: every merging rule of the operator's launches is here.
    void
    build_launch_plan()
    {
      using K        = LaunchKind;
      auto non_empty = [&](int B, bool constrained) -> GroupDev<T> * {
        for (auto &g : groups)
          if (g->n_slots && g->B == B && g->constrained == constrained)
            return g.get();
        return nullptr;
      };
      auto on_its_own = [&](GroupDev<T> *g, size_t begin, size_t end) {
        // single cells at p = 1 go through their cluster tables wherever the level has them (GroupDev::build_clusters)
        const K kind = g->has_clusters() ? K::CLUSTERS : (g->constrained ? K::LATTICE_CONSTRAINED : K::LATTICE);
        return LaunchStep{kind, g, nullptr, begin, end};
      };
      // The diagonal pass: no merges, lattice_diag_kernel on every group (the clusters have no diagonal kernel).
      for (auto &g : groups)
        if (g->n_slots)
          plan.diagonal.push_back({g->constrained ? K::LATTICE_CONSTRAINED : K::LATTICE, g.get(), nullptr, 0, g->n_slots});

      // An ordinary pass.  Two small groups that are a fraction of one round of workgroups each share a launch (a launch
      // costs a workgroup lifetime whatever it does):
      GroupDev<T> *cells = non_empty(1, false);
      // p >= 2: the 2^3 bricks and the single cells
      GroupDev<T> *bricks2 = (p >= 2 && cells) ? non_empty(2, false) : nullptr;
      // p = 1: the plain 8^3 bricks and the cell clusters, unless the 8^3 bricks are the dominant group of the level
      GroupDev<T> *bricks8 = (p == 1 && cells && cells->has_clusters() && dominant_B != 8) ? non_empty(8, false) : nullptr;
      for (auto &gp : groups)
        {
          GroupDev<T> *g = gp.get();
          if (!g->n_slots || (g == cells && (bricks2 || bricks8)))
            continue; // (the cells: launched with the bricks)
          if (g == bricks2)
            plan.ordinary.push_back({K::BRICKS_AND_CELLS, g, cells, 0, g->n_slots});
          else if (g == bricks8)
            plan.ordinary.push_back({K::BRICKS_AND_CLUSTERS, g, cells, 0, g->n_slots});
          else
            {
              // p = 1 (the only degree with constrained bricks above B = 2): the constrained bricks of one size ride with
              // the plain ones of that size, unless those ride with the cell clusters
              GroupDev<T> *other = (p == 1 && g->B > 2) ? non_empty(g->B, !g->constrained) : nullptr;
              if (other && other != bricks8)
                {
                  if (!g->constrained)
                    plan.ordinary.push_back({K::BRICK_PAIR, g, other, 0, g->n_slots});
                }
              else
                plan.ordinary.push_back(on_its_own(g, 0, g->n_slots));
            }
        }

      // The convective faces add into the tail accumulator like a slot's shell sums: after the slots, before the exchange and the
      // tail epilogue (level_operator_apply.hpp)
      const LaunchStep faces{K::ROBIN_FACES, nullptr, nullptr, 0, robin ? robin->n_faces : 0};
      if (robin)
        {
          plan.diagonal.push_back(faces);
          plan.ordinary.push_back(faces);
        }

      // The halo-overlap pass of a sharded level: no merges, every group split at the end of its halo slots (LevelTables
      // puts them at the front of every group).  Only where some slots are left to run under the exchange.
      if (!halo || !halo_overlap)
        return;
      auto halo_end = [&](const GroupDev<T> &g) {
        size_t nh = g.n_halo;
        if (g.has_clusters()) // the cluster kernel works on whole 256-cell clusters
          nh = std::min(g.n_slots, (nh + CLUSTER_CELLS - 1) / CLUSTER_CELLS * CLUSTER_CELLS);
        return nh;
      };
      for (auto &g : groups)
        if (halo_end(*g) < g->n_slots)
          plan.interior_slots.push_back(on_its_own(g.get(), halo_end(*g), g->n_slots));
      if (!plan.interior_slots.empty())
        for (auto &g : groups)
          if (halo_end(*g) > 0)
            plan.halo_slots.push_back(on_its_own(g.get(), 0, halo_end(*g)));
      // boundary DoFs may be shared: the faces run with the halo slots, and the exchange sums their contributions over the ranks
      if (robin && !plan.interior_slots.empty())
        plan.halo_slots.push_back(faces);
    }

    // tail[t] <- sum over the sharing ranks (ascending rank order) of their partial tail[t]
    void
    exchange_add_raw(T *tail, hipStream_t st = nullptr)
    {
      if (!halo)
        return;
      if (!st)
        st = ctx->stream;
      const uint32_t ns = (uint32_t)halo_plan->pack_idx.size();
      if (ns)
        hipLaunchKernelGGL(halo_pack_kernel<T>, grid_for(ns), 256, 0, st, halo->send.p, tail, halo->pack_idx.p, ns);
      comm->exchange(halo->send.p, halo->recv.p, halo_plan->peers, halo_plan->peer_offset, sizeof(T), st);
      const uint32_t nsh = (uint32_t)halo_plan->sh_tail.size();
      if (nsh)
        hipLaunchKernelGGL(halo_combine_kernel<T>, grid_for(nsh), 256, 0, st, tail, halo->recv.p, halo->sh_tail.p, halo->sh_ptr.p,
                           halo->sh_src.p, nsh);
      HIP_CHECK(hipGetLastError());
    }
    // tail[t] <- the owner's value, for the copies this rank holds of DoFs owned elsewhere
    void
    import_from_owner_raw(T *tail)
    {
      if (!halo)
        return;
      const uint32_t ns = (uint32_t)halo_plan->pack_idx.size();
      if (ns)
        hipLaunchKernelGGL(halo_pack_kernel<T>, grid_for(ns), 256, 0, ctx->stream, halo->send.p, tail, halo->pack_idx.p, ns);
      comm->exchange(halo->send.p, halo->recv.p, halo_plan->peers, halo_plan->peer_offset, sizeof(T), ctx->stream);
      const uint32_t nsh = (uint32_t)halo_plan->sh_tail.size();
      if (nsh)
        hipLaunchKernelGGL(halo_import_kernel<T>, grid_for(nsh), 256, 0, ctx->stream, tail, halo->recv.p, halo->sh_tail.p,
                           halo->sh_owner_src.p, nsh);
      HIP_CHECK(hipGetLastError());
    }
    void
    exchange_add_tail(mgamd_vec &v) override
    {
      if (v.n != n_dofs())
        throw std::invalid_argument("exchange_add_tail: vector size mismatch");
      exchange_add_raw(v.as<T>() + tables->n_interior);
    }
    double
    dot_raw_global(const T *x, const T *y)
    {
      const double local = dot_raw(ctx, x, y, n_dot());
      return comm ? comm->allreduce_sum_host(local, ctx->stream) : local;
    }
    double
    dot(const mgamd_vec &x, const mgamd_vec &y) override
    {
      if (x.n != n_dofs() || y.n != n_dofs())
        throw std::invalid_argument("dot: vector size mismatch");
      return dot_raw_global(x.as<T>(), y.as<T>());
    }

    template <int P>
    Mats<P, T>
    mats() const
    {
      Mats<P, T> m;
      const int n = P + 1;
      for (int i = 0; i < n * n; ++i)
        {
          m.M[i]  = tables->fe.M[i];
          m.K[i]  = tables->fe.K[i];
          m.I0[i] = tables->fe.I[0][i];
          m.I1[i] = tables->fe.I[1][i];
        }
      constexpr int NH = Mats<P>::NH, NO = Mats<P>::NO;
      auto          eo = [&](const double *A, T *Ae, T *Ao) {
        for (int i = 0; i < NH; ++i)
          for (int j = 0; j < NH; ++j)
            Ae[i * NH + j] = (j < NO) ? 0.5 * (A[i * n + j] + A[i * n + P - j]) : A[i * n + j];
        for (int i = 0; i < NO; ++i)
          for (int j = 0; j < NO; ++j)
            Ao[i * NO + j] = 0.5 * (A[i * n + j] - A[i * n + P - j]);
      };
      eo(tables->fe.M.data(), m.Me, m.Mo);
      eo(tables->fe.K.data(), m.Ke, m.Ko);
      return m;
    }

    // the cluster kernel's arguments for the single cells g in the pass described by a (clusters exist at p = 1 only)
    template <int P>
    ClusterArgs<T>
    cluster_args(const GroupDev<T> &g, const ApplyArgs<T, P> &a, bool first, bool mass_pass)
    {
      ClusterArgs<T> c;
      c.c          = g.cluster_view(mass_pass);
      c.m          = mats<1>();
      c.src        = a.src;
      c.tail_acc   = a.tail_acc;
      c.n_interior = a.n_interior;
      c.b          = a.epi.b;
      c.dinv       = a.epi.dinv;
      c.c0         = a.epi.c0;
      c.from_b     = first ? 1 : 0;
      c.cluster_offset = 0;
      c.sigma          = a.sigma;
      return c;
    }

    // the clusters that hold the cells [begin, end) of g
    template <int P, bool MASS_ONLY = false>
    void
    launch_clusters(hipStream_t st, const GroupDev<T> &g, const ApplyArgs<T, P> &a, bool first, size_t begin, size_t end)
    {
      ClusterArgs<T> c    = cluster_args(g, a, first, MASS_ONLY);
      c.cluster_offset    = (uint32_t)(begin / CLUSTER_CELLS);
      const uint32_t grid = (uint32_t)((end + CLUSTER_CELLS - 1) / CLUSTER_CELLS) - c.cluster_offset;
      hipLaunchKernelGGL((MASS_ONLY ? cell_cluster_mass_kernel<T> : cell_cluster_apply_kernel<T>), grid, CLUSTER_CELLS, g.cluster_lds_bytes(), st, c);
      HIP_CHECK(hipGetLastError());
    }

    // the plain bricks a.g and the constrained bricks of the same size in one launch
    template <int P, int B, int MODE>
    void
    launch_pair(hipStream_t st, const ApplyArgs<T, P> &a, GroupDev<T> *g_constrained)
    {
      using G = Geo<P, B>;
      BrickPairArgs<T, P> pa;
      pa.a             = a;
      pa.g_constrained = g_constrained->view(MODE == MODE_MASS);
      pa.n_wg_plain    = (uint32_t)((a.g.n_slots + G::SPW - 1) / G::SPW);
      const int n_wg   = (int)(pa.n_wg_plain + (uint32_t)((g_constrained->n_slots + G::SPW - 1) / G::SPW));
      if constexpr (persistent_lattice(G::N))
        {
          if (n_wg > persistent_grid(ctx, n_wg, 2, persistent_grid_cap))
            pa.n_wg_plain = 0; // every workgroup walks both kinds (kernels.hpp)
          void (*kern)(BrickPairArgs<T, P>) = lattice_apply_persistent_pair_kernel<T, P, B, MODE, false>;
          if constexpr (MODE != MODE_MASS) // (launch_lattice)
            if (a.sigma != 0.0)
              kern = lattice_apply_persistent_pair_kernel<T, P, B, MODE, true>;
          launch_persistent(ctx, st, kern, n_wg, 2, G::ABLOCK, apply_lds_bytes<T, P, B>(), pa, persistent_grid_cap);
        }
      else if constexpr (MODE != base_mode(MODE))
        throw std::runtime_error("fused transfers need the persistent brick kernel");
      else
        launch_lds(ctx, st, lattice_apply_pair_kernel<T, P, B, MODE>, n_wg, G::ABLOCK, apply_lds_bytes<T, P, B>(), pa);
      HIP_CHECK(hipGetLastError());
    }

    // the 17-point lattice group that carries fused transfers (slots [begin, begin + a.g.n_slots) of it)
    template <int P, int MODE>
    void
    launch_fused(hipStream_t st, ApplyArgs<T, P> &a, size_t begin, GroupDev<T> *partner_constrained, const FusedTransferHost<T> &f)
    {
      if constexpr (fused_transfer_supported(P))
        {
          constexpr int B = persistent_brick(P);
          using G         = Geo<P, B>;
          constexpr int NC = P * B / 2 + 1, NC3 = NC * NC * NC;
          if (f.nc3 != (uint32_t)NC3 || f.E.size() != (size_t)(2 * P + 1) * (P + 1))
            throw std::runtime_error("fused transfer: tables do not match the brick kernel");
          a.fused.flags      = f.flags + begin * G::ABLOCK;
          a.fused.coarse_idx = f.coarse_idx + begin * NC3;
          for (int i = 0; i < (P + 1) * (P + 1); ++i) // rows 0..P; the kernel uses E[2P - a][P - b] = E[a][b] for the rest
            a.fused.Eh[i] = f.E[i];
          for (int ar = 0; ar <= P; ++ar)
            for (int b = 0; b <= P; ++b)
              if (std::fabs(f.E[(2 * P - ar) * (P + 1) + (P - b)] - f.E[ar * (P + 1) + b]) > 1e-14)
                throw std::runtime_error("fused transfer: the 1D embedding is not centro-symmetric");
          a.fused.coarse  = f.coarse;
          a.fused.x_inout = f.x_inout;
          a.fused.scratch = f.scratch;
          if (partner_constrained)
            {
              if constexpr (P == 1)
                return launch_pair<P, B, MODE>(st, a, partner_constrained);
              throw std::runtime_error("brick pair launch: size not instantiated");
            }
          launch_persistent(ctx, st,
                            a.sigma != 0.0 ? lattice_apply_persistent_kernel<T, P, B, MODE, false, true> :
                                             lattice_apply_persistent_kernel<T, P, B, MODE, false, false>,
                            (int)a.g.n_slots, persistent_wgs_per_cu<T, P>(), G::ABLOCK, apply_lds_bytes<T, P, B>(), a, persistent_grid_cap);
          HIP_CHECK(hipGetLastError());
        }
      else
        throw std::runtime_error("fused transfers: degree without 17-point lattice kernel");
    }

    // the 8^3 bricks a.g and the cell clusters of gc in one launch (p = 1)
    template <int MODE>
    void
    launch_bricks_and_clusters(hipStream_t st, const ApplyArgs<T, 1> &a, const GroupDev<T> &gc)
    {
      using G8 = Geo<1, 8>;
      P1SmallArgs<T> sa;
      sa.a           = a;
      sa.c           = cluster_args(gc, a, MODE == MODE_CHEB_FIRST, MODE == MODE_MASS);
      sa.n_wg_bricks = (uint32_t)((a.g.n_slots + G8::SPW - 1) / G8::SPW);
      const uint32_t n_wg_cl = (uint32_t)((gc.n_slots + CLUSTER_CELLS - 1) / CLUSTER_CELLS);
      const size_t   lds     = std::max(apply_lds_bytes<T, 1, 8>(), gc.cluster_lds_bytes());
      hipLaunchKernelGGL((lattice_cluster_kernel<T, MODE>), sa.n_wg_bricks + n_wg_cl, 256, lds, st, sa);
      HIP_CHECK(hipGetLastError());
    }

    // the 2^3 bricks a.g and the single cells of g1 in one launch (p >= 2)
    template <int P, int MODE>
    void
    launch_bricks_and_cells(hipStream_t st, const ApplyArgs<T, P> &a, const GroupDev<T> &g1)
    {
      using G2 = Geo<P, 2>;
      SmallSlotsArgs<T, P> sa;
      sa.a           = a;
      sa.g_cells     = g1.view(MODE == MODE_MASS);
      sa.n_wg_bricks = (uint32_t)((a.g.n_slots + G2::SPW - 1) / G2::SPW);
      // the cells wave-scoped: four wavefronts per workgroup with their own cells (kernels.hpp cell_waves_body)
      using GW = Geo<P, 1, 64>;
      const uint32_t n_w        = (uint32_t)((g1.n_slots + GW::SPW - 1) / GW::SPW);
      const uint32_t n_wg_cells = (n_w + CELL_WAVES - 1) / CELL_WAVES;
      constexpr size_t lds      = small_slots_lds_bytes<T, P>();
      static_assert(lds <= 64 * 1024, "above the default dynamic-LDS limit the launch has to go through launch_lds");
      // (kernels.hpp: the mass term compiled out for sigma = 0 and compiled in otherwise; the mass pass has no mass term: MASS = false)
      hipLaunchKernelGGL((a.sigma == 0.0 || MODE == MODE_MASS ? lattice_apply_small_kernel<T, P, MODE, false> :
                                                                 lattice_apply_small_kernel<T, P, MODE, true>),
                         sa.n_wg_bricks + n_wg_cells, 256, lds, st, sa);
      HIP_CHECK(hipGetLastError());
    }

    // One step of the launch plan on stream st.  MODE_ a fused mode: the step of the group that carries the fused transfers
    // runs it (with the partner the plan gives it), every other step the base mode.  stamp: an ordinary pass (debug stamps).
    template <int P, int MODE_>
    void
    launch_step(hipStream_t st, ApplyArgs<T, P> &a, const LaunchStep &s, bool diag, const FusedTransferHost<T> *fused, bool stamp = false)
    {
      constexpr int MODE = base_mode(MODE_);
      using K            = LaunchKind;
      if (s.kind == K::ROBIN_FACES)
        return launch_robin_faces<P, MODE>(st, a, diag);
      GroupDev<T> *g     = s.g;
      a.g                = g->view(s.begin, s.end, MODE == MODE_MASS);
      a.stamps           = nullptr;
      a.tickets          = s.tickets;
      if constexpr (MODE_ != MODE)
        if (fused && fused->group >= 0 && g == groups[fused->group].get())
          return launch_fused<P, MODE_>(st, a, s.begin, s.partner, *fused);
      if (stamp && stamps.p && s.kind != K::BRICK_PAIR && g->B == dominant_B && !g->constrained && MODE == stamp_mode)
        a.stamps = stamps.p;
      bool done = false;
      switch (s.kind)
        {
          case K::LATTICE:
            if (!dispatch_brick_size<P, 1, 2, 4, 8, 16>(g->B, [&](auto B) { launch_lattice<T, P, B(), MODE>(ctx, st, a, diag, persistent_grid_cap); }))
              throw std::runtime_error("unsupported brick size");
            break;
          case K::LATTICE_CONSTRAINED:
            if constexpr (P == 1)
              done = dispatch_brick_size<P, 4, 8, 16>(g->B, [&](auto B) { launch_lattice<T, P, B(), MODE, true>(ctx, st, a, diag, persistent_grid_cap); });
            if (!done)
              throw std::runtime_error("constrained bricks of this size/degree are not instantiated");
            break;
          case K::BRICK_PAIR:
            if constexpr (P == 1)
              done = dispatch_brick_size<P, 8, 16>(g->B, [&](auto B) { launch_pair<P, B(), MODE>(st, a, s.partner); });
            if (!done)
              throw std::runtime_error("brick pair launch: size not instantiated");
            break;
          case K::BRICKS_AND_CELLS:
            if constexpr (P >= 2)
              launch_bricks_and_cells<P, MODE>(st, a, *s.partner);
            break;
          case K::BRICKS_AND_CLUSTERS:
            if constexpr (P == 1)
              launch_bricks_and_clusters<MODE>(st, a, *s.partner);
            break;
          case K::CLUSTERS:
            launch_clusters<P, MODE == MODE_MASS>(st, *g, a, MODE == MODE_CHEB_FIRST, s.begin, s.end);
            break;
          case K::ROBIN_FACES: // (above)
            break;
        }
    }

    // the face term of the convective faces into the tail accumulator (kernels.hpp robin_face_kernel); the mass pass has none
    template <int P, int MODE>
    void
    launch_robin_faces(hipStream_t st, const ApplyArgs<T, P> &a, bool diag)
    {
      if constexpr (MODE != MODE_MASS)
        {
          RobinArgs<T, P> r;
          r.idx     = robin->idx.p;
          r.flags   = robin->flags.p;
          r.scale   = robin->scale.p;
          r.n_faces = robin->n_faces;
          for (int i = 0; i < (P + 1) * (P + 1); ++i)
            {
              r.M[i]  = a.m.M[i];
              r.I0[i] = a.m.I0[i];
              r.I1[i] = a.m.I1[i];
            }
          r.src           = a.src;
          r.tail_acc      = a.tail_acc;
          r.n_interior    = a.n_interior;
          r.gather_limit  = a.gather_limit;
          r.scatter_limit = a.scatter_limit;
          r.b             = a.epi.b;
          r.dinv          = a.epi.dinv;
          r.c0            = a.epi.c0;
          r.dinv_code     = a.epi.dinv_code;
          r.dinv_table    = a.epi.dinv_table;
          // two groups of faces per workgroup where there are that many: the 1D matrices are staged in LDS once per workgroup
          const uint32_t n_groups = (r.n_faces + robin_faces_per_workgroup<P>() - 1) / robin_faces_per_workgroup<P>();
          const uint32_t grid     = std::min<uint32_t>(1024u, (n_groups + 1) / 2);
          if (diag)
            hipLaunchKernelGGL((robin_face_kernel<T, P, false, true>), grid, 256, 0, st, r);
          else if (MODE == MODE_CHEB_FIRST)
            hipLaunchKernelGGL((robin_face_kernel<T, P, true, false>), grid, 256, 0, st, r);
          else
            hipLaunchKernelGGL((robin_face_kernel<T, P, false, false>), grid, 256, 0, st, r);
          HIP_CHECK(hipGetLastError());
        }
    }

    template <int MODE>
    void
    launch_tail(hipStream_t st, uint32_t begin, uint32_t end, bool with_rest, const Epilogue<T> &epi_in, bool diag)
    {
      const uint32_t n_rest = with_rest ? tables->n_dofs - tables->n_interior - end : 0;
      const uint32_t n_t    = end - begin + n_rest;
      if (!n_t)
        return;
      Epilogue<T> epi = epi_in;
      if (epi.dinv_code)
        epi.dinv_code += begin;
      if (diag)
        hipLaunchKernelGGL((tail_kernel<T, MODE_INVDIAG>), grid_for(n_t), 256, 0, st, tail_acc.p + begin, tables->n_interior + begin, end - begin,
                           n_rest, epi);
      else
        hipLaunchKernelGGL((tail_kernel<T, MODE>), grid_for(n_t), 256, 0, st, tail_acc.p + begin, tables->n_interior + begin, end - begin, n_rest,
                           epi);
      HIP_CHECK(hipGetLastError());
    }

    // the tail epilogue on the rows of a chunk list only (FusedTransferHost::tail_chunks)
    template <int MODE>
    void
    launch_tail_runs(hipStream_t st, const uint32_t *chunks, uint32_t n_chunks, const Epilogue<T> &epi)
    {
      if (!n_chunks)
        return;
      constexpr uint32_t per_wg = 256 / TAIL_CHUNK * TAIL_U;
      hipLaunchKernelGGL((tail_runs_kernel<T, MODE>), (n_chunks + per_wg - 1) / per_wg, 256, 0, st, tail_acc.p, tables->n_interior, tables->n_tail,
                         chunks, n_chunks, epi);
      HIP_CHECK(hipGetLastError());
    }

    // One operator application: the steps of the launch plan (build_launch_plan), then the epilogue of the tail and the
    // constrained DoFs.
    // Refinement-edge DoFs of a local-smoothing level (LevelTables::n_edge, numbered right after the tail):
    //   EDGE_OUT   the level operator (Operator::vmult, ref:include/operator.h:152-183): zero input, identity rows
    //   EDGE_ROWS  zero input, but their ROWS are computed: the residual that is restricted (deal.II edge_out /
    //              vmult_interface_down)
    //   EDGE_IN    ordinary unconstrained DoFs: the edge matrix (vmult_interface_up, ref:include/operator.h:203-226)
    enum EdgeMode
    {
      EDGE_OUT  = 0,
      EDGE_ROWS = 1,
      EDGE_IN   = 2
    };

    // defined in level_operator_apply.hpp, instantiated in apply_inst.hip (one translation unit per number type and degree)
    template <int P, int MODE>
    void
    apply_P(const T *src, const Epilogue<T> &epi, bool diag, double words, int edge_mode, const FusedTransferHost<T> *fused);

    template <int MODE>
    void
    apply(const T *src, const Epilogue<T> &epi, bool diag = false, double words = 0, int edge_mode = EDGE_OUT,
          const FusedTransferHost<T> *fused = nullptr)
    {
      constexpr bool FUSED_MODE = MODE != base_mode(MODE);
      if (FUSED_MODE && (!fused || fused->group < 0 || !fused_transfer_supported(p)))
        throw std::runtime_error("fused transfer pass without fused tables");
      auto run = [&](auto P) {
        if constexpr (!FUSED_MODE || fused_transfer_supported(P())) // (apply_inst.hip instantiates no others)
          apply_P<P(), MODE>(src, epi, diag, words, edge_mode, fused);
      };
      if (!dispatch_degree(p, run))
        throw std::runtime_error("degree not instantiated");
    }

    // raw-pointer entry points used by smoother / multigrid
    void
    vmult_raw(T *dst, const T *src)
    {
      Epilogue<T> e{dst, src, nullptr, nullptr, nullptr, T(0), T(0), T(0)};
      apply<MODE_VMULT>(src, e);
    }
    // t = b - A x, the residual step of Multigrid::level_v_step.  The reference hands Multigrid an mg::Matrix built from
    // MatrixFreeOperators::MGInterfaceOperator<LevelMatrixType> (ref:multigrid_throughput.cc:857-862), whose vmult calls
    // Operator::vmult_interface_down (ref:include/operator.h:191-201): the plain cell loop, identity on the constrained
    // (Dirichlet) rows only -- on a local-smoothing level the refinement-edge DoFs are ordinary DoFs there, rows and columns
    // (EDGE_IN).  After the zero-start pre-smoother x vanishes on them, so the edge rows are t_E = b_E - A_{E,I} x_I.
    void
    residual_raw(T *t, const T *b, const T *x)
    {
      Epilogue<T> e{t, x, nullptr, b, nullptr, T(0), T(0), T(0)};
      apply<MODE_RESIDUAL>(x, e, false, 0, tables->n_edge ? EDGE_IN : EDGE_OUT);
    }
    // Operator::vmult_interface_down (ref:include/operator.h:191-201)
    void
    vmult_interface_down(mgamd_vec &dst, const mgamd_vec &src) override
    {
      if (dst.n != n_dofs() || src.n != n_dofs() || dst.data == src.data)
        throw std::invalid_argument("vmult_interface_down: bad vectors");
      Epilogue<T> e{dst.as<T>(), src.as<T>(), nullptr, nullptr, nullptr, T(0), T(0), T(0)};
      apply<MODE_VMULT>(src.as<T>(), e, false, 0, tables->n_edge ? EDGE_IN : EDGE_OUT);
    }
    // dst = A^{edge DoFs unconstrained} (src restricted to the refinement-edge DoFs); tmp: scratch of n_dofs entries
    // (Operator::vmult_interface_up, ref:include/operator.h:203-226)
    void
    interface_up_raw(T *dst, const T *src, T *tmp)
    {
      const size_t n = n_dofs(), first_edge = (size_t)tables->n_interior + tables->n_tail;
      HIP_CHECK(hipMemsetAsync(tmp, 0, n * sizeof(T), ctx->stream));
      if (tables->n_edge)
        HIP_CHECK(hipMemcpyAsync(tmp + first_edge, src + first_edge, (size_t)tables->n_edge * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
      Epilogue<T> e{dst, tmp, nullptr, nullptr, nullptr, T(0), T(0), T(0)};
      apply<MODE_VMULT>(tmp, e, false, 0, EDGE_IN);
    }
    void
    vmult_interface_up(mgamd_vec &dst, const mgamd_vec &src) override
    {
      if (dst.n != n_dofs() || src.n != n_dofs() || dst.data == src.data)
        throw std::invalid_argument("vmult_interface_up: bad vectors");
      DBuf<T> tmp;
      tmp.alloc(n_dofs());
      interface_up_raw(dst.as<T>(), src.as<T>(), tmp.p);
      ctx->sync();
    }
    // One-byte codes for D^-1 of the DoFs tail_kernel handles (tail, refinement-edge, Dirichlet, hanging): on a level only a
    // few hundred distinct values occur there (node type x cell size x summation order), so the 255 most frequent ones go
    // into a table and the rest keeps reading the vector.  Values are matched by bit pattern: results do not change.
    void
    build_dinv_codes(const T *dinv)
    {
      dinv_coded = nullptr;
      if (getenv("MGAMD_NO_DINV_CODES"))
        return;
      const size_t n0 = tables->n_interior, n = (size_t)n_dofs() - n0;
      if (n < 4096) // small levels are latency-bound: nothing to gain
        return;
      std::vector<T> h(n);
      ctx->sync();
      HIP_CHECK(hipMemcpy(h.data(), dinv + n0, n * sizeof(T), hipMemcpyDeviceToHost));
      using Bits = typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type;
      std::unordered_map<Bits, uint32_t> count;
      count.reserve(1024);
      auto bits = [](T v) {
        Bits b;
        std::memcpy(&b, &v, sizeof(T));
        return b;
      };
      for (size_t i = 0; i < n && count.size() < (1u << 20); ++i)
        ++count[bits(h[i])];
      std::vector<std::pair<uint32_t, Bits>> top;
      top.reserve(count.size());
      for (auto &kv : count)
        top.push_back({kv.second, kv.first});
      std::sort(top.begin(), top.end(), [](const auto &a, const auto &b) { return a.first > b.first || (a.first == b.first && a.second < b.second); });
      if (top.size() > 255)
        top.resize(255);
      std::vector<T>                    table(256, T(1));
      std::unordered_map<Bits, uint8_t> code_of;
      for (size_t k = 0; k < top.size(); ++k)
        {
          std::memcpy(&table[k], &top[k].second, sizeof(T));
          code_of[top[k].second] = (uint8_t)k;
        }
      std::vector<uint8_t> codes(n);
      for (size_t i = 0; i < n; ++i)
        {
          auto it  = code_of.find(bits(h[i]));
          codes[i] = it == code_of.end() ? (uint8_t)255 : it->second;
        }
      dinv_code.upload(codes);
      dinv_table.upload(table);
      dinv_coded = dinv;
    }

    void
    cheb_raw(T *out, const T *x, const T *xold, const T *b, const T *dinv, double f1, double f2, int from_b = 0, double c0 = 0.0,
             double *out_wide = nullptr)
    {
      // from_b = 1: x is c0 dinv b and xold = 0 (x is not read); from_b = 2: xold is c0 dinv b (xold is not read)
      // out_wide (float levels, plain Chebyshev pass only): the result goes there as doubles, `out` is not written
      Epilogue<T> e{out, x, from_b ? nullptr : xold, b, dinv, T(f1), T(f2), T(c0)};
      if (out_wide && (from_b != 0 || sizeof(T) != 4))
        throw std::invalid_argument("cheb_raw: a wide result needs a plain Chebyshev pass on float vectors");
      e.out_wide = out_wide;
      if (dinv == dinv_coded && dinv_code.p)
        {
          e.dinv_code  = dinv_code.p;
          e.dinv_table = dinv_table.p;
        }
      if (from_b == 1)
        apply<MODE_CHEB_FIRST>(x, e, false, 3.0);
      else if (from_b == 2)
        apply<MODE_CHEB_SECOND>(x, e, false, 4.0);
      else
        apply<MODE_CHEB>(x, e, false, xold ? 5.0 : 4.0);
    }

    // first pass of a smoothing step (x_old = 0, f1 = 0) on x + P x_c with the prolongation fused into the brick kernel
    // (kernels.hpp MODE_CHEB_PROLONGATE): x is updated in place to x + P x_c, f.scratch is clobbered on the tail
    void
    cheb_prolongate_raw(T *out, T *x, const T *b, const T *dinv, double f2, const FusedTransferHost<T> &f_in)
    {
      FusedTransferHost<T> f = f_in;
      f.x_inout              = x;
      Epilogue<T> e{out, x, nullptr, b, dinv, T(0), T(f2), T(0)};
      if (dinv == dinv_coded && dinv_code.p)
        {
          e.dinv_code  = dinv_code.p;
          e.dinv_table = dinv_table.p;
        }
      e.xs_flag = f.tail_flags;
      e.xs      = f.scratch;
      e.x_inout = x;
      apply<MODE_CHEB_PROLONGATE>(x, e, false, 4.0, EDGE_OUT, &f);
    }

    void
    vmult(mgamd_vec &dst, const mgamd_vec &src) override
    {
      if (dst.n != n_dofs() || src.n != n_dofs())
        throw std::invalid_argument("vmult: vector size mismatch");
      if (dst.data == src.data)
        throw std::invalid_argument("vmult: dst and src must differ");
      vmult_raw(dst.as<T>(), src.as<T>());
    }

    // dst = C^T M C src: the mass matrix of the level's space (kernels.hpp MODE_MASS); rows and columns of constrained DoFs are
    // zero, and sigma plays no role
    void
    vmult_mass_raw(T *dst, const T *src)
    {
      if (tables->ls_level)
        throw std::invalid_argument("vmult_mass: the operator of a local-smoothing level has refinement-edge DoFs, for which the mass "
                                    "matrix is not defined; use the active-mesh operator");
      Epilogue<T> e{dst, src, nullptr, nullptr, nullptr, T(0), T(0), T(0)};
      apply<MODE_MASS>(src, e);
    }
    void
    vmult_mass(mgamd_vec &dst, const mgamd_vec &src) override
    {
      if (dst.n != n_dofs() || src.n != n_dofs())
        throw std::invalid_argument("vmult_mass: vector size mismatch (" + std::to_string(dst.n) + ", " + std::to_string(src.n) +
                                    " for " + std::to_string(n_dofs()) + " DoFs)");
      if (dst.data == src.data)
        throw std::invalid_argument("vmult_mass: dst and src must differ");
      vmult_mass_raw(dst.as<T>(), src.as<T>());
    }

    // defined in level_operator_apply.hpp, instantiated in apply_inst.hip with the operator passes
    template <int P>
    void
    lift_P(T *dst, const T *g, double mass_sigma, double alpha);

    // dst += alpha C^T (K_a + [include_mass] sigma M) C g^ on the free rows, this rank's cells (kernels_boundary.hpp); nothing is
    // launched where no cell gathers a Dirichlet DoF
    void
    dirichlet_lift_add_raw(T *dst, const T *g, bool include_mass, double alpha)
    {
      tables->refuse_dirichlet_lift("rhs_dirichlet");
      if (!dirichlet)
        {
          dirichlet = std::make_unique<DirichletDev>();
          dirichlet->idx.upload(tables->dirichlet_cells.idx);
          dirichlet->mask.upload(tables->dirichlet_cells.mask);
          dirichlet->scale.upload(tables->dirichlet_cells.scale);
          dirichlet->n_cells = (uint32_t)tables->dirichlet_cells.size();
        }
      if (!dirichlet->n_cells)
        return;
      if (!dispatch_degree(p, [&](auto P) { lift_P<P()>(dst, g, include_mass ? sigma : 0.0, alpha); }))
        throw std::runtime_error("degree not instantiated");
    }
    // rhs = the lifting of g, completed over the ranks; constrained rows 0
    void
    rhs_dirichlet_raw(T *rhs, const T *g, bool include_mass)
    {
      HIP_CHECK(hipMemsetAsync(rhs, 0, (size_t)n_dofs() * sizeof(T), ctx->stream));
      dirichlet_lift_add_raw(rhs, g, include_mass, -1.0);
      exchange_add_raw(rhs + tables->n_interior);
    }
    void
    rhs_dirichlet(mgamd_vec &rhs, const mgamd_vec &g, bool include_mass) override
    {
      if (rhs.n != n_dofs() || g.n != n_dofs())
        throw std::invalid_argument("rhs_dirichlet: vector size mismatch (" + std::to_string(rhs.n) + ", " + std::to_string(g.n) + " for " +
                                    std::to_string(n_dofs()) + " DoFs)");
      if (rhs.data == g.data)
        throw std::invalid_argument("rhs_dirichlet: rhs and g must differ");
      rhs_dirichlet_raw(rhs.as<T>(), g.as<T>(), include_mass);
    }
    // x: the Dirichlet range from g, then the hanging DoFs from their parents (Dirichlet parents read the value just written)
    void
    distribute_values(mgamd_vec &x, const mgamd_vec &g) override
    {
      if (x.n != n_dofs() || g.n != n_dofs())
        throw std::invalid_argument("distribute_values: vector size mismatch (" + std::to_string(x.n) + ", " + std::to_string(g.n) + " for " +
                                    std::to_string(n_dofs()) + " DoFs)");
      if (tables->ls_level)
        throw std::invalid_argument("distribute_values: refused on the level of a local-smoothing hierarchy; use the active-mesh operator");
      distribute_values_core(x, g);
    }
    void
    distribute_values_core(mgamd_vec &x, const mgamd_vec &g) override
    {
      T       *xp = x.as<T>();
      const T *gp = g.as<T>();
      if (!hanging)
        {
          hanging = std::make_unique<HangingDev>();
          std::vector<uint32_t> ptr, col;
          std::vector<double>   val;
          tables->hanging_rows(ptr, col, val);
          hanging->n_rows = (uint32_t)ptr.size() - 1;
          if (col.empty())
            hanging->n_rows = 0;
          else
            {
              hanging->ptr.upload(ptr);
              hanging->col.upload(col);
              hanging->val.upload(val);
            }
        }
      const uint32_t d0 = tables->first_dirichlet(), d1 = d0 + tables->n_dirichlet;
      if (d1 > d0 && xp != gp)
        hipLaunchKernelGGL(dirichlet_copy_kernel<T>, grid_for(d1 - d0), 256, 0, ctx->stream, xp, gp, d0, d1);
      if (hanging->n_rows)
        hipLaunchKernelGGL(hanging_rows_kernel<T>, grid_for(hanging->n_rows), 256, 0, ctx->stream, xp, hanging->ptr.p, hanging->col.p,
                           hanging->val.p, d1, hanging->n_rows);
      HIP_CHECK(hipGetLastError());
    }

    // defined in level_operator_apply.hpp, instantiated in apply_inst.hip with the operator passes: the two launches of the
    // indicator on the device tables
    template <int P>
    void
    estimate_P(const T *u, const double *q);

    void
    estimate_error(const mgamd_vec &u, const double *q, double *eta) override
    {
      if (comm || halo_plan)
        throw std::invalid_argument("estimate_error: not implemented: sharded (the operator is distributed; the jumps across the cut "
                                    "need the neighbour rank's fluxes)");
      tables->refuse_estimate();
      if (!eta)
        throw std::invalid_argument("estimate_error: eta is null (a host array of n_cells values)");
      if (u.n != n_dofs())
        throw std::invalid_argument("estimate_error: vector size mismatch (" + std::to_string(u.n) + " for " + std::to_string(n_dofs()) + " DoFs)");
      const T *up = u.as<T>(); // (refuses the other number type)
      if (q)
        tables->check_boundary_flux(q);
      ensure_estimator(true, "estimate_error");
      HIP_CHECK(hipEventRecord(estimator->e0, ctx->stream));
      if (!dispatch_degree(p, [&](auto P) { estimate_P<P()>(up, q); }))
        throw std::runtime_error("degree not instantiated");
      HIP_CHECK(hipEventRecord(estimator->e1, ctx->stream));
      HIP_CHECK(hipMemcpyAsync(eta, estimator->eta.p, (size_t)estimator->n_cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      ctx->sync();
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, estimator->e0, estimator->e1));
      estimator->kernel_ms = ms;
    }
    void
    estimator_info(uint64_t &bytes, double &build_ms, double &kernel_ms) const override
    {
      bytes     = estimator ? estimator->bytes : 0;
      build_ms  = estimator ? estimator->build_ms : 0.0;
      kernel_ms = estimator ? estimator->kernel_ms : 0.0;
    }

    // defined in level_operator_apply.hpp, instantiated in apply_inst.hip: the launch of difference_norm_kernel
    template <int P>
    void
    difference_norm_P(const T *u, int kind, const T *values, const T *gradients, int n_q, int norm);

    void
    integrate_difference(const mgamd_vec &u, int kind, const mgamd_vec *values, const mgamd_vec *gradients, int n_q, int norm, double *out) override
    {
      const char *who = "integrate_difference";
      if (comm || halo_plan)
        throw std::invalid_argument("integrate_difference: not implemented: sharded (the operator is distributed; one rank only)");
      tables->refuse_estimate(who);
      if (!out)
        throw std::invalid_argument("integrate_difference: out is null (a host array of n_cells values)");
      if (norm != NORM_L2 && norm != NORM_H1_SEMINORM && norm != NORM_ENERGY && norm != NORM_LINFTY)
        throw std::invalid_argument("integrate_difference: unknown norm " + std::to_string(norm) +
                                    " (MGAMD_NORM_L2, MGAMD_NORM_H1_SEMINORM, MGAMD_NORM_ENERGY or MGAMD_NORM_LINFTY)");
      if (kind != -1 && kind != 0 && kind != 1)
        throw std::invalid_argument("integrate_difference: unknown kind " + std::to_string(kind) + " (0: w = 0, 1: the Gaussian)");
      const int nq = tables->resolve_n_q(n_q, who);
      if (u.n != n_dofs())
        throw std::invalid_argument("integrate_difference: vector size mismatch (" + std::to_string(u.n) + " for " + std::to_string(n_dofs()) + " DoFs)");
      const T     *up = u.as<T>(); // (refuses the other number type)
      const T     *vp = nullptr, *gp = nullptr;
      const size_t n_points = tables->tria->cells.size() * (size_t)nq * nq * nq;
      const bool   with_gradient = norm == NORM_H1_SEMINORM || norm == NORM_ENERGY;
      if (kind == -1)
        {
          if (norm != NORM_H1_SEMINORM)
            {
              if (!values)
                throw std::invalid_argument("integrate_difference: values is null (n_cells n_q^3 values of w at the quadrature points)");
              if (values->n != n_points)
                throw std::invalid_argument("integrate_difference: values size mismatch (" + std::to_string(values->n) + " for " +
                                            std::to_string(n_points) + " quadrature points)");
              vp = values->as<T>();
            }
          if (with_gradient)
            {
              if (!gradients)
                throw std::invalid_argument("integrate_difference: a gradient norm without gradients (3 n_cells n_q^3 values of grad w at the "
                                            "quadrature points)");
              if (gradients->n != 3 * n_points)
                throw std::invalid_argument("integrate_difference: gradients size mismatch (" + std::to_string(gradients->n) + " for 3 x " +
                                            std::to_string(n_points) + " quadrature points)");
              gp = gradients->as<T>();
            }
        }
      ensure_estimator(false, who);
      EstimatorDev &e = *estimator;
      if (!e.norms)
        {
          std::vector<double> o;
          tables->cell_origins(o);
          e.origin.upload(o);
          e.norm_out.alloc(e.n_cells);
          e.norm_bytes = (o.size() + e.n_cells) * sizeof(double);
          e.norms      = true;
        }
      HIP_CHECK(hipEventRecord(e.e0, ctx->stream));
      if (!dispatch_degree(p, [&](auto P) { difference_norm_P<P()>(up, kind, vp, gp, nq, norm); }))
        throw std::runtime_error("degree not instantiated");
      HIP_CHECK(hipEventRecord(e.e1, ctx->stream));
      HIP_CHECK(hipMemcpyAsync(out, e.norm_out.p, (size_t)e.n_cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      ctx->sync();
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, e.e0, e.e1));
      e.norm_kernel_ms = ms;
    }
    void
    error_norm_info(uint64_t &bytes, double &kernel_ms, int &neighbours_built) const override
    {
      const bool on    = estimator && estimator->norms;
      bytes            = on ? estimator->gather_bytes + estimator->norm_bytes : 0;
      kernel_ms        = on ? estimator->norm_kernel_ms : 0.0;
      neighbours_built = estimator && estimator->neighbours ? 1 : 0;
    }

    // Cell evaluate and integrate (kernels_cell_values.hpp).  They hold nothing of their own but the events of their timings: the
    // gather table is the estimator's (ensure_estimator(false)), neither the neighbour table nor the norms' part is built.
    struct CellValuesDev
    {
      hipEvent_t ev[4]     = {nullptr, nullptr, nullptr, nullptr}; // evaluate: 0, 1; integrate: 2, 3
      bool       timed[2]  = {false, false};
      ~CellValuesDev()
      {
        for (hipEvent_t e : ev)
          if (e)
            (void)hipEventDestroy(e);
      }
    };
    std::unique_ptr<CellValuesDev> cell_values;
    // the refusals the two calls share, then the shared table; returns the resolved n_q
    int
    ensure_cell_values(int n_q, const char *who)
    {
      if (comm || halo_plan)
        throw std::invalid_argument(std::string(who) + ": not implemented: sharded (the operator is distributed; one rank only)");
      tables->refuse_estimate(who);
      return tables->resolve_n_q(n_q, who);
    }
    void
    build_cell_values(const char *who)
    {
      ensure_estimator(false, who);
      if (!cell_values)
        {
          auto dev = std::make_unique<CellValuesDev>();
          for (hipEvent_t &e : dev->ev)
            HIP_CHECK(hipEventCreate(&e));
          cell_values = std::move(dev);
        }
    }
    // defined in level_operator_apply.hpp, instantiated in apply_inst.hip: the launches of cell_evaluate_kernel and cell_integrate_kernel
    template <int P>
    void
    cell_evaluate_P(const T *u, int n_q, T *values, T *gradients);
    template <int P>
    void
    cell_integrate_P(const T *values, const T *gradients, int n_q, T *b);

    void
    evaluate(const mgamd_vec *u, int n_q, mgamd_vec *values, mgamd_vec *gradients) override
    {
      const char *who = "evaluate";
      const int   nq  = ensure_cell_values(n_q, who);
      if (!u)
        throw std::invalid_argument("evaluate: u is null (a device vector of n_dofs values)");
      if (!values && !gradients)
        throw std::invalid_argument("evaluate: neither values nor gradients (at least one output)");
      if (u->n != n_dofs())
        throw std::invalid_argument("evaluate: vector size mismatch (" + std::to_string(u->n) + " for " + std::to_string(n_dofs()) + " DoFs)");
      const T     *up = u->as<T>(); // (refuses the other number type)
      T           *vp = nullptr, *gp = nullptr;
      const size_t n_points = tables->tria->cells.size() * (size_t)nq * nq * nq;
      if (values)
        {
          if (values->n != n_points)
            throw std::invalid_argument("evaluate: values size mismatch (" + std::to_string(values->n) + " for " + std::to_string(n_points) +
                                        " quadrature points)");
          vp = values->as<T>();
        }
      if (gradients)
        {
          if (gradients->n != 3 * n_points)
            throw std::invalid_argument("evaluate: gradients size mismatch (" + std::to_string(gradients->n) + " for 3 x " +
                                        std::to_string(n_points) + " quadrature points)");
          gp = gradients->as<T>();
        }
      if ((vp && (const void *)vp == (const void *)up) || (gp && (const void *)gp == (const void *)up) || (vp && vp == gp))
        throw std::invalid_argument("evaluate: u, values and gradients must differ");
      build_cell_values(who);
      HIP_CHECK(hipEventRecord(cell_values->ev[0], ctx->stream));
      if (!dispatch_degree(p, [&](auto P) { cell_evaluate_P<P()>(up, nq, vp, gp); }))
        throw std::runtime_error("degree not instantiated");
      HIP_CHECK(hipEventRecord(cell_values->ev[1], ctx->stream));
      cell_values->timed[0] = true;
    }
    void
    integrate(const mgamd_vec *values, const mgamd_vec *gradients, int n_q, mgamd_vec *b) override
    {
      const char *who = "integrate";
      const int   nq  = ensure_cell_values(n_q, who);
      if (!b)
        throw std::invalid_argument("integrate: b is null (a device vector of n_dofs values)");
      if (!values && !gradients)
        throw std::invalid_argument("integrate: neither values nor gradients (at least one input)");
      if ((values && values->data == b->data) || (gradients && gradients->data == b->data))
        throw std::invalid_argument(std::string("integrate: b aliases ") + (values && values->data == b->data ? "values" : "gradients") +
                                    " (b is overwritten before the data is read)");
      if (b->n != n_dofs())
        throw std::invalid_argument("integrate: vector size mismatch (" + std::to_string(b->n) + " for " + std::to_string(n_dofs()) + " DoFs)");
      T           *bp = b->as<T>(); // (refuses the other number type)
      const T     *vp = nullptr, *gp = nullptr;
      const size_t n_points = tables->tria->cells.size() * (size_t)nq * nq * nq;
      if (values)
        {
          if (values->n != n_points)
            throw std::invalid_argument("integrate: values size mismatch (" + std::to_string(values->n) + " for " + std::to_string(n_points) +
                                        " quadrature points)");
          vp = values->as<T>();
        }
      if (gradients)
        {
          if (gradients->n != 3 * n_points)
            throw std::invalid_argument("integrate: gradients size mismatch (" + std::to_string(gradients->n) + " for 3 x " +
                                        std::to_string(n_points) + " quadrature points)");
          gp = gradients->as<T>();
        }
      build_cell_values(who);
      HIP_CHECK(hipEventRecord(cell_values->ev[2], ctx->stream));
      HIP_CHECK(hipMemsetAsync(bp, 0, (size_t)n_dofs() * sizeof(T), ctx->stream));
      if (!dispatch_degree(p, [&](auto P) { cell_integrate_P<P()>(vp, gp, nq, bp); }))
        throw std::runtime_error("degree not instantiated");
      HIP_CHECK(hipEventRecord(cell_values->ev[3], ctx->stream));
      cell_values->timed[1] = true;
    }
    void
    cell_values_info(uint64_t &bytes, double &evaluate_ms, double &integrate_ms) const override
    {
      bytes       = cell_values && estimator ? estimator->gather_bytes : 0;
      evaluate_ms = integrate_ms = 0.0;
      for (int k = 0; k < 2; ++k)
        if (cell_values && cell_values->timed[k])
          {
            float ms = 0.f;
            HIP_CHECK(hipEventSynchronize(cell_values->ev[2 * k + 1]));
            HIP_CHECK(hipEventElapsedTime(&ms, cell_values->ev[2 * k], cell_values->ev[2 * k + 1]));
            (k == 0 ? evaluate_ms : integrate_ms) = ms;
          }
    }

    // Point evaluation and point sources (kernels_point_values.hpp).  Of the operator: the sorted Morton keys of the leaves and their
    // corners and edges in integer coordinates (8 + 16 bytes per leaf), uploaded by the first point set.  Of a point set: the leaf and
    // the reference coordinate per point (the locate kernel's outputs) and the CSR list of occupied leaves with the sorted points.
    // The binning by leaf runs on the HOST when the set is built (the stated debt for moving points: DESIGN.md).
    struct PointLocatorDev
    {
      DBuf<uint64_t> keys;
      DBuf<uint32_t> corner; // [n_cells][4]: i, j, k, edge, in integer coordinates
      uint32_t       n_cells = 0;
      uint64_t       bytes   = 0;
    };
    std::unique_ptr<PointLocatorDev> point_locator;
    struct PointSetDev : PointSetBase
    {
      LevelOperator *self = nullptr;
      DBuf<int32_t>  cell;
      DBuf<double>   ref;
      DBuf<uint32_t> leaf, ptr, perm, occ;
      uint32_t       n_occupied = 0;
      uint64_t       bytes      = 0;
      double         build_ms   = 0.0;
      hipEvent_t     ev[6]      = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // locate: 0, 1; evaluate: 2, 3; integrate: 4, 5
      bool           timed[3]   = {false, false, false};
      ~PointSetDev() override
      {
        for (hipEvent_t e : ev)
          if (e)
            (void)hipEventDestroy(e);
      }
      void
      orphan()
      {
        this->op = nullptr;
        self     = nullptr;
        for (DBuf<uint32_t> *b : {&leaf, &ptr, &perm, &occ})
          b->alloc(0);
        cell.alloc(0);
        ref.alloc(0);
        bytes = 0;
      }
      void
      alive(const char *who) const
      {
        if (!self)
          throw std::invalid_argument(std::string(who) + ": the point set's operator was destroyed");
      }
      void
      get(int32_t *cell_out, double *ref_out) const override
      {
        alive("point_set");
        if (!this->n)
          return;
        HIP_CHECK(hipStreamSynchronize(self->ctx->stream));
        if (cell_out)
          HIP_CHECK(hipMemcpy(cell_out, cell.p, this->n * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (ref_out)
          HIP_CHECK(hipMemcpy(ref_out, ref.p, 3 * this->n * sizeof(double), hipMemcpyDeviceToHost));
      }
      void
      evaluate(const mgamd_vec *u, mgamd_vec *values, mgamd_vec *gradients) override
      {
        alive("point_evaluate");
        self->point_evaluate(*this, u, values, gradients);
      }
      void
      integrate(const mgamd_vec *values, const mgamd_vec *gradients, mgamd_vec *b) override
      {
        alive("point_integrate");
        self->point_integrate(*this, values, gradients, b);
      }
      void
      info(uint64_t &bytes_out, double &build, double &locate_ms, double &evaluate_ms, double &integrate_ms) const override
      {
        bytes_out = bytes;
        build     = build_ms;
        double *out[3] = {&locate_ms, &evaluate_ms, &integrate_ms};
        for (int k = 0; k < 3; ++k)
          {
            *out[k] = 0.0;
            if (timed[k])
              {
                float ms = 0.f;
                HIP_CHECK(hipEventSynchronize(ev[2 * k + 1]));
                HIP_CHECK(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
                *out[k] = ms;
              }
          }
      }
    };
    // the operator's sets; a set whose handle outlives the operator is emptied here and refuses every later call
    struct PointSets
    {
      std::vector<std::shared_ptr<PointSetDev>> v;
      ~PointSets()
      {
        for (auto &ps : v)
          ps->orphan();
      }
    } point_sets;
    void
    refuse_points(const char *who) const
    {
      if (comm || halo_plan)
        throw std::invalid_argument(std::string(who) + ": not implemented: sharded (the operator is distributed; one rank only)");
      tables->refuse_estimate(who);
    }
    std::shared_ptr<PointSetBase>
    point_set_create(uint64_t n, const double *xyz) override
    {
      const char *who = "point_set";
      static_assert(LMAX <= 21, "spread3 takes 21 bits per coordinate");
      refuse_points(who);
      if (n && !xyz)
        throw std::invalid_argument("point_set: xyz is null (3 n doubles)");
      if (n > 0x7fffffffu)
        throw std::invalid_argument("point_set: " + std::to_string(n) + " points refused (at most 2^31 - 1 per set)");
      if (n && !point_locator) // (an empty set uploads and launches nothing)
        {
          auto                  dev = std::make_unique<PointLocatorDev>();
          std::vector<uint64_t> keys;
          tables->leaf_keys(keys);
          std::vector<uint32_t> corner(4 * keys.size());
          for (size_t ci = 0; ci < keys.size(); ++ci)
            {
              const Cell    &c = tables->tria->cells[ci];
              const uint32_t e = 1u << (LMAX - c.level);
              corner[4 * ci]     = c.i * e;
              corner[4 * ci + 1] = c.j * e;
              corner[4 * ci + 2] = c.k * e;
              corner[4 * ci + 3] = e;
            }
          dev->keys.upload(keys);
          dev->corner.upload(corner);
          dev->n_cells  = (uint32_t)keys.size();
          dev->bytes    = keys.size() * 8 + corner.size() * 4;
          point_locator = std::move(dev);
        }
      auto ps  = std::make_shared<PointSetDev>();
      ps->op   = this;
      ps->self = this;
      ps->n    = n;
      for (hipEvent_t &e : ps->ev)
        HIP_CHECK(hipEventCreate(&e));
      if (n)
        {
          // locate on the device; the coordinates are not kept
          DBuf<double> d_xyz;
          d_xyz.alloc(3 * n);
          HIP_CHECK(hipMemcpyAsync(d_xyz.p, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
          ps->cell.alloc(n);
          ps->ref.alloc(3 * n);
          PointLocateArgs a;
          a.xyz     = d_xyz.p;
          a.n       = n;
          a.keys    = point_locator->keys.p;
          a.corner  = point_locator->corner.p;
          a.n_cells = point_locator->n_cells;
          a.cell    = ps->cell.p;
          a.ref     = ps->ref.p;
          HIP_CHECK(hipEventRecord(ps->ev[0], ctx->stream));
          hipLaunchKernelGGL((point_locate_kernel<LMAX>), (unsigned)std::min<uint64_t>(4096u, (n + 255) / 256), 256, 0, ctx->stream, a);
          HIP_CHECK(hipGetLastError());
          HIP_CHECK(hipEventRecord(ps->ev[1], ctx->stream));
          ps->timed[0] = true;
          std::vector<int32_t> cell(n);
          HIP_CHECK(hipMemcpyAsync(cell.data(), ps->cell.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
          HIP_CHECK(hipStreamSynchronize(ctx->stream));
          // bin by leaf on the host: a counting sort, stable, so the points of a leaf keep the caller's order
          const auto            t0 = std::chrono::steady_clock::now();
          const uint32_t        nc = point_locator->n_cells;
          std::vector<uint32_t> count(nc + 1, 0), leaf, ptr, perm, occ;
          for (uint64_t k = 0; k < n; ++k)
            if (cell[k] >= 0)
              {
                if ((uint32_t)cell[k] >= nc)
                  throw std::runtime_error("point_set: the locate kernel returned a leaf outside the mesh");
                ++count[cell[k] + 1];
              }
          std::vector<uint32_t> slot(nc, 0); // leaf -> its occupied index
          ptr.push_back(0);
          for (uint32_t ci = 0; ci < nc; ++ci)
            {
              if (count[ci + 1])
                {
                  slot[ci] = (uint32_t)leaf.size();
                  leaf.push_back(ci);
                  ptr.push_back(ptr.back() + count[ci + 1]);
                }
              count[ci + 1] += count[ci]; // -> the first sorted position of leaf ci + 1
            }
          ps->n_found = ptr.back();
          perm.resize(ps->n_found);
          occ.resize(ps->n_found);
          for (uint64_t k = 0; k < n; ++k)
            if (cell[k] >= 0)
              {
                const uint32_t j = count[cell[k]]++;
                perm[j]          = (uint32_t)k;
                occ[j]           = slot[cell[k]];
              }
          ps->n_occupied = (uint32_t)leaf.size();
          ps->leaf.upload(leaf);
          ps->ptr.upload(ptr);
          ps->perm.upload(perm);
          ps->occ.upload(occ);
          ps->bytes    = n * (sizeof(int32_t) + 3 * sizeof(double)) + (leaf.size() + ptr.size() + perm.size() + occ.size()) * sizeof(uint32_t);
          ps->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
      point_sets.v.push_back(ps);
      return ps;
    }
    void
    point_set_destroy(PointSetBase *ps) override
    {
      for (size_t i = 0; i < point_sets.v.size(); ++i)
        if (point_sets.v[i].get() == ps)
          {
            HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (a kernel of the set may be in flight)
            point_sets.v[i]->orphan();
            point_sets.v.erase(point_sets.v.begin() + i);
            return;
          }
    }
    void
    point_tables_bytes(uint64_t &locator, uint64_t &gather) const override
    {
      locator = point_locator ? point_locator->bytes : 0;
      gather  = estimator ? estimator->gather_bytes : 0;
    }
    // defined in level_operator_apply.hpp, instantiated in apply_inst.hip: the launches of point_evaluate_kernel and point_integrate_kernel
    template <int P>
    void
    point_evaluate_P(const PointSetDev &ps, const T *u, T *values, T *gradients);
    template <int P>
    void
    point_integrate_P(const PointSetDev &ps, const T *values, const T *gradients, T *b);
    void
    point_evaluate(PointSetDev &ps, const mgamd_vec *u, mgamd_vec *values, mgamd_vec *gradients)
    {
      const char *who = "point_evaluate";
      refuse_points(who);
      if (!u)
        throw std::invalid_argument("point_evaluate: u is null (a device vector of n_dofs values)");
      if (!values && !gradients)
        throw std::invalid_argument("point_evaluate: neither values nor gradients (at least one output)");
      if (u->n != n_dofs())
        throw std::invalid_argument("point_evaluate: vector size mismatch (" + std::to_string(u->n) + " for " + std::to_string(n_dofs()) + " DoFs)");
      const T *up = u->as<T>(); // (refuses the other number type)
      T       *vp = nullptr, *gp = nullptr;
      if (values)
        {
          if (values->n != ps.n)
            throw std::invalid_argument("point_evaluate: values size mismatch (" + std::to_string(values->n) + " for " + std::to_string(ps.n) + " points)");
          vp = values->as<T>();
        }
      if (gradients)
        {
          if (gradients->n != 3 * ps.n)
            throw std::invalid_argument("point_evaluate: gradients size mismatch (" + std::to_string(gradients->n) + " for 3 x " + std::to_string(ps.n) +
                                        " points)");
          gp = gradients->as<T>();
        }
      if (ps.n && ((vp && (const void *)vp == (const void *)up) || (gp && (const void *)gp == (const void *)up) || (vp && vp == gp)))
        throw std::invalid_argument("point_evaluate: u, values and gradients must differ");
      if (!ps.n)
        return; // (nothing is built and nothing is launched)
      ensure_estimator(false, who);
      HIP_CHECK(hipEventRecord(ps.ev[2], ctx->stream));
      if (ps.n_found < ps.n) // points that were not found: exactly 0 in every output
        {
          if (vp)
            HIP_CHECK(hipMemsetAsync(vp, 0, ps.n * sizeof(T), ctx->stream));
          if (gp)
            HIP_CHECK(hipMemsetAsync(gp, 0, 3 * ps.n * sizeof(T), ctx->stream));
        }
      if (ps.n_found)
        if (!dispatch_degree(p, [&](auto P) { point_evaluate_P<P()>(ps, up, vp, gp); }))
          throw std::runtime_error("degree not instantiated");
      HIP_CHECK(hipEventRecord(ps.ev[3], ctx->stream));
      ps.timed[1] = true;
    }
    void
    point_integrate(PointSetDev &ps, const mgamd_vec *values, const mgamd_vec *gradients, mgamd_vec *b)
    {
      const char *who = "point_integrate";
      refuse_points(who);
      if (!b)
        throw std::invalid_argument("point_integrate: b is null (a device vector of n_dofs values)");
      if (!values && !gradients)
        throw std::invalid_argument("point_integrate: neither values nor gradients (at least one input)");
      if (ps.n && ((values && values->data == b->data) || (gradients && gradients->data == b->data)))
        throw std::invalid_argument(std::string("point_integrate: b aliases ") + (values && values->data == b->data ? "values" : "gradients") +
                                    " (b is overwritten before the data is read)");
      if (b->n != n_dofs())
        throw std::invalid_argument("point_integrate: vector size mismatch (" + std::to_string(b->n) + " for " + std::to_string(n_dofs()) + " DoFs)");
      T       *bp = b->as<T>(); // (refuses the other number type)
      const T *vp = nullptr, *gp = nullptr;
      if (values)
        {
          if (values->n != ps.n)
            throw std::invalid_argument("point_integrate: values size mismatch (" + std::to_string(values->n) + " for " + std::to_string(ps.n) + " points)");
          vp = values->as<T>();
        }
      if (gradients)
        {
          if (gradients->n != 3 * ps.n)
            throw std::invalid_argument("point_integrate: gradients size mismatch (" + std::to_string(gradients->n) + " for 3 x " + std::to_string(ps.n) +
                                        " points)");
          gp = gradients->as<T>();
        }
      if (ps.n_found)
        ensure_estimator(false, who);
      HIP_CHECK(hipEventRecord(ps.ev[4], ctx->stream));
      HIP_CHECK(hipMemsetAsync(bp, 0, (size_t)n_dofs() * sizeof(T), ctx->stream));
      if (ps.n_found)
        if (!dispatch_degree(p, [&](auto P) { point_integrate_P<P()>(ps, vp, gp, bp); }))
          throw std::runtime_error("degree not instantiated");
      HIP_CHECK(hipEventRecord(ps.ev[5], ctx->stream));
      ps.timed[2] = true;
    }

    size_t
    read_debug_stamps(unsigned long long *out, size_t max_count) override
    {
      ctx->sync();
      const size_t n = std::min(max_count, stamps.n);
      if (n)
        HIP_CHECK(hipMemcpy(out, stamps.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      return n;
    }

    void
    compute_inverse_diagonal(mgamd_vec &d) override
    {
      if (d.n != n_dofs())
        throw std::invalid_argument("compute_inverse_diagonal: vector size mismatch");
      Epilogue<T> e{d.as<T>(), nullptr, nullptr, nullptr, nullptr, T(0), T(0)};
      apply<MODE_VMULT>(nullptr, e, true);
    }
  };

} // namespace mgamd
