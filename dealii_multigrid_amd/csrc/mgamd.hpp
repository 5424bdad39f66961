// mgamd.hpp -- header-only C++ layer over the C ABI (include/mgamd.h) that re-exposes the MI355X path with
// the class and method names deal.II gives it in the reference, so that code written like
// ref:multigrid_throughput.cc:817-1666 (mg_solve / solve_with_global_coarsening) compiles against it:
//
//   mgamd::Triangulation          <-> parallel::distributed::Triangulation<3> + GridGenerator::create_*
//   mgamd::DoFHandler             <-> DoFHandler<3> + AffineConstraints + MatrixFree::reinit
//   mgamd::Vector                 <-> LinearAlgebra::distributed::Vector<Number>
//   mgamd::Operator               <-> Operator<3,1,Number>                 (ref:include/operator.h:11-557)
//   mgamd::PreconditionChebyshev  <-> PreconditionChebyshev<Operator,Vector,DiagonalMatrix<Vector>>
//   mgamd::MGTwoLevelTransfer     <-> MGTwoLevelTransfer<3,Vector>
//   mgamd::PreconditionMG         <-> Multigrid<Vector> + PreconditionMG + MGTransferGlobalCoarsening
//   mgamd::SolverCG / ReductionControl
//
// Status codes become exceptions (std::runtime_error), as AssertThrow does in the reference
// (ref:multigrid_throughput.cc:2444-2468 catches them in main).
#pragma once
#include "../../include/mgamd.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <thread>

#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace mgamd
{
  inline void
  check(int status)
  {
    if (status != MGAMD_OK)
      throw std::runtime_error(mgamd_last_error());
  }

  class Triangulation
  {
  public:
    Triangulation(const std::string &geometry_type, unsigned n_ref_global, unsigned n_ref_local = 0)
    {
      mgamd_tria *t = nullptr;
      check(mgamd_tria_create(geometry_type.c_str(), n_ref_global, n_ref_local, &t));
      h.reset(t, mgamd_tria_destroy);
      query();
    }
    // a caller-built octree over one root cell (the active cells of a parallel::distributed::Triangulation as (level, i, j, k));
    // checked for exact tiling and full 2:1 balance (mgamd_tria_create_from_leaves)
    static std::shared_ptr<Triangulation>
    from_leaves(const std::vector<uint8_t> &level, const std::vector<uint32_t> &i, const std::vector<uint32_t> &j, const std::vector<uint32_t> &k)
    {
      if (level.size() != i.size() || level.size() != j.size() || level.size() != k.size())
        throw std::runtime_error("from_leaves: arrays of different lengths");
      mgamd_tria *t = nullptr;
      check(mgamd_tria_create_from_leaves(level.size(), level.data(), i.data(), j.data(), k.data(), &t));
      auto r = std::shared_ptr<Triangulation>(new Triangulation());
      r->h.reset(t, mgamd_tria_destroy);
      r->query();
      return r;
    }
    // one step of MGTransferGlobalCoarseningTools::create_geometric_coarsening_sequence
    std::shared_ptr<Triangulation>
    coarsen() const
    {
      mgamd_tria *t = nullptr;
      check(mgamd_tria_coarsen(h.get(), &t));
      auto r = std::shared_ptr<Triangulation>(new Triangulation());
      r->h.reset(t, mgamd_tria_destroy);
      r->query();
      return r;
    }
    // Flagged refinement (mgamd_tria_refine; in deal.II: set_refine_flag + execute_coarsening_and_refinement): every leaf with a
    // non-zero flag (one per leaf, order of mgamd_tria_get_cells) is replaced by its eight children, then the minimal ripple to the
    // full 2:1 balance runs.  Children inherit their parent's coefficient value; the dirichlet_faces mask and the Robin
    // coefficients are copied.  parent, if given, receives per new leaf the index of the old leaf that is it or contains it.
    std::shared_ptr<Triangulation>
    refine(const std::vector<uint8_t> &flags, std::vector<uint64_t> *parent = nullptr) const
    {
      if (flags.size() != n_cells)
        throw std::runtime_error("refine: " + std::to_string(flags.size()) + " flags for " + std::to_string(n_cells) + " cells");
      if (parent)
        parent->assign(8 * n_cells, 0); // (mgamd_tria_refine: at most 8 n_cells new cells, every leaf split once)
      mgamd_tria *t = nullptr;
      check(mgamd_tria_refine(h.get(), flags.data(), &t, parent ? parent->data() : nullptr));
      auto r = std::shared_ptr<Triangulation>(new Triangulation());
      r->h.reset(t, mgamd_tria_destroy);
      r->query();
      if (parent)
        parent->resize(r->n_cells);
      return r;
    }
    // The diffusion coefficient a > 0 of -div(a grad u) + sigma u: one value per leaf in the order of mgamd_tria_get_cells; an empty
    // vector resets to a = 1.  coarsen() carries it down (the mean over each coarse leaf); DoFs copy it when they are built.
    void
    set_coefficient(const std::vector<double> &a)
    {
      if (!a.empty() && a.size() != n_cells)
        throw std::runtime_error("set_coefficient: " + std::to_string(a.size()) + " values for " + std::to_string(n_cells) + " cells");
      check(mgamd_tria_set_coefficient(h.get(), a.empty() ? nullptr : a.data()));
    }
    std::vector<double>
    coefficient() const
    {
      std::vector<double> a(n_cells);
      check(mgamd_tria_get_coefficient(h.get(), a.data()));
      return a;
    }
    bool
    has_coefficient() const
    {
      int has = 0;
      check(mgamd_tria_has_coefficient(h.get(), &has));
      return has != 0;
    }
    // Which faces of the cube are Dirichlet: bit f = 2 axis + side (0: x = -1, 1: x = +1, ... 5: z = +1); the others are natural
    // (Neumann).  Default 0x3F.  coarsen() inherits it; DoFs copy it when they are built (mgamd_tria_set_dirichlet_faces).
    void
    set_dirichlet_faces(unsigned mask)
    {
      check(mgamd_tria_set_dirichlet_faces(h.get(), mask));
    }
    unsigned
    dirichlet_faces() const
    {
      unsigned mask = 0;
      check(mgamd_tria_get_dirichlet_faces(h.get(), &mask));
      return mask;
    }
    // Convective (Robin) faces: a grad u . n + beta[f] (u - u_ext) = 0 on face f, beta[f] >= 0, default 0; refused on a Dirichlet
    // face.  coarsen() inherits the values; DoFs copy them when they are built (mgamd_tria_set_robin_coefficients).  The load of
    // u_ext is Operator::rhs_boundary_flux with q[f] = beta[f] u_ext.
    void
    set_robin_coefficients(const std::array<double, 6> &beta)
    {
      check(mgamd_tria_set_robin_coefficients(h.get(), beta.data()));
    }
    std::array<double, 6>
    robin_coefficients() const
    {
      std::array<double, 6> beta{};
      check(mgamd_tria_get_robin_coefficients(h.get(), beta.data()));
      return beta;
    }
    // local smoothing: all cells of refinement level `level`, active or not (the level of DoFHandler::distribute_mg_dofs)
    std::shared_ptr<Triangulation>
    level_mesh(unsigned level) const
    {
      mgamd_tria *t = nullptr;
      check(mgamd_tria_level_mesh(h.get(), level, &t));
      auto r = std::shared_ptr<Triangulation>(new Triangulation());
      r->h.reset(t, mgamd_tria_destroy);
      r->query();
      return r;
    }
    uint64_t
    n_global_active_cells() const
    {
      return n_cells;
    }
    unsigned
    n_global_levels() const
    {
      return n_levels;
    }
    uint64_t
    n_cells_with_hanging_nodes() const
    {
      return n_cells_hn;
    }
    mgamd_tria *
    get() const
    {
      return h.get();
    }

  private:
    Triangulation() = default;
    void
    query()
    {
      check(mgamd_tria_info(h.get(), &n_cells, &n_levels, &n_cells_hn));
    }
    std::shared_ptr<mgamd_tria> h;
    uint64_t                    n_cells = 0, n_cells_hn = 0;
    uint32_t                    n_levels = 0;
  };

  // The maximum strategy: flag every leaf with eta_K >= theta max eta.  A threshold keeps the exact ties of a symmetric mesh
  // together, which a fixed-number rule would cut by rounding.  An all-zero eta flags nothing, and so does an eta with a NaN in it.
  inline std::vector<uint8_t>
  mark_maximum(const std::vector<double> &eta, double theta)
  {
    double top = 0.0;
    for (double e : eta)
      top = std::isnan(e) ? e : std::max(top, e); // (NaN stays: std::max(NaN, x) is NaN)
    std::vector<uint8_t> flags(eta.size(), 0);
    if (top > 0.0)
      for (size_t t = 0; t < eta.size(); ++t)
        flags[t] = eta[t] >= theta * top ? 1 : 0;
    return flags;
  }

  // VectorTools::compute_global_error: the global norm from the per-leaf values of Operator::integrate_difference, the l2 norm of
  // the array for MGAMD_NORM_L2, _H1_SEMINORM and _ENERGY and its maximum for MGAMD_NORM_LINFTY
  inline double
  compute_global_error(const std::vector<double> &per_cell, int norm)
  {
    if (norm != MGAMD_NORM_L2 && norm != MGAMD_NORM_H1_SEMINORM && norm != MGAMD_NORM_ENERGY && norm != MGAMD_NORM_LINFTY)
      throw std::runtime_error("compute_global_error: unknown norm " + std::to_string(norm));
    double r = 0.0;
    for (double e : per_cell)
      r = norm == MGAMD_NORM_LINFTY ? std::max(r, e) : r + e * e;
    return norm == MGAMD_NORM_LINFTY ? r : std::sqrt(r);
  }

  // MGTransferGlobalCoarseningTools::create_geometric_coarsening_sequence (ref:multigrid_throughput.cc:2219-2224)
  inline std::vector<std::shared_ptr<const Triangulation>>
  create_geometric_coarsening_sequence(const std::shared_ptr<const Triangulation> &fine)
  {
    std::vector<std::shared_ptr<const Triangulation>> seq{fine};
    while (seq.back()->n_global_active_cells() > 1)
      seq.push_back(seq.back()->coarsen());
    return {seq.rbegin(), seq.rend()};
  }

  // MGTools::print_multigrid_statistics(triangulations) (ref:include/mg_tools.h:267-512, ref:multigrid_throughput.cc:1657-1665):
  // {workload_eff, workload_path_max, vertical_eff, horizontal_eff, mem_total} of the n_ranks-way partition of the level
  // meshes (coarse -> fine)
  inline std::vector<std::pair<std::string, double>>
  print_multigrid_statistics(const std::vector<std::shared_ptr<const Triangulation>> &triangulations, unsigned n_ranks = 1)
  {
    std::vector<const mgamd_tria *> t;
    for (const auto &x : triangulations)
      t.push_back(x->get());
    mgamd_partition *p = nullptr;
    check(mgamd_partition_create_ex(t.data(), (unsigned)t.size(), n_ranks, 2.0, 0, &p));
    double     st[5];
    const int  rc = mgamd_partition_statistics(p, st);
    mgamd_partition_destroy(p);
    check(rc);
    static const char *names[5] = {"workload_eff", "workload_path_max", "vertical_eff", "horizontal_eff", "mem_total"};
    std::vector<std::pair<std::string, double>> out;
    for (int i = 0; i < 5; ++i)
      out.emplace_back(names[i], st[i]);
    return out;
  }

  // The multigrid levels of `type` as (mesh index, degree), coarse -> fine, over n_meshes meshes, and whether they are local-smoothing
  // levels (mgamd_level_plan: the one place that knows the level structure of HMG-global, PMG, HPMG, HMG-local and HPMG-local)
  struct LevelPlan
  {
    std::vector<std::pair<unsigned, unsigned>> levels;
    bool                                       local_smoothing = false;
  };
  inline LevelPlan
  level_plan(const std::string &type, unsigned n_meshes, unsigned degree)
  {
    unsigned n = 0, mesh[64], deg[64];
    int      ls = 0;
    check(mgamd_level_plan(type.c_str(), n_meshes, degree, 64, &n, mesh, deg, &ls));
    LevelPlan plan;
    for (unsigned l = 0; l < n; ++l)
      plan.levels.emplace_back(mesh[l], deg[l]);
    plan.local_smoothing = ls != 0;
    return plan;
  }

  // ...::create_polynomial_coarsening_sequence(degree, bisect) (ref:multigrid_throughput.cc:1506-1510): the degrees of the PMG levels
  inline std::vector<unsigned>
  create_polynomial_coarsening_sequence(unsigned degree)
  {
    std::vector<unsigned> seq;
    for (const auto &level : level_plan("PMG", 1, degree).levels)
      seq.push_back(level.second);
    return seq;
  }

  // Domain decomposition of a level hierarchy, one rank per GPU (the reference partitions with p4est + RepartitioningPolicyTools,
  // ref:multigrid_throughput.cc:2066-2175): Morton cut of a root level into n_ranks weighted chunks; finer levels inherit it,
  // coarser levels are replicated.
  class Partition
  {
  public:
    // group > 1: two tiers -- levels below the root level with >= min_sub_root_cells cells are cut into n_ranks / group parts, each
    // held by `group` consecutive ranks (what the reference's agglomeration onto fewer processes is for,
    // ref:multigrid_throughput.cc:379-418,1464-1501); their operators take Communicator::subset(group)
    Partition(const std::vector<std::shared_ptr<const Triangulation>> &triangulations, unsigned n_ranks, double hanging_weight = 2.0,
              uint64_t min_root_cells = 0, unsigned group = 1, uint64_t min_sub_root_cells = 0)
      : triangulations(triangulations)
    {
      std::vector<const mgamd_tria *> t;
      for (const auto &x : triangulations)
        t.push_back(x->get());
      mgamd_partition *p = nullptr;
      check(mgamd_partition_create_tiered(t.data(), (unsigned)t.size(), n_ranks, hanging_weight, min_root_cells, group, min_sub_root_cells, &p));
      h.reset(p, mgamd_partition_destroy);
      check(mgamd_partition_info(h.get(), &root, &nr));
      check(mgamd_partition_tiers(h.get(), &sub_root, &grp));
    }
    unsigned
    root_level() const
    {
      return root;
    }
    unsigned
    sub_root_level() const // == root_level() without a subset tier
    {
      return sub_root;
    }
    unsigned
    group() const
    {
      return grp;
    }
    unsigned
    n_parts(unsigned level) const // pieces of the level: n_ranks, n_ranks / group on the subset tier, 1 = replicated
    {
      return level >= root ? nr : (level >= sub_root ? nr / grp : 1);
    }
    mgamd_partition *
    get() const
    {
      return h.get();
    }
    std::vector<std::shared_ptr<const Triangulation>> triangulations;

  private:
    std::shared_ptr<mgamd_partition> h;
    unsigned                         root = 0, sub_root = 0, grp = 1, nr = 1;
  };

  class DoFHandler
  {
  public:
    // mg_level = true: `tria` is Triangulation::level_mesh(l): the level DoFs of distribute_mg_dofs with the refinement-edge
    // set of MGConstrainedDoFs
    DoFHandler(const std::shared_ptr<const Triangulation> &tria, unsigned fe_degree, int max_brick = -1, bool mg_level = false)
      : tria(tria)
    {
      mgamd_dofs *d = nullptr;
      if (mg_level)
        check(mgamd_dofs_create_level(tria->get(), (int)fe_degree, max_brick, &d));
      else
        check(mgamd_dofs_create(tria->get(), (int)fe_degree, max_brick, &d));
      h.reset(d, mgamd_dofs_destroy);
      check(mgamd_dofs_info(h.get(), &info));
    }
    // one rank's share of level `level` of a partitioned hierarchy (mgamd_dofs_create_local): its cells + halo plan on a
    // distributed level, the whole level on a replicated one
    DoFHandler(const Partition &partition, unsigned level, unsigned rank, unsigned fe_degree, int max_brick = -1)
      : tria(partition.triangulations.at(level))
    {
      mgamd_dofs *d = nullptr;
      check(mgamd_dofs_create_local(partition.get(), level, rank, (int)fe_degree, max_brick, &d));
      h.reset(d, mgamd_dofs_destroy);
      check(mgamd_dofs_info(h.get(), &info));
    }
    uint64_t
    n_dofs() const
    {
      return info.n_dofs;
    }
    const Triangulation &
    get_triangulation() const
    {
      return *tria;
    }
    mgamd_dofs *
    get() const
    {
      return h.get();
    }
    // The mass term: operators, matrices and right-hand sides built from this handler AFTER the call represent K + sigma M
    // (mgamd_dofs_set_mass_coefficient).  sigma >= 0; local-smoothing levels (mg_level) only take 0.  The handle is shared by the
    // copies of this object, so the method is const like the handle's other uses.
    void
    set_mass_coefficient(double sigma) const
    {
      check(mgamd_dofs_set_mass_coefficient(h.get(), sigma));
    }
    double
    mass_coefficient() const
    {
      double s = 0.0;
      check(mgamd_dofs_mass_coefficient(h.get(), &s));
      return s;
    }
    // smallest and largest diffusion coefficient these DoFs were built with
    std::pair<double, double>
    coefficient_range() const
    {
      double lo = 1.0, hi = 1.0;
      check(mgamd_dofs_coefficient_range(h.get(), &lo, &hi));
      return {lo, hi};
    }
    // the dirichlet_faces mask these DoFs were built with
    unsigned
    dirichlet_faces() const
    {
      unsigned mask = 0;
      check(mgamd_dofs_dirichlet_faces(h.get(), &mask));
      return mask;
    }
    // the Robin coefficients these DoFs were built with
    std::array<double, 6>
    robin_coefficients() const
    {
      std::array<double, 6> beta{};
      check(mgamd_dofs_robin_coefficients(h.get(), beta.data()));
      return beta;
    }
    // Dirichlet data of one constant per face: v[f] on the Dirichlet DoFs of face f (the lowest-numbered Dirichlet face of a DoF on
    // several), 0 elsewhere; a host vector of n_dofs values for Vector::copy_from_host.  Refuses a non-zero value on a natural face.
    std::vector<double>
    dirichlet_face_values(const std::array<double, 6> &v) const
    {
      std::vector<double> g(info.n_dofs);
      check(mgamd_dofs_dirichlet_face_values(h.get(), v.data(), g.data()));
      return g;
    }
    // support points of the DoFs, xyz[3 i ..]: the nodal interpolant of a function is one loop over them
    std::vector<double>
    node_positions() const
    {
      std::vector<double> xyz(3 * (size_t)info.n_dofs);
      check(mgamd_dofs_node_positions(h.get(), xyz.data()));
      return xyz;
    }
    // The physical points of QGauss(n_q)^3 on every leaf (mgamd_dofs_quadrature_points; in deal.II: FEValues::get_quadrature_points):
    // xyz[3 (((cell n_q + qz) n_q + qy) n_q + qx) ..], the points at which Operator::integrate_difference expects caller data.
    // n_q: degree + 1 ... degree + 3; 0 stands for degree + 2.
    std::vector<double>
    quadrature_points(int n_q = 0) const
    {
      const int           nq    = n_q == 0 ? (int)info.degree + 2 : n_q;
      const bool          valid = nq >= (int)info.degree + 1 && nq <= (int)info.degree + 3;
      std::vector<double> xyz(valid ? 3 * (size_t)info.n_cells * nq * nq * nq : 1);
      check(mgamd_dofs_quadrature_points(h.get(), n_q, xyz.data())); // (refuses n_q by name before it writes)
      return xyz;
    }
    mgamd_dofs_info_t info;

  private:
    std::shared_ptr<const Triangulation> tria;
    std::shared_ptr<mgamd_dofs>          h;
  };

  class Context
  {
  public:
    explicit Context(int device = 0)
    {
      mgamd_ctx *c = nullptr;
      check(mgamd_ctx_create(device, &c));
      h.reset(c, mgamd_ctx_destroy);
    }
    void
    synchronize() const
    {
      check(mgamd_ctx_synchronize(h.get()));
    }
    mgamd_ctx *
    get() const
    {
      return h.get();
    }

  private:
    std::shared_ptr<mgamd_ctx> h;
  };

  // The communicator of a sharded run: RCCL over xGMI, one rank per GPU (what MPI_COMM_WORLD is to the reference,
  // ref:multigrid_throughput.cc:2403-2442).  Every rank calls rccl() with the same 128-byte id; exchange_id_through_file is the
  // host-side channel for launchers that only provide RANK / WORLD_SIZE (torchrun --no-python, a shell loop): rank 0 writes the
  // id, the others wait for the file.
  class Communicator
  {
  public:
    Communicator() = default;
    static std::array<char, 128>
    exchange_id_through_file(const std::string &path, unsigned rank, double timeout_s = 120.0)
    {
      std::array<char, 128> id{};
      if (rank == 0)
        {
          check(mgamd_comm_rccl_unique_id(id.data()));
          const std::string tmp = path + ".tmp";
          {
            std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
            f.write(id.data(), 128);
          }
          if (std::rename(tmp.c_str(), path.c_str()) != 0)
            throw std::runtime_error("cannot publish the RCCL id at " + path);
          return id;
        }
      const auto t0 = std::chrono::steady_clock::now();
      for (;;)
        {
          std::ifstream f(path, std::ios::binary);
          if (f && f.read(id.data(), 128) && f.gcount() == 128)
            return id;
          if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
            throw std::runtime_error("timed out waiting for the RCCL id at " + path);
          std::this_thread::sleep_for(std::chrono::milliseconds(20));
        }
    }
    static Communicator
    rccl(const Context &ctx, unsigned n_ranks, unsigned rank, const std::array<char, 128> &id)
    {
      Communicator c;
      mgamd_comm  *m = nullptr;
      check(mgamd_comm_rccl_create(ctx.get(), n_ranks, rank, id.data(), &m));
      c.h.reset(m, mgamd_comm_destroy);
      c.n = n_ranks;
      c.r = rank;
      return c;
    }
    // the communicator of the levels that are cut into n_ranks / group parts (Partition tiers): rank = part
    Communicator
    subset(unsigned group) const
    {
      if (group <= 1)
        return *this;
      Communicator c;
      mgamd_comm  *m = nullptr;
      check(mgamd_comm_subset(h.get(), group, &m));
      const std::shared_ptr<mgamd_comm> base = h; // (the C object keeps the base alive as well)
      c.h.reset(m, [base](mgamd_comm *x) { mgamd_comm_destroy(x); });
      c.n = n / group;
      c.r = r / group;
      return c;
    }
    double
    allreduce_sum(const Context &ctx, double v) const // Utilities::MPI::sum
    {
      double s = 0;
      check(mgamd_comm_allreduce_sum(h.get(), ctx.get(), v, &s));
      return s;
    }
    unsigned
    n_ranks() const
    {
      return n;
    }
    unsigned
    rank() const
    {
      return r;
    }
    mgamd_comm *
    get() const
    {
      return h.get();
    }

  private:
    std::shared_ptr<mgamd_comm> h;
    unsigned                    n = 1, r = 0;
  };

  class Vector
  {
  public:
    Vector() = default;
    explicit Vector(mgamd_vec *v)
    {
      h.reset(v, mgamd_vec_destroy);
    }
    Vector(const Context &ctx, uint64_t n, int number_type = MGAMD_F64)
    {
      mgamd_vec *v = nullptr;
      check(mgamd_vec_create(ctx.get(), n, number_type, &v));
      h.reset(v, mgamd_vec_destroy);
    }
    uint64_t
    size() const
    {
      uint64_t n = 0;
      check(mgamd_vec_size(h.get(), &n));
      return n;
    }
    Vector &
    operator=(double value)
    {
      check(mgamd_vec_set(h.get(), value));
      return *this;
    }
    void
    sadd(double s, double a, const Vector &x)
    {
      check(mgamd_vec_sadd(h.get(), s, a, x.get()));
    }
    void
    add(double a, const Vector &x)
    {
      check(mgamd_vec_axpy(h.get(), a, x.get()));
    }
    double
    operator*(const Vector &other) const
    {
      double r = 0;
      check(mgamd_vec_dot(h.get(), other.get(), &r));
      return r;
    }
    double
    l2_norm() const
    {
      double r = 0;
      check(mgamd_vec_norm2(h.get(), &r));
      return r;
    }
    void
    copy_from_host(const std::vector<double> &v)
    {
      check(mgamd_vec_from_host(h.get(), v.data()));
    }
    std::vector<double>
    copy_to_host() const
    {
      std::vector<double> v(size());
      check(mgamd_vec_to_host(h.get(), v.data()));
      return v;
    }
    mgamd_vec *
    get() const
    {
      return h.get();
    }

  private:
    std::shared_ptr<mgamd_vec> h;
  };

  // TrilinosWrappers::SparseMatrix as Type "AMG" uses it: Operator::get_system_matrix() (the reference's
  // get_trilinos_system_matrix / get_petsc_system_matrix, ref:include/operator.h:244-358) on the device, FP64, one rank
  class SparseMatrix
  {
  public:
    using VectorType = Vector;
    SparseMatrix() = default;
    SparseMatrix(const Context &ctx, const DoFHandler &dof_handler)
    {
      mgamd_matrix *a = nullptr;
      check(mgamd_matrix_create(ctx.get(), dof_handler.get(), &a));
      h.reset(a, mgamd_matrix_destroy);
    }
    uint64_t
    m() const
    {
      uint64_t n = 0;
      check(mgamd_matrix_info(h.get(), &n, nullptr, nullptr));
      return n;
    }
    uint64_t
    n_nonzero_elements() const
    {
      uint64_t n = 0;
      check(mgamd_matrix_info(h.get(), nullptr, &n, nullptr));
      return n;
    }
    // lanes per row of its products (64: one wavefront per row)
    int
    lanes_per_row() const
    {
      int l = 0;
      check(mgamd_matrix_info(h.get(), nullptr, nullptr, &l));
      return l;
    }
    void
    vmult(Vector &dst, const Vector &src) const
    {
      check(mgamd_matrix_vmult(h.get(), dst.get(), src.get()));
    }
    mgamd_matrix *
    get() const
    {
      return h.get();
    }

  private:
    std::shared_ptr<mgamd_matrix> h;
  };

  // Operator<dim=3, n_components=1, Number> (ref:include/operator.h:11)
  class Operator
  {
  public:
    using VectorType = Vector;
    // Operator::reinit(mapping, dof_handler, quad, constraints) (ref:include/operator.h:24-47): mapping is
    // MappingQ1 on cubes, the quadrature QGauss(degree+1), constraints zero Dirichlet + hanging nodes.
    void
    reinit(const Context &ctx, const DoFHandler &dof_handler, int number_type = MGAMD_F64)
    {
      mgamd_level_op *o = nullptr;
      check(mgamd_level_op_create(ctx.get(), dof_handler.get(), number_type, &o));
      h.reset(o, mgamd_level_op_destroy);
      context = std::make_shared<const Context>(ctx);
      dofs    = std::make_shared<const DoFHandler>(dof_handler);
    }
    // a level of a sharded hierarchy (DoFHandler(partition, level, rank, ...)): sums of shared DoFs are completed through `comm`
    // (nullptr: replicated level)
    void
    reinit(const Context &ctx, const DoFHandler &dof_handler, int number_type, const Communicator *comm)
    {
      mgamd_level_op *o = nullptr;
      check(mgamd_level_op_create_distributed(ctx.get(), dof_handler.get(), number_type, comm ? comm->get() : nullptr, &o));
      h.reset(o, mgamd_level_op_destroy);
      context = std::make_shared<const Context>(ctx);
      dofs    = std::make_shared<const DoFHandler>(dof_handler);
    }
    // Operator::get_trilinos_system_matrix / get_petsc_system_matrix (ref:include/operator.h:244-358): the assembled matrix of
    // this operator's DoFs, on the device (built at every call: keep the result); refuses distributed and local-smoothing levels
    SparseMatrix
    get_system_matrix() const
    {
      if (!dofs)
        throw std::runtime_error("Operator::get_system_matrix: reinit first");
      // the matrix is assembled from the handler's tables, which may have taken another mass coefficient since reinit
      if (dofs->mass_coefficient() != mass_coefficient())
        throw std::invalid_argument("Operator::get_system_matrix: the mass coefficient of the DoFHandler (" + std::to_string(dofs->mass_coefficient()) +
                                    ") was changed after this operator was built with " + std::to_string(mass_coefficient()) +
                                    "; the assembled matrix would be another operator's");
      return SparseMatrix(*context, *dofs);
    }
    // DoFs this rank owns (sums to DoFHandler::n_dofs() over the ranks)
    uint64_t
    n_owned() const
    {
      uint64_t n = 0;
      check(mgamd_level_op_n_owned(h.get(), &n));
      return n;
    }
    uint64_t
    m() const
    {
      uint64_t n = 0;
      check(mgamd_level_op_m(h.get(), &n));
      return n;
    }
    // the mass coefficient this operator was built with (DoFHandler::set_mass_coefficient before reinit)
    double
    mass_coefficient() const
    {
      double s = 0.0;
      check(mgamd_level_op_mass_coefficient(h.get(), &s));
      return s;
    }
    void
    initialize_dof_vector(Vector &vec) const
    {
      mgamd_vec *v = nullptr;
      check(mgamd_level_op_init_vector(h.get(), &v));
      vec = Vector(v);
    }
    void
    vmult(Vector &dst, const Vector &src) const
    {
      check(mgamd_level_op_vmult(h.get(), dst.get(), src.get()));
    }
    // dst = C^T M C src: the mass matrix of this operator's space, zero rows and columns on constrained DoFs (mgamd_level_op_vmult_mass)
    void
    vmult_mass(Vector &dst, const Vector &src) const
    {
      check(mgamd_level_op_vmult_mass(h.get(), dst.get(), src.get()));
    }
    void
    Tvmult(Vector &dst, const Vector &src) const
    {
      vmult(dst, src); // ref:include/operator.h:185-189
    }
    // ref:include/operator.h:191-201 and :203-226 (what MatrixFreeOperators::MGInterfaceOperator::vmult / Tvmult forward to)
    void
    vmult_interface_down(Vector &dst, const Vector &src) const
    {
      check(mgamd_level_op_vmult_interface_down(h.get(), dst.get(), src.get()));
    }
    void
    vmult_interface_up(Vector &dst, const Vector &src) const
    {
      check(mgamd_level_op_vmult_interface_up(h.get(), dst.get(), src.get()));
    }
    void
    compute_inverse_diagonal(Vector &diagonal) const
    {
      if (!diagonal.get())
        initialize_dof_vector(diagonal);
      check(mgamd_level_op_inverse_diagonal(h.get(), diagonal.get()));
    }
    // simulation_kind: 0 "Constant" (f = 1, g = 0), 1 "Gaussian" (ref:multigrid_throughput.cc:2286-2298)
    void
    rhs(Vector &system_rhs, int simulation_kind = 0) const
    {
      check(mgamd_level_op_rhs_kind(h.get(), simulation_kind, system_rhs.get()));
    }
    // boundary load of one constant flux q[f] per natural face f (mgamd_level_op_rhs_boundary_flux); add it to rhs()
    void
    rhs_boundary_flux(Vector &load, const std::array<double, 6> &q) const
    {
      check(mgamd_level_op_rhs_boundary_flux(h.get(), q.data(), load.get()));
    }
    // constraints.distribute(solution)
    void
    distribute(Vector &solution, int simulation_kind = 0) const
    {
      check(mgamd_level_op_distribute(h.get(), simulation_kind, solution.get()));
    }
    // Non-zero Dirichlet data g (a vector of n_dofs values, only its entries at Dirichlet DoFs are read): load = the lifting
    // -[C^T (K_a + sigma M) C g^] on the free rows, by the device kernel over the cells that gather a Dirichlet DoF
    // (mgamd_level_op_rhs_dirichlet); overwrites load, which is additive to rhs(), rhs_boundary_flux() and M f
    void
    rhs_dirichlet(Vector &load, const Vector &g, bool include_mass = true) const
    {
      check(mgamd_level_op_rhs_dirichlet(h.get(), g.get(), include_mass ? 1 : 0, load.get()));
    }
    // solution: Dirichlet DoFs from g, then hanging DoFs from their parents, on the device (mgamd_level_op_distribute_values)
    void
    distribute_values(Vector &solution, const Vector &g) const
    {
      check(mgamd_level_op_distribute_values(h.get(), solution.get(), g.get()));
    }
    // The jump error indicator eta_K of u per leaf, in the order of mgamd_tria_get_cells (mgamd_level_op_estimate_error; in
    // deal.II: KellyErrorEstimator): eta_K^2 = h_K / 24 sum over the faces of the integral of the squared jump of the normal flux
    // a d_n u.  q: the six boundary fluxes of rhs_boundary_flux for the residual q - beta u - a d_n u on natural and convective
    // faces, nullptr for no boundary term.  Only entries of u at free and Dirichlet DoFs are read.
    std::vector<double>
    estimate_error(const Vector &u, const std::array<double, 6> *q = nullptr) const
    {
      if (!dofs)
        throw std::runtime_error("Operator::estimate_error: reinit first");
      std::vector<double> eta(dofs->get_triangulation().n_global_active_cells());
      check(mgamd_level_op_estimate_error(h.get(), u.get(), q ? q->data() : nullptr, eta.data()));
      return eta;
    }
    // The error norms of u_h - w per leaf, in the order of mgamd_tria_get_cells (mgamd_level_op_integrate_difference; in deal.II:
    // VectorTools::integrate_difference).  norm: MGAMD_NORM_L2, _H1_SEMINORM, _ENERGY (a |grad e|^2 + sigma e^2, volume terms only) or
    // _LINFTY; n_q Gauss points per direction, 0 for degree + 2.  kind: the built-in w (0: zero, 1: the Gaussian).  Only entries of u
    // at free and Dirichlet DoFs are read.  compute_global_error gives the global value.
    std::vector<double>
    integrate_difference(const Vector &u, int kind, int norm, int n_q = 0) const
    {
      if (!dofs)
        throw std::runtime_error("Operator::integrate_difference: reinit first");
      std::vector<double> out(dofs->get_triangulation().n_global_active_cells());
      check(mgamd_level_op_integrate_difference(h.get(), u.get(), kind, n_q, norm, out.data()));
      return out;
    }
    // the same with caller data at DoFHandler::quadrature_points(n_q): values [cell][qz][qy][qx]
    std::vector<double>
    integrate_difference(const Vector &u, const Vector &values, int norm, int n_q = 0) const
    {
      if (!dofs)
        throw std::runtime_error("Operator::integrate_difference: reinit first");
      std::vector<double> out(dofs->get_triangulation().n_global_active_cells());
      check(mgamd_level_op_integrate_difference_values(h.get(), u.get(), values.get(), nullptr, n_q, norm, out.data()));
      return out;
    }
    // ... and gradients [cell][component][qz][qy][qx] for the two gradient norms (values may be an empty Vector for the H1 seminorm)
    std::vector<double>
    integrate_difference(const Vector &u, const Vector &values, const Vector &gradients, int norm, int n_q = 0) const
    {
      if (!dofs)
        throw std::runtime_error("Operator::integrate_difference: reinit first");
      std::vector<double> out(dofs->get_triangulation().n_global_active_cells());
      check(mgamd_level_op_integrate_difference_values(h.get(), u.get(), values.get(), gradients.get(), n_q, norm, out.data()));
      return out;
    }
    // u_h and grad u_h at DoFHandler::quadrature_points(n_q) on the device (mgamd_level_op_evaluate; in deal.II:
    // FEEvaluation::evaluate over a cell loop): values [cell][qz][qy][qx], n_cells n_q^3 entries, and gradients
    // [cell][component][qz][qy][qx], three times as many, in the operator's number type.  An empty Vector is an output not asked for.
    // Only entries of u at free and Dirichlet DoFs are read.  Stream-ordered, nothing is copied to the host.
    void
    evaluate(const Vector &u, Vector &values, Vector &gradients, int n_q = 0) const
    {
      check(mgamd_level_op_evaluate(h.get(), u.get(), n_q, values.get(), gradients.get()));
    }
    // load_i = sum_K sum_q w_q h_K^3 (values_q phi_i + gradients_q . grad phi_i) through C^T (mgamd_level_op_integrate; in deal.II:
    // FEEvaluation::integrate + distribute_local_to_global, VectorTools::create_right_hand_side): the load of a source f (values =
    // f at the points), the divergence-form load (gradients = F) or both.  An empty Vector is an input not given.  load is
    // overwritten, constrained rows are 0; no coefficient and no sigma are applied.  Additive to rhs_dirichlet() and
    // rhs_boundary_flux().  Stream-ordered, nothing is copied to the host; not bit-reproducible across calls (atomic adds).
    void
    integrate(Vector &load, const Vector &values, const Vector &gradients, int n_q = 0) const
    {
      check(mgamd_level_op_integrate(h.get(), values.get(), gradients.get(), n_q, load.get()));
    }
    mgamd_level_op *
    get() const
    {
      return h.get();
    }

  private:
    std::shared_ptr<mgamd_level_op>   h;
    std::shared_ptr<const Context>    context;
    std::shared_ptr<const DoFHandler> dofs;
  };

  // Utilities::MPI::RemotePointEvaluation with VectorTools::point_values / point_gradients and, for the transpose,
  // VectorTools::create_point_source_vector: caller points of [-1, 1]^3 located once on the leaves of one Operator (on the device,
  // mgamd_level_op_point_set_create), then used for many vectors.  A point on an interior face, edge or vertex belongs to the leaf on
  // its upper side (values do not depend on this, gradients are the one-sided gradients of that leaf); a point outside the cube is
  // NOT found, gets exactly 0 from point_values / point_gradients and adds nothing in point_source, silently: check
  // all_points_found().  The object keeps its Operator alive.
  class PointEvaluation
  {
  public:
    // the outputs are created in the operator's number type
    PointEvaluation(const Context &ctx, const Operator &op)
      : context(ctx)
      , op(op)
    {
      check(mgamd_level_op_number_type(op.get(), &number_type));
    }
    // points: xyz[3k...], always double
    void
    reinit(const std::vector<double> &points)
    {
      mgamd_point_set *p = nullptr;
      check(mgamd_level_op_point_set_create(op.get(), points.size() / 3, points.data(), &p));
      h.reset(p, mgamd_point_set_destroy);
      uint64_t n = 0;
      check(mgamd_point_set_get(p, &n, nullptr, nullptr, nullptr));
      cells.assign(n, -1);
      check(mgamd_point_set_get(p, nullptr, nullptr, cells.data(), nullptr));
    }
    uint64_t
    n_points() const
    {
      return cells.size();
    }
    bool
    all_points_found() const
    {
      for (int32_t c : cells)
        if (c < 0)
          return false;
      return true;
    }
    bool
    point_found(uint64_t k) const
    {
      return cells.at(k) >= 0;
    }
    // the leaf of point k in the order of the mesh's cells, -1 where the point was not found
    int32_t
    cell(uint64_t k) const
    {
      return cells.at(k);
    }
    // u_h(x_k), n entries in the caller's point order, on the device in the operator's number type (mgamd_point_set_evaluate)
    Vector
    point_values(const Vector &u) const
    {
      Vector values(context, n_points(), number_type);
      check(mgamd_point_set_evaluate(h.get(), op.get(), u.get(), values.get(), nullptr));
      return values;
    }
    // grad u_h(x_k), 3 n entries [component][point]
    Vector
    point_gradients(const Vector &u) const
    {
      Vector gradients(context, 3 * n_points(), number_type);
      check(mgamd_point_set_evaluate(h.get(), op.get(), u.get(), nullptr, gradients.get()));
      return gradients;
    }
    // b_i = sum_k w_k phi_i(x_k) through C^T: the load of the Dirac sources w_k delta(x - x_k) (mgamd_point_set_integrate;
    // VectorTools::create_point_source_vector).  b is overwritten, constrained rows are 0.  With `dipoles` (3 n entries
    // [component][point]) the terms W_k . grad phi_i(x_k) are added; an empty Vector is an input not given.
    void
    point_source(const Vector &w, Vector &b, const Vector &dipoles = Vector()) const
    {
      check(mgamd_point_set_integrate(h.get(), op.get(), w.get(), dipoles.get(), b.get()));
    }
    mgamd_point_set *
    get() const
    {
      return h.get();
    }

  private:
    Context                          context;
    Operator                         op;
    int                              number_type = MGAMD_F64;
    std::shared_ptr<mgamd_point_set> h;
    std::vector<int32_t>             cells;
  };

  class PreconditionChebyshev
  {
  public:
    struct AdditionalData
    {
      double   smoothing_range     = 20.;
      unsigned degree              = 5;
      unsigned eig_cg_n_iterations = 20;
    };
    void
    initialize(const Operator &matrix, const AdditionalData &data)
    {
      mgamd_cheb *c = nullptr;
      check(mgamd_cheb_create(matrix.get(), data.degree, data.smoothing_range, data.eig_cg_n_iterations, &c));
      h.reset(c, mgamd_cheb_destroy);
    }
    void
    vmult(Vector &dst, const Vector &src) const
    {
      check(mgamd_cheb_vmult(h.get(), dst.get(), src.get()));
    }
    void
    step(Vector &dst, const Vector &src) const
    {
      check(mgamd_cheb_step(h.get(), dst.get(), src.get()));
    }
    mgamd_cheb *
    get() const
    {
      return h.get();
    }

  private:
    std::shared_ptr<mgamd_cheb> h;
  };

  class MGTwoLevelTransfer
  {
  public:
    // reinit(dof_fine, dof_coarse, constraint_fine, constraint_coarse): the level operators carry all four
    void
    reinit(const Operator &fine, const Operator &coarse)
    {
      mgamd_transfer2 *t = nullptr;
      check(mgamd_transfer2_create(fine.get(), coarse.get(), &t));
      h.reset(t, mgamd_transfer2_destroy);
    }
    void
    prolongate_and_add(Vector &dst, const Vector &src) const
    {
      check(mgamd_transfer2_prolongate_and_add(h.get(), dst.get(), src.get()));
    }
    void
    restrict_and_add(Vector &dst, const Vector &src) const
    {
      check(mgamd_transfer2_restrict_and_add(h.get(), dst.get(), src.get()));
    }
    mgamd_transfer2 *
    get() const
    {
      return h.get();
    }

  private:
    std::shared_ptr<mgamd_transfer2> h;
  };

  // The levels of one multigrid hierarchy, coarse -> fine: what solve_with_global_coarsening / solve_with_local_smoothing build level
  // by level (DoFHandler + constraints, Operator, MGTwoLevelTransfer, PreconditionChebyshev; ref:multigrid_throughput.cc:1540-1621),
  // from the (mesh index, degree) list of level_plan()
  class LevelStack
  {
  public:
    // a sharded run: the levels are this rank's share of the partition's meshes; `comm` spans all ranks, `sub_comm` the parts of the
    // subset tier (Communicator::subset(partition->group()))
    struct Sharding
    {
      const Partition    *partition;
      const Communicator *comm, *sub_comm;
      const Communicator *
      mesh_comm(unsigned mesh) const // of a distributed mesh; nullptr: the mesh is replicated
      {
        if (comm->n_ranks() <= 1 || mesh < partition->sub_root_level())
          return nullptr;
        return mesh >= partition->root_level() ? comm : sub_comm;
      }
    };
    // a level that exists already: its DoFs (HPMG-local: level 0 acts on the DoFs of the local-smoothing cycle underneath) and, if the
    // whole level is another stack's, its operator and smoother too (the coarse stand-in ends on the level it stands in for)
    struct Given
    {
      unsigned                     level;
      const DoFHandler            *dofs;
      const Operator              *op       = nullptr;
      const PreconditionChebyshev *smoother = nullptr;
    };
    LevelStack() = default;
    // meshes: coarsest first (with `sharding`: the partition's); local_smoothing: they are Triangulation::level_mesh(l)
    LevelStack(const Context &ctx, const std::vector<std::shared_ptr<const Triangulation>> &meshes,
               const std::vector<std::pair<unsigned, unsigned>> &levels, int number_type, const PreconditionChebyshev::AdditionalData &smoother_data,
               const Sharding *sharding = nullptr, bool local_smoothing = false, const Given *given = nullptr, double mass_coefficient = 0.0)
      : operators(levels.size())
      , transfers(levels.size())
      , smoothers(levels.size())
      , comms(levels.size(), nullptr)
    {
      const unsigned n = levels.size();
      for (unsigned l = 0; l < n; ++l)
        if (given && given->level == l)
          dof_handlers.push_back(*given->dofs);
        else if (sharding)
          dof_handlers.emplace_back(*sharding->partition, levels[l].first, sharding->comm->rank(), levels[l].second);
        else
          dof_handlers.emplace_back(meshes[levels[l].first], levels[l].second, -1, local_smoothing);
      // the mass term of K + sigma M, on every level's handler before its operator is built (local-smoothing levels refuse sigma != 0)
      for (unsigned l = 0; l < n; ++l)
        if (!(given && given->level == l && given->op))
          dof_handlers[l].set_mass_coefficient(mass_coefficient);
      for (unsigned l = 0; l < n; ++l)
        {
          comms[l] = sharding ? sharding->mesh_comm(levels[l].first) : nullptr;
          if (given && given->level == l && given->op)
            operators[l] = *given->op;
          else if (sharding)
            operators[l].reinit(ctx, dof_handlers[l], number_type, comms[l]);
          else
            operators[l].reinit(ctx, dof_handlers[l], number_type);
        }
      for (unsigned l = 1; l < n; ++l)
        transfers[l].reinit(operators[l], operators[l - 1]);
      for (unsigned l = 0; l < n; ++l)
        if (given && given->level == l && given->smoother)
          smoothers[l] = *given->smoother;
        else
          smoothers[l].initialize(operators[l], smoother_data);
    }
    // DoFHandler::n_dofs() of the GLOBAL level: the owned DoFs summed over the pieces of a distributed level
    uint64_t
    n_dofs_global(const Context &ctx, unsigned l) const
    {
      return comms[l] ? (uint64_t)std::llround(comms[l]->allreduce_sum(ctx, (double)operators[l].n_owned())) : dof_handlers[l].n_dofs();
    }
    std::vector<DoFHandler>            dof_handlers;
    std::vector<Operator>              operators;
    std::vector<MGTwoLevelTransfer>    transfers; // transfers[l]: levels l - 1 and l; transfers[0] unused
    std::vector<PreconditionChebyshev> smoothers;
    std::vector<const Communicator *>  comms; // per level; nullptr: replicated (or one rank)
  };

  // Multigrid<VectorType> + PreconditionMG<dim,VectorType,MGTransferGlobalCoarsening> in one object
  class PreconditionMG
  {
  public:
    using StageSlot = std::function<void(bool /*start*/, unsigned /*level*/)>;
    // active_mesh_dofs: local smoothing (solve_with_local_smoothing, ref:multigrid_throughput.cc:1670-1873): mg_matrices are the
    // operators on the refinement levels (DoFHandler with mg_level = true), vmult acts on vectors of the active mesh.
    // coarse_mg: the geometric stand-in for the AMG coarse solvers on a large coarse level (an h-multigrid whose finest level
    // is mg_matrices[0]), applied n_cycles times per coarse solve
    PreconditionMG(const Context &ctx, const std::vector<Operator> &mg_matrices, const std::vector<MGTwoLevelTransfer> &transfers,
                   const std::vector<PreconditionChebyshev> &smoothers, const std::string &coarse_grid_solver_type,
                   const PreconditionMG *coarse_mg = nullptr, unsigned n_cycles = 1, const DoFHandler *active_mesh_dofs = nullptr)
    {
      const unsigned n = mg_matrices.size();
      const auto     L = handles<mgamd_level_op>(mg_matrices, n);
      const auto     T = handles<mgamd_transfer2>(transfers, n, 1);
      const auto     S = handles<mgamd_cheb>(smoothers, n);
      mgamd_mg      *m = nullptr;
      if (active_mesh_dofs)
        check(mgamd_mg_create_local_smoothing(ctx.get(), n, L.data(), T.data(), S.data(), active_mesh_dofs->get(),
                                              coarse_grid_solver_type.c_str(), &m));
      else // (n_cycles = CoarseSolverNCycles, also of the algebraic coarse solvers "amg" / "cg_with_amg")
        check(mgamd_mg_create_nested(ctx.get(), n, L.data(), T.data(), S.data(), coarse_grid_solver_type.c_str(),
                                     coarse_mg ? coarse_mg->get() : nullptr, n_cycles, &m));
      if (coarse_mg)
        nested = coarse_mg->h; // keep the nested hierarchy's handle alive
      adopt(m, n);
    }
    // The AMG coarse solvers ("amg", "cg_with_amg", "amg_petsc") on a SHARDED mg_matrices[0] (mgamd_mg_create_sharded_amg): replicated
    // setup from `global_coarse_dofs` (the DoFHandler of level 0's space on the whole mesh, built as a one-rank hierarchy builds
    // it), sharded cycle; levels of at most min_sharded_rows rows replicated.  Not the default: without it a sharded coarse level
    // takes the geometric stand-in (coarse_mg above).
    struct ShardedAMG
    {
      const DoFHandler *global_coarse_dofs;
      uint32_t          min_sharded_rows = MGAMD_AMG_MIN_SHARDED_ROWS_DEFAULT;
    };
    PreconditionMG(const Context &ctx, const std::vector<Operator> &mg_matrices, const std::vector<MGTwoLevelTransfer> &transfers,
                   const std::vector<PreconditionChebyshev> &smoothers, const std::string &coarse_grid_solver_type, const ShardedAMG &amg,
                   unsigned n_cycles = 1)
    {
      if (!amg.global_coarse_dofs)
        throw std::invalid_argument("PreconditionMG: ShardedAMG needs the global DoFs of level 0's space");
      const unsigned n = mg_matrices.size();
      const auto     L = handles<mgamd_level_op>(mg_matrices, n);
      const auto     T = handles<mgamd_transfer2>(transfers, n, 1);
      const auto     S = handles<mgamd_cheb>(smoothers, n);
      mgamd_mg      *m = nullptr;
      check(mgamd_mg_create_sharded_amg(ctx.get(), n, L.data(), T.data(), S.data(), coarse_grid_solver_type.c_str(),
                                        amg.global_coarse_dofs->get(), n_cycles, amg.min_sharded_rows, &m));
      adopt(m, n);
    }
    // the levels of the algebraic coarse solver that runs, finest first (mgamd_mg_amg_layout); empty: no AMG runs
    struct AmgLevelLayout
    {
      uint32_t global_rows, owned_rows, ghosts, peers;
      bool     replicated;
    };
    std::vector<AmgLevelLayout>
    amg_layout() const
    {
      uint32_t n = 0, info[5 * 32];
      check(mgamd_mg_amg_layout(h.get(), &n, info, 32));
      std::vector<AmgLevelLayout> out;
      for (uint32_t l = 0; l < n && l < 32; ++l)
        out.push_back({info[5 * l], info[5 * l + 1], info[5 * l + 2], info[5 * l + 3], info[5 * l + 4] != 0});
      return out;
    }
    // the coarse solver that actually runs: "direct" | "cg" | "cg_with_chebyshev" | "amg" | "cg_with_amg" | "gmg_vcycle" (mgamd.h)
    std::string
    coarse_solver_used() const
    {
      char name[32];
      check(mgamd_mg_coarse_solver_used(h.get(), name));
      return name;
    }
    // stage times of the UNCHANGED cycle from HIP events (no host synchronisation inside the cycle): enable, run solves,
    // then read_stage_times() adds seconds to t[stage][level] (stages as in the connect_* slots, 7/8 = transfer to mg/global)
    void
    enable_stage_timing(bool on) const
    {
      check(mgamd_mg_stage_timing(h.get(), on ? 1 : 0));
    }
    void
    read_stage_times(std::vector<std::vector<double>> &t) const
    {
      std::vector<double> ms(9 * (size_t)n_levels, 0.0);
      uint64_t            n = 0;
      check(mgamd_mg_stage_times(h.get(), ms.data(), n_levels, &n));
      t.assign(9, std::vector<double>(n_levels, 0.0));
      for (unsigned st = 0; st < 9; ++st)
        for (unsigned l = 0; l < n_levels; ++l)
          t[st][l] = ms[st * (size_t)n_levels + l] * 1e-3;
    }
    void
    vmult(Vector &dst, const Vector &src) const
    {
      check(mgamd_mg_vcycle(h.get(), dst.get(), src.get()));
    }
    // Multigrid::connect_* / PreconditionMG::connect_transfer_to_* (ref:multigrid_throughput.cc:1183-1192,1233-1234)
    void
    connect_pre_smoother_step(StageSlot s)
    {
      connect(0, std::move(s));
    }
    void
    connect_residual_step(StageSlot s)
    {
      connect(1, std::move(s));
    }
    void
    connect_restriction(StageSlot s)
    {
      connect(2, std::move(s));
    }
    void
    connect_coarse_solve(StageSlot s)
    {
      connect(3, std::move(s));
    }
    void
    connect_prolongation(StageSlot s)
    {
      connect(4, std::move(s));
    }
    void
    connect_edge_prolongation(StageSlot s)
    {
      connect(5, std::move(s));
    }
    void
    connect_post_smoother_step(StageSlot s)
    {
      connect(6, std::move(s));
    }
    void
    connect_transfer_to_mg(std::function<void(bool)> s)
    {
      connect(7, [s](bool f, unsigned) { s(f); });
    }
    void
    connect_transfer_to_global(std::function<void(bool)> s)
    {
      connect(8, [s](bool f, unsigned) { s(f); });
    }
    void
    disconnect_all()
    {
      for (auto &s : slots)
        s = nullptr;
      check(mgamd_mg_set_stage_callback(h.get(), nullptr, nullptr));
    }
    mgamd_mg *
    get() const
    {
      return h.get();
    }

  private:
    // a handle array of the C entry points: n entries, those below `from` null (transfers[0] is unused)
    template <typename Handle, typename Object>
    static std::vector<Handle *>
    handles(const std::vector<Object> &objects, unsigned n, unsigned from = 0)
    {
      std::vector<Handle *> out(n, nullptr);
      for (unsigned l = from; l < n; ++l)
        out[l] = objects[l].get();
      return out;
    }
    void
    adopt(mgamd_mg *m, unsigned n)
    {
      h.reset(m, mgamd_mg_destroy);
      slots.resize(9);
      n_levels = n;
    }
    void
    connect(int stage, StageSlot s)
    {
      slots[stage] = std::move(s);
      check(mgamd_mg_set_stage_callback(h.get(), &PreconditionMG::trampoline, this));
    }
    static void
    trampoline(int stage, int start, unsigned level, void *user)
    {
      auto *self = static_cast<PreconditionMG *>(user);
      if (stage >= 0 && stage < (int)self->slots.size() && self->slots[stage])
        self->slots[stage](start != 0, level);
    }
    std::shared_ptr<mgamd_mg> h, nested;
    std::vector<StageSlot>    slots;
    unsigned                  n_levels = 0;
  };

  class ReductionControl
  {
  public:
    ReductionControl(unsigned maxiter = 10000, double abstol = 1e-20, double reltol = 1e-4)
      : maxiter(maxiter)
      , abstol(abstol)
      , reltol(reltol)
    {}
    unsigned
    last_step() const
    {
      return steps;
    }
    double
    last_value() const
    {
      return value;
    }
    unsigned maxiter;
    double   abstol, reltol;
    unsigned steps = 0;
    double   value = 0;
  };

  // TrilinosWrappers::PreconditionAMG (ref:multigrid_throughput.cc:1907-1909): the library's smoothed-aggregation AMG on the matrix
  class PreconditionAMG
  {
  public:
    struct AdditionalData
    {
      unsigned n_cycles = 1;
    };
    void
    initialize(const SparseMatrix &matrix, const AdditionalData &data)
    {
      mgamd_amg *p = nullptr;
      check(mgamd_amg_create(matrix.get(), data.n_cycles, &p));
      h.reset(p, mgamd_amg_destroy);
    }
    void
    initialize(const SparseMatrix &matrix)
    {
      initialize(matrix, AdditionalData());
    }
    void
    vmult(Vector &dst, const Vector &src) const
    {
      check(mgamd_amg_vmult(h.get(), dst.get(), src.get()));
    }
    // rows of every AMG level, finest first
    std::vector<uint32_t>
    layout() const
    {
      uint32_t n = 0, rows[32];
      check(mgamd_amg_layout(h.get(), &n, rows, 32));
      return std::vector<uint32_t>(rows, rows + std::min<uint32_t>(n, 32));
    }
    mgamd_amg *
    get() const
    {
      return h.get();
    }

  private:
    std::shared_ptr<mgamd_amg> h;
  };

  class SolverCG
  {
  public:
    explicit SolverCG(ReductionControl &control)
      : control(control)
    {}
    // solve(A, x, b, preconditioner) starting from x = 0; non-convergence is reported through last_step()
    // == maxiter like the reference, which swallows SolverControl::NoConvergence (ref:multigrid_throughput.cc:1146,1250)
    void
    solve(const Operator &A, Vector &x, const Vector &b, const PreconditionMG &preconditioner)
    {
      check(mgamd_solve_cg(A.get(), preconditioner.get(), x.get(), b.get(), control.reltol, control.abstol, control.maxiter,
                           &control.steps, &control.value));
    }
    // CG on the assembled matrix with the AMG built on it (ref:multigrid_throughput.cc:1911-1915)
    void
    solve(const SparseMatrix &A, Vector &x, const Vector &b, const PreconditionAMG &preconditioner)
    {
      check(mgamd_solve_cg_matrix(A.get(), preconditioner.get(), x.get(), b.get(), control.reltol, control.abstol, control.maxiter,
                                  &control.steps, &control.value));
    }

  private:
    ReductionControl &control;
  };

  // theta-scheme for the heat equation M u' + K u = M f with constant step dt (mgamd_time_stepper): A is the operator K + sigma M
  // with sigma = mass_coefficient(theta, dt) on every level of its hierarchy (LevelStack's mass_coefficient), mg its multigrid.
  // Both must outlive the stepper.
  class ThetaTimeStepper
  {
  public:
    ThetaTimeStepper(const Operator &A, const PreconditionMG &mg, double theta, double dt)
    {
      mgamd_time_stepper *t = nullptr;
      check(mgamd_time_stepper_create(A.get(), mg.get(), theta, dt, &t));
      h.reset(t, mgamd_time_stepper_destroy);
    }
    // sigma = 1 / (theta dt)
    static double
    mass_coefficient(double theta, double dt)
    {
      return 1.0 / (theta * dt);
    }
    // one step without a source, u in place; returns the CG iterations of the increment
    unsigned
    step(Vector &u, double reltol, double abstol = 1e-20, unsigned maxiter = 10000)
    {
      unsigned it = 0;
      check(mgamd_time_stepper_step(h.get(), u.get(), nullptr, nullptr, reltol, abstol, maxiter, &it, &residual));
      return it;
    }
    // one step with the nodal source values at t (f_old) and t + dt (f_new)
    unsigned
    step(Vector &u, const Vector &f_old, const Vector &f_new, double reltol, double abstol = 1e-20, unsigned maxiter = 10000)
    {
      unsigned it = 0;
      check(mgamd_time_stepper_step(h.get(), u.get(), f_old.get(), f_new.get(), reltol, abstol, maxiter, &it, &residual));
      return it;
    }
    // one step with Dirichlet values g_old at t and g_new at t + dt, no source; load (may be null): a boundary load
    // theta l_new + (1 - theta) l_old (mgamd_time_stepper_step_data).  Operator::distribute_values(u, g_new) fills u for output.
    unsigned
    step(Vector &u, const Vector &g_old, const Vector &g_new, const Vector *load, double reltol, double abstol = 1e-20, unsigned maxiter = 10000)
    {
      unsigned it = 0;
      check(mgamd_time_stepper_step_data(h.get(), u.get(), nullptr, nullptr, g_old.get(), g_new.get(), load ? load->get() : nullptr, reltol,
                                         abstol, maxiter, &it, &residual));
      return it;
    }
    // the same with the nodal source values at t and t + dt
    unsigned
    step(Vector &u, const Vector &f_old, const Vector &f_new, const Vector &g_old, const Vector &g_new, const Vector *load, double reltol,
         double abstol = 1e-20, unsigned maxiter = 10000)
    {
      unsigned it = 0;
      check(mgamd_time_stepper_step_data(h.get(), u.get(), f_old.get(), f_new.get(), g_old.get(), g_new.get(), load ? load->get() : nullptr,
                                         reltol, abstol, maxiter, &it, &residual));
      return it;
    }
    double
    time() const
    {
      double t = 0;
      check(mgamd_time_stepper_time(h.get(), &t, nullptr));
      return t;
    }
    uint64_t
    n_steps() const
    {
      uint64_t n = 0;
      check(mgamd_time_stepper_time(h.get(), nullptr, &n));
      return n;
    }
    // residual norm of the last step's CG
    double
    last_residual() const
    {
      return residual;
    }

  private:
    std::shared_ptr<mgamd_time_stepper> h;
    double                              residual = 0;
  };
} // namespace mgamd
