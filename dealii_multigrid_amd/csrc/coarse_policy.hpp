// Which coarse solver a multigrid runs: names and their resolution, host only (no HIP), shared by the C ABI's host half
// (mgamd_coarse_plan, mgamd_debug_coarse_resolve) and the device runtime (CoarseSolver, runtime.hip).
#pragma once
#include "../../include/mgamd.h"

#include <cstdint>
#include <stdexcept>
#include <string>

namespace mgamd
{
  enum class CoarseKind { Direct, Cg, CgChebyshev, CgAmg, Amg, Nested };

  // the name a multigrid reports as coarse_solver_used() (harness table column / bench JSON)
  inline const char *
  coarse_kind_name(CoarseKind k)
  {
    static const char *const names[] = {"direct", "cg", "cg_with_chebyshev", "cg_with_amg", "amg", "gmg_vcycle"};
    return names[(int)k];
  }

  // the reference's Trilinos/PETSc choices (amg_petsc: BoomerAMG's role, the same smoothed-aggregation hierarchy as "amg")
  inline bool
  is_amg_name(const std::string &name)
  {
    return name == "amg" || name == "cg_with_amg" || name == "amg_petsc";
  }

  // ONE policy for what runs under a CoarseGridSolverType `name` on a level 0 of n_level0_dofs DoFs:
  //   the AMG names on a level of <= MGAMD_DIRECT_COARSE_MAX_DOFS DoFs (global coarsening ends on one cell): any AMG degenerates
  //     to an exact solve -> Direct;
  //   on a larger level (PMG, HPMG with MinLevel): the library's own smoothed-aggregation AMG on the assembled level matrix
  //     (amg.hpp, AmgCycle) -> Amg / CgAmg, built from ONE rank's matrix: an error on a sharded level without one of the two below;
  //   has_nested (a geometric multigrid on level 0's space, supplied by the caller) takes the AMG's place -> Nested, still the
  //     DEFAULT on a SHARDED coarse level;
  //   has_amg_global (the global tables of level 0's space, supplied by the caller) asks for the algebraic multigrid on a sharded
  //     level 0: replicated setup, sharded cycle -> Amg / CgAmg;
  //   "gmg_vcycle" without a nested multigrid: a small level is solved exactly, a large one is an error.
  // Whether a caller builds the nested multigrid or the global tables is mgamd_coarse_plan's decision (c_api_host.cpp).
  // Never a silent substitution: coarse_kind_name() of the result names what runs.
  inline CoarseKind
  resolve_coarse_kind(const std::string &name, uint64_t n_level0_dofs, bool level0_sharded, bool has_nested, bool has_amg_global)
  {
    const bool       amg_like = is_amg_name(name);
    const CoarseKind amg_kind = name == "cg_with_amg" ? CoarseKind::CgAmg : CoarseKind::Amg;
    if (has_amg_global && (has_nested || !amg_like))
      throw std::invalid_argument("multigrid: the sharded algebraic multigrid takes the place of the AMG coarse solvers (amg, "
                                  "cg_with_amg, amg_petsc) and excludes a nested multigrid");
    if (has_amg_global)
      return amg_kind;
    if (has_nested && !amg_like && name != "gmg_vcycle")
      throw std::invalid_argument("multigrid: a nested multigrid is the stand-in for the AMG coarse solvers only");
    if (has_nested)
      return CoarseKind::Nested;
    if (amg_like || name == "gmg_vcycle")
      {
        if (n_level0_dofs <= MGAMD_DIRECT_COARSE_MAX_DOFS)
          return CoarseKind::Direct;
        if (!amg_like)
          throw std::invalid_argument("multigrid: CoarseGridSolverType 'gmg_vcycle' on a level of more than " +
                                      std::to_string(MGAMD_DIRECT_COARSE_MAX_DOFS) + " DoFs needs a nested multigrid");
        if (level0_sharded)
          throw std::runtime_error("CoarseGridSolverType '" + name + "' on a sharded coarse level: the algebraic multigrid is built "
                                   "from one rank's assembled matrix; use the nested geometric multigrid (gmg_vcycle), cg or "
                                   "cg_with_chebyshev");
        return amg_kind;
      }
    for (const CoarseKind k : {CoarseKind::Direct, CoarseKind::Cg, CoarseKind::CgChebyshev})
      if (name == coarse_kind_name(k))
        return k;
    throw std::invalid_argument("CoarseGridSolverType '" + name + "' not implemented");
  }
} // namespace mgamd
