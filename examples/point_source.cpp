// A point heat source: -Laplace u = delta(x - x0) on the cube [-1, 1]^3, all six faces Dirichlet, with x0 = (0.13, -0.21, 0.07) off
// every node of every mesh.  The load is the point functional b_i = phi_i(x0), built on the device by PointEvaluation::point_source
// (in deal.II: VectorTools::create_point_source_vector); the Dirichlet data is the free-space solution g = 1 / (4 pi |x - x0|) at
// DoFHandler::node_positions, lifted by Operator::rhs_dirichlet, so the exact solution is g itself.  CG with the V-cycle (reltol
// 1e-12), then Operator::distribute_values.  Per mesh (hypercube, NRefGlobal 2, 3, ...) it prints the cells, the DoFs, the CG
// iterations and, at three fixed probe points away from x0 that are no nodes either, u_h and |u_h - g| read on the device with
// PointEvaluation::point_values (in deal.II: VectorTools::point_values).  The solution is singular at x0 (not in H^1), so no rate is
// claimed: the numbers are a record.  The example of INTEGRATION.md section 2f.
//   point_source [degree = 2] [refinements = 3]
#include "../dealii_multigrid_amd/csrc/mgamd.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace mgamd;

static const double source[3] = {0.13, -0.21, 0.07};

static double
exact(double x, double y, double z)
{
  const double pi = 3.14159265358979323846;
  const double dx = x - source[0], dy = y - source[1], dz = z - source[2];
  return 1.0 / (4.0 * pi * std::sqrt(dx * dx + dy * dy + dz * dz));
}

int
main(int argc, char **argv)
{
  try
    {
      const unsigned degree = argc > 1 ? (unsigned)std::atoi(argv[1]) : 2, refinements = argc > 2 ? (unsigned)std::atoi(argv[2]) : 3;
      const double   reltol = 1e-12;
      const Context  ctx(0);
      const std::vector<double> probes = {-0.5, 0.5, 0.25, 0.6, 0.6, -0.6, 0.7, -0.3, 0.4};

      for (unsigned r = 0; r < refinements; ++r)
        {
          const auto           fine   = std::make_shared<Triangulation>("hypercube", 2 + r);
          const auto           meshes = create_geometric_coarsening_sequence(fine);
          const auto           plan   = level_plan("HMG-global", meshes.size(), degree);
          const LevelStack     stack(ctx, meshes, plan.levels, MGAMD_F64, PreconditionChebyshev::AdditionalData(), nullptr, false, nullptr, 0.0);
          const PreconditionMG mg(ctx, stack.operators, stack.transfers, stack.smoothers, "amg");
          const Operator      &A    = stack.operators.back();
          const DoFHandler    &dofs = stack.dof_handlers.back();

          // the Dirichlet data: the free-space solution at the nodes (only its entries at Dirichlet DoFs are read)
          const std::vector<double> nodes = dofs.node_positions();
          std::vector<double>       g_host(dofs.n_dofs());
          for (size_t d = 0; d < dofs.n_dofs(); ++d)
            g_host[d] = exact(nodes[3 * d], nodes[3 * d + 1], nodes[3 * d + 2]);
          Vector g, b, lift, u;
          A.initialize_dof_vector(g);
          A.initialize_dof_vector(b);
          A.initialize_dof_vector(lift);
          A.initialize_dof_vector(u);
          g.copy_from_host(g_host);

          // the load: one Dirac source of weight 1 at x0
          PointEvaluation at_source(ctx, A);
          at_source.reinit(std::vector<double>(source, source + 3));
          if (!at_source.all_points_found())
            throw std::runtime_error("the source lies outside the cube");
          Vector weight(ctx, 1);
          weight = 1.0;
          at_source.point_source(weight, b);
          A.rhs_dirichlet(lift, g); // minus the lifting of the data
          b.add(1.0, lift);
          ReductionControl control(1000, 1e-20, reltol);
          SolverCG(control).solve(A, u, b, mg);
          A.distribute_values(u, g); // Dirichlet and hanging-node entries

          PointEvaluation at_probes(ctx, A);
          at_probes.reinit(probes);
          if (!at_probes.all_points_found())
            throw std::runtime_error("a probe lies outside the cube");
          const std::vector<double> u_h = at_probes.point_values(u).copy_to_host();
          std::printf("refinement %u cells %llu dofs %llu cg_iterations %u", 2 + r, (unsigned long long)fine->n_global_active_cells(),
                      (unsigned long long)dofs.n_dofs(), control.last_step());
          for (size_t k = 0; k < u_h.size(); ++k)
            std::printf(" u_%zu %.6e error_%zu %.6e", k, u_h[k], k, std::fabs(u_h[k] - exact(probes[3 * k], probes[3 * k + 1], probes[3 * k + 2])));
          std::printf("\n");
        }
      return 0;
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "point_source: %s\n", e.what());
      return 1;
    }
}
