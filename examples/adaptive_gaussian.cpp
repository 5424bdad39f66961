// The adaptive loop on the built-in Gaussian problem (SimulationType "Gaussian": -Laplace u = f with the narrow Gaussian around
// (-0.5, -0.5, -0.5) as the exact solution, its values as Dirichlet data): solve, estimate, mark, refine.  Starting from
// hypercube NRefGlobal 2, every cycle builds the HMG-global hierarchy of the current mesh, solves with CG (reltol 1e-10), fills the
// constrained entries, computes the jump error indicator eta_K on the device (Operator::estimate_error), flags the cells with
// eta_K >= 0.5 max eta (mark_maximum) and refines them (Triangulation::refine, which restores the 2:1 balance).  Prints per cycle the
// cells, the DoFs, sum eta_K^2, the largest nodal error against the exact solution, the L2 and H1 errors (Operator::integrate_difference)
// and the effectivity index sqrt(sum eta_K^2) / energy error.  The example of INTEGRATION.md section 2d.
//   adaptive_gaussian [degree = 2] [cycles = 4]
#include "../dealii_multigrid_amd/csrc/mgamd.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace mgamd;

int
main(int argc, char **argv)
{
  try
    {
      const unsigned degree = argc > 1 ? (unsigned)std::atoi(argv[1]) : 2, cycles = argc > 2 ? (unsigned)std::atoi(argv[2]) : 4;
      const double   width = 0.1, centre = -0.5, pi = 3.14159265358979323846;
      const Context  ctx(0);

      std::shared_ptr<const Triangulation> mesh = std::make_shared<Triangulation>("hypercube", 2);
      for (unsigned cycle = 0; cycle < cycles; ++cycle)
        {
          const auto           meshes = create_geometric_coarsening_sequence(mesh);
          const auto           plan   = level_plan("HMG-global", meshes.size(), degree);
          const LevelStack     stack(ctx, meshes, plan.levels, MGAMD_F64, PreconditionChebyshev::AdditionalData());
          const PreconditionMG mg(ctx, stack.operators, stack.transfers, stack.smoothers, "amg");
          const Operator      &A    = stack.operators.back();
          const DoFHandler    &dofs = stack.dof_handlers.back();

          Vector b, u;
          A.initialize_dof_vector(b);
          A.initialize_dof_vector(u);
          A.rhs(b, 1); // the Gaussian source and the lifting of its boundary values
          ReductionControl control(1000, 1e-20, 1e-10);
          SolverCG(control).solve(A, u, b, mg);
          A.distribute(u, 1); // Dirichlet and hanging-node entries

          const std::vector<double> eta = A.estimate_error(u);
          double                    sum = 0.0, error = 0.0;
          for (double e : eta)
            sum += e * e;
          const std::vector<double> xyz = dofs.node_positions(), uh = u.copy_to_host();
          for (size_t d = 0; d < dofs.n_dofs(); ++d)
            {
              double r2 = 0.0;
              for (int c = 0; c < 3; ++c)
                r2 += (xyz[3 * d + c] - centre) * (xyz[3 * d + c] - centre);
              const double exact = std::exp(-r2 / (width * width)) / std::pow(std::sqrt(2.0 * pi) * width, 3.0);
              error              = std::max(error, std::fabs(uh[d] - exact));
            }
          // the true error on the device (Operator::integrate_difference against the built-in Gaussian, QGauss(degree + 2) per leaf) and
          // the effectivity index sqrt(sum eta_K^2) / |||e|||: a = 1 and sigma = 0 here, so the energy norm is the H1 seminorm
          const double l2     = compute_global_error(A.integrate_difference(u, 1, MGAMD_NORM_L2, degree + 2), MGAMD_NORM_L2);
          const double h1     = compute_global_error(A.integrate_difference(u, 1, MGAMD_NORM_H1_SEMINORM, degree + 2), MGAMD_NORM_H1_SEMINORM);
          const double energy = compute_global_error(A.integrate_difference(u, 1, MGAMD_NORM_ENERGY, degree + 2), MGAMD_NORM_ENERGY);
          std::printf("cycle %u cells %llu dofs %llu cg_iterations %u sum_eta2 %.6e max_nodal_error %.6e l2_error %.6e h1_error %.6e "
                      "effectivity %.6e\n",
                      cycle, (unsigned long long)mesh->n_global_active_cells(), (unsigned long long)dofs.n_dofs(), control.last_step(), sum, error,
                      l2, h1, std::sqrt(sum) / energy);
          if (cycle + 1 < cycles)
            mesh = mesh->refine(mark_maximum(eta, 0.5));
        }
      return 0;
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "adaptive_gaussian: %s\n", e.what());
      return 1;
    }
}
