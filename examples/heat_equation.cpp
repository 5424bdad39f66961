// Heat equation u' - Laplace u = 0 on the cube [-1, 1]^3 with u = 0 on the boundary, from u(0) = 1: five Crank-Nicolson steps
// (theta = 0.5) with the library's time stepper on hypercube, NRefGlobal 3, degree 2, an HMG-global hierarchy.  Prints |u| per step.
// The example of INTEGRATION.md section 2a.
// With an argument, `heat_equation 1000`, a second material: the conductivity a of u' - div(a grad u) = 0 is that value in the
// inclusion [-0.5, 0]^3 and 1 elsewhere (one value per leaf, set on the finest mesh before the coarsening sequence is built).
#include "../dealii_multigrid_amd/csrc/mgamd.hpp"

#include <cstdio>
#include <cstdlib>

using namespace mgamd;

int
main(int argc, char **argv)
{
  try
    {
      const double   theta = 0.5, dt = 0.01, reltol = 1e-10;
      const unsigned degree = 2, n_steps = 5;
      const Context  ctx(0);

      // the operator of an implicit step is A = K + sigma M with sigma = 1 / (theta dt), on EVERY level of the hierarchy
      const double sigma  = ThetaTimeStepper::mass_coefficient(theta, dt);
      const auto   fine   = std::make_shared<Triangulation>("hypercube", 3);
      if (argc > 1)
        {
          // leaves as (level, i, j, k); the centre of a leaf is -1 + h (i + 0.5), h = 2 / 2^level
          const size_t          nc = fine->n_global_active_cells();
          std::vector<uint8_t>  level(nc);
          std::vector<uint32_t> ijk[3] = {std::vector<uint32_t>(nc), std::vector<uint32_t>(nc), std::vector<uint32_t>(nc)};
          check(mgamd_tria_get_cells(fine->get(), level.data(), ijk[0].data(), ijk[1].data(), ijk[2].data(), nullptr));
          std::vector<double> a(nc, 1.0);
          for (size_t c = 0; c < nc; ++c)
            {
              bool inside = true;
              for (int d = 0; d < 3; ++d)
                {
                  const double x = -1.0 + 2.0 / (double)(1u << level[c]) * (ijk[d][c] + 0.5);
                  inside         = inside && x > -0.5 && x < 0.0;
                }
              if (inside)
                a[c] = std::atof(argv[1]);
            }
          fine->set_coefficient(a); // refuses values that are not finite and > 0, by index
        }
      const auto meshes = create_geometric_coarsening_sequence(fine); // the coarse meshes carry the mean over each leaf
      if (fine->has_coefficient())
        {
          const auto range = DoFHandler(fine, degree).coefficient_range();
          std::printf("conductivity %g ... %g on the finest mesh, %.10g on the one-cell mesh\n", range.first, range.second,
                      meshes.front()->coefficient()[0]);
        }
      const auto   plan   = level_plan("HMG-global", meshes.size(), degree);
      const LevelStack     stack(ctx, meshes, plan.levels, MGAMD_F64, PreconditionChebyshev::AdditionalData(), nullptr, false, nullptr, sigma);
      const PreconditionMG mg(ctx, stack.operators, stack.transfers, stack.smoothers, "amg");
      const Operator      &A = stack.operators.back();

      ThetaTimeStepper stepper(A, mg, theta, dt);
      Vector           u;
      A.initialize_dof_vector(u);
      u = 1.0; // nodal values of u(0); entries on constrained DoFs are not read and come back as 0
      for (unsigned n = 0; n < n_steps; ++n)
        {
          const unsigned it = stepper.step(u, reltol);
          std::printf("step %u  t = %.4f  |u| = %.12e  CG iterations %u\n", (unsigned)stepper.n_steps(), stepper.time(), u.l2_norm(), it);
        }
      // (with a source: stepper.step(u, f_old, f_new, reltol) with the nodal values of f at t and t + dt; for output,
      // A.distribute(u) fills the hanging-node entries, and the vector may be passed back in)
      return 0;
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "heat_equation: %s\n", e.what());
      return 1;
    }
}
