// Heat equation u' - Laplace u = 0 on the cube [-1, 1]^3 with u = 0 on the boundary, from u(0) = 1: five Crank-Nicolson steps
// (theta = 0.5) with the library's time stepper on hypercube, NRefGlobal 3, degree 2, an HMG-global hierarchy.  Prints |u| per step.
// The example of INTEGRATION.md section 2a.
#include "../dealii_multigrid_amd/csrc/mgamd.hpp"

#include <cstdio>

using namespace mgamd;

int
main()
{
  try
    {
      const double   theta = 0.5, dt = 0.01, reltol = 1e-10;
      const unsigned degree = 2, n_steps = 5;
      const Context  ctx(0);

      // the operator of an implicit step is A = K + sigma M with sigma = 1 / (theta dt), on EVERY level of the hierarchy
      const double sigma  = ThetaTimeStepper::mass_coefficient(theta, dt);
      const auto   meshes = create_geometric_coarsening_sequence(std::make_shared<const Triangulation>("hypercube", 3));
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
