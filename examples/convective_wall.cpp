// Steady heat conduction through a three-layer wall that exchanges heat with its surroundings: -div(a grad u) = 0 on the cube
// [-1, 1]^3, u = 0 on the face x = -1, a convective face at x = +1, a grad u . n + beta (u - u_ext) = 0, the four other faces
// insulated.  The layers are [-1, -0.5], [-0.5, 0] and [0, 1] with the conductivities 1, 5 and 0.2 (examples/layered_wall.cpp).
// The solution is piecewise linear in x: the flux is q = beta u_ext / (1 + beta R), R = sum_k d_k / a_k the resistance of the wall,
// and the temperature of the convective face u(+1) = q R.  hypercube, NRefGlobal 3, degree 2, HMG-global.
// Prints the computed and the analytic face temperature.  The example of INTEGRATION.md section 2b.
#include "../dealii_multigrid_amd/csrc/mgamd.hpp"

#include <algorithm>
#include <cstdio>

using namespace mgamd;

int
main()
{
  try
    {
      const unsigned degree = 2;
      const double   beta = 2.0, u_ext = 7.0, reltol = 1e-12;
      const double   interfaces[2] = {-0.5, 0.0}, conductivity[3] = {1.0, 5.0, 0.2};
      const Context  ctx(0);

      const auto fine = std::make_shared<Triangulation>("hypercube", 3);
      // face f = 2 axis + side: only face 0 (x = -1) is Dirichlet; face 1 (x = +1) is convective, the four others stay natural.
      // The mask first: a convective face must not be Dirichlet.
      fine->set_dirichlet_faces(1u << 0);
      fine->set_robin_coefficients({{0.0, beta, 0.0, 0.0, 0.0, 0.0}});
      // one conductivity per leaf, by the x coordinate of its centre -1 + h (i + 0.5), h = 2 / 2^level
      const size_t          nc = fine->n_global_active_cells();
      std::vector<uint8_t>  level(nc);
      std::vector<uint32_t> i(nc);
      check(mgamd_tria_get_cells(fine->get(), level.data(), i.data(), nullptr, nullptr, nullptr));
      std::vector<double> a(nc);
      for (size_t c = 0; c < nc; ++c)
        {
          const double x = -1.0 + 2.0 / (double)(1u << level[c]) * (i[c] + 0.5);
          a[c]           = conductivity[(x > interfaces[0]) + (x > interfaces[1])];
        }
      fine->set_coefficient(a);
      // mask, Robin coefficients and coefficient are set before the coarsening sequence: the coarse meshes inherit the first two and
      // average the third
      const auto           meshes = create_geometric_coarsening_sequence(fine);
      const auto           plan   = level_plan("HMG-global", meshes.size(), degree);
      const LevelStack     stack(ctx, meshes, plan.levels, MGAMD_F64, PreconditionChebyshev::AdditionalData());
      const PreconditionMG mg(ctx, stack.operators, stack.transfers, stack.smoothers, "amg");
      const Operator      &A = stack.operators.back();

      // f = 0: the right-hand side is the load of the exterior temperature alone, beta u_ext int phi_i over the convective face,
      // which is the boundary flux load with q = beta u_ext
      Vector b, u;
      A.initialize_dof_vector(b);
      A.initialize_dof_vector(u);
      A.rhs_boundary_flux(b, {{0.0, beta * u_ext, 0.0, 0.0, 0.0, 0.0}});
      ReductionControl control(200, 1e-20, reltol);
      SolverCG(control).solve(A, u, b, mg);
      A.distribute(u); // Dirichlet and hanging-node entries

      // the DoFs on x = +1: those with the largest x key
      const DoFHandler    &dofs = stack.dof_handlers.back();
      std::vector<int32_t> keys(5 * dofs.n_dofs());
      check(mgamd_dofs_get_keys(dofs.get(), keys.data()));
      int32_t top = 0;
      for (size_t d = 0; d < dofs.n_dofs(); ++d)
        top = std::max(top, keys[5 * d]);
      const std::vector<double> uh = u.copy_to_host();
      double                    lo = 1e300, hi = -1e300;
      for (size_t d = 0; d < dofs.n_dofs(); ++d)
        if (keys[5 * d] == top)
          {
            lo = std::min(lo, uh[d]);
            hi = std::max(hi, uh[d]);
          }
      const double R     = 0.5 / conductivity[0] + 0.5 / conductivity[1] + 1.0 / conductivity[2];
      const double exact = beta * u_ext / (1.0 + beta * R) * R;
      std::printf("CG iterations %u\n", control.last_step());
      std::printf("face temperature computed %.12f ... %.12f  analytic %.12f\n", lo, hi, exact);
      return 0;
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "convective_wall: %s\n", e.what());
      return 1;
    }
}
