// A manufactured solution with a caller-built load: -div(a grad u) + sigma u = f on the cube [-1, 1]^3 with the three material layers
// of layered_wall.cpp (conductivities 1, 5, 0.2 in [-1, -0.5], [-0.5, 0], [0, 1]), sigma = 1 and all six faces Dirichlet, for
//   u* = sin(2x + 0.5) cos(1.5y) + 0.3 z^2 x.
// The Dirichlet data is g = u* at DoFHandler::node_positions, lifted by Operator::rhs_dirichlet.  The load is given in divergence
// form, tabulated at DoFHandler::quadrature_points and integrated on the device by Operator::integrate:
//   b_i = sum_K sum_q w_q h_K^3 ( sigma u*(x_q) phi_i(x_q) + a_K grad u*(x_q) . grad phi_i(x_q) ),
// which needs no derivative of a and no jump term on the layer interfaces: the discrete solution is the energy projection of u*
// whatever the jumps of a.  CG with the V-cycle (reltol 1e-12), then Operator::distribute_values.  Per mesh (hypercube, NRefGlobal
// 2, 3, ...: the layers are faces of the leaves) it prints the cells, the DoFs, the CG iterations, the L2 and H1 errors
// (Operator::integrate_difference against u* and its gradient at the same points) and the observed orders between successive meshes.
// The example of INTEGRATION.md section 2e.
//   manufactured_solution [degree = 2] [refinements = 3]
#include "../dealii_multigrid_amd/csrc/mgamd.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace mgamd;

static double
exact(double x, double y, double z)
{
  return std::sin(2.0 * x + 0.5) * std::cos(1.5 * y) + 0.3 * z * z * x;
}
static void
exact_gradient(double x, double y, double z, double g[3])
{
  g[0] = 2.0 * std::cos(2.0 * x + 0.5) * std::cos(1.5 * y) + 0.3 * z * z;
  g[1] = -1.5 * std::sin(2.0 * x + 0.5) * std::sin(1.5 * y);
  g[2] = 0.6 * z * x;
}

int
main(int argc, char **argv)
{
  try
    {
      const unsigned degree = argc > 1 ? (unsigned)std::atoi(argv[1]) : 2, refinements = argc > 2 ? (unsigned)std::atoi(argv[2]) : 3;
      const double   sigma = 1.0, reltol = 1e-12;
      const double   interfaces[2] = {-0.5, 0.0}, conductivity[3] = {1.0, 5.0, 0.2};
      const int      n_q = (int)degree + 2;
      const Context  ctx(0);

      double l2_before = 0.0, h1_before = 0.0;
      for (unsigned r = 0; r < refinements; ++r)
        {
          const auto fine = std::make_shared<Triangulation>("hypercube", 2 + r);
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
          const auto           meshes = create_geometric_coarsening_sequence(fine);
          const auto           plan   = level_plan("HMG-global", meshes.size(), degree);
          const LevelStack     stack(ctx, meshes, plan.levels, MGAMD_F64, PreconditionChebyshev::AdditionalData(), nullptr, false, nullptr, sigma);
          const PreconditionMG mg(ctx, stack.operators, stack.transfers, stack.smoothers, "amg");
          const Operator      &A    = stack.operators.back();
          const DoFHandler    &dofs = stack.dof_handlers.back();

          // the data at the quadrature points: values [cell][qz][qy][qx], gradients [cell][component][qz][qy][qx]; u* and its gradient
          // for the error norms, sigma u* and a_K grad u* for the load
          const std::vector<double> xyz = dofs.quadrature_points(n_q);
          const size_t              nq3 = (size_t)n_q * n_q * n_q;
          std::vector<double>       w(nc * nq3), grad_w(3 * nc * nq3), f(nc * nq3), F(3 * nc * nq3);
          for (size_t c = 0; c < nc; ++c)
            for (size_t q = 0; q < nq3; ++q)
              {
                const double *x = &xyz[3 * (c * nq3 + q)];
                double        g[3];
                exact_gradient(x[0], x[1], x[2], g);
                w[c * nq3 + q] = exact(x[0], x[1], x[2]);
                f[c * nq3 + q] = sigma * w[c * nq3 + q];
                for (int d = 0; d < 3; ++d)
                  {
                    grad_w[(c * 3 + d) * nq3 + q] = g[d];
                    F[(c * 3 + d) * nq3 + q]      = a[c] * g[d];
                  }
              }
          Vector w_dev(ctx, w.size()), grad_w_dev(ctx, grad_w.size()), f_dev(ctx, f.size()), F_dev(ctx, F.size());
          w_dev.copy_from_host(w);
          grad_w_dev.copy_from_host(grad_w);
          f_dev.copy_from_host(f);
          F_dev.copy_from_host(F);

          // the Dirichlet data: the nodal interpolant of u* (only its entries at Dirichlet DoFs are read)
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

          A.integrate(b, f_dev, F_dev, n_q); // the load, on the device
          A.rhs_dirichlet(lift, g);          // minus the lifting of the data, K + sigma M
          b.add(1.0, lift);
          ReductionControl control(1000, 1e-20, reltol);
          SolverCG(control).solve(A, u, b, mg);
          A.distribute_values(u, g); // Dirichlet and hanging-node entries

          const double l2 = compute_global_error(A.integrate_difference(u, w_dev, MGAMD_NORM_L2, n_q), MGAMD_NORM_L2);
          const double h1 = compute_global_error(A.integrate_difference(u, w_dev, grad_w_dev, MGAMD_NORM_H1_SEMINORM, n_q), MGAMD_NORM_H1_SEMINORM);
          std::printf("refinement %u cells %llu dofs %llu cg_iterations %u l2_error %.6e h1_error %.6e", 2 + r, (unsigned long long)nc,
                      (unsigned long long)dofs.n_dofs(), control.last_step(), l2, h1);
          if (r > 0)
            std::printf(" l2_order %.3f h1_order %.3f", std::log2(l2_before / l2), std::log2(h1_before / h1));
          std::printf("\n");
          l2_before = l2;
          h1_before = h1;
        }
      return 0;
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "manufactured_solution: %s\n", e.what());
      return 1;
    }
}
