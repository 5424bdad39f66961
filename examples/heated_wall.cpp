// Steady heat conduction through a three-layer wall held at two temperatures: -div(a grad u) = 0 on the cube [-1, 1]^3, u = T0 on the
// face x = -1 and u = T1 on the face x = +1, the four other faces insulated.  The layers are [-1, -0.5], [-0.5, 0] and [0, 1] with the
// conductivities 1, 5 and 0.2.  The solution is piecewise linear in x: the heat flux is q = (T1 - T0) / sum_i d_i / a_i (the thermal
// resistances in series) and the temperature of an interface is T0 + q times the resistance up to it.  hypercube, NRefGlobal 3,
// degree 2, HMG-global.  The Dirichlet values are caller data: Operator::rhs_dirichlet lifts them into the right-hand side on the
// device and Operator::distribute_values writes them back.  Prints the computed and the analytic interface temperatures.  The example
// of INTEGRATION.md section 2c.
#include "../dealii_multigrid_amd/csrc/mgamd.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>

using namespace mgamd;

int
main()
{
  try
    {
      const unsigned degree = 2;
      const double   T0 = 300.0, T1 = 400.0, reltol = 1e-12;
      const double   interfaces[2] = {-0.5, 0.0}, conductivity[3] = {1.0, 5.0, 0.2}, thickness[3] = {0.5, 0.5, 1.0};
      const Context  ctx(0);

      const auto fine = std::make_shared<Triangulation>("hypercube", 3);
      // face f = 2 axis + side: faces 0 (x = -1) and 1 (x = +1) are Dirichlet, the four others are natural
      fine->set_dirichlet_faces((1u << 0) | (1u << 1));
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
      const LevelStack     stack(ctx, meshes, plan.levels, MGAMD_F64, PreconditionChebyshev::AdditionalData());
      const PreconditionMG mg(ctx, stack.operators, stack.transfers, stack.smoothers, "amg");
      const Operator      &A    = stack.operators.back();
      const DoFHandler    &dofs = stack.dof_handlers.back();

      // the Dirichlet data: one constant per Dirichlet face (a value on a natural face is refused); f = 0, so the right-hand side
      // is the lifting of the data alone
      Vector g, b, u;
      A.initialize_dof_vector(g);
      A.initialize_dof_vector(b);
      A.initialize_dof_vector(u);
      g.copy_from_host(dofs.dirichlet_face_values({{T0, T1, 0.0, 0.0, 0.0, 0.0}}));
      A.rhs_dirichlet(b, g);
      ReductionControl control(200, 1e-20, reltol);
      SolverCG(control).solve(A, u, b, mg);
      A.distribute_values(u, g); // Dirichlet and hanging-node entries

      const std::vector<double> xyz = dofs.node_positions(), uh = u.copy_to_host();
      double                    resistance = 0.0;
      for (int l = 0; l < 3; ++l)
        resistance += thickness[l] / conductivity[l];
      const double q = (T1 - T0) / resistance;
      std::printf("CG iterations %u\n", control.last_step());
      double up_to = 0.0;
      for (int l = 0; l < 2; ++l)
        {
          up_to += thickness[l] / conductivity[l];
          double lo = 1e300, hi = -1e300;
          for (size_t d = 0; d < dofs.n_dofs(); ++d)
            if (std::fabs(xyz[3 * d] - interfaces[l]) < 1e-12)
              {
                lo = std::min(lo, uh[d]);
                hi = std::max(hi, uh[d]);
              }
          std::printf("interface x = %+.1f temperature computed %.10f ... %.10f  analytic %.10f\n", interfaces[l], lo, hi, T0 + q * up_to);
        }
      return 0;
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "heated_wall: %s\n", e.what());
      return 1;
    }
}
