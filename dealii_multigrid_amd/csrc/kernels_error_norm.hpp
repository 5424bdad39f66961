// Kernel of the error norms (DESIGN.md "Error norms"; in deal.II: VectorTools::integrate_difference): per leaf K with edge h_K and
// the tensor rule QGauss(n_q)^3, n_q = P + 1 ... P + 3 at run time,
//   L2      sqrt( sum_q w_q h^3 (u_h - w)^2 )                 H1 seminorm   sqrt( sum_q w_q h^3 |grad u_h - grad w|^2 )
//   energy  sqrt( sum_q w_q h^3 ( a_K |grad u_h - grad w|^2 + sigma (u_h - w)^2 ) )        Linfty   max_q |u_h - w|
// K12 difference_norm_kernel   gather through the table of the indicator (idx, mask, scale), C on the hanging faces and edges, then
//                              the sum-factorised evaluation at the quadrature points with the n_q x (P+1) matrices S (values) and
//                              G (derivatives), the difference against w, the weights and one sum (or maximum) per leaf.
// w is built in (kind 0: zero, kind 1: the Gaussian of SimulationType "Gaussian", LevelTables::gaussian_solution, with its gradient
// in closed form) or caller data at the quadrature points (kind -1): values [cell][qz][qy][qx] and, for the two gradient norms,
// gradients [cell][component][qz][qy][qx] in the number type of u, converted at the load.
// All arithmetic after the loads is double for both number types.  Only the entries of u at free and Dirichlet DoFs are read.  No
// atomics: the sum of a leaf is formed in a fixed order (per point: value, d_z, d_y, d_x; per row of points along qx; the rows in
// ascending order by one thread), so two calls give the same bits.
#pragma once
#include "kernels_boundary.hpp"

namespace mgamd
{
  // the values of MGAMD_NORM_* (include/mgamd.h)
  constexpr int NORM_L2 = 0, NORM_H1_SEMINORM = 1, NORM_ENERGY = 2, NORM_LINFTY = 3;

  template <typename T, int P>
  struct DifferenceNormArgs
  {
    static constexpr int NQM = P + 3; // the largest rule
    const uint32_t      *idx;         // [n_cells][N3], Dirichlet DoFs with their real index
    const uint16_t      *mask;        // [n_cells]
    const double        *scale;       // [n_cells][2]: a / h, h
    const double        *origin;      // [n_cells][3]: the lower corner (read for kind 1 only)
    uint32_t             n_cells, n_dofs;
    const T             *u, *values, *gradients; // values, gradients: caller data (kind -1), gradients for the gradient norms only
    double              *out;                    // [n_cells]
    int                  kind, norm, n_q;
    double               sigma;
    double               I0[(P + 1) * (P + 1)], I1[(P + 1) * (P + 1)];
    double               S[NQM * (P + 1)], G[NQM * (P + 1)]; // [q * (P+1) + a], the first n_q rows
    double               xq[NQM], wq[NQM];
  };
  static_assert(sizeof(DifferenceNormArgs<double, MAX_KERNEL_DEGREE>) <= KERNARG_LIMIT, "kernel arguments above the segment");

  // Packing as in face_flux_kernel: CPW = max(1, 256 / N3) leaves per workgroup pass (32, 9, 4, 2, 1, 1, 1 for P = 1..7), groups of
  // leaves walked with a grid stride whose trip count is uniform over the workgroup; kind, norm and n_q are kernel arguments, so
  // every branch around a barrier is uniform too, on the last, partial group as on any other.
  // LDS per leaf, sized for n_q = P + 3: the conforming nodal values bufU [N3], two sweep buffers bufA, bufB [(P+3)^3] and the
  // integrand bufC [(P+3)^3]: 52.9, 29.9, 23.7, 19.6, 15.5, 22.3, 30.6 KB for P = 1..7 with the 1D matrices (P = 1 holds 32 leaves):
  //   gather -> bufA;  C: bufA -> bufU -> bufA -> bufU
  //   bufA = X_x bufU  [az][ay][qx]        bufB = Y_y bufA  [az][qy][qx]        point (qz, qy, qx): Z_z bufB in registers
  // with (X, Y, Z) = (S, S, S) for the value and, from the same bufB, (S, S, G) for d_z; then (S, G, S) from the same bufA for d_y;
  // then (G, S, S) for d_x: five sweeps through LDS for the gradient norms, two for L2 and Linfty.  The integrand of a point is
  // kept in bufC over the passes by the one thread that owns the point (t = tid + 256 k in every pass); then one thread per row of
  // n_q points adds the weighted row into bufB, and one thread per leaf adds the n_q^2 rows.
  template <typename T, int P>
  __global__ void
  __launch_bounds__(256) difference_norm_kernel(DifferenceNormArgs<T, P> a)
  {
    constexpr int N = P + 1, N2 = N * N, N3 = N2 * N, CPW = dirichlet_cells_per_workgroup<P>();
    constexpr int NQM = P + 3, NQ3M = NQM * NQM * NQM;
    static_assert(MASK_FACE_SHIFT == 3 && MASK_EDGE_SHIFT == 6, "hanging_pass reads the mask bits by number");
    __shared__ double   bufU[CPW * N3], bufA[CPW * NQ3M], bufB[CPW * NQ3M], bufC[CPW * NQ3M];
    __shared__ double   sI[2 * N2], sS[NQM * N], sG[NQM * N], sx[NQM], sw[NQM];
    __shared__ double   s_a[CPW], s_h[CPW], s_o[CPW * 3];
    __shared__ uint32_t s_mask[CPW];
    const int           tid = threadIdx.x;
    const int           nq = a.n_q, nq2 = nq * nq, nq3 = nq2 * nq;
    const bool          linf = a.norm == NORM_LINFTY, with_value = a.norm != NORM_H1_SEMINORM;
    const bool          with_gradient = a.norm == NORM_H1_SEMINORM || a.norm == NORM_ENERGY;
    for (int i = tid; i < N2; i += 256)
      {
        sI[i]      = a.I0[i];
        sI[N2 + i] = a.I1[i];
      }
    for (int i = tid; i < nq * N; i += 256)
      {
        sS[i] = a.S[i];
        sG[i] = a.G[i];
      }
    if (tid < nq)
      {
        sx[tid] = a.xq[tid];
        sw[tid] = a.wq[tid];
      }
    const uint32_t n_groups = (a.n_cells + CPW - 1) / CPW;
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x)
      {
        const uint32_t cell0  = grp * CPW;
        const int      n_here = (int)(a.n_cells - cell0 < (uint32_t)CPW ? a.n_cells - cell0 : (uint32_t)CPW); // leaves of this group
        const int      n_act = n_here * N3, n_pts = n_here * nq3;
        for (int t = tid; t < n_act; t += 256)
          {
            const uint32_t gi = a.idx[(size_t)cell0 * N3 + t];
            bufA[t]           = gi < a.n_dofs ? (double)a.u[gi] : 0.0;
          }
        if (tid < n_here)
          {
            const double ah = a.scale[2 * (size_t)(cell0 + tid)], h = a.scale[2 * (size_t)(cell0 + tid) + 1];
            s_a[tid]        = ah * h; // (h is a power of two: a itself)
            s_h[tid]        = h;
            s_mask[tid]     = a.mask[cell0 + tid];
            for (int d = 0; d < 3; ++d)
              s_o[3 * tid + d] = a.kind == 1 ? a.origin[3 * (size_t)(cell0 + tid) + d] : 0.0;
          }
        __syncthreads();
        auto for_nodes = [&](auto body) {
          for (int t = tid; t < n_act; t += 256)
            {
              const int cl = t / N3, node = t - cl * N3;
              body(t, cl, cl * N3, node % N, (node / N) % N, node / N2);
            }
          __syncthreads();
        };
        for_nodes([&](int t, int cl, int base, int a0, int a1, int a2) {
          bufU[t] = hanging_pass<double, P, 0, false>(bufA + base, sI, s_mask[cl], a0, a1, a2);
        });
        for_nodes([&](int t, int cl, int base, int a0, int a1, int a2) {
          bufA[t] = hanging_pass<double, P, 1, false>(bufU + base, sI, s_mask[cl], a0, a1, a2);
        });
        for_nodes([&](int t, int cl, int base, int a0, int a1, int a2) {
          bufU[t] = hanging_pass<double, P, 2, false>(bufA + base, sI, s_mask[cl], a0, a1, a2);
        });
        // the conforming nodal values are in bufU.  bufA = X along x: [az][ay][qx]
        auto sweep_x = [&](const double *X) {
          const int per = N2 * nq, n_items = n_here * per;
          for (int it = tid; it < n_items; it += 256)
            {
              const int     cl = it / per, r = it - cl * per, line = r / nq, qx = r - line * nq;
              const double *in = bufU + cl * N3 + line * N;
              double        v  = 0.0;
#pragma unroll
              for (int b = 0; b < N; ++b)
                v += X[qx * N + b] * in[b];
              bufA[cl * NQ3M + r] = v;
            }
          __syncthreads();
        };
        // bufB = Y along y of bufA: [az][qy][qx]
        auto sweep_y = [&](const double *Y) {
          const int per = N * nq2, n_items = n_here * per;
          for (int it = tid; it < n_items; it += 256)
            {
              const int     cl = it / per, r = it - cl * per, az = r / nq2, rr = r - az * nq2, qy = rr / nq, qx = rr - qy * nq;
              const double *in = bufA + cl * NQ3M + az * N * nq + qx;
              double        v  = 0.0;
#pragma unroll
              for (int b = 0; b < N; ++b)
                v += Y[qy * N + b] * in[b * nq];
              bufB[cl * NQ3M + r] = v;
            }
          __syncthreads();
        };
        // w (component -1) or d_component w at point t of the group
        auto exact = [&](int t, int cl, int qx, int qy, int qz, int component) -> double {
          if (a.kind == 0)
            return 0.0;
          if (a.kind == 1)
            {
              const double width = 0.1, centre = -0.5, h = s_h[cl];
              const double x[3]  = {s_o[3 * cl] + h * sx[qx], s_o[3 * cl + 1] + h * sx[qy], s_o[3 * cl + 2] + h * sx[qz]};
              double       r2    = 0.0;
              for (int d = 0; d < 3; ++d)
                r2 += (x[d] - centre) * (x[d] - centre);
              const double s = sqrt(2.0 * 3.14159265358979323846) * width;
              const double g = exp(-r2 / (width * width)) / (s * s * s);
              return component < 0 ? g : -2.0 * (x[component] - centre) / (width * width) * g;
            }
          const int q = t - cl * nq3;
          if (component < 0)
            return (double)a.values[(size_t)cell0 * nq3 + t];
          return (double)a.gradients[((size_t)(cell0 + cl) * 3 + component) * nq3 + q];
        };
        // on every point of this thread (the same thread in every pass): Z along z of bufB (and, with `both`, G along z as well), into
        // the integrand bufC; the first pass stores, the later ones add
        auto points = [&](const double *Z, bool value, int component, bool both) {
          for (int t = tid; t < n_pts; t += 256)
            {
              const int     cl = t / nq3, q = t - cl * nq3, qz = q / nq2, rr = q - qz * nq2, qy = rr / nq, qx = rr - qy * nq;
              const double *in = bufB + cl * NQ3M + rr;
              double        v = 0.0, g = 0.0, sum = value ? 0.0 : bufC[cl * NQ3M + q];
#pragma unroll
              for (int b = 0; b < N; ++b)
                {
                  v += Z[qz * N + b] * in[b * nq2];
                  if (both)
                    g += sG[qz * N + b] * in[b * nq2];
                }
              if (value)
                {
                  const double e = v - exact(t, cl, qx, qy, qz, -1);
                  sum            = linf ? fabs(e) : (a.norm == NORM_ENERGY ? a.sigma : 1.0) * e * e;
                }
              else
                g = v;
              if (!value || both)
                {
                  const double e = g / s_h[cl] - exact(t, cl, qx, qy, qz, component);
                  sum += (a.norm == NORM_ENERGY ? s_a[cl] : 1.0) * e * e;
                }
              bufC[cl * NQ3M + q] = sum;
            }
          __syncthreads(); // the next sweep overwrites bufB
        };
        sweep_x(sS);
        sweep_y(sS);
        if (with_value)
          points(sS, true, 2, with_gradient);
        else
          {
            for (int t = tid; t < n_pts; t += 256)
              bufC[(t / nq3) * NQ3M + t % nq3] = 0.0; // (this thread's own points: no barrier)
            points(sG, false, 2, false);
          }
        if (with_gradient)
          {
            sweep_y(sG); // (bufA still holds S along x)
            points(sS, false, 1, false);
            sweep_x(sG);
            sweep_y(sS);
            points(sS, false, 0, false);
          }
        // the weights and the sum (the maximum) per leaf in a fixed order: along qx, then the rows in ascending order
        for (int it = tid; it < n_here * nq2; it += 256)
          {
            const int     cl = it / nq2, row = it - cl * nq2, qz = row / nq, qy = row - qz * nq;
            const double *in = bufC + cl * NQ3M + row * nq;
            double        s  = 0.0;
            for (int b = 0; b < nq; ++b)
              s = linf ? fmax(s, in[b]) : s + sw[b] * in[b];
            bufB[cl * NQ3M + row] = linf ? s : sw[qy] * sw[qz] * s;
          }
        __syncthreads();
        if (tid < n_here)
          {
            const double *in = bufB + tid * NQ3M;
            double        s  = 0.0;
            for (int b = 0; b < nq2; ++b)
              s = linf ? fmax(s, in[b]) : s + in[b];
            const double h     = s_h[tid];
            a.out[cell0 + tid] = linf ? s : sqrt(h * h * h * s);
          }
        __syncthreads(); // the next group's gather overwrites bufA and the scales of the leaves
      }
  }
} // namespace mgamd
