// Kernels of the cell evaluate and integrate (DESIGN.md "Cell evaluate and integrate"; in deal.II: FEEvaluation::evaluate /
// FEEvaluation::integrate over a cell loop and VectorTools::create_right_hand_side): per leaf K with edge h_K and the tensor rule
// QGauss(n_q)^3, n_q = P + 1 ... P + 3 at run time, weights w_q summing to 1,
//   K13 cell_evaluate_kernel    u  ->  u_h(x_q) [cell][qz][qy][qx]  and/or  grad u_h(x_q) [cell][component][qz][qy][qx]
//   K14 cell_integrate_kernel   v_q, V_q  ->  b_i = sum_K sum_q w_q h_K^3 ( v_q phi_i(x_q) + V_q . grad phi_i(x_q) ), through C^T
// at the points of LevelTables::quadrature_points, in the layouts of difference_norm_kernel's caller data.  Both walk the gather
// table of the indicator and the error norms (idx, mask, scale); neither applies a coefficient or sigma.
// All arithmetic between the loads and the stores is double for both number types.
// K13 has no atomics and a fixed order of every sum: two calls give the same bits.  K14 ends in an atomic add in the vector's number
// type on the rows below scatter_limit (as dirichlet_lift_kernel), so the order of the addends of a row shared by several leaves is
// not fixed: its result is NOT bit-reproducible across calls, except where every row has one addend.
#pragma once
#include "kernels_boundary.hpp"

namespace mgamd
{
  template <typename T, int P>
  struct CellEvaluateArgs
  {
    static constexpr int NQM = P + 3; // the largest rule
    const uint32_t      *idx;         // [n_cells][N3], Dirichlet DoFs with their real index
    const uint16_t      *mask;        // [n_cells]
    const double        *scale;       // [n_cells][2]: a / h, h
    uint32_t             n_cells, n_dofs;
    const T             *u;
    T                   *values, *gradients; // either may be null
    int                  n_q;
    double               I0[(P + 1) * (P + 1)], I1[(P + 1) * (P + 1)];
    double               S[NQM * (P + 1)], G[NQM * (P + 1)]; // [q * (P+1) + a], the first n_q rows
  };
  static_assert(sizeof(CellEvaluateArgs<double, MAX_KERNEL_DEGREE>) <= KERNARG_LIMIT, "kernel arguments above the segment");

  template <typename T, int P>
  struct CellIntegrateArgs
  {
    static constexpr int NQM = P + 3;
    const uint32_t      *idx;
    const uint16_t      *mask;
    const double        *scale;
    uint32_t             n_cells, scatter_limit; // rows below scatter_limit take the sums: the free rows
    const T             *values, *gradients;     // either may be null, not both
    T                   *dst;                    // zeroed before the launch
    int                  n_q;
    double               I0[(P + 1) * (P + 1)], I1[(P + 1) * (P + 1)];
    double               S[NQM * (P + 1)], G[NQM * (P + 1)];
    double               wq[NQM];
  };
  static_assert(sizeof(CellIntegrateArgs<double, MAX_KERNEL_DEGREE>) <= KERNARG_LIMIT, "kernel arguments above the segment");

  // Leaves per workgroup pass of K14.  It holds four buffers of (P+3)^3 doubles per leaf (below); with the 32 leaves of
  // dirichlet_cells_per_workgroup<1>() they alone are 64 KB, so P = 1 takes 16 leaves per pass (32 KB); every other degree follows
  // dirichlet_cells_per_workgroup (9, 4, 2, 1, 1, 1 leaves: 36.0, 27.6, 22.0, 16.4, 23.3, 32.0 KB).
  template <int P>
  constexpr int
  integrate_cells_per_workgroup()
  {
    return P == 1 ? 16 : dirichlet_cells_per_workgroup<P>();
  }

  // K13.  Packing and the first half as difference_norm_kernel: CPW = dirichlet_cells_per_workgroup<P>() leaves per workgroup pass,
  // groups walked with a grid stride whose trip count is uniform over the workgroup; n_q and which outputs are present are kernel
  // arguments, so every branch around a barrier is uniform.  LDS per leaf, sized for n_q = P + 3: the conforming nodal values bufU
  // [N3] and two sweep buffers bufA, bufB [(P+3)^3]:
  //   gather -> bufA;  C: bufA -> bufU -> bufA -> bufU
  //   bufA = X_x bufU  [az][ay][qx]        bufB = Y_y bufA  [az][qy][qx]        point (qz, qy, qx): Z_z bufB in registers, stored
  // with (X, Y, Z) = (S, S, S) for the value and, from the same bufB, (S, S, G) for d_z; then (S, G, S) from the same bufA for d_y;
  // then (G, S, S) for d_x: two sweeps through LDS for the values, five with the gradients.
  // Stores: point t = tid + 256 k of the group goes to values[cell0 n_q^3 + t], contiguous over qx and across the leaves of the
  // group; a gradient component of a leaf is one contiguous row of n_q^3 entries.
  template <typename T, int P>
  __global__ void
  __launch_bounds__(256) cell_evaluate_kernel(CellEvaluateArgs<T, P> a)
  {
    constexpr int N = P + 1, N2 = N * N, N3 = N2 * N, CPW = dirichlet_cells_per_workgroup<P>();
    constexpr int NQM = P + 3, NQ3M = NQM * NQM * NQM;
    static_assert(MASK_FACE_SHIFT == 3 && MASK_EDGE_SHIFT == 6, "hanging_pass reads the mask bits by number");
    __shared__ double   bufU[CPW * N3], bufA[CPW * NQ3M], bufB[CPW * NQ3M];
    __shared__ double   sI[2 * N2], sS[NQM * N], sG[NQM * N];
    __shared__ double   s_h[CPW];
    __shared__ uint32_t s_mask[CPW];
    const int           tid = threadIdx.x;
    const int           nq = a.n_q, nq2 = nq * nq, nq3 = nq2 * nq;
    const bool          with_value = a.values != nullptr, with_gradient = a.gradients != nullptr;
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
            s_h[tid]    = a.scale[2 * (size_t)(cell0 + tid) + 1];
            s_mask[tid] = a.mask[cell0 + tid];
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
        // Z along z of bufB at every point of the group, stored: the value (component < 0) or one gradient component, scaled by 1 / h
        auto points = [&](const double *Z, int component) {
          for (int t = tid; t < n_pts; t += 256)
            {
              const int     cl = t / nq3, q = t - cl * nq3, qz = q / nq2, rr = q - qz * nq2;
              const double *in = bufB + cl * NQ3M + rr;
              double        v  = 0.0;
#pragma unroll
              for (int b = 0; b < N; ++b)
                v += Z[qz * N + b] * in[b * nq2];
              if (component < 0)
                a.values[(size_t)cell0 * nq3 + t] = (T)v;
              else
                a.gradients[((size_t)(cell0 + cl) * 3 + component) * nq3 + q] = (T)(v / s_h[cl]);
            }
        };
        sweep_x(sS);
        sweep_y(sS);
        if (with_value)
          points(sS, -1);
        if (with_gradient)
          {
            points(sG, 2);
            __syncthreads(); // the next sweep overwrites bufB
            sweep_y(sG);     // (bufA still holds S along x)
            points(sS, 1);
            __syncthreads(); // the next sweeps overwrite bufA and bufB
            sweep_x(sG);
            sweep_y(sS);
            points(sS, 0);
          }
        __syncthreads(); // the next group's gather overwrites bufA and the scales of the leaves
      }
  }

  // K14, the transpose.  CPW = integrate_cells_per_workgroup<P>() leaves per workgroup pass, groups walked with a grid stride whose trip
  // count is uniform over the workgroup; n_q and which inputs are present are kernel arguments.  LDS per leaf: four buffers X0 ... X3
  // of (P+3)^3 doubles.  The data of a group is loaded with the weights w_qx w_qy w_qz h^3 (the gradient with h^2: its 1 / h folded
  // in; h is a power of two), one array at a time, and swept along x at once, so that the three gradient components never stand
  // side by side:
  //   X0 = f, X1 = Fx            X2 = A1 = S^T_x f + G^T_x Fx    [qz][qy][ax]
  //   X0 = Fy                    X1 = A2 = S^T_x Fy
  //   X0 = Fz                    X3 = A3 = S^T_x Fz
  //   X0 = B1 = S^T_y A1 + G^T_y A2,  then X1 = B2 = S^T_y A3    [qz][ay][ax]
  //   X2 = S^T_z B1 + G^T_z B2                                   [az][ay][ax]: ONE (P+1)^3 tensor per leaf
  //   C^T: directions 2, 1, 0 (X2 -> X3 -> X2 -> the atomic add on the rows below scatter_limit)
  template <typename T, int P>
  __global__ void
  __launch_bounds__(256) cell_integrate_kernel(CellIntegrateArgs<T, P> a)
  {
    constexpr int N = P + 1, N2 = N * N, N3 = N2 * N, CPW = integrate_cells_per_workgroup<P>();
    constexpr int NQM = P + 3, NQ3M = NQM * NQM * NQM;
    static_assert(MASK_FACE_SHIFT == 3 && MASK_EDGE_SHIFT == 6, "hanging_pass reads the mask bits by number");
    static_assert(4 * CPW * NQ3M * sizeof(double) + (2 * N2 + 2 * NQM * N + NQM + 2 * CPW) * sizeof(double) <= 64 * 1024, "LDS above 64 KB");
    __shared__ double   X0[CPW * NQ3M], X1[CPW * NQ3M], X2[CPW * NQ3M], X3[CPW * NQ3M];
    __shared__ double   sI[2 * N2], sS[NQM * N], sG[NQM * N], sw[NQM];
    __shared__ double   s_h[CPW];
    __shared__ uint32_t s_mask[CPW];
    const int           tid = threadIdx.x;
    const int           nq = a.n_q, nq2 = nq * nq, nq3 = nq2 * nq;
    const bool          with_value = a.values != nullptr, with_gradient = a.gradients != nullptr;
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
      sw[tid] = a.wq[tid];
    const uint32_t n_groups = (a.n_cells + CPW - 1) / CPW;
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x)
      {
        const uint32_t cell0  = grp * CPW;
        const int      n_here = (int)(a.n_cells - cell0 < (uint32_t)CPW ? a.n_cells - cell0 : (uint32_t)CPW); // leaves of this group
        const int      n_act = n_here * N3, n_pts = n_here * nq3;
        if (tid < n_here)
          {
            s_h[tid]    = a.scale[2 * (size_t)(cell0 + tid) + 1];
            s_mask[tid] = a.mask[cell0 + tid];
          }
        __syncthreads(); // (also: the 1D matrices and the weights on the first trip)
        // dst = the values (component < 0) or one gradient component of the group at its points, times the weights
        auto load = [&](double *dst, int component) {
          for (int t = tid; t < n_pts; t += 256)
            {
              const int    cl = t / nq3, q = t - cl * nq3, qz = q / nq2, rr = q - qz * nq2, qy = rr / nq, qx = rr - qy * nq;
              const double h = s_h[cl], w = sw[qx] * sw[qy] * sw[qz];
              dst[cl * NQ3M + q] = component < 0 ? w * (h * h * h) * (double)a.values[(size_t)cell0 * nq3 + t] :
                                                   w * (h * h) * (double)a.gradients[((size_t)(cell0 + cl) * 3 + component) * nq3 + q];
            }
        };
        // out [qz][qy][ax] = X^T along x of in0 (+ Y^T along x of in1); either input may be null
        auto sweep_x = [&](double *out, const double *X, const double *in0, const double *Y, const double *in1) {
          const int per = nq2 * N, n_items = n_here * per;
          for (int it = tid; it < n_items; it += 256)
            {
              const int cl = it / per, r = it - cl * per, row = r / N, ax = r - row * N, off = cl * NQ3M + row * nq;
              double    v = 0.0;
              if (in0)
                for (int b = 0; b < nq; ++b)
                  v += X[b * N + ax] * in0[off + b];
              if (in1)
                for (int b = 0; b < nq; ++b)
                  v += Y[b * N + ax] * in1[off + b];
              out[cl * NQ3M + r] = v;
            }
          __syncthreads();
        };
        // out [qz][ay][ax] = X^T along y of in0 [qz][qy][ax] (+ Y^T along y of in1)
        auto sweep_y = [&](double *out, const double *X, const double *in0, const double *Y, const double *in1) {
          const int per = nq * N2, n_items = n_here * per;
          for (int it = tid; it < n_items; it += 256)
            {
              const int cl = it / per, r = it - cl * per, qz = r / N2, rr = r - qz * N2, ay = rr / N, ax = rr - ay * N;
              const int off = cl * NQ3M + qz * nq * N + ax;
              double    v = 0.0;
              if (in0)
                for (int b = 0; b < nq; ++b)
                  v += X[b * N + ay] * in0[off + b * N];
              if (in1)
                for (int b = 0; b < nq; ++b)
                  v += Y[b * N + ay] * in1[off + b * N];
              out[cl * NQ3M + r] = v;
            }
          __syncthreads();
        };
        if (with_value)
          load(X0, -1);
        if (with_gradient)
          load(X1, 0);
        __syncthreads();
        sweep_x(X2, sS, with_value ? X0 : nullptr, sG, with_gradient ? X1 : nullptr); // A1
        if (with_gradient)
          {
            load(X0, 1);
            __syncthreads();
            sweep_x(X1, sS, X0, nullptr, nullptr); // A2
            load(X0, 2);
            __syncthreads();
            sweep_x(X3, sS, X0, nullptr, nullptr); // A3
          }
        sweep_y(X0, sS, X2, sG, with_gradient ? X1 : nullptr); // B1
        if (with_gradient)
          sweep_y(X1, sS, X3, nullptr, nullptr); // B2
        // along z: X2 [cl * N3 + node] = S^T B1 (+ G^T B2)
        for (int t = tid; t < n_act; t += 256)
          {
            const int cl = t / N3, node = t - cl * N3, az = node / N2, rr = node - az * N2, off = cl * NQ3M + rr;
            double    v = 0.0;
            for (int b = 0; b < nq; ++b)
              v += sS[b * N + az] * X0[off + b * N2];
            if (with_gradient)
              for (int b = 0; b < nq; ++b)
                v += sG[b * N + az] * X1[off + b * N2];
            X2[t] = v;
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
        // C^T: directions 2, 1, 0, the last one into the destination
        for_nodes([&](int t, int cl, int base, int a0, int a1, int a2) {
          X3[t] = hanging_pass<double, P, 2, true>(X2 + base, sI, s_mask[cl], a0, a1, a2);
        });
        for_nodes([&](int t, int cl, int base, int a0, int a1, int a2) {
          X2[t] = hanging_pass<double, P, 1, true>(X3 + base, sI, s_mask[cl], a0, a1, a2);
        });
        // (its barrier: the next group's loads overwrite the buffers and the scales of the leaves)
        for_nodes([&](int t, int cl, int base, int a0, int a1, int a2) {
          const double   v  = hanging_pass<double, P, 0, true>(X2 + base, sI, s_mask[cl], a0, a1, a2);
          const uint32_t gi = a.idx[(size_t)cell0 * N3 + t];
          if (gi < a.scatter_limit)
            atomic_add(&a.dst[gi], (T)v);
        });
      }
  }
} // namespace mgamd
