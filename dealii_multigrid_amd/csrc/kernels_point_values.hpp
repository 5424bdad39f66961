// Kernels of point evaluation and point sources (DESIGN.md "Point evaluation and point sources"; in deal.II:
// Utilities::MPI::RemotePointEvaluation with VectorTools::point_values / point_gradients, FEPointEvaluation, and the transpose
// VectorTools::create_point_source_vector): for caller points x_k of [-1, 1]^3, always double,
//   K15 point_locate_kernel      x_k  ->  the leaf that holds x_k (-1: not found) and its reference coordinate xi_k in [0, 1]^3
//   K16 point_evaluate_kernel    u    ->  u_h(x_k) [n]  and/or  grad u_h(x_k) [3][n], in the caller's point order
//   K17 point_integrate_kernel   w_k, W_k  ->  b_i = sum_k ( w_k phi_i(x_k) + W_k . grad phi_i(x_k) ), through C^T
// Location is octree.hpp point_key and LevelTables::locate_point restated: s = (x + 1) 2^(LMAX-1) per coordinate, found iff every s
// lies in [0, 2^LMAX], integer coordinate min(2^LMAX - 1, floor(s)), the leaf is upper_bound - 1 of the Morton key in the sorted
// keys of the leaves.  A point on an interior face, edge or vertex belongs to the leaf on its upper side, a point on a face = +1
// to the last leaf; u_h is continuous, so values do not depend on this rule, and gradients are the ONE-SIDED gradients of that leaf.
// K16 and K17 walk the OCCUPIED leaves of a point set (a CSR list built when the set is built) with the gather table of the
// indicator, the norms and the cell values (idx, mask, scale); neither applies a coefficient, sigma, a quadrature weight or h^3.
// All arithmetic between the loads and the stores is double for both number types.
// K16 has no atomics and a fixed order of every sum: two calls give the same bits.  K17 sums the points of a leaf in their sorted
// order (no LDS atomics) and ends in an atomic add in the vector's number type on the rows below scatter_limit (as
// cell_integrate_kernel), so a row shared by several occupied leaves takes its addends in no fixed order: its result is NOT
// bit-reproducible across calls, except where every row has one addend.
#pragma once
#include "kernels_boundary.hpp"

namespace mgamd
{
  __device__ __forceinline__ uint64_t
  point_spread3(uint64_t x)
  {
    x &= 0x1fffff;
    x = (x | x << 32) & 0x1f00000000ffffULL;
    x = (x | x << 16) & 0x1f0000ff0000ffULL;
    x = (x | x << 8) & 0x100f00f00f00f00fULL;
    x = (x | x << 4) & 0x10c30c30c30c30c3ULL;
    x = (x | x << 2) & 0x1249249249249249ULL;
    return x;
  }

  struct PointLocateArgs
  {
    const double   *xyz;    // [n][3]
    uint64_t        n;
    const uint64_t *keys;   // [n_cells], ascending, keys[0] == 0: leaf t covers [keys[t], keys[t + 1])
    const uint32_t *corner; // [n_cells][4]: the lower corner in integer coordinates (units of 2^-(LMAX-1)) and the edge in the same units
    uint32_t        n_cells;
    int32_t        *cell; // [n], -1: not found
    double         *ref;  // [n][3], 0 where not found
  };

  // K15: one thread per point, grid stride.  L is the depth of the integer coordinates, octree.hpp LMAX (the launch passes it; a
  // template also lets the kernel live in a header of several translation units)
  template <int L>
  __global__ void
  __launch_bounds__(256) point_locate_kernel(PointLocateArgs a)
  {
    constexpr double POINT_UNITS = (double)(1u << (L - 1)); // integer coordinates per unit length
    const uint64_t   top         = ((uint64_t)1 << L) - 1;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < a.n; k += (uint64_t)gridDim.x * 256)
      {
        double   s[3];
        uint64_t c[3];
        bool     found = true;
#pragma unroll
        for (int d = 0; d < 3; ++d)
          {
            s[d]  = (a.xyz[3 * k + d] + 1.0) * POINT_UNITS;
            found = found && s[d] >= 0.0 && s[d] <= 2.0 * POINT_UNITS; // (NaN: false)
            const uint64_t f = found ? (uint64_t)s[d] : 0;
            c[d]             = f < top ? f : top;
          }
        int32_t cell = -1;
        double  r[3] = {0.0, 0.0, 0.0};
        if (found)
          {
            const uint64_t key = point_spread3(c[0]) | (point_spread3(c[1]) << 1) | (point_spread3(c[2]) << 2);
            uint32_t       lo = 0, hi = a.n_cells; // the first leaf whose key is above the point's
            while (lo < hi)
              {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.keys[mid] <= key)
                  lo = mid + 1;
                else
                  hi = mid;
              }
            cell = (int32_t)lo - 1; // (lo >= 1: keys[0] == 0)
            const uint32_t *q = a.corner + 4 * (size_t)cell;
            const double    e = (double)q[3];
#pragma unroll
            for (int d = 0; d < 3; ++d)
              r[d] = (s[d] - (double)q[d]) / e;
          }
        a.cell[k] = cell;
#pragma unroll
        for (int d = 0; d < 3; ++d)
          a.ref[3 * k + d] = r[d];
      }
  }

  // what the two per-degree kernels share: the gather table, the CSR list of occupied leaves and the 1D element
  template <int P>
  struct PointWalkArgs
  {
    const uint32_t *idx;   // [n_cells][N3], Dirichlet DoFs with their real index
    const uint16_t *mask;  // [n_cells]
    const double   *scale; // [n_cells][2]: a / h, h
    const uint32_t *leaf;  // [n_occupied]: the occupied leaves, ascending
    const uint32_t *ptr;   // [n_occupied + 1]: the sorted points of occupied leaf o are [ptr[o], ptr[o + 1])
    const uint32_t *perm;  // [n_found]: sorted point -> the caller's point, ascending within a leaf
    const uint32_t *occ;   // [n_found]: sorted point -> its occupied leaf o
    const double   *ref;   // [n][3], the caller's order
    uint32_t        n_occupied, n_points; // n_points: the caller's n, the stride of the gradient components
    double          I0[(P + 1) * (P + 1)], I1[(P + 1) * (P + 1)];
    double          nodes[P + 1], inv_den[P + 1]; // GLL nodes and 1 / prod_{b != a} (x_a - x_b)
  };

  template <typename T, int P>
  struct PointEvaluateArgs
  {
    PointWalkArgs<P> w;
    uint32_t         n_dofs;
    const T         *u;
    T               *values, *gradients; // either may be null
  };
  static_assert(sizeof(PointEvaluateArgs<double, MAX_KERNEL_DEGREE>) <= KERNARG_LIMIT, "kernel arguments above the segment");

  template <typename T, int P>
  struct PointIntegrateArgs
  {
    PointWalkArgs<P> w;
    uint32_t         scatter_limit;       // rows below scatter_limit take the sums: the free rows
    const T         *values, *gradients;  // either may be null, not both
    T               *dst;                 // zeroed before the launch
  };
  static_assert(sizeof(PointIntegrateArgs<double, MAX_KERNEL_DEGREE>) <= KERNARG_LIMIT, "kernel arguments above the segment");

  // One function of the Lagrange basis on the GLL nodes and its derivative, from the differences d_b = x - x_b: the product rule
  // over the factors b != a, (val, der) <- (val d_b, der d_b + val), then both over den_a = prod_{b != a} (x_a - x_b).  No division
  // by a difference: exact at a node.  The loop is unrolled and b a constant, so d stays in registers; a may be a run-time value
  // that is uniform over the wave (the comparison is a uniform branch, inv_den[a] a scalar load of a kernel argument).
  template <int P>
  __device__ __forceinline__ void
  point_lagrange_one(const double (&d)[P + 1], const double (&inv_den)[P + 1], int a, double &val, double &der)
  {
    double v = 1.0, s = 0.0;
#pragma unroll
    for (int b = 0; b < P + 1; ++b)
      if (b != a)
        {
          s = s * d[b] + v;
          v *= d[b];
        }
    val = v * inv_den[a];
    der = s * inv_den[a];
  }
  // the whole basis at x, every loop unrolled and every index a constant: the arrays stay in registers
  template <int P>
  __device__ __forceinline__ void
  point_lagrange(const double (&nodes)[P + 1], const double (&inv_den)[P + 1], double x, double (&val)[P + 1], double (&der)[P + 1])
  {
    constexpr int N = P + 1;
    double        d[N];
#pragma unroll
    for (int b = 0; b < N; ++b)
      d[b] = x - nodes[b];
#pragma unroll
    for (int a = 0; a < N; ++a)
      point_lagrange_one<P>(d, inv_den, a, val[a], der[a]);
  }

  // K16.  CPW = dirichlet_cells_per_workgroup<P>() OCCUPIED leaves per workgroup pass, groups walked with a grid stride whose trip
  // count is uniform over the workgroup; which outputs are present is a kernel argument, so every branch around a barrier is uniform.
  // First half as cell_evaluate_kernel: gather through idx -> bufA;  C: bufA -> bufU -> bufA -> bufU, the conforming nodal tensor of
  // every leaf of the group in LDS (2 CPW (P+1)^3 doubles).  Then the threads stride over the sorted points of the group (a leaf may
  // hold far more than 256, the stride takes them all): each forms the 1D bases along x and y at xi in registers (4 (P+1) doubles) and
  // contracts the (P+1)^3 entries of its leaf plane by plane, x innermost, in a fixed order; the loop over the planes is NOT unrolled
  // (unrolled, the compiler hoists the (P+1)^3 LDS reads and spills from p = 5 on) and forms the two basis values of its plane along z
  // on the way, its counter being uniform over the wave.  The results are stored through perm to the caller's order.
  template <typename T, int P>
  __global__ void
  __launch_bounds__(256) point_evaluate_kernel(PointEvaluateArgs<T, P> a)
  {
    constexpr int N = P + 1, N2 = N * N, N3 = N2 * N, CPW = dirichlet_cells_per_workgroup<P>();
    static_assert(MASK_FACE_SHIFT == 3 && MASK_EDGE_SHIFT == 6, "hanging_pass reads the mask bits by number");
    static_assert((2 * CPW * N3 + 2 * N2 + CPW) * sizeof(double) + CPW * sizeof(uint32_t) <= 64 * 1024, "LDS above 64 KB");
    __shared__ double   bufU[CPW * N3], bufA[CPW * N3];
    __shared__ double   sI[2 * N2];
    __shared__ double   s_h[CPW];
    __shared__ uint32_t s_mask[CPW];
    const int           tid = threadIdx.x;
    const bool          with_value = a.values != nullptr, with_gradient = a.gradients != nullptr;
    for (int i = tid; i < N2; i += 256)
      {
        sI[i]      = a.w.I0[i];
        sI[N2 + i] = a.w.I1[i];
      }
    const uint32_t n_groups = (a.w.n_occupied + CPW - 1) / CPW;
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x)
      {
        const uint32_t o0     = grp * CPW;
        const int      n_here = (int)(a.w.n_occupied - o0 < (uint32_t)CPW ? a.w.n_occupied - o0 : (uint32_t)CPW); // leaves of this group
        const int      n_act  = n_here * N3;
        for (int t = tid; t < n_act; t += 256)
          {
            const int      cl = t / N3;
            const uint32_t gi = a.w.idx[(size_t)a.w.leaf[o0 + cl] * N3 + (t - cl * N3)];
            bufA[t]           = gi < a.n_dofs ? (double)a.u[gi] : 0.0;
          }
        if (tid < n_here)
          {
            const uint32_t ci = a.w.leaf[o0 + tid];
            s_h[tid]          = a.w.scale[2 * (size_t)ci + 1];
            s_mask[tid]       = a.w.mask[ci];
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
        // the conforming nodal values are in bufU; the sorted points of the group
        const uint32_t j_end = a.w.ptr[o0 + n_here];
        for (uint32_t j = a.w.ptr[o0] + tid; j < j_end; j += 256)
          {
            const uint32_t k  = a.w.perm[j];
            const int      cl = (int)(a.w.occ[j] - o0);
            double         lx[N], dx[N], ly[N], dy[N], zd[N];
            point_lagrange<P>(a.w.nodes, a.w.inv_den, a.w.ref[3 * (size_t)k], lx, dx);
            point_lagrange<P>(a.w.nodes, a.w.inv_den, a.w.ref[3 * (size_t)k + 1], ly, dy);
            const double z = a.w.ref[3 * (size_t)k + 2];
#pragma unroll
            for (int b = 0; b < N; ++b)
              zd[b] = z - a.w.nodes[b];
            const double *in = bufU + cl * N3;
            double        v = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
#pragma unroll 1
            for (int c = 0; c < N; ++c)
              {
                double lz_c, dz_c;
                point_lagrange_one<P>(zd, a.w.inv_den, c, lz_c, dz_c);
                double p0 = 0.0, p1 = 0.0, p2 = 0.0; // ly lx, ly dx, dy lx over the plane c
#pragma unroll
                for (int b = 0; b < N; ++b)
                  {
                    double r0 = 0.0, r1 = 0.0; // lx, dx over the line (b, c)
#pragma unroll
                    for (int i = 0; i < N; ++i)
                      {
                        const double w = in[(c * N + b) * N + i];
                        r0 += lx[i] * w;
                        r1 += dx[i] * w;
                      }
                    p0 += ly[b] * r0;
                    p1 += ly[b] * r1;
                    p2 += dy[b] * r0;
                  }
                v += lz_c * p0;
                gx += lz_c * p1;
                gy += lz_c * p2;
                gz += dz_c * p0;
              }
            if (with_value)
              a.values[k] = (T)v;
            if (with_gradient)
              {
                const double h                         = s_h[cl];
                a.gradients[k]                         = (T)(gx / h);
                a.gradients[(size_t)a.w.n_points + k]     = (T)(gy / h);
                a.gradients[2 * (size_t)a.w.n_points + k] = (T)(gz / h);
              }
          }
        __syncthreads(); // the next group's gather overwrites bufA, bufU and the scales of the leaves
      }
  }

  // points of a group whose 1D bases are staged in LDS at a time (K17)
  constexpr int POINT_BATCH = 64;

  // K17, the transpose, on the same walk.  LDS per group: two buffers X0, X1 of CPW (P+1)^3 doubles, and per point of a batch of
  // POINT_BATCH sorted points the six 1D bases and the four weights w, W_x / h, W_y / h, W_z / h (a missing input is weight 0).  Per
  // batch: thread (point, direction) forms the bases of one direction; then ONE thread per node of the group adds, in sorted order,
  // the points of the batch that lie in its leaf to the node's entry of X0: a fixed order and no LDS atomics.  After the last batch
  //   C^T: directions 2, 1, 0 (X0 -> X1 -> X0 -> the atomic add on the rows below scatter_limit).
  template <typename T, int P>
  __global__ void
  __launch_bounds__(256) point_integrate_kernel(PointIntegrateArgs<T, P> a)
  {
    constexpr int N = P + 1, N2 = N * N, N3 = N2 * N, CPW = dirichlet_cells_per_workgroup<P>(), B = POINT_BATCH;
    static_assert(MASK_FACE_SHIFT == 3 && MASK_EDGE_SHIFT == 6, "hanging_pass reads the mask bits by number");
    static_assert(3 * B <= 256, "one thread per (point, direction) of a batch");
    static_assert((2 * CPW * N3 + 2 * N2 + B * (6 * N + 4) + CPW) * sizeof(double) + (2 * CPW + 1) * sizeof(uint32_t) <= 64 * 1024, "LDS above 64 KB");
    __shared__ double   X0[CPW * N3], X1[CPW * N3];
    __shared__ double   sI[2 * N2];
    __shared__ double   sL[B * 3 * N], sD[B * 3 * N]; // [point][direction][a]
    __shared__ double   sW[B * 4];
    __shared__ double   s_h[CPW];
    __shared__ uint32_t s_mask[CPW], s_ptr[CPW + 1];
    const int           tid = threadIdx.x;
    const bool          with_value = a.values != nullptr, with_gradient = a.gradients != nullptr;
    for (int i = tid; i < N2; i += 256)
      {
        sI[i]      = a.w.I0[i];
        sI[N2 + i] = a.w.I1[i];
      }
    const uint32_t n_groups = (a.w.n_occupied + CPW - 1) / CPW;
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x)
      {
        const uint32_t o0     = grp * CPW;
        const int      n_here = (int)(a.w.n_occupied - o0 < (uint32_t)CPW ? a.w.n_occupied - o0 : (uint32_t)CPW); // leaves of this group
        const int      n_act  = n_here * N3;
        if (tid < n_here)
          {
            const uint32_t ci = a.w.leaf[o0 + tid];
            s_h[tid]          = a.w.scale[2 * (size_t)ci + 1];
            s_mask[tid]       = a.w.mask[ci];
          }
        if (tid <= n_here)
          s_ptr[tid] = a.w.ptr[o0 + tid];
        for (int t = tid; t < n_act; t += 256)
          X0[t] = 0.0;
        __syncthreads(); // (also: the interpolation matrices on the first trip)
        const uint32_t j_begin = s_ptr[0], j_end = s_ptr[n_here];
        for (uint32_t j0 = j_begin; j0 < j_end; j0 += B) // (uniform: the bounds are the group's)
          {
            const int n_batch = (int)(j_end - j0 < (uint32_t)B ? j_end - j0 : (uint32_t)B);
            if (tid < 3 * n_batch)
              {
                const int      q = tid / 3, d = tid - 3 * q;
                const uint32_t k = a.w.perm[j0 + q];
                double         l[N], g[N];
                point_lagrange<P>(a.w.nodes, a.w.inv_den, a.w.ref[3 * (size_t)k + d], l, g);
#pragma unroll
                for (int i = 0; i < N; ++i)
                  {
                    sL[(q * 3 + d) * N + i] = l[i];
                    sD[(q * 3 + d) * N + i] = g[i];
                  }
                const double h = s_h[a.w.occ[j0 + q] - o0];
                if (d == 0)
                  sW[4 * q] = with_value ? (double)a.values[k] : 0.0;
                sW[4 * q + 1 + d] = with_gradient ? (double)a.gradients[d * (size_t)a.w.n_points + k] / h : 0.0;
              }
            __syncthreads();
            for (int t = tid; t < n_act; t += 256)
              {
                const int      cl = t / N3, node = t - cl * N3, i0 = node % N, i1 = (node / N) % N, i2 = node / N2;
                const uint32_t lo = s_ptr[cl] > j0 ? s_ptr[cl] : j0, hi = s_ptr[cl + 1] < j0 + n_batch ? s_ptr[cl + 1] : j0 + n_batch;
                double         acc = X0[t];
                for (uint32_t j = lo; j < hi; ++j)
                  {
                    const int     q = (int)(j - j0);
                    const double *L = sL + q * 3 * N, *D = sD + q * 3 * N, *W = sW + 4 * q;
                    const double  lx = L[i0], ly = L[N + i1], lz = L[2 * N + i2];
                    acc += W[0] * (lx * ly * lz) + W[1] * (D[i0] * ly * lz) + W[2] * (lx * D[N + i1] * lz) + W[3] * (lx * ly * D[2 * N + i2]);
                  }
                X0[t] = acc;
              }
            __syncthreads(); // the next batch overwrites the bases
          }
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
          X1[t] = hanging_pass<double, P, 2, true>(X0 + base, sI, s_mask[cl], a0, a1, a2);
        });
        for_nodes([&](int t, int cl, int base, int a0, int a1, int a2) {
          X0[t] = hanging_pass<double, P, 1, true>(X1 + base, sI, s_mask[cl], a0, a1, a2);
        });
        // (its barrier: the next group overwrites the buffers, the scales and the point ranges of the leaves)
        for_nodes([&](int t, int cl, int base, int a0, int a1, int a2) {
          const double   v  = hanging_pass<double, P, 0, true>(X0 + base, sI, s_mask[cl], a0, a1, a2);
          const uint32_t gi = a.w.idx[(size_t)a.w.leaf[o0 + cl] * N3 + (t - base)];
          if (gi < a.scatter_limit)
            atomic_add(&a.dst[gi], (T)v);
        });
      }
  }
} // namespace mgamd
