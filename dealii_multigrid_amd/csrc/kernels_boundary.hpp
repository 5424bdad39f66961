// Kernels of the non-zero Dirichlet data (DESIGN.md "Dirichlet data"): the lifting  dst += alpha C^T (K_a + s sigma M) C g^  over the
// cells that gather a Dirichlet DoF, and the interpolation of the hanging DoFs from their parents.
#pragma once
#include "kernels_common.hpp"

namespace mgamd
{
  // One entry of the cell table (level_tables.hpp, DirichletCells) is one cell with N3 = (P+1)^3 nodes: gather g on the Dirichlet
  // DoFs (0 on every other node), C on the flagged hanging faces and edges, the sum-factorised cell operator
  //   a h (K (x) M (x) M + M (x) K (x) M + M (x) M (x) K) + s sigma h^3 M (x) M (x) M,
  // C^T, scale alpha, atomic add on the rows below scatter_limit (the free rows).
  // Packing: a workgroup of 256 threads holds CPW = max(1, 256 / N3) cells at a time (32, 9, 4, 2, 1, 1, 1 for P = 1..7), one thread
  // per node where the cells fit and two nodes per thread at P = 6, 7 (343 and 512 nodes); every pass reads one LDS buffer and
  // writes another, so no thread keeps values of its own between passes.  Four buffers of one value per node: the three
  // interpolation passes ping-pong between two of them, the operator needs all four:
  //   x:  U -> X = M_x U, V = K_x U        y:  X, V -> U = M_y X, W = M_y V + K_y X        z:  U, W -> X = a h (M_z W + K_z U) + m M_z U
  // with m = s sigma h^3.
  // The groups of cells are walked with a grid stride; the trip count is uniform over the workgroup, so the barriers are safe.
  template <typename T, int P>
  struct DirichletLiftArgs
  {
    const uint32_t *idx;   // [n_cells][N3], Dirichlet DoFs with their real index
    const uint16_t *mask;  // [n_cells]
    const double   *scale; // [n_cells][2]: a h, h
    uint32_t        n_cells;
    T               K[(P + 1) * (P + 1)], M[(P + 1) * (P + 1)], I0[(P + 1) * (P + 1)], I1[(P + 1) * (P + 1)];
    const T        *g;
    T              *dst;
    uint32_t        dirichlet_begin, dirichlet_end, scatter_limit;
    T               alpha, sigma; // sigma = 0: stiffness only
  };
  static_assert(sizeof(DirichletLiftArgs<double, MAX_KERNEL_DEGREE>) <= KERNARG_LIMIT, "kernel arguments above the segment");

  template <int P>
  constexpr int
  dirichlet_cells_per_workgroup()
  {
    return 256 / ((P + 1) * (P + 1) * (P + 1)) > 0 ? 256 / ((P + 1) * (P + 1) * (P + 1)) : 1;
  }

  // one hanging-node pass along direction D on node (a0, a1, a2) of a cell: the interpolated value on a flagged line, the value
  // itself elsewhere (level_tables.hpp interpolate_hanging, one direction)
  template <typename T, int P, int D, bool TRANSPOSE>
  __device__ __forceinline__ T
  hanging_pass(const T *in, const T *sI, uint32_t mask, int a0, int a1, int a2)
  {
    constexpr int N = P + 1, N2 = N * N;
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    const int     a[3]  = {a0, a1, a2};
    const int     st[3] = {1, N, N2};
    const int     node  = a0 + a1 * N + a2 * N2;
    const bool    on_e = a[E] == (int)((mask >> E) & 1u) * P, on_f = a[F] == (int)((mask >> F) & 1u) * P;
    const bool    flagged = (((mask >> (3 + E)) & 1u) && on_e) || (((mask >> (3 + F)) & 1u) && on_f) || (((mask >> (6 + D)) & 1u) && on_e && on_f);
    if (!flagged)
      return in[node];
    const T *Ic   = sI + ((mask >> D) & 1u) * N2;
    const T *line = in + node - a[D] * st[D];
    T        v    = T(0);
#pragma unroll
    for (int b = 0; b < N; ++b)
      v += (TRANSPOSE ? Ic[b * N + a[D]] : Ic[a[D] * N + b]) * line[b * st[D]];
    return v;
  }

  template <typename T, int P>
  __global__ void
  __launch_bounds__(256) dirichlet_lift_kernel(DirichletLiftArgs<T, P> a)
  {
    constexpr int N = P + 1, N2 = N * N, N3 = N2 * N, CPW = dirichlet_cells_per_workgroup<P>(), NODES = CPW * N3;
    static_assert(MASK_FACE_SHIFT == 3 && MASK_EDGE_SHIFT == 6, "hanging_pass reads the mask bits by number");
    __shared__ T        bufX[NODES], bufU[NODES], bufV[NODES], bufW[NODES], sK[N2], sM[N2], sI[2 * N2];
    __shared__ T        s_ah[CPW], s_m[CPW];
    __shared__ uint32_t s_mask[CPW];
    const int           tid = threadIdx.x;
    for (int i = tid; i < N2; i += 256)
      {
        sK[i]      = a.K[i];
        sM[i]      = a.M[i];
        sI[i]      = a.I0[i];
        sI[N2 + i] = a.I1[i];
      }
    const uint32_t n_groups = (a.n_cells + CPW - 1) / CPW;
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x)
      {
        const uint32_t cell0 = grp * CPW;
        const int      n_act = (int)(a.n_cells - cell0 < (uint32_t)CPW ? a.n_cells - cell0 : (uint32_t)CPW) * N3; // nodes of this group's cells
        // gather
        for (int t = tid; t < n_act; t += 256)
          {
            const uint32_t gi = a.idx[(size_t)cell0 * N3 + t];
            bufX[t]           = (gi >= a.dirichlet_begin && gi < a.dirichlet_end) ? a.g[gi] : T(0);
          }
        if (tid < CPW && cell0 + tid < a.n_cells)
          {
            const double ah = a.scale[2 * (size_t)(cell0 + tid)], h = a.scale[2 * (size_t)(cell0 + tid) + 1];
            s_ah[tid]       = (T)ah;
            s_m[tid]        = (T)((double)a.sigma * h * h * h);
            s_mask[tid]     = a.mask[cell0 + tid];
          }
        __syncthreads();
        // body(t, cl, base, node, a0, a1, a2) on every node t of the group's cells (cell cl of the group, its buffers at base), then
        // the barrier before the next pass
        auto for_nodes = [&](auto body) {
          for (int t = tid; t < n_act; t += 256)
            {
              const int cl = t / N3, node = t - cl * N3;
              body(t, cl, cl * N3, node, node % N, (node / N) % N, node / N2);
            }
          __syncthreads();
        };
        // C: directions 0, 1, 2
        for_nodes([&](int t, int cl, int base, int, int a0, int a1, int a2) {
          bufU[t] = hanging_pass<T, P, 0, false>(bufX + base, sI, s_mask[cl], a0, a1, a2);
        });
        for_nodes([&](int t, int cl, int base, int, int a0, int a1, int a2) {
          bufX[t] = hanging_pass<T, P, 1, false>(bufU + base, sI, s_mask[cl], a0, a1, a2);
        });
        for_nodes([&](int t, int cl, int base, int, int a0, int a1, int a2) {
          bufU[t] = hanging_pass<T, P, 2, false>(bufX + base, sI, s_mask[cl], a0, a1, a2);
        });
        // the cell operator on bufU.  Along x: bufX = M x, bufV = K x
        for_nodes([&](int t, int, int base, int node, int a0, int, int) {
          const T *line = bufU + base + node - a0;
          T        m = T(0), k = T(0);
#pragma unroll
          for (int b = 0; b < N; ++b)
            {
              m += sM[a0 * N + b] * line[b];
              k += sK[a0 * N + b] * line[b];
            }
          bufX[t] = m;
          bufV[t] = k;
        });
        // along y: bufU = M M x, bufW = (M K + K M) x
        for_nodes([&](int t, int, int base, int node, int, int a1, int) {
          const int off = base + node - a1 * N;
          T         mm = T(0), w = T(0);
#pragma unroll
          for (int b = 0; b < N; ++b)
            {
              mm += sM[a1 * N + b] * bufX[off + b * N];
              w += sM[a1 * N + b] * bufV[off + b * N] + sK[a1 * N + b] * bufX[off + b * N];
            }
          bufU[t] = mm;
          bufW[t] = w;
        });
        // along z, with the scales of the cell
        for_nodes([&](int t, int cl, int base, int node, int, int, int a2) {
          const int off = base + node - a2 * N2;
          T         st = T(0), ms = T(0);
#pragma unroll
          for (int b = 0; b < N; ++b)
            {
              st += sM[a2 * N + b] * bufW[off + b * N2] + sK[a2 * N + b] * bufU[off + b * N2];
              ms += sM[a2 * N + b] * bufU[off + b * N2];
            }
          bufX[t] = s_ah[cl] * st + s_m[cl] * ms;
        });
        // C^T: directions 2, 1, 0, the last one into the destination
        for_nodes([&](int t, int cl, int base, int, int a0, int a1, int a2) {
          bufU[t] = hanging_pass<T, P, 2, true>(bufX + base, sI, s_mask[cl], a0, a1, a2);
        });
        for_nodes([&](int t, int cl, int base, int, int a0, int a1, int a2) {
          bufX[t] = hanging_pass<T, P, 1, true>(bufU + base, sI, s_mask[cl], a0, a1, a2);
        });
        // (its barrier: the next group's gather overwrites bufX and the scales of the cells)
        for_nodes([&](int t, int cl, int base, int, int a0, int a1, int a2) {
          const T        v  = hanging_pass<T, P, 0, true>(bufX + base, sI, s_mask[cl], a0, a1, a2);
          const uint32_t gi = a.idx[(size_t)cell0 * N3 + t];
          if (gi < a.scatter_limit)
            atomic_add(&a.dst[gi], a.alpha * v);
        });
      }
  }

  // x[i] = g[i] on the Dirichlet range
  template <typename T>
  __global__ void
  __launch_bounds__(256) dirichlet_copy_kernel(T *x, const T *g, uint32_t begin, uint32_t end)
  {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride)
      x[i] = g[i];
  }
  // the hanging DoFs from their parents (LevelTables::hanging_rows): one thread per hanging DoF; a DoF without entries is left alone
  template <typename T>
  __global__ void
  __launch_bounds__(256) hanging_rows_kernel(T *x, const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ col,
                                             const double *__restrict__ val, uint32_t first_hanging, uint32_t n_rows)
  {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride)
      {
        const uint32_t b = ptr[r], e = ptr[r + 1];
        if (b == e)
          continue;
        double s = 0.0;
        for (uint32_t k = b; k < e; ++k)
          s += val[k] * (double)x[col[k]];
        x[first_hanging + r] = (T)s;
      }
  }
} // namespace mgamd
