// Kernels of the jump error indicator (DESIGN.md "Error indicator and refinement"):
//   eta_K^2 = (h_K / 24) sum_{F in dK} int_F r_F^2 dS,   r_F the jump of the normal flux a d_n u across F (or the boundary residual).
// K10 face_flux_kernel   one pass over all leaves: gather, C on the hanging faces and edges, then the nodal normal flux
//                        a d_d u at the (P+1)^2 nodes of each of the six faces, to the scratch array [cell][6][(P+1)^2]; on a
//                        boundary face the residual q_f - beta_f u - a d_n u itself (0 on Dirichlet faces and without q).
// K11 flux_jump_kernel   per leaf: its own six face fluxes and, through the neighbour table, those of its neighbours; I0 / I1
//                        on the coarse side where the levels differ; int_F r^2 = h_F^2 r^T (M (x) M) r; eta_K.
// All arithmetic after the gather is double for both number types: an FP32 vector is converted at the load.  Only the entries of
// the vector at free and Dirichlet DoFs are read (the index table resolves hanging entities to their parents).
// A face has N2 = (P+1)^2 nodes, the lower of its two in-face axes (u < v) fastest: node au + N av.  Both cells at a face use the
// same derivative direction d, so the jump is a plain difference.
#pragma once
#include "kernels_boundary.hpp"
#include "octree.hpp"

namespace mgamd
{
  template <typename T, int P>
  struct FaceFluxArgs
  {
    const uint32_t *idx;   // [n_cells][N3], Dirichlet DoFs with their real index
    const uint16_t *mask;  // [n_cells]
    const double   *scale; // [n_cells][2]: a / h, h
    const uint8_t  *code;  // [n_cells][6], Tria::face_neighbours
    uint32_t        n_cells, n_dofs;
    const T        *u;
    double         *flux; // [n_cells][6][N2]
    double          D[2 * (P + 1)], I0[(P + 1) * (P + 1)], I1[(P + 1) * (P + 1)];
    double          q[6], beta[6];
    uint32_t        natural; // bit f: boundary face f has a residual (q given and the face is not Dirichlet)
  };
  static_assert(sizeof(FaceFluxArgs<double, MAX_KERNEL_DEGREE>) <= KERNARG_LIMIT, "kernel arguments above the segment");

  // Packing as in dirichlet_lift_kernel: CPW = max(1, 256 / N3) cells per workgroup pass, one thread per node (two at P = 6, 7);
  // the three interpolation passes ping-pong between two LDS buffers.  Then one item per face node of the group's cells: the
  // scratch rows of a group are contiguous, so the stores are coalesced.
  template <typename T, int P>
  __global__ void
  __launch_bounds__(256) face_flux_kernel(FaceFluxArgs<T, P> a)
  {
    constexpr int N = P + 1, N2 = N * N, N3 = N2 * N, CPW = dirichlet_cells_per_workgroup<P>(), NODES = CPW * N3;
    static_assert(MASK_FACE_SHIFT == 3 && MASK_EDGE_SHIFT == 6, "hanging_pass reads the mask bits by number");
    __shared__ double   bufX[NODES], bufU[NODES], sD[2 * N], sI[2 * N2];
    __shared__ double   s_ah[CPW];
    __shared__ uint32_t s_mask[CPW];
    const int           tid = threadIdx.x;
    for (int i = tid; i < N2; i += 256)
      {
        sI[i]      = a.I0[i];
        sI[N2 + i] = a.I1[i];
      }
    if (tid < 2 * N)
      sD[tid] = a.D[tid];
    const uint32_t n_groups = (a.n_cells + CPW - 1) / CPW;
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x)
      {
        const uint32_t cell0   = grp * CPW;
        const int      n_here  = (int)(a.n_cells - cell0 < (uint32_t)CPW ? a.n_cells - cell0 : (uint32_t)CPW); // cells of this group
        const int      n_act   = n_here * N3;
        for (int t = tid; t < n_act; t += 256)
          {
            const uint32_t gi = a.idx[(size_t)cell0 * N3 + t];
            bufX[t]           = gi < a.n_dofs ? (double)a.u[gi] : 0.0;
          }
        if (tid < n_here)
          {
            s_ah[tid]   = a.scale[2 * (size_t)(cell0 + tid)];
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
          bufU[t] = hanging_pass<double, P, 0, false>(bufX + base, sI, s_mask[cl], a0, a1, a2);
        });
        for_nodes([&](int t, int cl, int base, int a0, int a1, int a2) {
          bufX[t] = hanging_pass<double, P, 1, false>(bufU + base, sI, s_mask[cl], a0, a1, a2);
        });
        for_nodes([&](int t, int cl, int base, int a0, int a1, int a2) {
          bufU[t] = hanging_pass<double, P, 2, false>(bufX + base, sI, s_mask[cl], a0, a1, a2);
        });
        // the conforming nodal values are in bufU: the six faces
        const int n_items = n_here * 6 * N2;
        for (int it = tid; it < n_items; it += 256)
          {
            const int cl = it / (6 * N2), r = it - cl * 6 * N2, f = r / N2, t = r - f * N2;
            const int d = f >> 1, side = f & 1;
            const int su = d == 0 ? N : 1, sv = d == 2 ? N : N2, sd = d == 0 ? 1 : (d == 1 ? N : N2);
            const int base = cl * N3 + (t % N) * su + (t / N) * sv;
            double    g    = 0.0;
#pragma unroll
            for (int m = 0; m < N; ++m)
              g += sD[side * N + m] * bufU[base + m * sd];
            double v = s_ah[cl] * g; // a d_d u
            if (a.code[(size_t)(cell0 + cl) * 6 + f] == Tria::NB_BOUNDARY)
              v = ((a.natural >> f) & 1u) ? a.q[f] - a.beta[f] * bufU[base + side * P * sd] - (side ? v : -v) : 0.0;
            a.flux[(size_t)cell0 * 6 * N2 + it] = v;
          }
        __syncthreads(); // the next group's gather overwrites bufX and the scales; its passes overwrite bufU
      }
  }

  template <typename T, int P>
  struct FluxJumpArgs
  {
    const double   *flux;  // [n_cells][6][N2], written by face_flux_kernel
    const uint8_t  *code;  // [n_cells][6]
    const uint32_t *nbr;   // [n_cells][6][4]
    const double   *scale; // [n_cells][2]: a / h, h
    uint32_t        n_cells;
    double         *eta; // [n_cells]
    double          M[(P + 1) * (P + 1)], I0[(P + 1) * (P + 1)], I1[(P + 1) * (P + 1)];
  };
  static_assert(sizeof(FluxJumpArgs<double, MAX_KERNEL_DEGREE>) <= KERNARG_LIMIT, "kernel arguments above the segment");

  template <int P>
  constexpr int
  jump_cells_per_workgroup()
  {
    return 256 / ((P + 1) * (P + 1));
  }

  // CPB = 256 / N2 leaves per workgroup pass (64, 28, 16, 10, 7, 5, 4 for P = 1..7), one thread per face node.  The loop over the
  // six faces and the four quarters of a face is uniform over the workgroup (a pair that no leaf of the pass needs is skipped by a
  // workgroup vote), so every barrier is reached by all threads.  Per pair, on the nodes of one (sub-)face, sum-factorised:
  //   A = coarse side's flux       T = I_c1 along u        restricted = I_c2 along v        r = fine side - restricted
  //   A = r                        T = M along u           w = M along v                    partial = r w
  // and thread 0 of the leaf adds the N2 partials in node order.  eta_K is written by that one thread, faces and quarters in
  // ascending order: no atomics, two calls give the same bits.  T is a tag: it keeps the symbols of the two number types apart.
  template <typename T, int P>
  __global__ void
  __launch_bounds__(256) flux_jump_kernel(FluxJumpArgs<T, P> a)
  {
    constexpr int N = P + 1, N2 = N * N, CPB = jump_cells_per_workgroup<P>();
    __shared__ double bufA[256], bufT[256], bufP[256], sM[N2], sI[2 * N2];
    const int         tid = threadIdx.x, cl = tid / N2, t = tid - cl * N2, au = t % N, av = t / N, row = cl * N2;
    for (int i = tid; i < N2; i += 256)
      {
        sM[i]      = a.M[i];
        sI[i]      = a.I0[i];
        sI[N2 + i] = a.I1[i];
      }
    __syncthreads();
    const uint32_t n_groups = (a.n_cells + CPB - 1) / CPB;
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x)
      {
        const uint32_t cell  = grp * CPB + cl;
        const bool     valid = cl < CPB && cell < a.n_cells;
        const double   h     = valid ? a.scale[2 * (size_t)cell + 1] : 0.0;
        double         acc   = 0.0;
        for (int f = 0; f < 6; ++f)
          {
            const int       c   = valid ? (int)a.code[(size_t)cell * 6 + f] : -1;
            const uint32_t *nb  = a.nbr + ((size_t)cell * 6 + f) * 4; // (dereferenced for valid leaves only)
            const double    own_t = valid ? a.flux[((size_t)cell * 6 + f) * N2 + t] : 0.0; // this leaf's flux at the thread's node
            for (int s = 0; s < 4; ++s)
              {
                const bool active = valid && (s == 0 || c == Tria::NB_FINER);
                if (!__syncthreads_or(active))
                  continue;
                const bool coarser = active && c >= Tria::NB_COARSER && c < Tria::NB_FINER, finer = active && c == Tria::NB_FINER;
                const int  c1 = coarser ? ((c - Tria::NB_COARSER) & 1) : (s & 1), c2 = coarser ? ((c - Tria::NB_COARSER) >> 1) : (s >> 1);
                // the opposite face of the neighbour that this (sub-)face is shared with
                const double *other = (active && c != Tria::NB_BOUNDARY) ? a.flux + ((size_t)nb[finer ? s : 0] * 6 + (f ^ 1)) * N2 : nullptr;
                bufA[tid] = coarser ? other[t] : (finer ? own_t : 0.0);
                __syncthreads();
                double v = 0.0;
                if (coarser || finer)
                  {
#pragma unroll
                    for (int b = 0; b < N; ++b)
                      v += sI[c1 * N2 + au * N + b] * bufA[row + av * N + b];
                  }
                bufT[tid] = v;
                __syncthreads();
                double r = 0.0;
                if (coarser || finer)
                  {
                    double res = 0.0;
#pragma unroll
                    for (int b = 0; b < N; ++b)
                      res += sI[c2 * N2 + av * N + b] * bufT[row + b * N + au];
                    r = (coarser ? own_t : other[t]) - res;
                  }
                else if (active)
                  r = c == Tria::NB_BOUNDARY ? own_t : own_t - other[t];
                bufA[tid] = r;
                __syncthreads();
                v = 0.0;
                if (active)
                  {
#pragma unroll
                    for (int b = 0; b < N; ++b)
                      v += sM[au * N + b] * bufA[row + av * N + b];
                  }
                bufT[tid] = v;
                __syncthreads();
                v = 0.0;
                if (active)
                  {
#pragma unroll
                    for (int b = 0; b < N; ++b)
                      v += sM[av * N + b] * bufT[row + b * N + au];
                  }
                bufP[tid] = r * v;
                __syncthreads();
                if (active && t == 0)
                  {
                    double sum = 0.0;
                    for (int b = 0; b < N2; ++b)
                      sum += bufP[row + b];
                    const double hf = finer ? 0.5 * h : h;
                    acc += hf * hf * sum;
                  }
              }
          }
        if (valid && t == 0)
          a.eta[cell] = sqrt(fmax(h / 24.0 * acc, 0.0));
      }
  }
} // namespace mgamd
