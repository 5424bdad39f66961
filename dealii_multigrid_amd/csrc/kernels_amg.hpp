#pragma once
#include "kernels_common.hpp"
#include "kernels_vector.hpp"

// ------------------------------------------------------------------------------------------------
// K7  CSR kernels of the algebraic coarse solver (amg.hpp; runtime.hip AmgCycle): one row per group of LANES adjacent lanes
// (the level matrices have 27-70 entries per row), fused with the vector update they feed; one body, two entry points
// (all rows / a range of rows):
//   SPMV_PLAIN   y = A x                      SPMV_ADD      y += A x  (prolongation)
//   SPMV_RESID   y = b - A x                  SPMV_CHEB     y = x + f1 (x - xold) + f2 dinv (b - A x)   (xold may be null)
//   SPMV_DOT     y = A x and, in the same pass, the block partials of x . y (square matrices, whole-matrix launches, FP64): one
//                double per block in `partial`, summed by vec_dot_final_kernel; no atomics, the same sum on every run
// K8  the same products for LONG rows (the assembled fine-level matrix at degree 2-4: rows of 100-1500 entries; runtime.hip
// AssembledMatrix): one wave64 per row, 4 rows per block, the epilogues of K7.
// ------------------------------------------------------------------------------------------------
namespace mgamd
{
  enum SpmvMode
  {
    SPMV_PLAIN = 0,
    SPMV_ADD   = 1,
    SPMV_RESID = 2,
    SPMV_CHEB  = 3,
    SPMV_DOT   = 4
  };
  // what K7 and K8 do with the finished sum s of a row (one lane per row calls it); SPMV_DOT: returns the row's term of x . y
  template <typename T, int MODE>
  __device__ __forceinline__ double
  csr_spmv_epilogue(uint32_t row, T s, const T *__restrict__ x, T *__restrict__ y, const T *__restrict__ b, const T *__restrict__ xold,
                    const T *__restrict__ dinv, T f1, T f2)
  {
    if (MODE == SPMV_PLAIN)
      y[row] = s;
    else if (MODE == SPMV_ADD)
      y[row] += s;
    else if (MODE == SPMV_RESID)
      y[row] = b[row] - s;
    else if (MODE == SPMV_CHEB)
      {
        const T xv = x[row], xo = xold ? xold[row] : T(0);
        y[row]     = xv + f1 * (xv - xo) + f2 * dinv[row] * (b[row] - s);
      }
    else
      {
        y[row] = s;
        return (double)x[row] * (double)s;
      }
    return 0.0;
  }
  // SPMV_DOT: the block's sum of the lanes' terms (wave reduce, then the four waves in a fixed order) -> partial[block]
  __device__ __forceinline__ void
  csr_spmv_store_block_dot(double dot, double *__restrict__ partial)
  {
    __shared__ double wsum[4];
    dot = wave_reduce_sum(dot);
    if ((threadIdx.x & 63) == 0)
      wsum[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0)
      partial[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  }
  // the rows [row_begin, row_end) of the product: the one body of both entry points below
  template <typename T, int MODE, int LANES>
  __device__ __forceinline__ void
  csr_spmv_rows(uint32_t row_begin, uint32_t row_end, const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ col,
                const T *__restrict__ val, const T *__restrict__ x, T *__restrict__ y, const T *__restrict__ b,
                const T *__restrict__ xold, const T *__restrict__ dinv, T f1, T f2, double *__restrict__ partial = nullptr)
  {
    double         dot            = 0.0;
    const uint32_t rows_per_block = 256 / LANES;
    const uint32_t sub = threadIdx.x % LANES, lrow = threadIdx.x / LANES;
    for (uint32_t row0 = row_begin + blockIdx.x * rows_per_block; row0 < row_end; row0 += gridDim.x * rows_per_block)
      {
        const uint32_t row = row0 + lrow;
        T              s   = T(0);
        if (row < row_end)
          {
            const uint32_t e = ptr[row + 1];
            for (uint32_t k = ptr[row] + sub; k < e; k += LANES)
              s += val[k] * x[col[k]];
          }
#pragma unroll
        for (int off = LANES / 2; off > 0; off >>= 1)
          s += __shfl_down(s, off, LANES);
        if (row < row_end && sub == 0)
          dot += csr_spmv_epilogue<T, MODE>(row, s, x, y, b, xold, dinv, f1, f2);
      }
    if constexpr (MODE == SPMV_DOT)
      csr_spmv_store_block_dot(dot, partial);
  }

  // all rows: the products of a whole level (one rank; the replicated levels of a sharded cycle) and mgamd_debug_csr_spmv
  template <typename T, int MODE, int LANES>
  __global__ void
  __launch_bounds__(256) csr_spmv_kernel(uint32_t n_rows, const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ col,
                                         const T *__restrict__ val, const T *__restrict__ x, T *__restrict__ y, const T *__restrict__ b,
                                         const T *__restrict__ xold, const T *__restrict__ dinv, T f1, T f2, double *__restrict__ partial)
  {
    csr_spmv_rows<T, MODE, LANES>(0, n_rows, ptr, col, val, x, y, b, xold, dinv, f1, f2, partial);
  }

  // K8: one wave64 per row, 4 rows per block, grid-stride over the rows.  Lane l takes the entries begin + l + 64 j, so one wave
  // instruction reads 512 contiguous bytes of val and 256 of col.  Four entries per lane and pass are loaded before the first is
  // used (4 x (8 + 4) B of matrix and 4 gathered x per lane in flight); the last, partial pass loads clamped indices and drops
  // the products past the end, so that its loads are as independent as the full pass's.  A lane adds its entry j to partial sum
  // j mod 4; the four are combined as (s0 + s1) + (s2 + s3), then the 64 lanes by __shfl_down: the order of additions in a row
  // depends on the row alone, not on the grid.
  template <typename T, int MODE>
  __global__ void
  __launch_bounds__(256) csr_spmv_wave_kernel(uint32_t n_rows, const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ col,
                                              const T *__restrict__ val, const T *__restrict__ x, T *__restrict__ y, const T *__restrict__ b,
                                              const T *__restrict__ xold, const T *__restrict__ dinv, T f1, T f2, double *__restrict__ partial)
  {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double         dot  = 0.0;
    for (uint32_t row0 = blockIdx.x * 4; row0 < n_rows; row0 += gridDim.x * 4)
      {
        const uint32_t row = row0 + wave;
        T              s   = T(0);
        if (row < n_rows)
          {
            const uint32_t e = ptr[row + 1];
            uint32_t       k = ptr[row] + lane;
            T              s0 = T(0), s1 = T(0), s2 = T(0), s3 = T(0);
            for (; k < e && e - k > 192; k += 256)
              {
                const uint32_t c0 = col[k], c1 = col[k + 64], c2 = col[k + 128], c3 = col[k + 192];
                const T        v0 = val[k], v1 = val[k + 64], v2 = val[k + 128], v3 = val[k + 192];
                const T        x0 = x[c0], x1 = x[c1], x2 = x[c2], x3 = x[c3];
                s0 += v0 * x0;
                s1 += v1 * x1;
                s2 += v2 * x2;
                s3 += v3 * x3;
              }
            if (k < e)
              {
                const uint32_t left = e - k; // 1 ... 192: at most three more entries of this lane
                const bool     p1 = left > 64, p2 = left > 128;
                const uint32_t k1 = p1 ? k + 64 : k, k2 = p2 ? k + 128 : k;
                const uint32_t c0 = col[k], c1 = col[k1], c2 = col[k2];
                const T        v0 = val[k], v1 = val[k1], v2 = val[k2];
                const T        x0 = x[c0], x1 = x[c1], x2 = x[c2];
                s0 += v0 * x0;
                s1 += p1 ? v1 * x1 : T(0);
                s2 += p2 ? v2 * x2 : T(0);
              }
            s = (s0 + s1) + (s2 + s3);
          }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
          s += __shfl_down(s, off, 64);
        if (row < n_rows && lane == 0)
          dot += csr_spmv_epilogue<T, MODE>(row, s, x, y, b, xold, dinv, f1, f2);
      }
    if constexpr (MODE == SPMV_DOT)
      csr_spmv_store_block_dot(dot, partial);
  }

  // The rows [row_begin, row_end) only: a sharded level of the cycle (runtime.hip AmgCycle) launches its interior rows, imports the
  // ghost columns underneath them, then launches the boundary rows.  The same lanes per row and the same order of additions within
  // a row as csr_spmv_kernel, so a row's result does not depend on how the rows are cut.
  template <typename T, int MODE, int LANES>
  __global__ void
  __launch_bounds__(256) csr_spmv_range_kernel(uint32_t row_begin, uint32_t row_end, const uint32_t *__restrict__ ptr,
                                               const uint32_t *__restrict__ col, const T *__restrict__ val, const T *__restrict__ x,
                                               T *__restrict__ y, const T *__restrict__ b, const T *__restrict__ xold,
                                               const T *__restrict__ dinv, T f1, T f2)
  {
    csr_spmv_rows<T, MODE, LANES>(row_begin, row_end, ptr, col, val, x, y, b, xold, dinv, f1, f2);
  }

  // owned entries -> send buffer of the ghost import (idx: local row per send slot; 0xFFFFFFFF: padding of the pair's segment)
  template <typename T>
  __global__ void
  amg_pack_ghosts_kernel(T *__restrict__ send, const T *__restrict__ v, const uint32_t *__restrict__ idx, uint32_t n)
  {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
      {
        const uint32_t j = idx[i];
        send[i]          = j == 0xFFFFFFFFu ? T(0) : v[j];
      }
  }
  // level 0, entry: rows of the AMG vector <- entries of the geometric vector (local [I|T|D|H] numbering); a null index: identity
  template <typename T>
  __global__ void
  amg_level0_gather_kernel(T *__restrict__ amg, const uint32_t *__restrict__ amg_idx, const T *__restrict__ geo,
                           const uint32_t *__restrict__ geo_idx, uint32_t n)
  {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
      amg[amg_idx ? amg_idx[i] : i] = geo[geo_idx[i]];
  }
  // level 0, exit: entries of the geometric vector <- rows of the AMG result
  template <typename T>
  __global__ void
  amg_level0_scatter_kernel(T *__restrict__ geo, const uint32_t *__restrict__ geo_idx, const T *__restrict__ amg,
                            const uint32_t *__restrict__ amg_idx, uint32_t n)
  {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
      geo[geo_idx[i]] = amg[amg_idx ? amg_idx[i] : i];
  }
} // namespace mgamd

