#pragma once
#include "kernels_common.hpp"

// ------------------------------------------------------------------------------------------------
// K7  CSR kernels of the algebraic coarse solver (amg.hpp; runtime.hip AmgCycle): one row per group of LANES adjacent lanes
// (the level matrices have 27-70 entries per row), fused with the vector update they feed; one body, two entry points
// (all rows / a range of rows):
//   SPMV_PLAIN   y = A x                      SPMV_ADD      y += A x  (prolongation)
//   SPMV_RESID   y = b - A x                  SPMV_CHEB     y = x + f1 (x - xold) + f2 dinv (b - A x)   (xold may be null)
// ------------------------------------------------------------------------------------------------
namespace mgamd
{
  enum SpmvMode
  {
    SPMV_PLAIN = 0,
    SPMV_ADD   = 1,
    SPMV_RESID = 2,
    SPMV_CHEB  = 3
  };
  // the rows [row_begin, row_end) of the product: the one body of both entry points below
  template <typename T, int MODE, int LANES>
  __device__ __forceinline__ void
  csr_spmv_rows(uint32_t row_begin, uint32_t row_end, const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ col,
                const T *__restrict__ val, const T *__restrict__ x, T *__restrict__ y, const T *__restrict__ b,
                const T *__restrict__ xold, const T *__restrict__ dinv, T f1, T f2)
  {
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
          {
            if (MODE == SPMV_PLAIN)
              y[row] = s;
            else if (MODE == SPMV_ADD)
              y[row] += s;
            else if (MODE == SPMV_RESID)
              y[row] = b[row] - s;
            else
              {
                const T xv = x[row], xo = xold ? xold[row] : T(0);
                y[row]     = xv + f1 * (xv - xo) + f2 * dinv[row] * (b[row] - s);
              }
          }
      }
  }

  // all rows: the products of a whole level (one rank; the replicated levels of a sharded cycle) and mgamd_debug_csr_spmv
  template <typename T, int MODE, int LANES>
  __global__ void
  __launch_bounds__(256) csr_spmv_kernel(uint32_t n_rows, const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ col,
                                         const T *__restrict__ val, const T *__restrict__ x, T *__restrict__ y, const T *__restrict__ b,
                                         const T *__restrict__ xold, const T *__restrict__ dinv, T f1, T f2)
  {
    csr_spmv_rows<T, MODE, LANES>(0, n_rows, ptr, col, val, x, y, b, xold, dinv, f1, f2);
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

