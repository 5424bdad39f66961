// HIP kernels for gfx950 (CDNA4, wave64).  Hand-written for MI355X: no hipify, no dual paths.
//
// K1  lattice_apply_kernel   the level operator (ref:include/operator.h:152-183,461-472) on one SLOT
//                            (brick of B^3 cells or single cell) per work-item group: node lattice
//                            of N = p*B+1 points per direction staged in LDS, three 1D sweeps with
//                            one thread per lattice line and the line in registers, epilogue fused
//                            (vmult / residual / Chebyshev update) for slot-interior DoFs, partial
//                            sums of shell DoFs atomically added to the small 'tail' accumulator.
// K1c cell_cluster_apply_kernel  the same operator on single cells at p = 1: one cell per thread, nodes deduplicated per
//                            256-cell cluster in LDS (one load and one global atomic per distinct node).
// K2  tail_kernel            same epilogue for the tail + constrained DoFs (identity rows).
// K3  lattice_diag_kernel    diagonal of C^T K C (ref:include/operator.h:228-242).
// K4  prolongate/restrict    MGTwoLevelTransfer embeddings (ref:multigrid_throughput.cc:1600-1604).
// K5  vector kernels         set/copy/axpy/sadd/scaled pointwise product/dot.
// K6  dense_matvec_kernel    coarse-grid direct solve (precomputed inverse).
//
// Because every cell is a cube (ref:include/grid_generator.h, MappingQ1) the brick operator is
//   A_brick = h (K (x) M (x) M + M (x) K (x) M + M (x) M (x) K)
// with 1D matrices assembled over the B cells of a lattice line; each 1D product is evaluated
// cell by cell with the dense (p+1)^2 reference matrices held in SGPRs (kernel arguments).
// The same kernels in MODE_MASS apply the mass matrix h^3 M (x) M (x) M of the brick instead: three mass products on one lattice
// (mass_sweeps), zero rows on constrained DoFs.
//
// K7  csr_spmv_kernel        CSR products of the algebraic coarse solver, fused with the Chebyshev update; one body
//                            (csr_spmv_rows), two entry points: all rows, and csr_spmv_range_kernel for a sharded level's rows.
//
// K9  dirichlet_lift_kernel  the lifting of non-zero Dirichlet data over the cells that gather a Dirichlet DoF
//
// K10 face_flux_kernel      the error indicator: nodal normal fluxes a d_n u on the six faces of every leaf
// K11 flux_jump_kernel      the error indicator: jumps across the faces through the neighbour table, eta_K
//
// K12 difference_norm_kernel  the error norms: u_h and grad u_h at the Gauss points of every leaf against w, L2 / H1 / energy / Linfty
//
// K13 cell_evaluate_kernel    u_h and grad u_h at the Gauss points of every leaf, stored
// K14 cell_integrate_kernel   the transpose: data at the Gauss points tested against phi_i and grad phi_i, through C^T into a vector
//
// K15 point_locate_kernel     caller points -> leaf and reference coordinate (Morton key, binary search over the sorted leaf keys)
// K16 point_evaluate_kernel   u_h and grad u_h at the located points of the occupied leaves, stored in the caller's order
// K17 point_integrate_kernel  the transpose: point loads (Dirac, dipole) tested against phi_i and grad phi_i, through C^T into a vector
//
// The kernels live in kernels_common.hpp (1D products, sweeps, constraint passes, argument structs), kernels_apply.hpp (K1-K3),
// kernels_boundary.hpp (K9), kernels_estimator.hpp (K10, K11), kernels_error_norm.hpp (K12), kernels_cell_values.hpp (K13, K14), kernels_point_values.hpp (K15-K17), kernels_transfer.hpp (K4), kernels_vector.hpp (K5, K6) and kernels_amg.hpp (K7); this header
// includes them all.
#pragma once
#include "kernels_common.hpp"
#include "kernels_apply.hpp"
#include "kernels_boundary.hpp"
#include "kernels_estimator.hpp"
#include "kernels_error_norm.hpp"
#include "kernels_cell_values.hpp"
#include "kernels_point_values.hpp"
#include "kernels_transfer.hpp"
#include "kernels_vector.hpp"
#include "kernels_amg.hpp"
