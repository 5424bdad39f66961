// Explicit instantiations of LevelOperator<T>::apply_P<P, MODE> for ONE number type and ONE degree
// (-DMGAMD_INST_T=double|float -DMGAMD_INST_P=1..7): the kernels of kernels.hpp are compiled here, in fourteen translation units
// built in parallel (Makefile), instead of in one.
#include "level_operator_apply.hpp"

#if !defined(MGAMD_INST_T) || !defined(MGAMD_INST_P)
#error "compile with -DMGAMD_INST_T=<double|float> -DMGAMD_INST_P=<degree>"
#endif

namespace mgamd
{
#define MGAMD_INST(MODE)                                                                                                                  \
  template void LevelOperator<MGAMD_INST_T>::apply_P<MGAMD_INST_P, MODE>(const MGAMD_INST_T *, const Epilogue<MGAMD_INST_T> &, bool, double, \
                                                                         int, const FusedTransferHost<MGAMD_INST_T> *);
  MGAMD_INST(MODE_VMULT)
  MGAMD_INST(MODE_RESIDUAL)
  MGAMD_INST(MODE_CHEB)
  MGAMD_INST(MODE_CHEB_FIRST)
  MGAMD_INST(MODE_CHEB_SECOND)
  MGAMD_INST(MODE_MASS)
  // the passes with fused level transfers: degrees with a persistent 17-point lattice kernel
#if MGAMD_INST_P == 1 || MGAMD_INST_P == 2 || MGAMD_INST_P == 4
  MGAMD_INST(MODE_RESIDUAL_RESTRICT)
  MGAMD_INST(MODE_CHEB_PROLONGATE)
#endif
#undef MGAMD_INST
  // the lifting of non-zero Dirichlet data (kernels_boundary.hpp)
  template void LevelOperator<MGAMD_INST_T>::lift_P<MGAMD_INST_P>(MGAMD_INST_T *, const MGAMD_INST_T *, double, double);
  // the jump error indicator (kernels_estimator.hpp)
  template void LevelOperator<MGAMD_INST_T>::estimate_P<MGAMD_INST_P>(const MGAMD_INST_T *, const double *);
  // the error norms (kernels_error_norm.hpp)
  template void LevelOperator<MGAMD_INST_T>::difference_norm_P<MGAMD_INST_P>(const MGAMD_INST_T *, int, const MGAMD_INST_T *, const MGAMD_INST_T *, int,
                                                                             int);
  // the cell evaluate and integrate (kernels_cell_values.hpp)
  template void LevelOperator<MGAMD_INST_T>::cell_evaluate_P<MGAMD_INST_P>(const MGAMD_INST_T *, int, MGAMD_INST_T *, MGAMD_INST_T *);
  template void LevelOperator<MGAMD_INST_T>::cell_integrate_P<MGAMD_INST_P>(const MGAMD_INST_T *, const MGAMD_INST_T *, int, MGAMD_INST_T *);
  // point evaluation and point sources (kernels_point_values.hpp)
  template void LevelOperator<MGAMD_INST_T>::point_evaluate_P<MGAMD_INST_P>(const LevelOperator<MGAMD_INST_T>::PointSetDev &, const MGAMD_INST_T *,
                                                                            MGAMD_INST_T *, MGAMD_INST_T *);
  template void LevelOperator<MGAMD_INST_T>::point_integrate_P<MGAMD_INST_P>(const LevelOperator<MGAMD_INST_T>::PointSetDev &, const MGAMD_INST_T *,
                                                                             const MGAMD_INST_T *, MGAMD_INST_T *);
} // namespace mgamd
