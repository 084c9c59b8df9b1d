// Instance unit of libomgx.so: ipm_solve_kernel with LEAN, for the launches with every optional feature off: the same three
// modes as the refinement, never together with it.
#include "omgx_solve_kernels.h"

ipm_kernel_t solve_lean_kernel(int mode) {
  switch (mode) {
    case omgx::WS_LDS: return ipm_solve_kernel<omgx::WS_LDS, true, false, false, true>;
    case omgx::WS_JAC_ONLY: return ipm_solve_kernel<omgx::WS_JAC_ONLY, true, false, false, true>;
    case omgx::WS_JAC_HV: return ipm_solve_kernel<omgx::WS_JAC_HV, true, false, false, true>;
    default: return nullptr;
  }
}
