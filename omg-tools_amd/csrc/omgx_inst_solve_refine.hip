// Instance unit of libomgx.so: ipm_solve_kernel with REFINE, the refinement of regularised steps (omgx_options.refine):
// templates on the wave path, not general.
#include "omgx_solve_kernels.h"

ipm_kernel_t solve_refine_kernel(int mode) {
  switch (mode) {
    case omgx::WS_LDS: return ipm_solve_kernel<omgx::WS_LDS, true, false, true>;
    case omgx::WS_JAC_ONLY: return ipm_solve_kernel<omgx::WS_JAC_ONLY, true, false, true>;
    case omgx::WS_JAC_HV: return ipm_solve_kernel<omgx::WS_JAC_HV, true, false, true>;
    default: return nullptr;
  }
}
