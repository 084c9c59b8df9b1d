// Instance unit of libomgx.so: ipm_solve_kernel with the blocked factorisation (classes off the wave path and the spill modes),
// not general.
#include "omgx_solve_kernels.h"

ipm_kernel_t solve_blocked_kernel(int mode) {
  switch (mode) {
    case omgx::WS_LDS: return ipm_solve_kernel<omgx::WS_LDS, false, false>;
    case omgx::WS_KKT_HBM: return ipm_solve_kernel<omgx::WS_KKT_HBM, false, false>;
    case omgx::WS_JAC_HBM: return ipm_solve_kernel<omgx::WS_JAC_HBM, false, false>;
    default: return ipm_solve_kernel<omgx::WS_ROWS_HBM, false, false>;
  }
}
