// Instance unit of libomgx.so: ipm_solve_kernel on the wave path with every feature (modes 0 / 4 / 5, not general).
#include "omgx_solve_kernels.h"

ipm_kernel_t solve_wave_kernel(int mode) {
  switch (mode) {
    case omgx::WS_LDS: return ipm_solve_kernel<omgx::WS_LDS, true, false>;
    case omgx::WS_JAC_ONLY: return ipm_solve_kernel<omgx::WS_JAC_ONLY, true, false>;
    case omgx::WS_JAC_HV: return ipm_solve_kernel<omgx::WS_JAC_HV, true, false>;      // (the headline instance)
    default: return nullptr;
  }
}
