// Instance unit of libomgx.so: ipm_solve_kernel with GEN -- the instances that carry the terms with four factors, the cos / sin
// atoms and the basis rows of any degree (Dims::general); the others are the kernels of the benchmark classes, free of that code.
#include "omgx_solve_kernels.h"

ipm_kernel_t solve_general_kernel(int mode, int wave_ok) {
  switch (mode) {
    case omgx::WS_LDS: return wave_ok ? ipm_solve_kernel<omgx::WS_LDS, true, true> : ipm_solve_kernel<omgx::WS_LDS, false, true>;
    case omgx::WS_KKT_HBM: return ipm_solve_kernel<omgx::WS_KKT_HBM, false, true>;
    case omgx::WS_JAC_HBM: return ipm_solve_kernel<omgx::WS_JAC_HBM, false, true>;
    case omgx::WS_JAC_ONLY: return ipm_solve_kernel<omgx::WS_JAC_ONLY, true, true>;
    case omgx::WS_JAC_HV: return ipm_solve_kernel<omgx::WS_JAC_HV, true, true>;
    case omgx::WS_ROOT_HBM: return ipm_solve_kernel<omgx::WS_ROOT_HBM, false, true>;      // (the one instance of mode 6: pick_mode hands it to general templates only)
    default: return ipm_solve_kernel<omgx::WS_ROWS_HBM, false, true>;
  }
}
