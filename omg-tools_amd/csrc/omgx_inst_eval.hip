// Instance unit of libomgx.so: ipm_eval_kernel (omgx_batch_eval) and ipm_prepare_kernel (omgx_batch_set_prepare).
#include "omgx_solve_kernels.h"

template <bool GEN>
static ipm_eval_kernel_t ipm_eval_kernel_gen(int mode, int wave_ok) {
  switch (mode) {
    case omgx::WS_LDS: return wave_ok ? ipm_eval_kernel<omgx::WS_LDS, true, GEN> : ipm_eval_kernel<omgx::WS_LDS, false, GEN>;
    case omgx::WS_KKT_HBM: return ipm_eval_kernel<omgx::WS_KKT_HBM, false, GEN>;
    case omgx::WS_JAC_HBM: return ipm_eval_kernel<omgx::WS_JAC_HBM, false, GEN>;
    case omgx::WS_JAC_ONLY: return ipm_eval_kernel<omgx::WS_JAC_ONLY, true, GEN>;
    case omgx::WS_JAC_HV: return ipm_eval_kernel<omgx::WS_JAC_HV, true, GEN>;
    case omgx::WS_ROOT_HBM: return ipm_eval_kernel<omgx::WS_ROOT_HBM, false, true>;      // (one instance: pick_mode hands mode 6 to general templates only)
    default: return ipm_eval_kernel<omgx::WS_ROWS_HBM, false, GEN>;
  }
}
ipm_eval_kernel_t ipm_eval_kernel_for(int mode, int wave_ok, int general) {
  return general ? ipm_eval_kernel_gen<true>(mode, wave_ok) : ipm_eval_kernel_gen<false>(mode, wave_ok);
}

ipm_prepare_kernel_t ipm_prepare_kernel_for(int general) {
  return general ? ipm_prepare_kernel<true> : ipm_prepare_kernel<false>;
}
