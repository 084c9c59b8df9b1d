// Instance unit of libomgx.so: the six ipm_rollout_kernel instances of workspace mode 5 (WS_JAC_HV).
#include "omgx_rollout_kernel.h"

template ipm_rollout_t rollout_kernel_of<omgx::WS_JAC_HV>(int, int, int);
