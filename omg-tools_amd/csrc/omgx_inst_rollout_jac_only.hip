// Instance unit of libomgx.so: the six ipm_rollout_kernel instances of workspace mode 4 (WS_JAC_ONLY).
#include "omgx_rollout_kernel.h"

template ipm_rollout_t rollout_kernel_of<omgx::WS_JAC_ONLY>(int, int, int);
