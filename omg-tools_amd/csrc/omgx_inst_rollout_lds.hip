// Instance unit of libomgx.so: the six ipm_rollout_kernel instances of workspace mode 0 (WS_LDS), and beside them the glue
// kernels that share their out-of-line routines (omgx_agent_kernels.h).
#include "omgx_rollout_kernel.h"
#include "omgx_agent_kernels.h"

template ipm_rollout_t rollout_kernel_of<omgx::WS_LDS>(int, int, int);
