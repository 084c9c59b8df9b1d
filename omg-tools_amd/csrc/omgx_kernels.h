// omgx_kernels.h -- the glue kernels of the host unit: the small gfx950 kernels that omgx.hip launches by name and that share no
// out-of-line routine with the rollout kernel (signals reduce, predict, order, shift, feedback, Quadrotor predict, free-T advance,
// ADMM, two-sided rows, transfer; sample_kernel<float> is instantiated here from the template of omgx_device.h).  Included by
// omgx.hip only: compiled into the host unit's code object, a few kB each.  The glue kernels that do share such a routine are in
// omgx_agent_kernels.h, the ipm_* kernels in omgx_solve_kernels.h / omgx_rollout_kernel.h: instance units only.
//
//   shift_kernel       warm-start shift T*coeffs (`spline_extra.py:165-191`).
#pragma once
#include "omgx_device.h"

// What `problem.final()` reports per vehicle, from the log (omgx_batch_signals_reduce): one wave per agent.  summary[b] =
// {columns, motion time, path length, largest |input|, largest |dinput|, |state_last - target|, |input_last|, 0}; Euclidean norms
// over the n_spl splines, each square and each sum rounded on its own (no fused multiply-add: a host check in plain numpy
// statements gets the same bits).  Lane l takes the columns l, l + 64, ... in order and the lanes are combined by a fixed
// butterfly: the same result in every run.
__global__ void __launch_bounds__(64)
signals_reduce_kernel(const double* __restrict__ log, const int32_t* __restrict__ count, const double* __restrict__ target,
                      double* __restrict__ summary, int n_der, int n_spl, int cap, double sample_time) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, lane = threadIdx.x;
  int n = count[b];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const double* lg = log + (size_t)b * n_der * n_spl * cap;
  double path = 0.0, vmax = 0.0, amax = 0.0;
  for (int c = lane; c < n; c += 64) {
    if (c >= 1) {
      double s2 = 0.0;
      for (int k = 0; k < n_spl; ++k) { const double dd = lg[(size_t)k * cap + c] - lg[(size_t)k * cap + c - 1]; s2 = s2 + dd * dd; }
      path = path + sqrt(s2);
    }
    if (n_der >= 2) {
      double s2 = 0.0;
      for (int k = 0; k < n_spl; ++k) { const double v = lg[((size_t)n_spl + k) * cap + c]; s2 = s2 + v * v; }
      vmax = fmax(vmax, sqrt(s2));
    }
    if (n_der >= 3) {
      double s2 = 0.0;
      for (int k = 0; k < n_spl; ++k) { const double v = lg[((size_t)2 * n_spl + k) * cap + c]; s2 = s2 + v * v; }
      amax = fmax(amax, sqrt(s2));
    }
  }
  for (int m = 32; m >= 1; m >>= 1) {
    path = path + __shfl_xor(path, m, 64);
    vmax = fmax(vmax, __shfl_xor(vmax, m, 64));
    amax = fmax(amax, __shfl_xor(amax, m, 64));
  }
  if (lane == 0) {
    double dist = 0.0, vlast = 0.0;
    if (n >= 1) {
      double s2 = 0.0;
      for (int k = 0; k < n_spl; ++k) { const double dd = lg[(size_t)k * cap + n - 1] - target[(size_t)b * n_spl + k]; s2 = s2 + dd * dd; }
      dist = sqrt(s2);
      if (n_der >= 2) {
        s2 = 0.0;
        for (int k = 0; k < n_spl; ++k) { const double v = lg[((size_t)n_spl + k) * cap + n - 1]; s2 = s2 + v * v; }
        vlast = sqrt(s2);
      }
    }
    double* sm = summary + (size_t)b * 8;
    sm[0] = (double)n; sm[1] = n >= 1 ? (n - 1) * sample_time : 0.0; sm[2] = path; sm[3] = vmax; sm[4] = amax;
    sm[5] = dist; sm[6] = vlast; sm[7] = 0.0;
  }
}

// (ord_iters != nullptr: the launch carries one more workgroup, which computes the launch order of the next solve --
// the receding-horizon step then has one launch less in front of its solve kernel)
__global__ void __launch_bounds__(256)
predict_kernel(const double* __restrict__ x, int n_var, double* __restrict__ p, int n_par, int B, PredictArgs a,
               const int32_t* __restrict__ ord_iters, int32_t* __restrict__ ord_out, const double* __restrict__ ord_dw) {
  if (ord_iters && blockIdx.x == gridDim.x - 1) { order_block(ord_iters, ord_dw, ord_out, B); return; }
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * a.n_spl) return;
  const int b = id / a.n_spl, k = id - b * a.n_spl;
  const int L = a.n_knots - a.degree - 1;
  const double* c = x + (size_t)b * n_var + a.coeff_off + k * L;
  double* pb = p + (size_t)b * n_par;
  const int j = span_of(a.knots.k, a.degree, a.n_knots, a.tau);
  double sc = 1.0;
  for (int o = 0; o < a.n_out; ++o) {
    if (a.p_off[o] >= 0 && !(o == 0 && a.mode == OMGX_PREDICT_RK4))
      pb[a.p_off[o] + k] = spline_der_at(c, a.knots.k, a.degree, j, a.tau, o) * sc;
    sc *= a.inv_T;
  }
  if (a.mode == OMGX_PREDICT_RK4 && a.p_off[0] >= 0) {
    // k1 = k2 = k3 = u_i, k4 = u_{i+1} for an integrator; h = sample time
    const double h = a.dtau / a.inv_T;
    double st = a.state_in[(size_t)b * a.n_spl + k];
    double u0 = a.tau - a.n_sub * a.dtau;
    double ui = spline_der_at(c, a.knots.k, a.degree, span_of(a.knots.k, a.degree, a.n_knots, u0), u0, 1) * a.inv_T;
    for (int i = 0; i < a.n_sub; ++i) {
      const double u1 = a.tau - (a.n_sub - 1 - i) * a.dtau;
      const double un = spline_der_at(c, a.knots.k, a.degree, span_of(a.knots.k, a.degree, a.n_knots, u1), u1, 1) * a.inv_T;
      st += (h / 6.0) * (ui + 2.0 * ui + 2.0 * ui + un);
      ui = un;
    }
    pb[a.p_off[0] + k] = st;
  }
  if (k == 0 && a.p_t >= 0) pb[a.p_t] = a.t_value;
}

__global__ void __launch_bounds__(256)
predict_quadrotor_kernel(const double* __restrict__ x, int n_var, double* __restrict__ p, int n_par, int B, PredictArgs a,
                         double g, double* __restrict__ state_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int L = a.n_knots - a.degree - 1;
  const double* cx = x + (size_t)b * n_var + a.coeff_off;
  const double* cy = cx + L;
  double* pb = p + (size_t)b * n_par;
  const double h = a.dtau / a.inv_T;
  double s[5];
  for (int q = 0; q < 5; ++q) s[q] = a.state_in[(size_t)b * 5 + q];
  double u1a, u2a;
  quad_inputs(cx, cy, a, a.tau - a.n_sub * a.dtau, g, &u1a, &u2a);
  for (int i = 0; i < a.n_sub; ++i) {
    double u1b, u2b, k1[5], k2[5], k3[5], k4[5], st[5];
    quad_inputs(cx, cy, a, a.tau - (a.n_sub - 1 - i) * a.dtau, g, &u1b, &u2b);
    const double u1m = 0.5 * (u1a + u1b), u2m = 0.5 * (u2a + u2b);
    quad_ode(s, u1a, u2a, g, k1);
    for (int q = 0; q < 5; ++q) st[q] = s[q] + 0.5 * h * k1[q];
    quad_ode(st, u1m, u2m, g, k2);
    for (int q = 0; q < 5; ++q) st[q] = s[q] + 0.5 * h * k2[q];
    quad_ode(st, u1m, u2m, g, k3);
    for (int q = 0; q < 5; ++q) st[q] = s[q] + h * k3[q];
    quad_ode(st, u1b, u2b, g, k4);
    for (int q = 0; q < 5; ++q) s[q] += (h / 6.0) * (k1[q] + 2.0 * k2[q] + 2.0 * k3[q] + k4[q]);
    u1a = u1b; u2a = u2b;
  }
  if (state_out) for (int q = 0; q < 5; ++q) state_out[(size_t)b * 5 + q] = s[q];
  const int j = span_of(a.knots.k, a.degree, a.n_knots, a.tau);
  if (a.p_off[0] >= 0) { pb[a.p_off[0]] = s[0]; pb[a.p_off[0] + 1] = s[1]; }
  double sc = a.inv_T;
  for (int o = 1; o < a.n_out; ++o) {
    if (a.p_off[o] >= 0) {
      pb[a.p_off[o]] = spline_der_at(cx, a.knots.k, a.degree, j, a.tau, o) * sc;
      pb[a.p_off[o] + 1] = spline_der_at(cy, a.knots.k, a.degree, j, a.tau, o) * sc;
    }
    sc *= a.inv_T;
  }
  if (a.p_t >= 0) pb[a.p_t] = a.t_value;
}

__global__ void __launch_bounds__(1024)
order_kernel(const int32_t* __restrict__ iters, const double* __restrict__ dw, int32_t* __restrict__ order, int B) { order_block(iters, dw, order, B); }

__global__ void __launch_bounds__(64)
shift_kernel(double* __restrict__ x, int x_stride, const uint8_t* __restrict__ mask,
             const int32_t* __restrict__ entries, int n_ent, const double* __restrict__ Tm) {
  extern __shared__ __align__(16) double lds[];
  const int b = blockIdx.x;
  if (mask && !mask[b]) return;
  shift_row(x + (size_t)b * x_stride, entries, n_ent, Tm, lds);
}

// one workgroup per agent; the launch carries the launch order of the next solve as plant_predict_kernel does (block B is not an agent)
__global__ void __launch_bounds__(256)
feedback_predict_kernel(const double* __restrict__ x, int n_var, double* __restrict__ p, int n_par, int B, FeedbackArgs fb, double tau,
                        double t_value, const int32_t* __restrict__ ord_iters, int32_t* __restrict__ ord_out,
                        const double* __restrict__ ord_dw) {
  extern __shared__ __align__(16) double lds[];
  if (ord_iters && blockIdx.x == gridDim.x - 1) { order_block(ord_iters, ord_dw, ord_out, B); return; }
  const int b = blockIdx.x;
  if (b >= B) return;
  feedback_predict_agent(fb, b, x + (size_t)b * n_var + fb.coeff_off, p + (size_t)b * n_par, tau, t_value, lds);
}

// One wave per agent.  Lanes over (derivative order, spline) for the prediction; per column of an entry lanes over the old
// coefficients (into LDS), then over the fit points (samples into LDS), then over the new coefficients, each a sum over the
// samples in ascending order.  Nothing of a column is written before its samples are staged, nothing of x before the prediction
// has read the old plan, and x[o_T] last.
__global__ void __launch_bounds__(64)
free_t_advance_kernel(double* __restrict__ x, int n_var, double* __restrict__ p, int n_par, const FreeTArgs* __restrict__ ftp,
                      double update_time, int32_t* __restrict__ under_way) {
#pragma clang fp contract(off)
  __shared__ double kn[40];
  __shared__ double c_old[OMGX_FREE_T_MAX_ROWS];
  __shared__ double y[OMGX_FREE_T_MAX_FIT];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (under_way && under_way[b] == 0) return;
  const FreeTArgs& ft = *ftp;
  double* xb = x + (size_t)b * n_var;
  double* pb = p + (size_t)b * n_par;
  const double T = xb[ft.o_T];
  // (one wave: every lane has its loads of the flag and of T behind it before lane 0 stores either)
  __builtin_amdgcn_wave_barrier();
  if (!(T >= update_time)) {
    if (under_way && lane == 0) under_way[b] = 0;
    return;
  }
  // prediction on the old plan and the old T
  for (int i = lane; i < ft.n_knots; i += 64) kn[i] = ft.knots.k[i];
  __syncthreads();
  const double tau = update_time / T;
  const int L = ft.n_knots - ft.degree - 1;
  const int jt = span_of(kn, ft.degree, ft.n_knots, tau);
  for (int e = lane; e < ft.n_out * ft.n_spl; e += 64) {
    const int o = e / ft.n_spl, k = e - o * ft.n_spl;
    if (ft.p_off[o] < 0) continue;
    double v = spline_der_at(xb + ft.coeff_off + k * L, kn, ft.degree, jt, tau, o);
    for (int q = 0; q < o; ++q) v = v / T;
    pb[ft.p_off[o] + k] = v;
  }
  if (lane == 0 && ft.p_t >= 0) pb[ft.p_t] = 0.0;
  // init_step: the plan re-expressed on what is left of it
  double dt = update_time, rem = T - update_time;
  if (T < 2.0 * update_time) { dt = T - update_time; rem = T; }
  const double s = dt / rem, w = 1.0 - s;
  for (int e = 0; e < ft.n_ent; ++e) {
    const int off = ft.ent[e][0], rows = ft.ent[e][1], cols = ft.ent[e][2];
    const FreeTBasis& bs = ft.basis[ft.ent[e][3]];
    const int degree = bs.degree, n_knots = bs.n_knots, n_fit = bs.n_fit;
    __syncthreads();      // (the samples of the previous entry, and the prediction, have read kn)
    for (int i = lane; i < n_knots; i += 64) kn[i] = bs.knots.k[i];
    for (int k = 0; k < cols; ++k) {
      double* c = xb + off + k * rows;
      __syncthreads();    // (the previous column's sums have read y; its samples c_old)
      for (int i = lane; i < rows; i += 64) c_old[i] = c[i];
      __syncthreads();
      for (int j = lane; j < n_fit; j += 64) {
        const double u = s + w * bs.fit[j];
        y[j] = deboor_at(c_old, kn, degree, span_of(kn, degree, n_knots, u), u);
      }
      __syncthreads();
      for (int r = lane; r < rows; r += 64) {
        const double* pr = bs.proj + (size_t)r * n_fit;
        double acc = 0.0;
        for (int j = 0; j < n_fit; ++j) acc = acc + pr[j] * y[j];
        c[r] = acc;
      }
    }
  }
  __syncthreads();
  if (lane == 0) xb[ft.o_T] = rem;
}

// ---------------------------------------------------------------------------
// Formation ADMM kernels (all pointers are device pointers; tiny, memory-bound)
// ---------------------------------------------------------------------------
// (elements [B ns, (B + n_pub) ns): the rows other ranks need, written to the send buffer of the exchange by the same
// launch -- x_send[i] = row pub_rows[i])
__global__ void admm_center_kernel(omgx_admm_layout lay, const double* __restrict__ x, int n_var,
                                   const double* __restrict__ p, int n_par, double* __restrict__ x_i, int B,
                                   const int32_t* __restrict__ pub_rows, int n_pub, double* __restrict__ x_send) {
  const int ns = lay.n_dim * lay.L;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (B + n_pub) * ns) return;
  const int row = i / ns, q = i - row * ns, k = q / lay.L;
  const int b = row < B ? row : pub_rows[row - B];
  const double v = x[(size_t)b * n_var + lay.x_spl + q] + p[(size_t)b * n_par + lay.p_rel + k];
  if (row < B) x_i[i] = v; else x_send[(size_t)(row - B) * ns + q] = v;
}

// one block per agent; thread r owns row r of the stacked vectors (n_all <= blockDim)
__global__ void __launch_bounds__(256)
admm_update_kernel(omgx_admm_layout lay, const double* __restrict__ x_ext, const int32_t* __restrict__ nbr,
                   const double* __restrict__ M, const double* __restrict__ F, double rho,
                   double* __restrict__ p, int n_par, double* __restrict__ z_ij, double* __restrict__ l_ij, int zl_stride,
                   double* __restrict__ res, double* __restrict__ sums, int* __restrict__ done,
                   const int32_t* __restrict__ pub_slot, double* __restrict__ zl_send, int send_stride) {
  extern __shared__ __align__(16) double lds[];
  const int ns = lay.n_dim * lay.L, nn = lay.n_nghb, na = (1 + nn) * ns;
  double* xa = lds; double* la = lds + na; double* zp = lds + 2 * na; double* va = lds + 3 * na;
  double* d1 = lds + 4 * na; double* d2 = lds + 5 * na; double* red = lds + 6 * na;
  const int b = blockIdx.x, r = threadIdx.x;
  double* pb = p + (size_t)b * n_par;
  if (r < na) {
    const int blk = r / ns, q = r - blk * ns;
    if (blk == 0) { xa[r] = x_ext[(size_t)b * ns + q]; la[r] = pb[lay.p_li + q]; zp[r] = pb[lay.p_zi + q]; }
    else {
      const int j = nbr[b * nn + blk - 1];
      xa[r] = x_ext[(size_t)j * ns + q];
      la[r] = l_ij[(size_t)b * zl_stride + (blk - 1) * ns + q];
      zp[r] = z_ij[(size_t)b * zl_stride + (blk - 1) * ns + q];
    }
    va[r] = xa[r] + la[r] / rho;
  }
  __syncthreads();
  double zr = 0.0, lr = 0.0;
  if (r < na) {
    const double* Mr = M + (size_t)r * na;
    for (int c = 0; c < na; ++c) zr += Mr[c] * va[c];
    lr = la[r] + rho * (xa[r] - zr);
    d1[r] = xa[r] - zr; d2[r] = zr - zp[r];
    const int blk = r / ns, q = r - blk * ns;
    if (blk == 0) { pb[lay.p_zi + q] = zr; pb[lay.p_li + q] = lr; }
    else {
      z_ij[(size_t)b * zl_stride + (blk - 1) * ns + q] = zr; l_ij[(size_t)b * zl_stride + (blk - 1) * ns + q] = lr;
      // a row another rank needs goes to the send buffer of the second exchange as well: [z_ij | l_ij]
      const int ps = pub_slot ? pub_slot[b] : -1;
      if (ps >= 0) {
        zl_send[(size_t)ps * send_stride + (blk - 1) * ns + q] = zr;
        zl_send[(size_t)ps * send_stride + nn * ns + (blk - 1) * ns + q] = lr;
      }
    }
  }
  __syncthreads();
  double pr = 0.0, dr = 0.0;
  if (r < na) {
    const double* Fr = F + (size_t)r * na;
    double a1 = 0.0, a2 = 0.0;
    for (int c = 0; c < na; ++c) { a1 += Fr[c] * d1[c]; a2 += Fr[c] * d2[c]; }
    pr = a1 * a1; dr = a2 * a2;
  }
  // block sum of (pr, dr)
  for (int off = 32; off > 0; off >>= 1) { pr += __shfl_down(pr, off, 64); dr += __shfl_down(dr, off, 64); }
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[2 * wave] = pr; red[2 * wave + 1] = dr; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double P = 0.0, D = 0.0;
    for (int w = 0; w < nw; ++w) { P += red[2 * w]; D += red[2 * w + 1]; }
    D *= rho;
    res[3 * b] = P; res[3 * b + 1] = D; res[3 * b + 2] = rho * P + D;
  }
  if (!sums) return;
  // Fleet sums of the three residuals by the workgroup that finishes last (no second launch): thread t adds the
  // agents t, t + 256, ... in that order, then a fixed tree over the 256 partial sums -- the same bits whichever
  // workgroup happens to be the last one.
  __shared__ int last;
  if (threadIdx.x == 0) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); last = atomicAdd(done, 1) == (int)gridDim.x - 1 ? 1 : 0; }
  __syncthreads();
  if (!last) return;
  // (acquire at device scope: the other workgroups' res rows -- written before their release + counter increment --
  // are visible to plain loads from here on, which the compiler can keep in flight together)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const int B = gridDim.x;
  const double* rv = res;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 4
  for (int a = threadIdx.x; a < B; a += blockDim.x) { s0 += rv[3 * a]; s1 += rv[3 * a + 1]; s2 += rv[3 * a + 2]; }
  double* t3 = lds;                       // (6 na + 16 doubles are there; 3 x 256 are needed: see the launch)
  t3[threadIdx.x] = s0; t3[256 + threadIdx.x] = s1; t3[512 + threadIdx.x] = s2;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      t3[threadIdx.x] += t3[threadIdx.x + off]; t3[256 + threadIdx.x] += t3[256 + threadIdx.x + off];
      t3[512 + threadIdx.x] += t3[512 + threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { sums[0] = t3[0]; sums[1] = t3[256]; sums[2] = t3[512]; *done = 0; }
}

// (sum_rows: the residual sums every rank sent along with its rows, [n_sum_rows] rows of sum_stride doubles with the
// three sums in front; their total over the ranks goes to sums_out -- rank order, the same bits on every rank)
__global__ void admm_comm_kernel(omgx_admm_layout lay, const int32_t* __restrict__ nbr,
                                 const int32_t* __restrict__ slot, const double* __restrict__ z_ext,
                                 const double* __restrict__ l_ext, int zl_stride, double* __restrict__ p, int n_par, int B,
                                 const double* __restrict__ sum_rows, int n_sum_rows, int sum_stride, double* __restrict__ sums_out) {
  const int ns = lay.n_dim * lay.L, nn = lay.n_nghb;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3 && sums_out) {
    double acc = 0.0;
    for (int r = 0; r < n_sum_rows; ++r) acc += sum_rows[(size_t)r * sum_stride + i];
    sums_out[i] = acc;
  }
  if (i >= B * nn * ns) return;
  const int b = i / (nn * ns), rem = i - b * nn * ns, k = rem / ns, q = rem - k * ns;
  const size_t src = (size_t)nbr[b * nn + k] * zl_stride + (size_t)slot[b * nn + k] * ns + q;
  p[(size_t)b * n_par + lay.p_zji + k * ns + q] = z_ext[src];
  p[(size_t)b * n_par + lay.p_lji + k * ns + q] = l_ext[src];
}

namespace {
// ---- two-sided rows: caller's rows <-> the kernel's rows ----------------------------------------------------------
__global__ void range_expand_bounds(const double* __restrict__ lb_u, const double* __restrict__ ub_u, double* __restrict__ lb_i,
                                    double* __restrict__ ub_i, int sets, int nu, int ni, const int32_t* __restrict__ src,
                                    const int32_t* __restrict__ dup) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= sets * ni) return;
  const int s = id / ni, r = id - s * ni;
  if (r < nu) {                                  // a two-sided row keeps its upper bound here
    lb_i[id] = dup[r] >= 0 ? -INFINITY : lb_u[(size_t)s * nu + r];
    ub_i[id] = ub_u[(size_t)s * nu + r];
  } else {                                       // its copy carries the lower bound
    lb_i[id] = lb_u[(size_t)s * nu + src[r - nu]];
    ub_i[id] = INFINITY;
  }
}
// multipliers in: lam_g of a two-sided row is positive when its upper bound is active, negative for the lower one
__global__ void range_expand_lam(const double* __restrict__ lam_u, double* __restrict__ lam_i, int B, int nu, int ni,
                                 const int32_t* __restrict__ src, const int32_t* __restrict__ dup) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * ni) return;
  const int b = id / ni, r = id - b * ni;
  if (r < nu) { const double v = lam_u[(size_t)b * nu + r]; lam_i[id] = dup[r] >= 0 ? fmax(v, 0.0) : v; }
  else lam_i[id] = fmin(lam_u[(size_t)b * nu + src[r - nu]], 0.0);
}
__global__ void range_contract_lam(const double* __restrict__ lam_i, double* __restrict__ lam_u, int B, int nu, int ni,
                                   const int32_t* __restrict__ dup) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * nu) return;
  const int b = id / nu, r = id - b * nu;
  lam_u[id] = lam_i[(size_t)b * ni + r] + (dup[r] >= 0 ? lam_i[(size_t)b * ni + dup[r]] : 0.0);
}
}  // namespace

extern "C" {      // (the kernel keeps its C name)
// omgx_batch_transfer: up to OMGX_TRANSFER_MAX segments moved by one launch (device <-> pinned host memory over the host link, or
// device <-> device): a workgroup range per segment in proportion to its size, 16-byte words, coalesced
struct TransferArgs { const double* src[OMGX_TRANSFER_MAX]; double* dst[OMGX_TRANSFER_MAX]; long long n8[OMGX_TRANSFER_MAX]; int blk0[OMGX_TRANSFER_MAX + 1]; int n_seg; };
__global__ void __launch_bounds__(256)
transfer_kernel(TransferArgs a) {
  int sg = 0;
  while (sg + 1 < a.n_seg && (int)blockIdx.x >= a.blk0[sg + 1]) ++sg;
  const int nb = a.blk0[sg + 1] - a.blk0[sg], lb = blockIdx.x - a.blk0[sg];
  const long long n8 = a.n8[sg], n16 = n8 >> 1;
  const bool wide = ((((size_t)a.src[sg]) | ((size_t)a.dst[sg])) & 15) == 0;
  if (wide) {
    const double2* s = (const double2*)a.src[sg];
    double2* d = (double2*)a.dst[sg];
    for (long long i = (long long)lb * 256 + threadIdx.x; i < n16; i += (long long)nb * 256) d[i] = s[i];
    if ((n8 & 1) && lb == 0 && threadIdx.x == 0) a.dst[sg][n8 - 1] = a.src[sg][n8 - 1];
  } else {
    for (long long i = (long long)lb * 256 + threadIdx.x; i < n8; i += (long long)nb * 256) a.dst[sg][i] = a.src[sg][i];
  }
}
}  // extern "C"
