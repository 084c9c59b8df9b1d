// omgx_device.h -- what the host unit (omgx.hip) and the kernel instance units (omgx_inst_*.hip) of libomgx.so share: the kernel
// argument structs, the __host__ __device__ size helpers, the device routines that both a glue kernel and a solve / rollout kernel
// call (sample_agent, signals_append_agent, plant_*_agent, obstacles_advance_agent, mission_next_leg_agent, shift_row, ...), the
// function-pointer types of the ipm_* kernels and the declarations of their selectors.  No kernel is compiled from this header
// alone: the glue kernels are in omgx_kernels.h (host unit only) and omgx_agent_kernels.h (the ones that share an out-of-line
// routine with the rollout kernel: compiled beside it, declared here), the ipm_* kernel templates in omgx_solve_kernels.h /
// omgx_rollout_kernel.h (instance units only).  The library is built without relocatable device code, so every unit that calls
// one of the out-of-line routines here carries a copy of its own in its own code object.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/omgx.h"
#include "omgx_types.h"

// out[b, o, k, i] = d^o/dt^o spline_k(t0[b] + i*dt); one block = (agent, 1024-sample chunk).
//
// Bound: HBM writes (8 n_der n_spl bytes per sample).  The de Boor recursion per sample (about 20
// fp64 divisions for 3 derivative orders of 2 cubic splines) kept the first version at 20 % of the HBM
// roofline, so the recursion is run once per knot span instead of once per sample: every block turns
// its agent's splines into local power series  p_{o,k,j}(h) = sum_m S_k^{(o+m)}(k_j+) / m!  h^m  around
// the left knot of each span j (a few dozen small de Boor evaluations, spread over the block) and a
// sample is a span look-up plus one Horner evaluation per output value.
struct KnotArg { double k[40]; };
#define OMGX_SAMPLE_CHUNK 1024      // samples per block: the per-block set-up is amortised over 4 samples per thread

// What `Vehicle.store` extracts from a solution (reference `vehicles/vehicle.py:250-300` ->
// `splines2signals`, e.g. `vehicles/holonomic.py:116-124`): derivative orders 0 .. n_der-1 of the n_spl
// splines on a time grid, order o scaled by inv_T^o (time derivatives), and optionally the speed
// v_tot = |first derivative|.  Passed by value to the kernels; out == nullptr: nothing to do.
// `omgx_admm_center_ex` fused behind the solve (omgx_batch_set_center): x_i[b] = shared coefficients of the solution + the
// agent's relative position, and its published copy
struct CenterArgs {
  int x_spl, p_rel, n_dim, L;
  double* x_i;
  const int32_t* pub_inv;     // [B] slot of the agent's row in x_send (-1: not published); nullptr: nothing published
  double* x_send;
};
// The reference's stop criterion inside the solve launch (omgx_batch_set_stop): parameter offsets of the state, the input and
// the target of the vehicle, its dimension, the tolerance; under_way [B] (device, owned by the caller): 1 while the agent's loop runs
struct StopArgs {
  int o_state, o_input, o_pose, n_dim;
  double tol;
  int32_t* under_way;
};
struct StoreArgs {
  double* out;            // [B, n_der, n_spl, n_samp]
  double* v_tot;          // [B, n_samp] or nullptr (needs n_der >= 2)
  const double* t0;       // [B] first sample, spline domain
  int coeff_off, n_spl, degree, n_knots, n_der, n_samp;
  double dt, inv_T;
  KnotArg knots;
};
// The travelled trajectories (omgx_batch_set_signals): what `Vehicle.simulate` with `ideal_update` appends to `vehicle.signals`
// after every update (reference `vehicles/vehicle.py:359-369`) -- samples 1 .. n_samp of the fresh plan, ahead of the first
// update's also sample 0.  log [B, n_der, n_spl, cap]: order o = time-derivative order of spline k (state, input, dinput),
// scaled by inv_T^o as in sample_agent; count [B]: columns written so far; overflow [B] (or nullptr): 1 = an append did not fit.
struct SignalArgs {
  double* log;
  int32_t* count;
  int32_t* overflow;
  int coeff_off, n_spl, degree, n_knots, n_der, n_samp, cap, p_t;
  double sample_time, inv_T;
  KnotArg knots;
};
// What the `stp` argument of the solve and rollout kernels points at in device memory: the fused store and, right behind it, the
// fused log (st.out == nullptr / sg.log == nullptr: that part is off; the pointer itself is null when both are)
struct StoreBlock { StoreArgs st; SignalArgs sg; };

__host__ __device__ inline size_t sample_scratch_doubles(int n_spl, int degree, int n_knots, int n_der) {
  const int L = n_knots - degree - 1, n_span = n_knots - 2 * degree - 1, D1 = degree + 1;
  return (size_t)n_knots + (size_t)D1 * n_spl * L + (size_t)D1 * n_spl * n_span + (size_t)n_der * n_spl * n_span * D1;
}

// value at u of the spline with coefficients c on the knot vector kk (degree dg <= 5), inside span jo.
// Fully unrolled triangle with compile-time indices: a dynamically indexed local array would live in
// scratch (global) memory.
__device__ __forceinline__ double deboor_at(const double* c, const double* kk, int dg, int jo, double u) {
  double dbo[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) dbo[r] = (r <= dg) ? c[jo - dg + r] : 0.0;
#pragma unroll
  for (int lev = 1; lev <= 5; ++lev) {
#pragma unroll
    for (int r = 5; r >= 1; --r) {
      if (lev <= dg && r >= lev && r <= dg) {
        const int idx = jo - dg + r;
        const double den = kk[idx + dg - lev + 1] - kk[idx];
        const double a = den != 0.0 ? (u - kk[idx]) / den : 0.0;
        dbo[r] = (1.0 - a) * dbo[r - 1] + a * dbo[r];
      }
    }
  }
  return dg == 0 ? dbo[0] : (dg == 1 ? dbo[1] : (dg == 2 ? dbo[2] : (dg == 3 ? dbo[3] : (dg == 4 ? dbo[4] : dbo[5]))));
}

// Samples [i_begin, i_end) of one agent by the whole workgroup.  coeffs: [n_spl][L] (global memory or
// LDS), scratch: sample_scratch_doubles() doubles the workgroup may overwrite.  Used by sample_kernel and
// by the epilogue of the solve kernel (the solution is still in LDS there).
template <typename OutT>
__device__ void sample_agent(const double* coeffs, double* scratch, int n_spl, int degree, const KnotArg& knots,
                             int n_knots, int n_der, double tb, double dt, double inv_T, int n_samp, int i_begin,
                             int i_end, OutT* out_b, OutT* vtot_b) {
  const int L = n_knots - degree - 1;
  const int n_span = n_knots - 2 * degree - 1;    // spans j = degree .. degree + n_span - 1
  const int D1 = degree + 1;
  double* kn = scratch;                           // [n_knots]
  double* cf = kn + n_knots;                      // [D1][n_spl][L]      coefficients of every derivative order
  double* val = cf + D1 * n_spl * L;              // [D1][n_spl][n_span] S^{(q)}(k_j+)
  double* pw = val + D1 * n_spl * n_span;         // [n_der][n_spl][n_span][D1] local power series
  for (int i = threadIdx.x; i < n_knots; i += blockDim.x) kn[i] = knots.k[i];
  for (int i = threadIdx.x; i < n_spl * L; i += blockDim.x) cf[i] = coeffs[i];
  __syncthreads();
  for (int o = 1; o <= degree; ++o) {             // c^(o)_i = (d-o+1) (c^(o-1)_{i+1}-c^(o-1)_i)/(k_{i+d+1}-k_{i+o})
    const int Lo = L - o, dd = degree - o + 1;
    for (int e = threadIdx.x; e < n_spl * Lo; e += blockDim.x) {
      const int k = e / Lo, i = e - k * Lo;
      const double* src = cf + ((o - 1) * n_spl + k) * L;
      const double den = kn[i + degree + 1] - kn[i + o];
      cf[(o * n_spl + k) * L + i] = den != 0.0 ? dd * (src[i + 1] - src[i]) / den : 0.0;
    }
    __syncthreads();
  }
  // right-hand limits of every derivative order at the left knot of every span
  for (int e = threadIdx.x; e < D1 * n_spl * n_span; e += blockDim.x) {
    const int q = e / (n_spl * n_span), r = e - q * n_spl * n_span, k = r / n_span, sp = r - k * n_span;
    const int j = degree + sp;
    // the q-th derivative lives on the knot vector kn[q .. n_knots-q), its span index there is j - q
    val[e] = deboor_at(cf + (q * n_spl + k) * L, kn + q, degree - q, j - q, kn[j]);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n_der * n_spl * n_span * D1; e += blockDim.x) {
    const int m = e % D1, r = e / D1;             // r = (o, k, sp)
    const int o = r / (n_spl * n_span), ks = r - o * n_spl * n_span;
    double f = 1.0;
    for (int q = 2; q <= m; ++q) f *= q;
    for (int q = 0; q < o; ++q) f /= inv_T;       // time derivative of order o: spline-domain derivative * inv_T^o
    pw[e] = (o + m <= degree) ? val[(o + m) * n_spl * n_span + ks] / f : 0.0;
  }
  __syncthreads();
  for (int i = i_begin + threadIdx.x; i < i_end; i += blockDim.x) {
    const double u = tb + i * dt;
    // span j: k_j < u <= k_{j+1} (reference convention, `basics/spline.py:131-136`)
    int j = degree;
    for (int q = degree + 1; q < n_knots - degree - 1; ++q) if (kn[q] < u) j = q;
    const double h = u - kn[j];
    const int sp = j - degree;
    double v2 = 0.0;
    for (int o = 0; o < n_der; ++o) {
      const int dg = degree - o;
      for (int k = 0; k < n_spl; ++k) {
        const double* c = pw + (((o * n_spl + k) * n_span) + sp) * D1;
        double v = c[dg];
        for (int m = dg - 1; m >= 0; --m) v = fma(v, h, c[m]);
        out_b[((size_t)o * n_spl + k) * n_samp + i] = (OutT)v;
        if (o == 1) v2 = fma(v, v, v2);
      }
    }
    if (vtot_b) vtot_b[i] = (OutT)sqrt(v2);
  }
}

// One append of the travelled-trajectory log for agent b by the whole workgroup: the batched twin of `Vehicle.simulate` with
// `ideal_update` (reference `vehicles/vehicle.py:359-369`).  coeffs: the plan just solved ([n_spl][L], global memory or LDS),
// t_rel: the time since the last knot it was solved at (p[p_t]), scratch: sample_scratch_doubles() doubles.  Column 0 (the
// plan at t_rel, `trajectories[:, 0]`) goes ahead of the first append; then the n_samp columns at t_rel + i sample_time,
// i = 1 .. n_samp.  An append that does not fit writes nothing but overflow[b] = 1.  The one routine behind
// signals_append_kernel, the epilogue of the solve kernel and the step loop of the rollout kernel: sample_agent's arithmetic
// per column does not depend on the workgroup size, so the three write the same bits.  Barriers inside: every thread of the
// workgroup calls it, with the same arguments.
__device__ __noinline__ void signals_append_agent(const SignalArgs& sg, int b, const double* coeffs, double t_rel, double* scratch) {
  __syncthreads();      // (the scratch may still be read by the fused store; every thread reads count[b] before thread 0 moves it)
  const int cnt = sg.count[b];
  const int first = cnt == 0 ? 0 : 1;
  const int n_col = sg.n_samp + 1 - first;
  if (cnt < 0 || cnt > sg.cap - n_col) {      // (the same branch in every thread)
    if (threadIdx.x == 0 && sg.overflow) sg.overflow[b] = 1;
    return;
  }
  // sample i of the plan -> column cnt - first + i of the agent's block: rows of `cap` columns, i = first .. n_samp
  sample_agent<double>(coeffs, scratch, sg.n_spl, sg.degree, sg.knots, sg.n_knots, sg.n_der, t_rel * sg.inv_T, sg.sample_time * sg.inv_T,
                       sg.inv_T, sg.cap, first, sg.n_samp + 1, sg.log + (size_t)b * sg.n_der * sg.n_spl * sg.cap + (cnt - first),
                       (double*)nullptr);
  __syncthreads();
  if (threadIdx.x == 0) sg.count[b] = cnt + n_col;
}

// The slot queue of the persistent kernels: next_slot[0] counts the slots handed out, next_slot[1] the workgroups that have left;
// both are zero at every launch because the workgroup that leaves last resets them.  Called by thread 0 behind its last solve.
// No fence on either side of it:
//  * nothing a workgroup has stored (x, lam, status, iters, dw_state, its slab, the statistics) is read by another workgroup of
//    the same launch; later launches read it behind the kernel boundary, which writes the caches back.  A __threadfence() here is
//    a write-back of the whole L2 of the compute die plus an L1 invalidate, once per workgroup: with one agent per workgroup, once
//    per solve, right after the solve has dirtied its Jacobian slab.
//  * the counters are only ever touched by device-scope atomics, the reset included (exchanges, not plain stores: they are
//    performed where the next launch's adds are performed, whatever a cache still holds).  Thread 0 has consumed the value of
//    its last atomicAdd(next_slot) -- it wrote it to LDS and passed a barrier -- before it adds to next_slot[1], so an add that
//    has returned has been performed.  The workgroup that reads gridDim.x - 1 therefore resets a queue no add is in flight on:
//    every other thread 0 made its last add to next_slot[0] before its add to next_slot[1], and that one before ours returned.
__device__ __forceinline__ void queue_leave(int* next_slot) {
  if (atomicAdd(next_slot + 1, 1) == (int)gridDim.x - 1) {
    __hip_atomic_exchange(next_slot, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_exchange(next_slot + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// dynamic LDS of ipm_prepare_kernel (omgx_solve_kernels.h): slots, atoms, knots, x and the reduction scratch
__host__ __device__ inline size_t prepare_lds_doubles(const omgx::Dims& d) {
  return (size_t)d.n_slots + d.n_atoms + d.n_knots + d.N + 64;
}

// Prediction of one receding-horizon step: thread (agent b, spline k) evaluates the plan and its time
// derivatives at tau by de Boor on the active span and writes them into the parameter vector (state0 /
// input0 / ...), thread k == 0 also the time since the last knot crossing.  RK4 mode: the state is the
// caller's current state integrated over the n_sub sample intervals before tau with the inputs the plan
// holds there, by the statements of the reference's `Vehicle::integrate` (export/vehicles/Vehicle.cpp:82-110)
// for the integrator models (`ode` = input: Holonomic, Holonomic3D).
struct PredictArgs {
  KnotArg knots;
  int coeff_off, n_spl, degree, n_knots, n_out, p_off[4], p_t, mode, n_sub;
  double tau, inv_T, t_value, dtau;
  const double* state_in;
};

// d-th derivative (spline-domain units) at u of the spline whose coefficients on span j are c[j-degree .. j]
__device__ __forceinline__ double spline_der_at(const double* c, const double* kk, int degree, int j, double u, int dord) {
  double v[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) v[r] = (r <= degree) ? c[j - degree + r] : 0.0;
  // after o differences v[r] (r = o .. degree) holds c^(o)_{j-degree+r}
#pragma unroll
  for (int o = 1; o <= 3; ++o) {
    if (o <= dord) {
#pragma unroll
      for (int r = 5; r >= 1; --r) {
        if (r >= o && r <= degree) {
          const int i = j - degree + r;                       // c^(o)_i = (degree-o+1) (c^(o-1)_i - c^(o-1)_{i-1}) / (k_{i+degree-o+1} - k_i)
          const double den = kk[i + degree - o + 1] - kk[i];
          v[r] = den != 0.0 ? (degree - o + 1) * (v[r] - v[r - 1]) / den : 0.0;
        }
      }
    }
  }
  const int dg = degree - dord;
#pragma unroll
  for (int lev = 1; lev <= 5; ++lev) {
#pragma unroll
    for (int r = 5; r >= 1; --r) {
      if (lev <= dg && r >= dord + lev && r <= degree) {
        const int i = j - degree + r;
        const double den = kk[i + dg - lev + 1] - kk[i];
        const double a = den != 0.0 ? (u - kk[i]) / den : 0.0;
        v[r] = (1.0 - a) * v[r - 1] + a * v[r];
      }
    }
  }
  double out = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) if (r == degree) out = v[r];
  return out;
}

__device__ __forceinline__ int span_of(const double* kk, int degree, int n_knots, double u) {
  int j = degree;                                  // span: k_j < u <= k_{j+1} (`basics/spline.py:131-136`)
  for (int q = degree + 1; q < n_knots - degree - 1; ++q) if (kk[q] < u) j = q;
  return j;
}

// Launch order for the next solve: agents bucketed by the iteration count of their previous solve,
// largest first (64 buckets, counting sort in LDS by one workgroup; the order inside a bucket is
// arbitrary).  Replaces a device-wide sort: this is ~10 us.
// Round 4: among the agents with the same previous count (most have 1) those that carry a heavy inertia correction go
// first -- a large dw is the signature of the slow ones (multipliers of 5-20 on bilinear rows: the regularised Newton
// iteration converges linearly).  On the host model of the step (512 slots, greedy queue) the total time of 20 headline
// steps drops by 4 % against the count alone; the perfect order would gain 6.6 %.
__device__ __forceinline__ int order_bucket(int it, double dw) {
  const int a = it < 0 ? 0 : (it > 15 ? 15 : it);
  const int q = dw > 10.0 ? 3 : (dw > 1.0 ? 2 : (dw > 0.1 ? 1 : 0));
  return 63 - (4 * a + q);
}
__device__ __forceinline__ void order_block(const int32_t* __restrict__ iters, const double* __restrict__ dw, int32_t* __restrict__ order, int B) {
  __shared__ int cnt[64], off[64];
  if (threadIdx.x < 64) cnt[threadIdx.x] = 0;
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += blockDim.x) atomicAdd(&cnt[order_bucket(iters[b], dw ? dw[b] : 0.0)], 1);
  __syncthreads();
  if (threadIdx.x == 0) { int a = 0; for (int k = 0; k < 64; ++k) { off[k] = a; a += cnt[k]; } }
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += blockDim.x) order[atomicAdd(&off[order_bucket(iters[b], dw ? dw[b] : 0.0)], 1)] = b;
}

// Non-ideal prediction of the Quadrotor (`vehicles/vehicle.py:323-337` with the model's own `ode`,
// `vehicles/quadrotor.py:149-152`: state (x, y, dx, dy, theta), inputs (u1, u2) = thrust and pitch rate, which the plan
// holds as functions of its second and third derivatives, `quadrotor.py:121-140`).  One thread per agent: the inputs at
// the n_sub + 1 sample points that end at tau, classical Runge-Kutta over the sample intervals with the input taken
// linearly between the samples (the reference integrates with odeint on a linear interpolation of the sampled inputs,
// `vehicle.py:412-423`), the position of the integrated state into spl0, the plan's own derivatives at tau into
// dspl0 / ddspl0 (`quadrotor.py:110-114`: only state[:2] of the prediction enters the parameters).
// (kk: the knots, wherever they lie -- the kernel argument, or LDS for the plant kernels below)
__device__ __forceinline__ void quad_inputs(const double* cx, const double* cy, const double* kk, int degree, int n_knots, double inv_T, double u,
                                            double g, double* u1, double* u2) {
  const int j = span_of(kk, degree, n_knots, u);
  const double s2 = inv_T * inv_T, s3 = s2 * inv_T;
  const double ddx = spline_der_at(cx, kk, degree, j, u, 2) * s2, ddy = spline_der_at(cy, kk, degree, j, u, 2) * s2;
  const double dddx = spline_der_at(cx, kk, degree, j, u, 3) * s3, dddy = spline_der_at(cy, kk, degree, j, u, 3) * s3;
  const double n2 = (ddy + g) * (ddy + g) + ddx * ddx;
  *u1 = sqrt(n2);
  *u2 = (dddx * (ddy + g) - ddx * dddy) / n2;
}
__device__ __forceinline__ void quad_inputs(const double* cx, const double* cy, const PredictArgs& a, double u, double g, double* u1, double* u2) {
  quad_inputs(cx, cy, a.knots.k, a.degree, a.n_knots, a.inv_T, u, g, u1, u2);
}

__device__ __forceinline__ void quad_ode(const double* s, double u1, double u2, double g, double* k) {
  k[0] = s[2]; k[1] = s[3]; k[2] = u1 * sin(s[4]); k[3] = u1 * cos(s[4]) - g; k[4] = u2;
}

// warm-start shift of one row: every entry block <- T * block (`spline_extra.py:165-191`); scratch: LDS doubles for the
// largest block; all threads of the workgroup take part (barriers inside)
__device__ __forceinline__ void shift_row(double* __restrict__ xrow, const int32_t* __restrict__ entries, int n_ent,
                                          const double* __restrict__ Tm, double* scratch) {
  for (int e = 0; e < n_ent; ++e) {
    const int off = entries[4 * e], rows = entries[4 * e + 1], cols = entries[4 * e + 2];
    const double* Tmat = Tm + entries[4 * e + 3];
    double* xe = xrow + off;
    for (int i = threadIdx.x; i < rows * cols; i += blockDim.x) scratch[i] = xe[i];
    __syncthreads();
    for (int i = threadIdx.x; i < rows * cols; i += blockDim.x) {
      const int k = i / rows, r = i - k * rows;
      double acc = 0.0;
      for (int q = 0; q < rows; ++q) acc += Tmat[r * rows + q] * scratch[k * rows + q];
      xe[i] = acc;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// The plant in the loop (omgx_batch_set_plant; include/omgx.h states the semantics): a simulated integrator vehicle per agent --
// `Vehicle.simulate` / `Vehicle.predict` of the reference with its default options (`vehicles/vehicle.py:326-337, 370-390`),
// `ode` = input (Holonomic, Holonomic3D).  Two routines, called by the whole workgroup of an agent with the same arguments;
// thread k < n_spl owns spline k and adds its samples up in index order, every product and sum rounded on its own: the
// stand-alone kernels and the rollout kernel write the same bits.  With lag_tc set (omgx_batch_set_plant_lag) simulate passes the
// applied inputs through the reference's first-order actuator lag (`vehicle.py:378-381, 429-431`) in closed form on the sample grid.
// ---------------------------------------------------------------------------
struct PlantArgs {
  double* state; double* state_prev; double* input_last;      // [B, n_spl]
  const double* dist;                                         // [B, n_spl, max_updates, n_samp + 1] or nullptr
  int32_t* n_upd; int32_t* overflow; int32_t* under_way;      // [B]; overflow / under_way may be nullptr
  int coeff_off, n_spl, degree, n_knots, n_samp, max_updates, p_t, p_state0, p_input0, p_poseT;
  double sample_time, inv_T, stop_tol;
  KnotArg knots;
  const double* lag_tc; const double* lag_decay;              // [B] (omgx_batch_set_plant_lag): time constant, exp(-sample_time / it); nullptr: no lag
};
// what the rollout kernel's plant instance reads from device memory: the plant and the log its simulate writes (sg.log == nullptr: none)
struct PlantBlock { PlantArgs pl; SignalArgs sg; };

// LDS doubles the two routines stage the knots and the plan in (the de Boor recursions then read LDS, not device memory)
__host__ __device__ inline size_t plant_stage_doubles(int n_spl, int degree, int n_knots) {
  return (size_t)n_knots + (size_t)n_spl * (n_knots - degree - 1);
}
// knots -> stage[0 .. n_knots), coefficients [n_spl][L] -> behind them; every thread of the workgroup, a barrier at the end
// (Args: PlantArgs, or the FeedbackArgs of omgx_batch_predict_measured -- the plan fields of either)
template <class Args>
__device__ __forceinline__ void plant_stage(const Args& pl, const double* coeffs, double* stage) {
  const int n_c = pl.n_spl * (pl.n_knots - pl.degree - 1);
  for (int i = threadIdx.x; i < pl.n_knots; i += blockDim.x) stage[i] = pl.knots.k[i];
  for (int i = threadIdx.x; i < n_c; i += blockDim.x) stage[pl.n_knots + i] = coeffs[i];
  __syncthreads();
}

// nominal input of spline c (time derivative of the plan) at sample i of the update solved at t_rel; kk: the knots
template <class Args>
__device__ __forceinline__ double plant_input_at(const Args& pl, const double* kk, const double* c, double t_rel, int i) {
#pragma clang fp contract(off)
  const double u = (t_rel + i * pl.sample_time) * pl.inv_T;
  return spline_der_at(c, kk, pl.degree, span_of(kk, pl.degree, pl.n_knots, u), u, 1) * pl.inv_T;
}

// simulate: the vehicle of agent b travels the update just solved (coeffs [n_spl][L]: its plan, global memory or LDS; t_rel = p[p_t]
// of that solve).  sg (or nullptr): the log that takes the travelled samples; scratch (LDS): sample_scratch_doubles() doubles when sg
// is given, and plant_stage_doubles() behind them.  Barriers inside.
__device__ __noinline__ void plant_simulate_agent(const PlantArgs& pl, const SignalArgs* sg, int b, const double* coeffs, double t_rel,
                                                  double* scratch) {
  __syncthreads();      // (every thread reads n_upd[b] / count[b] before thread 0 moves them; the scratch may still be read by the fused store)
  const int nu = pl.n_upd[b];
  if (nu < 0 || nu >= pl.max_updates) {      // (the same branch in every thread) no disturbance block left
    if (threadIdx.x == 0 && pl.overflow) pl.overflow[b] = 1;
    return;
  }
  const int n_samp = pl.n_samp, L = pl.n_knots - pl.degree - 1;
  int cnt = 0, first = 1, n_col = 0;
  bool log_on = sg != nullptr;
  if (log_on) {
    cnt = sg->count[b];
    first = cnt == 0 ? 0 : 1;
    n_col = n_samp + 1 - first;
    if (cnt < 0 || cnt > sg->cap - n_col) {      // the log is full: this append is dropped as a whole, the vehicle travels on
      if (threadIdx.x == 0 && sg->overflow) sg->overflow[b] = 1;
      log_on = false;
    }
  }
  double* stage = scratch + (sg ? sample_scratch_doubles(sg->n_spl, sg->degree, sg->n_knots, sg->n_der) : 0);
  plant_stage(pl, coeffs, stage);
  double* lg = nullptr;
  if (log_on) {
    // the plan's own columns, as signals_append_agent writes them: column 0 ahead of the first append and the dinput row stay
    lg = sg->log + (size_t)b * sg->n_der * sg->n_spl * sg->cap + (cnt - first);
    sample_agent<double>(coeffs, scratch, sg->n_spl, sg->degree, sg->knots, sg->n_knots, sg->n_der, t_rel * sg->inv_T, sg->sample_time * sg->inv_T,
                         sg->inv_T, sg->cap, first, n_samp + 1, lg, (double*)nullptr);
    __syncthreads();
  }
  if ((int)threadIdx.x < pl.n_spl) {
#pragma clang fp contract(off)
    const int k = threadIdx.x;
    const double* kk = stage;
    const double* c = stage + pl.n_knots + k * L;
    const double* db = pl.dist ? pl.dist + (((size_t)b * pl.n_spl + k) * pl.max_updates + nu) * (size_t)(n_samp + 1) : nullptr;
    double s0;
    if (nu == 0) {      // the first simulate starts from the plan's own sample 0
      const double u0 = t_rel * pl.inv_T;
      s0 = spline_der_at(c, kk, pl.degree, span_of(kk, pl.degree, pl.n_knots, u0), u0, 0);
    } else s0 = pl.state[(size_t)b * pl.n_spl + k];
    double a0 = plant_input_at(pl, kk, c, t_rel, 0);
    double acc = 0.0, s = s0;
    if (pl.lag_tc) {      // (the same branch in every thread of the launch) the first-order actuator lag, include/omgx.h OMGX_HAS_PLANT_LAG
      const double tc = pl.lag_tc[b], decay = pl.lag_decay[b];
      // the lagged input starts from the last applied one; ahead of the first simulate from the plan's own sample 0, undisturbed
      double v0 = nu == 0 ? a0 : pl.input_last[(size_t)b * pl.n_spl + k];
      if (db) a0 = a0 + db[0];
      for (int i = 1; i <= n_samp; ++i) {
        double a1 = plant_input_at(pl, kk, c, t_rel, i);
        if (db) a1 = a1 + db[i];
        const double d = a1 - a0;
        const double sl = d / pl.sample_time;
        const double r = tc * sl;
        const double part = a1 - r;
        const double e0 = v0 - a0;
        const double hom = e0 + r;
        const double dec = hom * decay;
        const double v1 = part + dec;      // exact under the linearly interpolated command: particular solution + decayed rest
        const double w = v0 + v1;
        const double h = w / 2.0;
        acc = acc + h;
        const double m = pl.sample_time * acc;
        s = s0 + m;
        if (lg) {
          lg[(size_t)k * sg->cap + i] = s;
          if (sg->n_der >= 2) lg[((size_t)sg->n_spl + k) * sg->cap + i] = v1;
        }
        a0 = a1; v0 = v1;
      }
      a0 = v0;      // (input_last <- v_n)
    } else {
      if (db) a0 = a0 + db[0];
      for (int i = 1; i <= n_samp; ++i) {
        double a1 = plant_input_at(pl, kk, c, t_rel, i);
        if (db) a1 = a1 + db[i];
        const double h = (a0 + a1) / 2.0;
        acc = acc + h;
        const double m = pl.sample_time * acc;
        s = s0 + m;
        if (lg) {
          lg[(size_t)k * sg->cap + i] = s;
          if (sg->n_der >= 2) lg[((size_t)sg->n_spl + k) * sg->cap + i] = a1;
        }
        a0 = a1;
      }
    }
    pl.state_prev[(size_t)b * pl.n_spl + k] = s0;
    pl.state[(size_t)b * pl.n_spl + k] = s;
    pl.input_last[(size_t)b * pl.n_spl + k] = a0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    pl.n_upd[b] = nu + 1;
    if (log_on) sg->count[b] = cnt + n_col;
  }
}

// predict + stop test at the head of an update: reads the OLD plan (coeffs, global memory) and the OLD p[p_t], writes state0 / input0 /
// t into p.  Returns false when the agent's loop has ended (under_way[b] == 0 on entry, or the travelled state meets the criterion now:
// the flag is cleared) -- p is left as it is then.  Every thread computes the same numbers from the same loads.  stage (LDS):
// plant_stage_doubles() doubles.  Barriers inside.
__device__ __noinline__ bool plant_predict_agent(const PlantArgs& pl, int b, const double* coeffs, double* pb, double tau, double t_value,
                                                 double* stage) {
  const int nu = pl.n_upd[b];
  if (pl.under_way) {
    bool go = pl.under_way[b] != 0;
    if (go && nu >= 1) {
#pragma clang fp contract(off)
      double e2 = 0.0, u2 = 0.0;
      for (int k = 0; k < pl.n_spl; ++k) {
        const double e = pl.state[(size_t)b * pl.n_spl + k] - pb[pl.p_poseT + k], u = pl.input_last[(size_t)b * pl.n_spl + k];
        const double ee = e * e, uu = u * u;
        e2 = e2 + ee; u2 = u2 + uu;
      }
      if (sqrt(e2) <= pl.stop_tol && sqrt(u2) <= pl.stop_tol) go = false;
    }
    __syncthreads();      // (a thread that read the flag after thread 0 cleared it would take the same branch; the barrier keeps the loads ahead anyway)
    if (!go) {
      if (threadIdx.x == 0) pl.under_way[b] = 0;
      return false;
    }
  }
  const double t_rel = pb[pl.p_t];      // (the time the plan was solved at: read by every thread before thread 0 writes the new one)
  plant_stage(pl, coeffs, stage);
  if ((int)threadIdx.x < pl.n_spl) {
#pragma clang fp contract(off)
    const int k = threadIdx.x, L = pl.n_knots - pl.degree - 1;
    const double* kk = stage;
    const double* c = stage + pl.n_knots + k * L;
    double s0;
    if (nu <= 0) {      // (no simulate yet: the vehicle stands at the plan's own sample 0)
      const double u0 = t_rel * pl.inv_T;
      s0 = spline_der_at(c, kk, pl.degree, span_of(kk, pl.degree, pl.n_knots, u0), u0, 0);
    } else s0 = pl.state_prev[(size_t)b * pl.n_spl + k];
    double u_a = plant_input_at(pl, kk, c, t_rel, 0), acc = 0.0;
    for (int i = 1; i <= pl.n_samp; ++i) {
      const double u_b = plant_input_at(pl, kk, c, t_rel, i);
      const double h = (u_a + u_b) / 2.0;
      acc = acc + h;
      u_a = u_b;
    }
    const double m = pl.sample_time * acc;
    pb[pl.p_state0 + k] = s0 + m;
    pb[pl.p_input0 + k] = spline_der_at(c, kk, pl.degree, span_of(kk, pl.degree, pl.n_knots, tau), tau, 1) * pl.inv_T;
    if (k == 0) pb[pl.p_t] = t_value;
  }
  return true;
}

// ---------------------------------------------------------------------------
// States measured outside the loop (omgx_batch_predict_measured; include/omgx.h states the semantics): the prediction of
// `Vehicle.predict(state0=...)` / `enforce_states` / `enforce_inputs` (`vehicles/vehicle.py:302-337`) for the integrator classes.
// state / input / fresh may lie in pinned host memory: every value is read once, by the thread that owns it.
// ---------------------------------------------------------------------------
struct FeedbackArgs {
  const double* state; const double* input;      // [B, n_spl]; input: nullptr or the enforce form's
  const int32_t* fresh;                          // [B] or nullptr (= all)
  int coeff_off, n_spl, degree, n_knots, n_samp, n_out, p_off[4], p_t, enforce;
  double sample_time, inv_T;
  KnotArg knots;
};

// Agent b, called by its whole workgroup: reads the OLD plan (coeffs, global memory) and the OLD p[p_t], writes the initial
// conditions and the new t into p.  A fresh measurement: p_off[0] from the statements of plant_predict_agent with the measured state
// in the place of state_prev (the same bits for the same state), or the given values as they are (enforce); none: the statements of
// predict_kernel.  stage (LDS): feedback_lds_doubles() doubles -- the staged knots and plan, the nominal inputs behind them.  Barriers inside.
__host__ __device__ inline size_t feedback_lds_doubles(int n_spl, int degree, int n_knots, int n_samp) {
  return plant_stage_doubles(n_spl, degree, n_knots) + (size_t)n_spl * ((size_t)n_samp + 1);
}
__device__ __noinline__ void feedback_predict_agent(const FeedbackArgs& fb, int b, const double* coeffs, double* pb, double tau, double t_value,
                                                    double* stage) {
  const bool fresh = !fb.fresh || fb.fresh[b] != 0;      // (the same branch in every thread of the workgroup)
  const int k = threadIdx.x;
  if (fresh && fb.enforce) {
    if (k < fb.n_spl) {
      pb[fb.p_off[0] + k] = fb.state[(size_t)b * fb.n_spl + k];
      for (int o = 1; o < fb.n_out; ++o)
        if (fb.p_off[o] >= 0) pb[fb.p_off[o] + k] = (o == 1 && fb.input) ? fb.input[(size_t)b * fb.n_spl + k] : 0.0;
      if (k == 0) pb[fb.p_t] = t_value;
    }
    return;
  }
  const double t_rel = pb[fb.p_t];      // (the time the plan was solved at: read by every thread before thread 0 writes the new one)
  plant_stage(fb, coeffs, stage);
  const int L = fb.n_knots - fb.degree - 1, n_u = fb.n_samp + 1;
  const double* kk = stage;
  double* ub = stage + plant_stage_doubles(fb.n_spl, fb.degree, fb.n_knots);      // [n_spl][n_samp + 1]: the nominal inputs
  if (fresh) {
    // one (spline, sample) per thread: plant_input_at is a function of its arguments alone, the same bits whichever thread evaluates
    // it -- the de Boor recursions of an update run side by side instead of one after the other in the owner thread
    for (int q = k; q < fb.n_spl * n_u; q += blockDim.x) {
      const int ks = q / n_u;
      ub[q] = plant_input_at(fb, kk, stage + fb.n_knots + ks * L, t_rel, q - ks * n_u);
    }
    __syncthreads();
  }
  if (k >= fb.n_spl) return;
  const double* c = stage + fb.n_knots + k * L;
  const int j = span_of(kk, fb.degree, fb.n_knots, tau);
  if (fresh) {
#pragma clang fp contract(off)
    const double s0 = fb.state[(size_t)b * fb.n_spl + k];
    const double* u = ub + k * n_u;
    double u_a = u[0], acc = 0.0;
    for (int i = 1; i <= fb.n_samp; ++i) {      // (the owner thread adds up in index order: the statements of plant_predict_agent)
      const double u_b = u[i];
      const double h = (u_a + u_b) / 2.0;
      acc = acc + h;
      u_a = u_b;
    }
    const double m = fb.sample_time * acc;
    pb[fb.p_off[0] + k] = s0 + m;
  } else {
    pb[fb.p_off[0] + k] = spline_der_at(c, kk, fb.degree, j, tau, 0);
  }
  double sc = fb.inv_T;
  for (int o = 1; o < fb.n_out; ++o) {
    if (fb.p_off[o] >= 0) pb[fb.p_off[o] + k] = spline_der_at(c, kk, fb.degree, j, tau, o) * sc;
    sc *= fb.inv_T;
  }
  if (k == 0) pb[fb.p_t] = t_value;
}

// ---------------------------------------------------------------------------
// The Quadrotor's plant (omgx_batch_plant_quadrotor_simulate / _predict; include/omgx.h OMGX_HAS_PLANT_QUADROTOR states the
// semantics): `Vehicle.simulate` / `Vehicle.predict` of the reference with the model's own `ode` (`vehicles/quadrotor.py:149-152`) and
// `Quadrotor.check_terminal_conditions` (104-110).  Stand-alone launches only, one workgroup of 64 threads per agent, shaped like
// feedback_predict_kernel: knots and plan staged in LDS, lane i <= n_samp evaluates the inputs of sample i (quad_inputs: a function
// of its arguments alone), one owner lane walks the Runge-Kutta chain in index order, lanes write the log columns.  The arguments
// travel by value: every pointer is a kernel argument.
// ---------------------------------------------------------------------------
struct QuadPlantArgs {
  double* state; double* state_prev;                          // [B, 5]
  double* input_last; double* dspl_last;                      // [B, 2]
  const double* dist;                                         // [B, 2, max_updates, n_samp + 1] or nullptr
  int32_t* n_upd; int32_t* overflow; int32_t* under_way;      // [B]; overflow / under_way may be nullptr
  double* log_state; double* log_input;                       // [B, 5, cap], [B, 2, cap] next to the spline log, or nullptr
  int coeff_off, n_spl, degree, n_knots, n_samp, max_updates, p_t, p_poseT, p_off[3];
  double sample_time, inv_T, stop_tol, g;
  KnotArg knots;
};

// LDS doubles behind the staged knots and plan: inputs [2][n_samp + 1], state samples [5][n_samp + 1], the nominal inputs of sample 0 [2]
__host__ __device__ inline size_t quad_plant_lds_doubles(int degree, int n_knots, int n_samp) {
  return plant_stage_doubles(2, degree, n_knots) + 7 * ((size_t)n_samp + 1) + 2;
}

// abscissa of sample i of the update solved at t_rel: one statement for simulate and predict (the same bits)
__device__ __forceinline__ double quad_sample_u(const QuadPlantArgs& pl, double t_rel, int i) {
#pragma clang fp contract(off)
  return (t_rel + i * pl.sample_time) * pl.inv_T;
}

// the plan's own state at u: (x, y, dx, dy, atan2(ddx, ddy + g)) (`quadrotor.py:136-140`); kk, cx, cy: LDS
__device__ __forceinline__ void quad_plan_state(const QuadPlantArgs& pl, const double* kk, const double* cx, const double* cy, double u, double* s) {
  const int j = span_of(kk, pl.degree, pl.n_knots, u);
  const double s2 = pl.inv_T * pl.inv_T;
  s[0] = spline_der_at(cx, kk, pl.degree, j, u, 0);
  s[1] = spline_der_at(cy, kk, pl.degree, j, u, 0);
  s[2] = spline_der_at(cx, kk, pl.degree, j, u, 1) * pl.inv_T;
  s[3] = spline_der_at(cy, kk, pl.degree, j, u, 1) * pl.inv_T;
  s[4] = atan2(spline_der_at(cx, kk, pl.degree, j, u, 2) * s2, spline_der_at(cy, kk, pl.degree, j, u, 2) * s2 + pl.g);
}

// one sample interval of the chain: the stage statements of predict_quadrotor_kernel, every product and sum rounded on its own
__device__ __forceinline__ void quad_rk4_step(double* s, double u1a, double u2a, double u1b, double u2b, double h, double g) {
#pragma clang fp contract(off)
  double k1[5], k2[5], k3[5], k4[5], st[5];
  const double u1m = 0.5 * (u1a + u1b), u2m = 0.5 * (u2a + u2b);
  quad_ode(s, u1a, u2a, g, k1);
#pragma unroll
  for (int q = 0; q < 5; ++q) st[q] = s[q] + 0.5 * h * k1[q];
  quad_ode(st, u1m, u2m, g, k2);
#pragma unroll
  for (int q = 0; q < 5; ++q) st[q] = s[q] + 0.5 * h * k2[q];
  quad_ode(st, u1m, u2m, g, k3);
#pragma unroll
  for (int q = 0; q < 5; ++q) st[q] = s[q] + h * k3[q];
  quad_ode(st, u1b, u2b, g, k4);
#pragma unroll
  for (int q = 0; q < 5; ++q) s[q] += (h / 6.0) * (k1[q] + 2.0 * k2[q] + 2.0 * k3[q] + k4[q]);
}

// ---------------------------------------------------------------------------
// Obstacle scripts (omgx_batch_set_obstacle_script; include/omgx.h OMGX_HAS_OBSTACLE_SCRIPT states the semantics): the reference's
// `simulation={'trajectories': ...}` -- at given times a value is added to an obstacle's position, velocity or acceleration, between
// the jumps it moves with constant acceleration (`environment/obstacle.py:172-264`).  One routine carries the parameters x, v, a of
// every listed obstacle of an agent over one update; lane 4 q + i (i < n_dim <= 3, q < n_obst <= 8: the first 32 lanes of whoever
// calls) owns component i of obstacle q and walks the agent's event list on its own.  Every product and sum is rounded on its
// own: an update without an event writes the bits of `splines.advance_obstacles`, the stand-alone kernel and the rollout kernel
// write the same bits.  No barrier inside; lanes >= 32 return at once.
// ---------------------------------------------------------------------------
struct ObstacleScriptArgs {
  const double* time; const int32_t* what; const double* value;      // [B, n_ev] ascending per agent (pads +inf), [B, n_ev], [B, n_ev, 3]
  int n_ev, n_obst, obst[8][4];                                      // {p_x, p_v, p_a, n_dim}
  const double* t_abs; int n_t;                                      // the rollout's: absolute time of every step boundary [n_t]
};

constexpr double kScriptEps = 1e-9;      // (the tolerance of `splines.since_knot`)

__device__ __noinline__ void obstacles_advance_agent(const ObstacleScriptArgs& sc, int b, double* pb, double t_prev, double t_now, double dt,
                                                     int lane) {
#pragma clang fp contract(off)
  const int q = lane >> 2, i = lane & 3;
  if (lane < 0 || q >= sc.n_obst || q >= 8) return;
  const int ox = sc.obst[q][0], ov = sc.obst[q][1], oa = sc.obst[q][2], nd = sc.obst[q][3];
  if (i >= nd) return;
  double x = pb[ox + i], v = pb[ov + i], a = pb[oa + i];
  const double* te = sc.time + (size_t)b * sc.n_ev;
  const int32_t* we = sc.what + (size_t)b * sc.n_ev;
  const double* ve = sc.value + (size_t)b * sc.n_ev * 3;
  const double lo = t_prev + kScriptEps, hi = t_now + kScriptEps;
  double t_cur = t_prev;
  bool any = false, a_moved = false;
  for (int e = 0; e < sc.n_ev; ++e) {
    const double t_e = te[e];
    if (!(t_e > lo)) continue;      // (behind this update; a NaN is no event)
    if (t_e > hi) break;            // (ascending: the rest lies ahead)
    any = true;
    double h = 0.0, c2 = 0.0;
    if (t_cur == t_prev && t_now - t_e <= kScriptEps) {      // the event sits on t_now and nothing split the update: the whole-interval statements
      h = dt; c2 = 0.5 * dt * dt; t_cur = t_now;
    } else {
      const double t_to = t_e < t_now ? t_e : t_now;
      const double hh = t_to - t_cur;
      if (hh > kScriptEps) { h = hh; c2 = 0.5 * hh * hh; t_cur = t_to; }
    }
    if (h > 0.0) {
      const double m1 = h * v, m2 = c2 * a, m3 = h * a;
      const double s1 = m1 + m2;
      x = x + s1;
      v = v + m3;
    }
    const int w = we[e];
    if (w >= 3 * q && w < 3 * q + 3) {
      const double val = ve[3 * (size_t)e + i];
      if (w == 3 * q) x = x + val;
      else if (w == 3 * q + 1) v = v + val;
      else { a = a + val; a_moved = true; }
    }
  }
  double h = dt, c2 = 0.5 * dt * dt;
  if (any) { h = t_now - t_cur; c2 = 0.5 * h * h; }
  if (!any || h > kScriptEps) {
    const double m1 = h * v, m2 = c2 * a, m3 = h * a;
    const double s1 = m1 + m2;
    x = x + s1;
    v = v + m3;
  }
  pb[ox + i] = x;
  pb[ov + i] = v;
  if (a_moved) pb[oa + i] = a;
}

// ---------------------------------------------------------------------------
// Missions (omgx_batch_set_mission; include/omgx.h OMGX_HAS_MISSION states the semantics): a list of goals per agent.  When the stop
// rule holds for an agent that has a goal left, the next leg starts: what the reference does between two `simulator.run()` calls --
// `set_terminal_conditions`, `reinitialize`, the first update with `enforce_states`.  mission_next_leg_agent is the only statement
// of that switch; its two callers are the stand-alone kernel below and the rollout kernel's MISSION instances.
// ---------------------------------------------------------------------------
struct MissionArgs {
  const double* goals; const int32_t* n_goals;      // [B, G, n_spl], [B]
  int32_t* leg; int32_t* clock; int32_t* arrivals;  // [B], [B], [B, 1 + G]
  const double* x_reset;                            // [n_var]: the agent-independent row of the first guess (the handle's device copy)
  int G, o_state0, o_input0, o_poseT, p_t, coeff_off, n_spl, L, n_var, n_con;
  int K, step0;                                     // the following rollout: steps per agent, and the count its first step is stamped with
  omgx::Opts o_cold;                                // the option set of a leg's first solve
};

// The leg switch of agent b, called by `nthr` threads tid = 0 .. nthr - 1 that own the agent (a workgroup, or one wave) with the same
// arguments.  lg = leg[b], read by the caller ahead of its last barrier: the goal to fly to is goals[b][lg].  s_old (thread k <
// n_spl: spline k): p[state0 + k] of the PREVIOUS update, where the guess starts; now [n_spl]: where the vehicle is (may be
// p + o_state0 itself: thread k reads now[k] before it writes).  Thread k writes the L coefficients of spline k by numpy's linspace
// statement, every product and sum rounded on its own.  No barrier inside: the caller parts it from what reads x, lam and p next.
__device__ __noinline__ void mission_next_leg_agent(const MissionArgs& ms, int b, int lg, double* pb, double* xb, double* lamb, double s_old,
                                                    const double* now, int step_index, int tid, int nthr) {
#pragma clang fp contract(off)
  const int n = ms.n_spl, L = ms.L, c_lo = ms.coeff_off, c_hi = ms.coeff_off + n * L;
  for (int i = tid; i < ms.n_var; i += nthr)
    if (i < c_lo || i >= c_hi) xb[i] = ms.x_reset[i];
  for (int i = tid; i < ms.n_con; i += nthr) lamb[i] = 0.0;
  if (tid < n) {
    const int k = tid;
    const double g = ms.goals[((size_t)b * ms.G + lg) * n + k], here = now[k];
    const double delta = g - s_old;
    const double step = delta / (double)(L - 1);
    double* c = xb + c_lo + k * L;
    for (int i = 0; i < L - 1; ++i) {
      const double m = (double)i * step;
      c[i] = m + s_old;
    }
    c[L - 1] = g;
    pb[ms.o_poseT + k] = g;
    pb[ms.o_state0 + k] = here;
    pb[ms.o_input0 + k] = 0.0;
    if (k == 0) {
      pb[ms.p_t] = 0.0;
      ms.clock[b] = 0;
      ms.arrivals[(size_t)b * (ms.G + 1) + lg] = step_index;
      ms.leg[b] = lg + 1;
    }
  }
}

// the plant's stop rule on the travelled state (the statements of plant_predict_agent's test)
__device__ __forceinline__ bool mission_plant_arrived(const PlantArgs& pl, int b, const double* pb) {
#pragma clang fp contract(off)
  if (pl.n_upd[b] < 1) return false;
  double e2 = 0.0, u2 = 0.0;
  for (int k = 0; k < pl.n_spl; ++k) {
    const double e = pl.state[(size_t)b * pl.n_spl + k] - pb[pl.p_poseT + k], u = pl.input_last[(size_t)b * pl.n_spl + k];
    const double ee = e * e, uu = u * u;
    e2 = e2 + ee; u2 = u2 + uu;
  }
  return sqrt(e2) <= pl.stop_tol && sqrt(u2) <= pl.stop_tol;
}

// ---------------------------------------------------------------------------
// Free end time (omgx_batch_set_free_t; include/omgx.h OMGX_HAS_FREE_T states the semantics): the step glue of a batch whose motion
// time T is a variable of every agent's own, x[o_T] -- the first stop clause, the prediction and the warm-start shift all read it, so
// none of them can be a host-side table.  The shift of a column is  c' = proj . y,  y_j = the old spline at s + (1 - s) fit_j, with
// the two constant tables of its basis; FreeTArgs lives in device memory (the handle's copy), fit / proj behind it.
// ---------------------------------------------------------------------------
struct FreeTBasis {
  int degree, n_knots, n_fit, rows;
  const double* fit;        // [n_fit]
  const double* proj;       // [rows][n_fit]
  KnotArg knots;
};
struct FreeTArgs {
  KnotArg knots;                                    // the plan, as PredictArgs holds it
  int coeff_off, n_spl, degree, n_knots, n_out, p_off[4], p_t;
  int o_T, n_ent, n_basis;
  double update_time;                               // (read by the append)
  int ent[OMGX_FREE_T_MAX_ENT][4];                  // {offset, rows, cols, basis}
  FreeTBasis basis[OMGX_FREE_T_MAX_BASIS];
};

// ---------------------------------------------------------------------------
// Rollout: K receding-horizon steps of every agent in ONE launch (omgx_batch_rollout).  Agents of a point-to-point batch
// are independent, so nothing in the protocol asks for a barrier between the steps of different agents: a persistent
// workgroup takes an agent and runs its whole loop -- ideal prediction from the current plan, obstacles advanced, the
// knot-crossing shift of the plan and of the multipliers, warm-started solve -- K times, statement for statement what
// `BatchP2P.step` issues as separate launches (predict_kernel, tensor updates, shift_kernel, index_select, solve): the same
// bits per agent (tests/test_gpu_rollout.py).  What it removes is the step barrier: with 1024 agents on 512 resident
// workgroups a step launched on its own is two rounds plus a third for whoever a straggler displaced.
// ---------------------------------------------------------------------------
struct RolloutStep { double tau, t_rel; int32_t crossed, pad; };
struct RolloutArgs {
  KnotArg knots;
  int coeff_off, n_spl, degree, n_knots, n_out, p_off[4], p_t;
  double inv_T, dt;
  int n_obst, obst[8][4];
  const int32_t* sh_ent; int n_ent; const double* sh_T;
  const int32_t* lam_perm;
  const RolloutStep* steps; int K;
  omgx::Opts o_cross;
  unsigned long long* stats;            // [K][4] {solved, sum of iterations, max, agents} or nullptr
  int32_t* iters_log; int32_t* status_log;     // [K][n_agents] or nullptr
  StopArgs stop; int stop_on;           // omgx_batch_set_stop: an agent's loop ends at the step its state meets the criterion
  const PlantBlock* plant;              // omgx_batch_set_plant: read by the PLANT instance only
  const ObstacleScriptArgs* script;     // omgx_batch_set_obstacle_script: read by the SCRIPT instances only
  const MissionArgs* mission;           // omgx_batch_set_mission: read by the MISSION instances only ...
  int n_table;                          // ... as is the length of `steps`, there a table indexed by the agent's own leg clock
};

// ---------------------------------------------------------------------------
// The glue kernels that call an out-of-line routine of this header which the rollout kernel calls too (omgx_agent_kernels.h).
// The compiler sizes such a routine for the largest workgroup that calls it inside the same code object, so these kernels are
// compiled where the 512-thread callers are -- beside the rollout instances of mode 0, omgx_inst_rollout_lds.hip -- and the
// stand-alone launch and the rollout launch run one and the same copy of the routine.  The host unit launches them by name
// through these declarations; sample_kernel is a template whose <float> instance belongs to the host unit and whose <double>
// instance (sample_agent<double> is what the fused store and the log call) is instantiated in that unit.
// ---------------------------------------------------------------------------
__global__ void signals_append_kernel(const double* __restrict__ x, int n_var, const double* __restrict__ p, int n_par,
                                      const int32_t* __restrict__ under_way, SignalArgs sg);
__global__ void plant_simulate_kernel(const double* __restrict__ x, int n_var, const double* __restrict__ p, int n_par, const PlantBlock* __restrict__ pb);
__global__ void plant_predict_kernel(const double* __restrict__ x, int n_var, double* __restrict__ p, int n_par, int B, const PlantBlock* __restrict__ pb,
                                     double tau, double t_value, const int32_t* __restrict__ ord_iters, int32_t* __restrict__ ord_out,
                                     const double* __restrict__ ord_dw);
__global__ void plant_quadrotor_simulate_kernel(const double* __restrict__ x, int n_var, const double* __restrict__ p, int n_par, QuadPlantArgs pl, SignalArgs sg);
// (the Quadrotor plant's predict kernel calls none of those routines: it goes where its simulate kernel goes, the two come out of
// the compiler as they did only when they are compiled together)
__global__ void plant_quadrotor_predict_kernel(const double* __restrict__ x, int n_var, double* __restrict__ p, int n_par, int B, QuadPlantArgs pl, double tau,
                                               double t_value, const double* __restrict__ states, const int32_t* __restrict__ fresh_mask, int enforce,
                                               const int32_t* __restrict__ ord_iters, int32_t* __restrict__ ord_out, const double* __restrict__ ord_dw);
__global__ void obstacles_advance_kernel(double* __restrict__ p, int n_par, int B, const ObstacleScriptArgs* __restrict__ sc, double t_prev, double t_now, double dt);
__global__ void mission_advance_kernel(double* __restrict__ p, double* __restrict__ x, double* __restrict__ lam, int n_par, int B,
                                       const MissionArgs* __restrict__ msp, StopArgs sa, const PlantBlock* __restrict__ plant, int step_index);
__global__ void free_t_append_kernel(const double* __restrict__ x, int n_var, const int32_t* __restrict__ under_way, SignalArgs sg, int o_T, double update_time);

template <typename OutT>
__global__ void __launch_bounds__(256)
sample_kernel(const double* __restrict__ x, int x_stride, int coeff_off, int n_spl, int degree,
              KnotArg knots, int n_knots, int n_der,
              const double* __restrict__ t0, double dt, double inv_T, int n_samp, OutT* __restrict__ out,
              OutT* __restrict__ v_tot) {
  extern __shared__ __align__(16) double lds[];
  const int b = blockIdx.y;
  const int i_end = min(n_samp, (int)(blockIdx.x + 1) * OMGX_SAMPLE_CHUNK);
  sample_agent<OutT>(x + (size_t)b * x_stride + coeff_off, lds, n_spl, degree, knots, n_knots, n_der, t0[b], dt, inv_T,
                     n_samp, blockIdx.x * OMGX_SAMPLE_CHUNK, i_end, out + (size_t)b * n_der * n_spl * n_samp,
                     v_tot ? v_tot + (size_t)b * n_samp : nullptr);
}
extern template __global__ void sample_kernel<double>(const double*, int, int, int, int, KnotArg, int, int, const double*, double, double, int, double*, double*);

// ---------------------------------------------------------------------------
// The ipm_* kernels as the host unit sees them: pointer types and selectors.  Every selector below is DEFINED in exactly one
// instance unit, and that definition is the one place where its template instances are named -- an instance named in two units
// would be compiled and registered twice (tests/test_build_units_cpu.py).
// ---------------------------------------------------------------------------
typedef void (*ipm_kernel_t)(omgx::Dims, omgx::Tables, omgx::Opts, int, const double*, const double*, const double*,
                             const double*, int, double*, double*, int32_t*, int32_t*, int, long long*, double*, size_t, double*,
                             const int32_t*, const StoreArgs*, int, int*, const double*, int, int32_t*, unsigned long long*, int, const CenterArgs*,
                             double*, size_t, const StopArgs*);
typedef void (*ipm_prepare_kernel_t)(omgx::Dims, omgx::Tables, omgx::Opts, const double*, const double*, const double*, const double*, int,
                                     const double*, const int32_t*, int, double*, size_t, int);
typedef void (*ipm_eval_kernel_t)(omgx::Dims, omgx::Tables, int, const double*, const double*, const double*, int, double*,
                                  size_t, double*);
typedef void (*ipm_rollout_t)(omgx::Dims, omgx::Tables, omgx::Opts, int, double*, double*, const double*, const double*, int, double*,
                              int32_t*, int32_t*, int, double*, size_t, double*, int*, const RolloutArgs*, int, const int32_t*, const StoreArgs*);

// (the selectors are internal to the library: hidden, so that its dynamic symbol table stays the C ABI of include/omgx.h)
#define OMGX_UNIT __attribute__((visibility("hidden")))
// The solve kernel's instances by family; each returns null for a mode its family has no instance of.
OMGX_UNIT ipm_kernel_t solve_wave_kernel(int mode);                    // wave path, every feature: modes 0 / 4 / 5    (omgx_inst_solve_wave.hip)
OMGX_UNIT ipm_kernel_t solve_refine_kernel(int mode);                  // the same three with REFINE                   (omgx_inst_solve_refine.hip)
OMGX_UNIT ipm_kernel_t solve_lean_kernel(int mode);                    // the same three with LEAN                     (omgx_inst_solve_lean.hip)
OMGX_UNIT ipm_kernel_t solve_blocked_kernel(int mode);                 // blocked factorisation: modes 0 - 3, never null (omgx_inst_solve_blocked.hip)
OMGX_UNIT ipm_kernel_t solve_general_kernel(int mode, int wave_ok);    // GEN, every mode, never null                  (omgx_inst_solve_general.hip)
OMGX_UNIT ipm_eval_kernel_t ipm_eval_kernel_for(int mode, int wave_ok, int general);      // (omgx_inst_eval.hip, as the next one)
OMGX_UNIT ipm_prepare_kernel_t ipm_prepare_kernel_for(int general);
// The rollout kernel's instances of one workspace mode: the (PLANT, SCRIPT, MISSION) table, written once in
// omgx_rollout_kernel.h and instantiated in the unit of the mode (omgx_inst_rollout_lds.hip, _jac_only, _jac_hv).
template <int MODE> OMGX_UNIT ipm_rollout_t rollout_kernel_of(int plant, int script, int mission);
extern template ipm_rollout_t rollout_kernel_of<omgx::WS_LDS>(int, int, int);
extern template ipm_rollout_t rollout_kernel_of<omgx::WS_JAC_ONLY>(int, int, int);
extern template ipm_rollout_t rollout_kernel_of<omgx::WS_JAC_HV>(int, int, int);
