// omgx_agent_kernels.h -- the glue kernels that call an out-of-line routine the rollout kernel calls too: signals_append_agent /
// sample_agent<double>, plant_simulate_agent, plant_predict_agent, obstacles_advance_agent, mission_next_leg_agent.  Included by
// omgx_inst_rollout_lds.hip and by nothing else (omgx_device.h says why, and declares them for the host unit, which launches them
// by name).  plant_quadrotor_predict_kernel calls none of them and is here because plant_quadrotor_simulate_kernel is.
#pragma once
#include "omgx_device.h"

// stand-alone append for a given x, p (omgx_batch_signals_append): one workgroup per agent; under_way (optional): agents whose
// loop the stop rule has ended are not appended
__global__ void __launch_bounds__(256)
signals_append_kernel(const double* __restrict__ x, int n_var, const double* __restrict__ p, int n_par,
                      const int32_t* __restrict__ under_way, SignalArgs sg) {
  extern __shared__ __align__(16) double lds[];
  const int b = blockIdx.x;
  if (under_way && under_way[b] == 0) return;
  signals_append_agent(sg, b, x + (size_t)b * n_var + sg.coeff_off, p[(size_t)b * n_par + sg.p_t], lds);
}

// stand-alone launches (omgx_batch_plant_simulate / omgx_batch_plant_predict): one workgroup per agent; an agent whose loop the stop
// rule has ended is not simulated.  The predict launch carries the launch order of the next solve as predict_kernel does.
__global__ void __launch_bounds__(256)
plant_simulate_kernel(const double* __restrict__ x, int n_var, const double* __restrict__ p, int n_par, const PlantBlock* __restrict__ pb) {
  extern __shared__ __align__(16) double lds[];
  const int b = blockIdx.x;
  const PlantArgs& pl = pb->pl;
  if (pl.under_way && pl.under_way[b] == 0) return;
  plant_simulate_agent(pl, pb->sg.log ? &pb->sg : nullptr, b, x + (size_t)b * n_var + pl.coeff_off, p[(size_t)b * n_par + pl.p_t], lds);
}

__global__ void __launch_bounds__(256)
plant_predict_kernel(const double* __restrict__ x, int n_var, double* __restrict__ p, int n_par, int B, const PlantBlock* __restrict__ pb,
                     double tau, double t_value, const int32_t* __restrict__ ord_iters, int32_t* __restrict__ ord_out,
                     const double* __restrict__ ord_dw) {
  extern __shared__ __align__(16) double lds[];
  if (ord_iters && blockIdx.x == gridDim.x - 1) { order_block(ord_iters, ord_dw, ord_out, B); return; }
  const int b = blockIdx.x;
  if (b >= B) return;
  const PlantArgs& pl = pb->pl;
  (void)plant_predict_agent(pl, b, x + (size_t)b * n_var + pl.coeff_off, p + (size_t)b * n_par, tau, t_value, lds);
}

// simulate: the vehicle of agent blockIdx.x travels the update just solved.  sg.log == nullptr: no log.  Dynamic LDS:
// sample_scratch_doubles() (with a log) + quad_plant_lds_doubles() doubles.
__global__ void __launch_bounds__(64)
plant_quadrotor_simulate_kernel(const double* __restrict__ x, int n_var, const double* __restrict__ p, int n_par, QuadPlantArgs pl, SignalArgs sg) {
  extern __shared__ __align__(16) double lds[];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (pl.under_way && pl.under_way[b] == 0) return;
  const int nu = pl.n_upd[b];      // (every thread reads n_upd[b] / count[b]; lane 0 moves them behind the last barrier)
  if (nu < 0 || nu >= pl.max_updates) {      // (the same branch in every thread) no disturbance block left
    if (lane == 0 && pl.overflow) pl.overflow[b] = 1;
    return;
  }
  const int n_samp = pl.n_samp, n_u = n_samp + 1, L = pl.n_knots - pl.degree - 1;
  int cnt = 0, first = 1, n_col = 0;
  bool log_on = sg.log != nullptr;
  if (log_on) {
    cnt = sg.count[b];
    first = cnt == 0 ? 0 : 1;
    n_col = n_u - first;
    if (cnt < 0 || cnt > sg.cap - n_col) {      // the log is full: this append is dropped as a whole, the vehicle travels on
      if (lane == 0 && sg.overflow) sg.overflow[b] = 1;
      log_on = false;
    }
  }
  const double* coeffs = x + (size_t)b * n_var + pl.coeff_off;
  const double t_rel = p[(size_t)b * n_par + pl.p_t];
  double* stage = lds + (sg.log ? sample_scratch_doubles(sg.n_spl, sg.degree, sg.n_knots, sg.n_der) : 0);
  plant_stage(pl, coeffs, stage);
  if (log_on) {
    // the plan's own columns (the reference's `dspl` / `ddspl` signals), as signals_append_agent writes them
    sample_agent<double>(coeffs, lds, sg.n_spl, sg.degree, sg.knots, sg.n_knots, sg.n_der, t_rel * sg.inv_T, sg.sample_time * sg.inv_T, sg.inv_T,
                         sg.cap, first, n_u, sg.log + (size_t)b * sg.n_der * sg.n_spl * sg.cap + (cnt - first), (double*)nullptr);
  }
  const double* kk = stage;
  const double* cx = stage + pl.n_knots;
  const double* cy = cx + L;
  double* ua = stage + plant_stage_doubles(2, pl.degree, pl.n_knots);      // [2][n_u] applied inputs
  double* ss = ua + 2 * n_u;                                                // [5][n_u] state samples
  double* un0 = ss + 5 * n_u;                                               // [2] nominal inputs of sample 0
  if (lane < n_u) {
    double u1, u2;
    quad_inputs(cx, cy, kk, pl.degree, pl.n_knots, pl.inv_T, quad_sample_u(pl, t_rel, lane), pl.g, &u1, &u2);
    if (lane == 0) { un0[0] = u1; un0[1] = u2; }
    if (pl.dist) {
      const double* db = pl.dist + ((size_t)b * 2 * pl.max_updates + nu) * (size_t)n_u + lane;
      u1 = u1 + db[0];
      u2 = u2 + db[(size_t)pl.max_updates * n_u];
    }
    ua[lane] = u1; ua[n_u + lane] = u2;
  }
  __syncthreads();
  if (lane == 0) {      // the owner lane: the chain in index order
    double s[5], s0[5];
    quad_plan_state(pl, kk, cx, cy, quad_sample_u(pl, t_rel, 0), s0);      // (column 0 of the log; the start of the first simulate)
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      s[q] = nu == 0 ? s0[q] : pl.state[(size_t)b * 5 + q];
      pl.state_prev[(size_t)b * 5 + q] = s[q];
      ss[q * n_u] = s0[q];
    }
    for (int i = 0; i < n_samp; ++i) {
      quad_rk4_step(s, ua[i], ua[n_u + i], ua[i + 1], ua[n_u + i + 1], pl.sample_time, pl.g);
#pragma unroll
      for (int q = 0; q < 5; ++q) ss[q * n_u + i + 1] = s[q];
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) pl.state[(size_t)b * 5 + q] = s[q];
    pl.input_last[(size_t)b * 2] = ua[n_samp];
    pl.input_last[(size_t)b * 2 + 1] = ua[n_u + n_samp];
  } else if (lane <= 2) {      // lanes 1, 2: the plan's velocity at the last travelled sample
    const int k = lane - 1;
    pl.dspl_last[(size_t)b * 2 + k] = plant_input_at(pl, kk, k ? cy : cx, t_rel, n_samp);
  }
  __syncthreads();
  if (log_on && pl.log_state) {
    double* ls = pl.log_state + (size_t)b * 5 * sg.cap + (cnt - first);
    double* li = pl.log_input + (size_t)b * 2 * sg.cap + (cnt - first);
    for (int e = lane; e < 5 * n_u; e += 64) {
      const int q = e / n_u, i = e - q * n_u;
      if (i >= first) ls[(size_t)q * sg.cap + i] = ss[e];
    }
    for (int e = lane; e < 2 * n_u; e += 64) {
      const int q = e / n_u, i = e - q * n_u;
      if (i >= first) li[(size_t)q * sg.cap + i] = i == 0 ? un0[q] : ua[e];      // (column 0: the plan's sample 0, undisturbed)
    }
  }
  if (lane == 0) {
    pl.n_upd[b] = nu + 1;
    if (log_on) sg.count[b] = cnt + n_col;
  }
}

// predict + stop test at the head of an update (states == nullptr), or the prediction from measured states [B, 5] (device or pinned
// host memory: every value is read once, by the owner lane) with a `fresh` mask [B] (nullptr: all) and the `enforce` form.  Reads the
// OLD plan and the OLD p[p_t], writes spl0 / dspl0 / ddspl0 and the new t into p.  The launch carries the launch order of the next
// solve as plant_predict_kernel does (block B is not an agent).  Dynamic LDS: quad_plant_lds_doubles() doubles.
__global__ void __launch_bounds__(64)
plant_quadrotor_predict_kernel(const double* __restrict__ x, int n_var, double* __restrict__ p, int n_par, int B, QuadPlantArgs pl, double tau,
                               double t_value, const double* __restrict__ states, const int32_t* __restrict__ fresh_mask, int enforce,
                               const int32_t* __restrict__ ord_iters, int32_t* __restrict__ ord_out, const double* __restrict__ ord_dw) {
  extern __shared__ __align__(16) double lds[];
  if (ord_iters && blockIdx.x == gridDim.x - 1) { order_block(ord_iters, ord_dw, ord_out, B); return; }
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  double* pb = p + (size_t)b * n_par;
  int nu = 1;
  if (!states) {
    nu = pl.n_upd[b];
    if (pl.under_way) {
      bool go = pl.under_way[b] != 0;
      if (go && nu >= 1) {
#pragma clang fp contract(off)
        const double ex = pl.state[(size_t)b * 5] - pb[pl.p_poseT], ey = pl.state[(size_t)b * 5 + 1] - pb[pl.p_poseT + 1];
        const double vx = pl.dspl_last[(size_t)b * 2], vy = pl.dspl_last[(size_t)b * 2 + 1];
        const double exx = ex * ex, eyy = ey * ey, vxx = vx * vx, vyy = vy * vy;
        const double e2 = exx + eyy, v2 = vxx + vyy;
        if (sqrt(e2) <= pl.stop_tol && sqrt(v2) <= pl.stop_tol) go = false;
      }
      __syncthreads();      // (every thread has read the flag before lane 0 clears it)
      if (!go) {
        if (lane == 0) pl.under_way[b] = 0;
        return;
      }
    }
  }
  const bool fresh = !states || !fresh_mask || fresh_mask[b] != 0;      // (the same branch in every thread of the workgroup)
  if (states && fresh && enforce) {      // `Quadrotor.set_initial_conditions`: the measured position, at rest
    if (lane < 2) {
      pb[pl.p_off[0] + lane] = states[(size_t)b * 5 + lane];
      pb[pl.p_off[1] + lane] = 0.0;
      pb[pl.p_off[2] + lane] = 0.0;
      if (lane == 0) pb[pl.p_t] = t_value;
    }
    return;
  }
  const double t_rel = pb[pl.p_t];      // (the time the plan was solved at: read by every thread before lane 0 writes the new one)
  plant_stage(pl, x + (size_t)b * n_var + pl.coeff_off, lds);
  const int n_samp = pl.n_samp, n_u = n_samp + 1, L = pl.n_knots - pl.degree - 1;
  const double* kk = lds;
  const double* cx = lds + pl.n_knots;
  const double* cy = cx + L;
  double* ua = lds + plant_stage_doubles(2, pl.degree, pl.n_knots);      // [2][n_u] nominal inputs
  if (fresh) {
    if (lane < n_u) quad_inputs(cx, cy, kk, pl.degree, pl.n_knots, pl.inv_T, quad_sample_u(pl, t_rel, lane), pl.g, &ua[lane], &ua[n_u + lane]);
    __syncthreads();
    if (lane == 0) {
      double s[5];
      if (states || nu >= 1) {
        const double* src = states ? states + (size_t)b * 5 : pl.state_prev + (size_t)b * 5;
#pragma unroll
        for (int q = 0; q < 5; ++q) s[q] = src[q];
      } else quad_plan_state(pl, kk, cx, cy, quad_sample_u(pl, t_rel, 0), s);      // (no simulate yet: the vehicle stands at the plan's own sample 0)
      for (int i = 0; i < n_samp; ++i) quad_rk4_step(s, ua[i], ua[n_u + i], ua[i + 1], ua[n_u + i + 1], pl.sample_time, pl.g);
      pb[pl.p_off[0]] = s[0];
      pb[pl.p_off[0] + 1] = s[1];
    }
  }
  if (lane >= 2) return;
  const double* c = lane ? cy : cx;
  const int j = span_of(kk, pl.degree, pl.n_knots, tau);
  if (!fresh) pb[pl.p_off[0] + lane] = spline_der_at(c, kk, pl.degree, j, tau, 0);      // (the statements of predict_kernel)
  double sc = pl.inv_T;
  for (int o = 1; o < 3; ++o) {
    pb[pl.p_off[o] + lane] = spline_der_at(c, kk, pl.degree, j, tau, o) * sc;
    sc *= pl.inv_T;
  }
  if (lane == 0) pb[pl.p_t] = t_value;
}

// stand-alone launch (omgx_batch_obstacles_advance): eight agents share a workgroup, 32 lanes each
__global__ void __launch_bounds__(256)
obstacles_advance_kernel(double* __restrict__ p, int n_par, int B, const ObstacleScriptArgs* __restrict__ sc, double t_prev, double t_now, double dt) {
  const int b = blockIdx.x * 8 + (threadIdx.x >> 5);
  if (b >= B) return;
  obstacles_advance_agent(*sc, b, p + (size_t)b * n_par, t_prev, t_now, dt, threadIdx.x & 31);
}

// stand-alone launch (omgx_batch_mission_advance): the arrival test and the switch without a solve; four agents share a workgroup,
// one wave each.  plant (or nullptr): the rule is the plant's and the leg starts from the travelled state.
__global__ void __launch_bounds__(256)
mission_advance_kernel(double* __restrict__ p, double* __restrict__ x, double* __restrict__ lam, int n_par, int B,
                       const MissionArgs* __restrict__ msp, StopArgs sa, const PlantBlock* __restrict__ plant, int step_index) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const MissionArgs& ms = *msp;
  double* pb = p + (size_t)b * n_par;
  if (sa.under_way[b] == 0) return;
  const bool hit = plant ? mission_plant_arrived(plant->pl, b, pb) : omgx::stop_criterium(pb, sa.o_state, sa.o_input, sa.o_pose, sa.n_dim, sa.tol);
  if (!hit) return;
  const int lg = ms.leg[b];
  if (lg < 0 || lg > ms.G) return;
  const double s_old = lane < ms.n_spl ? pb[ms.o_state0 + lane] : 0.0;
  // (one wave: every lane has its loads of the flag, the leg and the state behind it before lane 0 stores any of them)
  __builtin_amdgcn_wave_barrier();
  if (lg < ms.G && lg < ms.n_goals[b]) {
    mission_next_leg_agent(ms, b, lg, pb, x + (size_t)b * ms.n_var, lam + (size_t)b * ms.n_con, s_old,
                           plant ? plant->pl.state + (size_t)b * ms.n_spl : pb + ms.o_state0, step_index, lane, 64);
  } else if (lane == 0) {
    sa.under_way[b] = 0;
    ms.arrivals[(size_t)b * (ms.G + 1) + lg] = step_index;
  }
}

// The travelled log for a per-agent horizon (omgx_batch_free_t_append): signals_append_agent with the agent's own inv_T = 1 / T,
// t_rel = 0 and its own number of samples -- all of an update's, or what is left of the plan (`Problem.simulate`'s shortened span),
// or none.  One workgroup per agent; T is the same in every thread, so every branch is the workgroup's.
__global__ void __launch_bounds__(256)
free_t_append_kernel(const double* __restrict__ x, int n_var, const int32_t* __restrict__ under_way, SignalArgs sg, int o_T, double update_time) {
  extern __shared__ __align__(16) double lds[];
  const int b = blockIdx.x;
  if (under_way && under_way[b] == 0) return;
  const double T = x[(size_t)b * n_var + o_T];
  if (!(T >= sg.sample_time)) return;      // (a NaN too)
  if (!(T >= update_time)) {
    const int n_b = (int)floor(T / sg.sample_time + 5e-7);
    sg.n_samp = n_b < sg.n_samp ? n_b : sg.n_samp;
  }
  if (sg.n_samp < 1) return;
  sg.inv_T = 1.0 / T;
  signals_append_agent(sg, b, x + (size_t)b * n_var + sg.coeff_off, 0.0, lds);
}

// (the <double> instance of the sampling kernel: the one that shares sample_agent<double> with the fused store and the log)
template __global__ void sample_kernel<double>(const double*, int, int, int, int, KnotArg, int, int, const double*, double, double, int, double*, double*);
