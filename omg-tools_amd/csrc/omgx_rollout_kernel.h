// omgx_rollout_kernel.h -- the ipm_rollout_kernel template (its argument structs and what it removes: omgx_device.h, "Rollout")
// and the table of its instances per workspace mode.  Included by the three units omgx_inst_rollout_*.hip and by nothing else.
#pragma once
#include "omgx_device.h"
#include "omgx_core.h"

// PLANT (omgx_batch_set_plant): step (1) is the plant's predict + stop test on the travelled state, and after the solve the plant's
// simulate takes the place of the log append; every other statement is the same one.
// SCRIPT (omgx_batch_set_obstacle_script): step (2) is obstacles_advance_agent between the absolute times of the step; every other
// statement is the same one.
// MISSION (omgx_batch_set_mission): the step record is steps[clock[b]], the agent's own leg clock; where the stop rule holds and the
// agent has a goal left, mission_next_leg_agent runs instead of the end of the loop and that step's solve is the cold one; every other
// statement is the same one.
template <int MODE, bool WAVE_ONLY, bool GEN, bool PLANT = false, bool SCRIPT = false, bool MISSION = false>
__global__ void __launch_bounds__(512)
ipm_rollout_kernel(omgx::Dims d, omgx::Tables T, omgx::Opts o, int kkt_doubles, double* __restrict__ p, double* __restrict__ x,
                   const double* __restrict__ lb, const double* __restrict__ ub, int bounds_shared, double* __restrict__ lam,
                   int32_t* __restrict__ status, int32_t* __restrict__ iters, int n_agents, double* __restrict__ slabs,
                   size_t slab_doubles, double* __restrict__ dw_state, int* __restrict__ next_slot,
                   const RolloutArgs* __restrict__ rop, int stagger, const int32_t* __restrict__ order,
                   const StoreArgs* __restrict__ stp) {
  extern __shared__ __align__(16) double lds[];
  omgx::Work w;
  omgx::work_carve_split<MODE>(w, lds, MODE == omgx::WS_LDS ? nullptr : slabs + (size_t)blockIdx.x * slab_doubles, d, kkt_doubles);
  omgx::CtxT<omgx::SolveFlags<MODE, WAVE_ONLY, GEN>> c; c.red = w.red;
  c.prof = nullptr;
  __shared__ int slot_lds[2];      // (the slot queue as in the solve kernel: null when the grid covers the batch, else asked ahead)
  int slot_par = 0;
  if (stagger > 0 && (__builtin_amdgcn_s_getreg(6148) & 1))
    for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(127);
  const int K = rop->K;
  // (agents in the caller's order -- the ones whose last solve was slow first: a workgroup that gets a long loop early is
  // given a short one by the queue afterwards)
  for (int slot = blockIdx.x; slot < n_agents;) {
    const int b = order ? order[slot] : slot;
    if (next_slot && threadIdx.x == 0) slot_lds[slot_par] = gridDim.x + atomicAdd(next_slot, 1);
    double* pb = p + (size_t)b * d.n_par;
    double* xb = x + (size_t)b * d.n_var;
    double* lamb = lam + (size_t)b * d.n_con;
    const double* lbb = lb + (bounds_shared ? 0 : (size_t)b * d.n_con);
    const double* ubb = ub + (bounds_shared ? 0 : (size_t)b * d.n_con);
    for (int k = 0; k < K; ++k) {
      int ck = k;
      [[maybe_unused]] bool leg_start = false;      // (MISSION: this step starts the agent's next leg)
      [[maybe_unused]] double s_old = 0.0;          // (MISSION: p[state0] of the previous update, read ahead of the prediction)
      if constexpr (MISSION) {
        const MissionArgs& ms = *rop->mission;
        ck = ms.clock[b];
        if (ck < 0 || ck >= rop->n_table) break;      // (a clock outside the table the caller filled: the loop ends, nothing is read)
        if ((int)threadIdx.x < ms.n_spl) s_old = pb[ms.o_state0 + threadIdx.x];
      }
      const RolloutStep st = rop->steps[ck];
      // (1) ideal prediction (predict_kernel): the plan and its time derivatives at tau, the new t
      if constexpr (PLANT) {
        // the plant's: state0 from the state the vehicle had one update ago, the stop rule on the travelled state -- an agent that
        // has arrived ends its loop here, ahead of the glue of the step: plan, multipliers and status stay as they are
        if constexpr (MISSION) {
          // (the flag ahead of the test tells a loop that ends now from one that had ended: only the former may start a leg)
          const MissionArgs& ms = *rop->mission;
          const int was = rop->plant->pl.under_way ? rop->plant->pl.under_way[b] : 0;
          if (!plant_predict_agent(rop->plant->pl, b, xb + rop->plant->pl.coeff_off, pb, st.tau, st.t_rel, w.kkt)) {
            const int lg = ms.leg[b];
            leg_start = was != 0 && lg >= 0 && lg < ms.G && lg < ms.n_goals[b];
            __syncthreads();      // (every thread has read the leg; thread 0 has cleared the flag)
            if (leg_start) {
              // the next leg starts from the travelled state; p is as the previous update left it: p[state0] is the stale one
              mission_next_leg_agent(ms, b, lg, pb, xb, lamb, s_old, rop->plant->pl.state + (size_t)b * ms.n_spl, ms.step0 + k, threadIdx.x, blockDim.x);
              if (threadIdx.x == 0) rop->plant->pl.under_way[b] = 1;
            } else {
              if (threadIdx.x == 0) {
                if (was != 0 && lg >= 0 && lg <= ms.G) ms.arrivals[(size_t)b * (ms.G + 1) + lg] = ms.step0 + k;
                iters[b] = 0;
                for (int k2 = k; k2 < K; ++k2) {
                  if (rop->iters_log) rop->iters_log[(size_t)k2 * n_agents + b] = 0;
                  if (rop->status_log) rop->status_log[(size_t)k2 * n_agents + b] = status[b];
                }
              }
              break;
            }
          }
        } else
        if (!plant_predict_agent(rop->plant->pl, b, xb + rop->plant->pl.coeff_off, pb, st.tau, st.t_rel, w.kkt)) {      // (the KKT store is idle between two solves: scratch)
          if (threadIdx.x == 0) {
            iters[b] = 0;
            for (int k2 = k; k2 < K; ++k2) {
              if (rop->iters_log) rop->iters_log[(size_t)k2 * n_agents + b] = 0;
              if (rop->status_log) rop->status_log[(size_t)k2 * n_agents + b] = status[b];
            }
          }
          break;
        }
      } else {
        const int n_spl = rop->n_spl, degree = rop->degree, n_knots = rop->n_knots, n_out = rop->n_out;
        const int L = n_knots - degree - 1;
        if ((int)threadIdx.x < n_spl) {
          const int ks = threadIdx.x;
          const double* cc = xb + rop->coeff_off + ks * L;
          const int j = span_of(rop->knots.k, degree, n_knots, st.tau);
          double sc = 1.0;
          for (int q = 0; q < n_out; ++q) {
            if (rop->p_off[q] >= 0) pb[rop->p_off[q] + ks] = spline_der_at(cc, rop->knots.k, degree, j, st.tau, q) * sc;
            sc *= rop->inv_T;
          }
          if (ks == 0 && rop->p_t >= 0) pb[rop->p_t] = st.t_rel;
        }
      }
      // (2) obstacles move on: x <- x + (dt v + dt^2 / 2 a), v <- v + dt a (each product and sum rounded on its own, as the
      //     tensor statements of BatchP2P.step are)
      if constexpr (SCRIPT) {
        // with a script: the same motion, split at the events of this update (absolute times t_abs[k] .. t_abs[k + 1])
        const ObstacleScriptArgs* sc = rop->script;
        obstacles_advance_agent(*sc, b, pb, sc->t_abs[k], sc->t_abs[k + 1], rop->dt, threadIdx.x);
      } else for (int q = 0; q < rop->n_obst; ++q) {
        const int ox = rop->obst[q][0], ov = rop->obst[q][1], oa = rop->obst[q][2], nd = rop->obst[q][3];
        if ((int)threadIdx.x < nd) {
#pragma clang fp contract(off)      // (no fused multiply-add here: the tensor statements round every product)
          const int i = threadIdx.x;
          const double dt = rop->dt, c2 = 0.5 * dt * dt;
          const double pv = pb[ov + i], pa = pb[oa + i];
          const double m1 = dt * pv, m2 = c2 * pa, m3 = dt * pa;
          const double s1 = m1 + m2;
          pb[ox + i] = pb[ox + i] + s1;
          pb[ov + i] = pv + m3;
        }
      }
      __syncthreads();
      // (3) knot crossing: plan <- T plan, multipliers by index (the KKT store is idle between two solves: scratch)
      if (st.crossed && !leg_start) {      // (a leg that starts here has a fresh plan and no multipliers)
        shift_row(xb, rop->sh_ent, rop->n_ent, rop->sh_T, w.kkt);
        for (int i = threadIdx.x; i < d.n_con; i += blockDim.x) w.kkt[i] = lamb[i];
        __syncthreads();
        for (int i = threadIdx.x; i < d.n_con; i += blockDim.x) { const int s = rop->lam_perm[i]; lamb[i] = s >= 0 ? w.kkt[s] : 0.0; }
        __syncthreads();
      }
      // stop rule (omgx_batch_set_stop), where the solve kernel of the per-step path tests it -- after the glue of the step: the
      // vehicle has arrived, its loop ends here (`execution/simulator.py:39-62`): plan, multipliers and status stay as they are,
      // the remaining steps of the call log iters 0
      if (rop->stop_on) {
        const StopArgs sa = rop->stop;
        bool go = sa.under_way[b] != 0;
        [[maybe_unused]] const bool was = go;
        if (go && omgx::stop_criterium(pb, sa.o_state, sa.o_input, sa.o_pose, sa.n_dim, sa.tol)) go = false;
        __syncthreads();
        if constexpr (MISSION && !PLANT) {
          if (was && !go) {      // (arrived now: the same branch in every thread)
            const MissionArgs& ms = *rop->mission;
            const int lg = ms.leg[b];
            leg_start = lg >= 0 && lg < ms.G && lg < ms.n_goals[b];
            __syncthreads();      // (every thread has read the leg)
            if (leg_start) {
              // the state the prediction of this step wrote is where the vehicle is now; the arrival test is not repeated on the new goal
              mission_next_leg_agent(ms, b, lg, pb, xb, lamb, s_old, pb + ms.o_state0, ms.step0 + k, threadIdx.x, blockDim.x);
              __syncthreads();
              go = true;
            } else if (lg >= 0 && lg <= ms.G && threadIdx.x == 0) ms.arrivals[(size_t)b * (ms.G + 1) + lg] = ms.step0 + k;
          }
        }
        if (!go) {
          if (threadIdx.x == 0) {
            sa.under_way[b] = 0; iters[b] = 0;
            for (int k2 = k; k2 < K; ++k2) {
              if (rop->iters_log) rop->iters_log[(size_t)k2 * n_agents + b] = 0;
              if (rop->status_log) rop->status_log[(size_t)k2 * n_agents + b] = status[b];
            }
          }
          break;
        }
      }
      // (4) warm-started solve, results back to the agent's rows
      omgx::Result r;
      if constexpr (MISSION) {
        // (a leg's first solve is the cold one: its own option set, no multipliers, no status, no carried inertia correction)
        omgx::Opts os = st.crossed ? rop->o_cross : o;
        if (leg_start) os = rop->mission->o_cold;
        const bool warm = o.warm_start && !leg_start;
        r = omgx::ipm_solve(c, d, T, os, w, pb, xb, lbb, ubb, warm ? lamb : nullptr, warm ? status[b] : 0, kkt_doubles, warm ? dw_state[b] : 0.0);
      } else
      r = omgx::ipm_solve(c, d, T, st.crossed ? rop->o_cross : o, w, pb, xb, lbb, ubb, o.warm_start ? lamb : nullptr,
                          o.warm_start ? status[b] : 0, kkt_doubles, o.warm_start ? dw_state[b] : 0.0);
      __builtin_amdgcn_s_setprio(0);
      __syncthreads();
      for (int i = threadIdx.x; i < d.n_var; i += blockDim.x) xb[i] = w.x[i];
      for (int q = threadIdx.x; q < d.n_con; q += blockDim.x)
        lamb[q] = (r.status == 3 || w.rtype[q] == omgx::ROW_FREE) ? 0.0 : w.rho[q] * w.z[q];
      if (threadIdx.x == 0) {
        status[b] = r.status; iters[b] = r.iters; dw_state[b] = r.dw;
        if (rop->stats) {
          unsigned long long* sk = rop->stats + 4 * (size_t)k;
          atomicAdd(sk + 0, r.status == 0 ? 1ull : 0ull);
          atomicAdd(sk + 1, (unsigned long long)r.iters);
          atomicMax(sk + 2, (unsigned long long)r.iters);
          atomicAdd(sk + 3, 1ull);
        }
        if (rop->iters_log) rop->iters_log[(size_t)k * n_agents + b] = r.iters;
        if (rop->status_log) rop->status_log[(size_t)k * n_agents + b] = r.status;
        if constexpr (MISSION) { if (!leg_start) rop->mission->clock[b] = ck + 1; }      // (the switch has set a new leg's clock to 0)
      }
      if (stp) {      // `Vehicle.store` of this step (omgx_batch_set_store), as in the solve kernel's epilogue
        const StoreArgs st2 = *stp;
        if (st2.out) {
          __syncthreads();
          sample_agent<double>(w.x + st2.coeff_off, w.kkt, st2.n_spl, st2.degree, st2.knots, st2.n_knots, st2.n_der, st2.t0[b],
                               st2.dt, st2.inv_T, st2.n_samp, 0, st2.n_samp, st2.out + (size_t)b * st2.n_der * st2.n_spl * st2.n_samp,
                               st2.v_tot ? st2.v_tot + (size_t)b * st2.n_samp : nullptr);
        }
        // the travelled trajectory of this step (omgx_batch_set_signals): every update of the manoeuvre is logged inside the launch
        if constexpr (!PLANT) {
        const SignalArgs& sg = reinterpret_cast<const StoreBlock*>(stp)->sg;
        if (sg.log) signals_append_agent(sg, b, w.x + sg.coeff_off, pb[sg.p_t], w.kkt);
        }
      }
      // the vehicle travels this update (plant_simulate_agent): the travelled samples go to the plant's own log
      if constexpr (PLANT) {
        const PlantBlock* pk = rop->plant;
        plant_simulate_agent(pk->pl, pk->sg.log ? &pk->sg : nullptr, b, w.x + pk->pl.coeff_off, pb[pk->pl.p_t], w.kkt);
      }
      __syncthreads();
    }
    // (a loop that ended early left without a barrier: this one parts the agent's last use of the scratch from the next agent's
    // first, and publishes the slot thread 0 asked for)
    __syncthreads();
    slot = next_slot ? slot_lds[slot_par] : slot + (int)gridDim.x;
    slot_par ^= 1;
  }
  if (next_slot && threadIdx.x == 0) queue_leave(next_slot);
}

// The instances of one mode (the classes of the wave path without quartic terms / cos / sin atoms: the receding-horizon classes
// that fit LDS): with and without the plant, and with an obstacle script or a mission or neither -- none with both.
template <int MODE>
ipm_rollout_t rollout_kernel_of(int plant, int script, int mission) {
  if (mission) {
    if (script) return nullptr;
    return plant ? ipm_rollout_kernel<MODE, true, false, true, false, true> : ipm_rollout_kernel<MODE, true, false, false, false, true>;
  }
  if (script) return plant ? ipm_rollout_kernel<MODE, true, false, true, true> : ipm_rollout_kernel<MODE, true, false, false, true>;
  return plant ? ipm_rollout_kernel<MODE, true, false, true> : ipm_rollout_kernel<MODE, true, false>;
}
