// omgx_solve_kernels.h -- the kernel templates around one solve: ipm_solve_kernel, ipm_prepare_kernel, ipm_eval_kernel.  Included
// by the instance units that name their instances (omgx_inst_solve_*.hip, omgx_inst_eval.hip) and by nothing else: the host unit
// sees the kernels only as the pointers the selectors of omgx_device.h return.
//
//   ipm_solve_kernel   one 512-thread workgroup (8 waves) per agent, whole interior-point
//                      solve with every per-agent array resident in LDS
//                      (<= 160 KiB / CU); only p, x0, bounds are read from HBM and
//                      x, lam_g, status written back.
//                      Instances: per workspace mode, general or not, and -- for the benchmark
//                      classes (wave path, modes 0 / 4 / 5) -- REFINE (refinement of regularised steps)
//                      and LEAN (every optional block compiled out: stop rule, restarts, prepared
//                      setup, ADMM centre, fused store / log, absolute tolerances).  omgx_batch_solve
//                      picks per launch: LEAN exactly when the launch uses none of them.
#pragma once
#include "omgx_device.h"
#include "omgx_core.h"

// LEAN: the instance for launches that leave every optional feature off -- no stop rule, no fused store / signals, no ADMM centre, no
// prepared setup, no restart pass or restart guesses, no absolute tolerances (omgx::CtxFlags lean), no refinement: the plain
// receding-horizon solve of the benchmark classes.  Those blocks are compiled out (the arguments stay: one signature, one launch
// site); omgx_batch_solve picks the instance per launch from what it is about to pass (lean_launch).  What stays is what such a
// launch uses: order, stats, dw_state, stagger, prio_iter, warm start, the dynamic slot hand-out, bounds_shared.
template <int MODE, bool WAVE_ONLY, bool GEN, bool REFINE = false, bool LEAN = false>
__global__ void __launch_bounds__(512)
ipm_solve_kernel(omgx::Dims d, omgx::Tables T, omgx::Opts o, int kkt_doubles,
                 const double* __restrict__ p, const double* __restrict__ x0,
                 const double* __restrict__ lb, const double* __restrict__ ub, int bounds_shared,
                 double* __restrict__ x, double* __restrict__ lam, int32_t* __restrict__ status,
                 int32_t* __restrict__ iters, int n_agents, long long* __restrict__ prof,
                 double* __restrict__ slabs, size_t slab_doubles, double* __restrict__ dw_state,
                 const int32_t* __restrict__ order, const StoreArgs* __restrict__ stp, int only_failed,
                 int* __restrict__ next_slot, const double* __restrict__ x0_alt, int n_alt, int32_t* __restrict__ attempts,
                 unsigned long long* __restrict__ stats, int stagger, const CenterArgs* __restrict__ ctr,
                 double* __restrict__ prep, size_t prep_doubles, const StopArgs* __restrict__ stop) {
#ifdef OMGX_PROFILE
  long long t_mark = clock64();      // kernel entry, then the end of every solve of this workgroup (PH_WG_HEAD, PH_WG_TAIL)
  int b_last = -1;
#endif
  extern __shared__ __align__(16) double lds[];
  omgx::Work w;
    omgx::work_carve_split<MODE>(w, lds, MODE == omgx::WS_LDS ? nullptr : slabs + (size_t)blockIdx.x * slab_doubles,
                               d, kkt_doubles);
  omgx::CtxT<omgx::SolveFlags<MODE, WAVE_ONLY, GEN, REFINE, LEAN>> c; c.red = w.red;
#ifdef OMGX_PROFILE
  __shared__ long long prof_lds[omgx::PH_COUNT];
  c.prof = prof_lds;
#else
  c.prof = nullptr;
#endif
  // `prep` (round 6): the setup of every agent's solve -- parameter stage, Jacobian and rows at x0, classification, scaling, start
  // values -- was done for the whole batch by ipm_prepare_kernel ahead of this launch; a solve then starts by loading its record.
  // The matrix descriptors (the same for every agent) are written once per workgroup.
  [[maybe_unused]] double* const jval_own = w.jval;      // (the lean instance never rebinds w.jval)
  // (the descriptors are rewritten per solve only where the fused trajectory store may use the space behind a small KKT store as scratch)
  const bool describe_once = LEAN || prep != nullptr || stp == nullptr;
  if (describe_once) omgx::kkt_descriptors(c, d, T, w, true);
  // mode 0: one workgroup per agent.  Spill modes: the grid is capped at the number of HBM
  // slabs and every workgroup walks over its agents.
  // `order` (optional) maps launch slots to agents: the host can put expected stragglers first so
  // that their long solves overlap the rest of the batch instead of trailing it
  // Spill modes hand the launch slots out dynamically (next_slot[0]: a counter that is zero at every launch -- the
  // workgroup that finishes last resets it, next_slot[1] counts the finished ones):
  // solves differ by a factor of several in their iteration counts, and a fixed share of agents per workgroup would
  // leave most of the chip waiting for the unluckiest one.  Which workgroup solves an agent does not change its result.
  // A launch whose grid covers the batch (one agent per workgroup) gets next_slot = nullptr from the host: every fetch would
  // return a slot past the end.  Otherwise thread 0 asks for the next slot BEFORE the solve and the workgroup reads the answer
  // behind the barrier that ends the iteration: the atomic's round trip runs under the solve, no barrier of its own.  Two words,
  // used in turn: thread 0 may be writing the answer of iteration i + 1 while a slower wave still reads that of iteration i.
  __shared__ int slot_lds[2];
  int slot_par = 0;
  // Two workgroups per CU start together and would run their (equally long) solves in lockstep -- both in a one-wave
  // phase, then both in an all-waves phase.  The workgroup in the second wave slot starts `stagger` x 8 k cycles late.
  if (stagger > 0 && (__builtin_amdgcn_s_getreg(6148) & 1))      // HW_ID[3:0] = wave slot within the SIMD
    for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(127);
  for (int slot = blockIdx.x; slot < n_agents;) {
    const int b = order ? order[slot] : slot;
    if (next_slot && threadIdx.x == 0) slot_lds[slot_par] = gridDim.x + atomicAdd(next_slot, 1);
    // (the slot of the next iteration, behind a barrier that every path out of this one passes)
    const auto next_agent = [&]() { slot = next_slot ? slot_lds[slot_par] : slot + (int)gridDim.x; slot_par ^= 1; };
    // restart pass (OMGX_ONLY_FAILED): agents that are solved already keep x, lam_g, status, iters
    if constexpr (!LEAN) { if (only_failed && status[b] == 0) { __syncthreads(); next_agent(); continue; } }
    // stop rule (omgx_batch_set_stop): a vehicle whose loop has ended -- the criterion held at this or an earlier update -- is not
    // solved again: it keeps its plan (x <- x0), its multipliers and its status; iters = 0.  Every thread evaluates the same
    // numbers from the same loads (a thread that reads the flag after thread 0 cleared it takes the same branch).
    if constexpr (!LEAN)
    if (stop) {
      const StopArgs sa = *stop;
      bool go = sa.under_way[b] != 0;
      if (go && omgx::stop_criterium(p + (size_t)b * d.n_par, sa.o_state, sa.o_input, sa.o_pose, sa.n_dim, sa.tol)) go = false;
      if (!go) {
        for (int i = threadIdx.x; i < d.n_var; i += blockDim.x) x[(size_t)b * d.n_var + i] = x0[(size_t)b * d.n_var + i];
        if (threadIdx.x == 0) { sa.under_way[b] = 0; iters[b] = 0; }
        __syncthreads();
        next_agent();
        continue;
      }
    }
#ifdef OMGX_PROFILE
    if (threadIdx.x < omgx::PH_COUNT) prof_lds[threadIdx.x] = 0;
    __syncthreads();
    const long long t_begin = clock64();
    // (what PH_TOTAL does not cover: from kernel entry, or from the end of the workgroup's previous solve, to here)
    if (threadIdx.x == 0) prof_lds[omgx::PH_WG_HEAD] = t_begin - t_mark;
    b_last = b;
#endif
    const double* lbb = lb + (bounds_shared ? 0 : (size_t)b * d.n_con);
    const double* ubb = ub + (bounds_shared ? 0 : (size_t)b * d.n_con);
    // Restart guesses (omgx_batch_set_restarts; cold solves only): an agent that does not converge from x0 is solved
    // again from x0_alt[0], x0_alt[1], ... by the same workgroup right away -- a separate pass over the failed agents
    // would leave the chip to a handful of them for as long as their slowest solve takes.
    omgx::Result r;
    int attempt = 0;
    if constexpr (LEAN) {      // (one setup, one iteration: the statements of attempt 0 below without a prepared record)
      const omgx::Start st = omgx::ipm_setup(c, d, T, o, w, p + (size_t)b * d.n_par, x0 + (size_t)b * d.n_var, lbb, ubb,
                                             o.warm_start ? lam + (size_t)b * d.n_con : nullptr, o.warm_start ? status[b] : 0, kkt_doubles, false);
      r = omgx::ipm_iterate(c, d, T, o, w, lbb, ubb, st, kkt_doubles, o.warm_start ? dw_state[b] : 0.0);
      __builtin_amdgcn_s_setprio(0);
      __syncthreads();
    } else
    for (;;) {
      const double* xs = attempt == 0 ? x0 + (size_t)b * d.n_var : x0_alt + ((size_t)(attempt - 1) * n_agents + b) * d.n_var;
      omgx::Start st;
      if (prep && attempt == 0) {
        double* rec = prep + (size_t)b * prep_doubles;
        if (omgx::ws_jac_hbm(MODE)) w.jval = rec + omgx::prep_layout(d).jval;      // (the scaled Jacobian stays where the setup kernel left it)
        st = omgx::ipm_load_start<omgx::ws_jac_hbm(MODE)>(c, d, w, rec);
      } else {
        w.jval = jval_own;
        st = omgx::ipm_setup(c, d, T, o, w, p + (size_t)b * d.n_par, xs, lbb, ubb, o.warm_start ? lam + (size_t)b * d.n_con : nullptr,
                             o.warm_start ? status[b] : 0, kkt_doubles, !describe_once);
      }
      r = omgx::ipm_iterate(c, d, T, o, w, lbb, ubb, st, kkt_doubles, o.warm_start ? dw_state[b] : 0.0);
      __builtin_amdgcn_s_setprio(0);
      __syncthreads();
      if (r.status == 0 || o.warm_start || attempt >= n_alt) break;
      ++attempt;
    }
    if constexpr (!LEAN) { if (attempts && threadIdx.x == 0) attempts[b] = attempt; }
    for (int i = threadIdx.x; i < d.n_var; i += blockDim.x) x[(size_t)b * d.n_var + i] = w.x[i];
    for (int q = threadIdx.x; q < d.n_con; q += blockDim.x)
      lam[(size_t)b * d.n_con + q] =
          (r.status == 3 || w.rtype[q] == omgx::ROW_FREE) ? 0.0 : w.rho[q] * w.z[q];
    if (threadIdx.x == 0) {
      status[b] = r.status; iters[b] = r.iters; dw_state[b] = r.dw;
      if (stats) {      // launch statistics (omgx_batch_set_stats): integer atomics, the same totals in any order
        atomicAdd(stats + 0, r.status == 0 ? 1ull : 0ull);
        atomicAdd(stats + 1, (unsigned long long)r.iters);
        atomicMax(stats + 2, (unsigned long long)r.iters);
        atomicAdd(stats + 3, 1ull);
      }
    }
    if constexpr (!LEAN)
    if (ctr) {
      // the ADMM x-update's centre (`omgx_admm_center_ex`) from the solution in LDS: no launch of its own
      const CenterArgs ca = *ctr;
      const int ns = ca.n_dim * ca.L;
      const int slot = ca.pub_inv ? ca.pub_inv[b] : -1;
      for (int q = threadIdx.x; q < ns; q += blockDim.x) {
        const double v = w.x[ca.x_spl + q] + p[(size_t)b * d.n_par + ca.p_rel + q / ca.L];
        ca.x_i[(size_t)b * ns + q] = v;
        if (slot >= 0) ca.x_send[(size_t)slot * ns + q] = v;
      }
    }
    if constexpr (!LEAN)
    if (stp) {
      // `Vehicle.store` fused behind the solve (reference `vehicles/vehicle.py:250-300`): the trajectories of
      // this agent straight from the solution in LDS; the KKT store is free now and serves as scratch
      // (the specification sits in device memory: as a by-value kernel argument its 90 dwords would be kept in
      // scalar registers across the whole solve)
      const StoreArgs st = *stp;
      if (st.out) {
        __syncthreads();
        sample_agent<double>(w.x + st.coeff_off, w.kkt, st.n_spl, st.degree, st.knots, st.n_knots, st.n_der, st.t0[b],
                             st.dt, st.inv_T, st.n_samp, 0, st.n_samp, st.out + (size_t)b * st.n_der * st.n_spl * st.n_samp,
                             st.v_tot ? st.v_tot + (size_t)b * st.n_samp : nullptr);
      }
      // the travelled trajectory of this update (omgx_batch_set_signals): the specification sits behind the store's
      const SignalArgs& sg = reinterpret_cast<const StoreBlock*>(stp)->sg;
      if (sg.log) signals_append_agent(sg, b, w.x + sg.coeff_off, p[(size_t)b * d.n_par + sg.p_t], w.kkt);
      if (prep) { __syncthreads(); omgx::kkt_descriptors(c, d, T, w, true); }      // (the scratch may have reached the descriptors)
    }
#ifdef OMGX_PROFILE
    __syncthreads();
    if (threadIdx.x == 0) prof_lds[omgx::PH_TOTAL] = clock64() - t_begin;
    __syncthreads();
    if (prof && threadIdx.x < omgx::PH_COUNT) prof[(size_t)b * omgx::PH_COUNT + threadIdx.x] = prof_lds[threadIdx.x];
    t_mark = clock64();
#endif
    __syncthreads();
    next_agent();
  }
  if (next_slot && threadIdx.x == 0) queue_leave(next_slot);
#ifdef OMGX_PROFILE
  // from the end of the workgroup's last solve to its exit, on the account of that solve (the thread that zeroed the entry with
  // the solve's other counters writes it: same thread, same address, program order)
  if (threadIdx.x == 0) prof_lds[omgx::PH_WG_TAIL] = clock64() - t_mark;
  __syncthreads();
  if (prof && b_last >= 0 && threadIdx.x == omgx::PH_WG_TAIL) prof[(size_t)b_last * omgx::PH_COUNT + omgx::PH_WG_TAIL] = prof_lds[omgx::PH_WG_TAIL];
#endif
}

// Round 6: the setup of a batch of solves as a kernel of its own -- north_star's "basis evaluation on the sample grid and the
// constraint Jacobian assembled with coalesced loads across a batch of agents".  One workgroup per agent, a few KB of LDS
// (atoms, knots, slots, x) and half the registers of the solve kernel: four to eight workgroups per CU hide the table-load
// latencies that the same statements pay in full at the head of the solve kernel, where two agents fill a CU (78 k of the
// 339 k cycles of a warm-started solve, profiles/r05_phase_cycles_mpc.json).  Same device function (omgx::ipm_setup), same
// thread count as the solve kernel (the fixed-order reductions depend on it): the same bits as the in-kernel setup.
// Output: the agent's record (omgx::prep_layout) -- start point, slots, row arrays, scaled Jacobian, start scalars.
template <bool GEN>
__global__ void __launch_bounds__(512, 4)      // (second argument: waves per SIMD the register allocation must leave room for -- 128 VGPRs)
ipm_prepare_kernel(omgx::Dims d, omgx::Tables T, omgx::Opts o, const double* __restrict__ p, const double* __restrict__ x0,
                   const double* __restrict__ lb, const double* __restrict__ ub, int bounds_shared,
                   const double* __restrict__ lam, const int32_t* __restrict__ status, int n_agents,
                   double* __restrict__ prep, size_t prep_doubles, int only_failed) {
  extern __shared__ __align__(16) double lds[];
  const int b = blockIdx.x;
  if (b >= n_agents) return;
  if (only_failed && status[b] == 0) return;
  const omgx::PrepLayout L = omgx::prep_layout(d);
  double* rec = prep + (size_t)b * prep_doubles;
  omgx::Work w;
  {
    double* q = lds;
    w.slots = q; q += d.n_slots; w.atoms = q; q += d.n_atoms; w.knots = q; q += d.n_knots;
    w.x = q; q += d.N; w.red = q; q += 64;
    w.xt = nullptr; w.gbar = nullptr; w.sol = nullptr; w.dinv = nullptr; w.kkt = nullptr; w.col = nullptr; w.root = nullptr;
    w.ht = nullptr; w.ds = nullptr;
    w.hv = rec + L.hv; w.rho = rec + L.rho; w.vv = rec + L.vv; w.z = rec + L.z;
    w.rtype = (int8_t*)(rec + L.rtype); w.jval = rec + L.jval;
  }
  omgx::CtxT<omgx::PrepareFlags<GEN>> c; c.red = w.red; c.prof = nullptr;
  const double* lbb = lb + (bounds_shared ? 0 : (size_t)b * d.n_con);
  const double* ubb = ub + (bounds_shared ? 0 : (size_t)b * d.n_con);
  const omgx::Start st = omgx::ipm_setup(c, d, T, o, w, p + (size_t)b * d.n_par, x0 + (size_t)b * d.n_var, lbb, ubb,
                                         o.warm_start ? lam + (size_t)b * d.n_con : nullptr, o.warm_start ? status[b] : 0, 0);
  __syncthreads();
  for (int i = threadIdx.x; i < d.N; i += blockDim.x) rec[L.x + i] = w.x[i];
  for (int i = threadIdx.x; i < d.n_slots; i += blockDim.x) rec[L.slots + i] = w.slots[i];
  if (threadIdx.x == 0) {
    rec[L.sc] = (double)st.status; rec[L.sc + 1] = (double)st.warm; rec[L.sc + 2] = (double)st.use_t;
    rec[L.sc + 3] = st.mu; rec[L.sc + 4] = st.zt; rec[L.sc + 5] = st.f;
  }
}

// Verification entry (omgx_batch_eval): one workgroup evaluates the tables of the solve at a caller's point and dumps the
// raw arrays -- row values, objective, Jacobian entries, the KKT store holding the Lagrangian Hessian -- to `out`
// [agent][n_con + 1 + nnz_j + kkt_doubles]; the host scatters them into dense matrices.
template <int MODE, bool WAVE_ONLY, bool GEN>
__global__ void __launch_bounds__(512)
ipm_eval_kernel(omgx::Dims d, omgx::Tables T, int kkt_doubles, const double* __restrict__ p, const double* __restrict__ x,
                const double* __restrict__ lam, int n_agents, double* __restrict__ slabs, size_t slab_doubles,
                double* __restrict__ out) {
  extern __shared__ __align__(16) double lds[];
  omgx::Work w;
  omgx::work_carve_split<MODE>(w, lds, MODE == omgx::WS_LDS ? nullptr : slabs + (size_t)blockIdx.x * slab_doubles,
                               d, kkt_doubles);
  omgx::CtxT<omgx::SolveFlags<MODE, WAVE_ONLY, GEN>> c; c.red = w.red; c.prof = nullptr;
  const size_t stride = (size_t)d.n_con + 1 + d.nnz_j + kkt_doubles;
  for (int b = blockIdx.x; b < n_agents; b += gridDim.x) {
    double* o = out + (size_t)b * stride;
    omgx::ipm_eval(c, d, T, w, p + (size_t)b * d.n_par, x + (size_t)b * d.n_var, lam + (size_t)b * d.n_con, kkt_doubles,
                   o + d.n_con);
    for (int i = threadIdx.x; i < d.n_con; i += blockDim.x) o[i] = w.hv[i];
    for (int i = threadIdx.x; i < d.nnz_j; i += blockDim.x) o[d.n_con + 1 + i] = w.jval[i];
    for (int i = threadIdx.x; i < kkt_doubles; i += blockDim.x) o[d.n_con + 1 + d.nnz_j + i] = w.kkt[i];
    __syncthreads();
  }
}

