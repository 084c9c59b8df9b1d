// omgx_kernels.h -- the device half of libomgx.so: kernel argument structs, the gfx950 kernels and the selectors that map a
// workspace mode to a template instance.  Included by omgx.hip only, after omgx_core.h / omgx_plan.h; an edit that leaves this
// file and those headers alone leaves the code object alone.
//
// Kernels (all hand-written HIP for CDNA4, wave64):
//   ipm_solve_kernel   one 512-thread workgroup (8 waves) per agent, whole interior-point
//                      solve with every per-agent array resident in LDS
//                      (<= 160 KiB / CU); only p, x0, bounds are read from HBM and
//                      x, lam_g, status written back.
//                      Instances: per workspace mode, general or not, and -- for the benchmark
//                      classes (wave path, modes 0 / 4 / 5) -- REFINE (refinement of regularised steps)
//                      and LEAN (every optional block compiled out: stop rule, restarts, prepared
//                      setup, ADMM centre, fused store / log, absolute tolerances).  omgx_batch_solve
//                      picks per launch: LEAN exactly when the launch uses none of them.
//   sample_kernel      post-solve trajectory sampling (reference
//                      `vehicles/vehicle.py:250-300`, `spline_extra.py:406-410`,
//                      C++ `Vehicle::sampleSplines` Vehicle.cpp:112-129): the
//                      HBM-write-bound stage, coalesced along the sample index.
//   shift_kernel       warm-start shift T*coeffs (`spline_extra.py:165-191`).
#pragma once

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

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
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

// LEAN: the instance for launches that leave every optional feature off -- no stop rule, no fused store / signals, no ADMM centre, no
// prepared setup, no restart pass or restart guesses, no absolute tolerances (omgx::CtxT kLean), no refinement: the plain
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
  omgx::CtxT<omgx::ws_kkt_hbm(MODE), WAVE_ONLY, omgx::ws_root_lds(MODE), GEN, false, REFINE, LEAN> c; c.red = w.red;
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
__host__ __device__ inline size_t prepare_lds_doubles(const omgx::Dims& d) {
  return (size_t)d.n_slots + d.n_atoms + d.n_knots + d.N + 64;
}
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
  omgx::CtxT<false, false, false, GEN, true> c; c.red = w.red; c.prof = nullptr;
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
  omgx::CtxT<omgx::ws_kkt_hbm(MODE), WAVE_ONLY, omgx::ws_root_lds(MODE), GEN> c; c.red = w.red; c.prof = nullptr;
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

typedef void (*ipm_eval_kernel_t)(omgx::Dims, omgx::Tables, int, const double*, const double*, const double*, int, double*,
                                  size_t, double*);
template <bool GEN>
static ipm_eval_kernel_t ipm_eval_kernel_gen(int mode, int wave_ok) {
#ifdef OMGX_ONLY_HEADLINE
  return ipm_eval_kernel<omgx::WS_JAC_HV, true, false>;
#else
  switch (mode) {
    case omgx::WS_LDS: return wave_ok ? ipm_eval_kernel<omgx::WS_LDS, true, GEN> : ipm_eval_kernel<omgx::WS_LDS, false, GEN>;
    case omgx::WS_KKT_HBM: return ipm_eval_kernel<omgx::WS_KKT_HBM, false, GEN>;
    case omgx::WS_JAC_HBM: return ipm_eval_kernel<omgx::WS_JAC_HBM, false, GEN>;
    case omgx::WS_JAC_ONLY: return ipm_eval_kernel<omgx::WS_JAC_ONLY, true, GEN>;
    case omgx::WS_JAC_HV: return ipm_eval_kernel<omgx::WS_JAC_HV, true, GEN>;
    case omgx::WS_ROOT_HBM: return ipm_eval_kernel<omgx::WS_ROOT_HBM, false, true>;      // (one instance: pick_mode hands mode 6 to general templates only)
    default: return ipm_eval_kernel<omgx::WS_ROWS_HBM, false, GEN>;
  }
#endif
}
static ipm_eval_kernel_t ipm_eval_kernel_for(int mode, int wave_ok, int general) {
  return general ? ipm_eval_kernel_gen<true>(mode, wave_ok) : ipm_eval_kernel_gen<false>(mode, wave_ok);
}

typedef void (*ipm_kernel_t)(omgx::Dims, omgx::Tables, omgx::Opts, int, const double*, const double*, const double*,
                             const double*, int, double*, double*, int32_t*, int32_t*, int, long long*, double*, size_t, double*,
                             const int32_t*, const StoreArgs*, int, int*, const double*, int, int32_t*, unsigned long long*, int, const CenterArgs*,
                             double*, size_t, const StopArgs*);
// (GEN: the instance that carries the terms with four factors, the cos / sin atoms and the basis rows of any degree --
// Dims::general; the other one is the kernel of the benchmark classes, free of that code)
template <bool GEN>
static ipm_kernel_t ipm_kernel_gen(int mode, int wave_ok, int refine = 0, int lean = 0) {
  // (the refinement of regularised steps -- omgx_options.refine -- has instances of its own: templates on the wave path, not general)
  if (refine && wave_ok && !GEN) {
    switch (mode) {
      case omgx::WS_LDS: return ipm_solve_kernel<omgx::WS_LDS, true, false, true>;
      case omgx::WS_JAC_ONLY: return ipm_solve_kernel<omgx::WS_JAC_ONLY, true, false, true>;
      case omgx::WS_JAC_HV: return ipm_solve_kernel<omgx::WS_JAC_HV, true, false, true>;
      default: break;
    }
  }
  // (and so have the launches with every optional feature off -- LEAN above: the same three modes; not with the refinement)
  if (lean && !refine && wave_ok && !GEN) {
    switch (mode) {
#ifndef OMGX_ONLY_HEADLINE
      case omgx::WS_LDS: return ipm_solve_kernel<omgx::WS_LDS, true, false, false, true>;
      case omgx::WS_JAC_ONLY: return ipm_solve_kernel<omgx::WS_JAC_ONLY, true, false, false, true>;
#endif
      case omgx::WS_JAC_HV: return ipm_solve_kernel<omgx::WS_JAC_HV, true, false, false, true>;
      default: break;
    }
  }
#ifdef OMGX_ONLY_HEADLINE      // developer builds (register counts of one instance in a third of the compile time): only the kernel of the benchmark class
  return ipm_solve_kernel<omgx::WS_JAC_HV, true, false>;
#else
  switch (mode) {
    case omgx::WS_LDS: return wave_ok ? ipm_solve_kernel<omgx::WS_LDS, true, GEN> : ipm_solve_kernel<omgx::WS_LDS, false, GEN>;
    case omgx::WS_KKT_HBM: return ipm_solve_kernel<omgx::WS_KKT_HBM, false, GEN>;
    case omgx::WS_JAC_HBM: return ipm_solve_kernel<omgx::WS_JAC_HBM, false, GEN>;
    case omgx::WS_JAC_ONLY: return ipm_solve_kernel<omgx::WS_JAC_ONLY, true, GEN>;
    case omgx::WS_JAC_HV: return ipm_solve_kernel<omgx::WS_JAC_HV, true, GEN>;
    case omgx::WS_ROOT_HBM: return ipm_solve_kernel<omgx::WS_ROOT_HBM, false, true>;
    default: return ipm_solve_kernel<omgx::WS_ROWS_HBM, false, GEN>;
  }
#endif
}
static ipm_kernel_t ipm_kernel_for(int mode, int wave_ok, int general, int refine = 0, int lean = 0) {
  return general ? ipm_kernel_gen<true>(mode, wave_ok) : ipm_kernel_gen<false>(mode, wave_ok, refine, lean);
}

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

__global__ void __launch_bounds__(64)
shift_kernel(double* __restrict__ x, int x_stride, const uint8_t* __restrict__ mask,
             const int32_t* __restrict__ entries, int n_ent, const double* __restrict__ Tm) {
  extern __shared__ __align__(16) double lds[];
  const int b = blockIdx.x;
  if (mask && !mask[b]) return;
  shift_row(x + (size_t)b * x_stride, entries, n_ent, Tm, lds);
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

// stand-alone launch (omgx_batch_obstacles_advance): eight agents share a workgroup, 32 lanes each
__global__ void __launch_bounds__(256)
obstacles_advance_kernel(double* __restrict__ p, int n_par, int B, const ObstacleScriptArgs* __restrict__ sc, double t_prev, double t_now, double dt) {
  const int b = blockIdx.x * 8 + (threadIdx.x >> 5);
  if (b >= B) return;
  obstacles_advance_agent(*sc, b, p + (size_t)b * n_par, t_prev, t_now, dt, threadIdx.x & 31);
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
  omgx::CtxT<omgx::ws_kkt_hbm(MODE), WAVE_ONLY, omgx::ws_root_lds(MODE), GEN> c; c.red = w.red;
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

typedef void (*ipm_rollout_t)(omgx::Dims, omgx::Tables, omgx::Opts, int, double*, double*, const double*, const double*, int, double*,
                              int32_t*, int32_t*, int, double*, size_t, double*, int*, const RolloutArgs*, int, const int32_t*, const StoreArgs*);
// (the classes of the wave path without quartic terms / cos / sin atoms: the receding-horizon classes that fit LDS)
static ipm_rollout_t rollout_kernel_for(int mode, int wave_ok, int general, int plant = 0, int script = 0, int mission = 0) {
  if (!wave_ok || general) return nullptr;
  if (mission) {      // (the instances with a mission: the same three modes, with and without the plant; none with a script)
    if (script) return nullptr;
    switch (mode) {
      case omgx::WS_LDS: return plant ? ipm_rollout_kernel<omgx::WS_LDS, true, false, true, false, true> : ipm_rollout_kernel<omgx::WS_LDS, true, false, false, false, true>;
      case omgx::WS_JAC_ONLY: return plant ? ipm_rollout_kernel<omgx::WS_JAC_ONLY, true, false, true, false, true> : ipm_rollout_kernel<omgx::WS_JAC_ONLY, true, false, false, false, true>;
      case omgx::WS_JAC_HV: return plant ? ipm_rollout_kernel<omgx::WS_JAC_HV, true, false, true, false, true> : ipm_rollout_kernel<omgx::WS_JAC_HV, true, false, false, false, true>;
      default: return nullptr;
    }
  }
  if (script) {      // (the instances with an obstacle script: the same three modes, with and without the plant)
    switch (mode) {
      case omgx::WS_LDS: return plant ? ipm_rollout_kernel<omgx::WS_LDS, true, false, true, true> : ipm_rollout_kernel<omgx::WS_LDS, true, false, false, true>;
      case omgx::WS_JAC_ONLY: return plant ? ipm_rollout_kernel<omgx::WS_JAC_ONLY, true, false, true, true> : ipm_rollout_kernel<omgx::WS_JAC_ONLY, true, false, false, true>;
      case omgx::WS_JAC_HV: return plant ? ipm_rollout_kernel<omgx::WS_JAC_HV, true, false, true, true> : ipm_rollout_kernel<omgx::WS_JAC_HV, true, false, false, true>;
      default: return nullptr;
    }
  }
  if (plant) {      // (the plant instances: the same three modes)
    switch (mode) {
      case omgx::WS_LDS: return ipm_rollout_kernel<omgx::WS_LDS, true, false, true>;
      case omgx::WS_JAC_ONLY: return ipm_rollout_kernel<omgx::WS_JAC_ONLY, true, false, true>;
      case omgx::WS_JAC_HV: return ipm_rollout_kernel<omgx::WS_JAC_HV, true, false, true>;
      default: return nullptr;
    }
  }
  switch (mode) {
    case omgx::WS_LDS: return ipm_rollout_kernel<omgx::WS_LDS, true, false>;
    case omgx::WS_JAC_ONLY: return ipm_rollout_kernel<omgx::WS_JAC_ONLY, true, false>;
    case omgx::WS_JAC_HV: return ipm_rollout_kernel<omgx::WS_JAC_HV, true, false>;
    default: return nullptr;
  }
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
