// omgx.hip -- the host unit of libomgx.so: the omgx_batch handle and the C ABI (include/omgx.h), and the glue kernels it launches
// by name (omgx_kernels.h).  It instantiates no ipm_solve / ipm_prepare / ipm_eval / ipm_rollout kernel: those are compiled in the
// instance units (omgx_inst_*.hip) and reach this file only as the pointers the selectors of omgx_device.h return, so an edit
// here recompiles this unit and none of theirs.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/omgx.h"
#include "omgx_types.h"
#include "omgx_plan.h"
#include "omgx_kernels.h"
#include "omgx_table_cache.h"

namespace {

thread_local std::string g_err;

#define HIPCHK(call)                                                              \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) {                                                       \
      g_err = std::string(#call) + ": " + hipGetErrorString(e_);                  \
      return OMGX_E_HIP;                                                          \
    }                                                                             \
  } while (0)

// a refused call: the message (built on this path only) and the code to return; bad(...): a refused argument
__attribute__((format(printf, 2, 3))) int fail(int code, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define bad(...) fail(OMGX_E_INVALID, __VA_ARGS__)
#define TRY(call) do { const int rc_ = (call); if (rc_ != OMGX_OK) return rc_; } while (0)

constexpr int kThreads = 512;
constexpr int kLdsLimit = 160 * 1024;
constexpr int kLdsHalf = kLdsLimit / 2 - 512;      // two workgroups per CU (their static LDS and the allocation granule taken off)

}  // namespace

// The solve kernel of a class: the general instance carries everything; otherwise the refinement and the lean launches have
// instances of their own on the wave path (modes 0 / 4 / 5), and a class without the one asked for gets its full instance.
static ipm_kernel_t ipm_kernel_for(int mode, int wave_ok, int general, int refine = 0, int lean = 0) {
  if (general || mode == omgx::WS_ROOT_HBM) return solve_general_kernel(mode, wave_ok);
  ipm_kernel_t k = nullptr;
  if (wave_ok && refine) k = solve_refine_kernel(mode);
  else if (wave_ok && lean) k = solve_lean_kernel(mode);
  if (!k && (wave_ok || mode != omgx::WS_LDS)) k = solve_wave_kernel(mode);      // (mode 0 holds classes off the wave path too)
  return k ? k : solve_blocked_kernel(mode);
}
// (the classes of the wave path without quartic terms / cos / sin atoms: the receding-horizon classes that fit LDS)
static ipm_rollout_t rollout_kernel_for(int mode, int wave_ok, int general, int plant = 0, int script = 0, int mission = 0) {
  if (!wave_ok || general) return nullptr;
  switch (mode) {
    case omgx::WS_LDS: return rollout_kernel_of<omgx::WS_LDS>(plant, script, mission);
    case omgx::WS_JAC_ONLY: return rollout_kernel_of<omgx::WS_JAC_ONLY>(plant, script, mission);
    case omgx::WS_JAC_HV: return rollout_kernel_of<omgx::WS_JAC_HV>(plant, script, mission);
    default: return nullptr;
  }
}

// The kernel instances of a handle's template class, resolved once per handle (omgx_batch_create) through the selectors above and
// those of the instance units (omgx_device.h).  refine / lean / rollout[][] are null where the class has no such instance (the
// general instance, classes off the wave path, the spill modes).
enum { RO_PLAIN = 0, RO_SCRIPT = 1, RO_MISSION = 2, RO_FEATURES = 3 };      // (omgx_batch_set_obstacle_script, omgx_batch_set_mission: never both)
struct Instances {
  ipm_kernel_t full = nullptr, refine = nullptr, lean = nullptr;
  ipm_eval_kernel_t eval = nullptr;
  ipm_rollout_t rollout[2][RO_FEATURES] = {};      // [plant in the loop (omgx_batch_set_plant)][feature]
  ipm_prepare_kernel_t prepare = nullptr;
};
static Instances instances_for(int mode, int wave_ok, int general) {
  Instances in;
  in.full = ipm_kernel_for(mode, wave_ok, general);
  const ipm_kernel_t refine = ipm_kernel_for(mode, wave_ok, general, 1), lean = ipm_kernel_for(mode, wave_ok, general, 0, 1);
  if (refine != in.full) in.refine = refine;      // (a class without the instance gets the full one back)
  if (lean != in.full) in.lean = lean;
  in.eval = ipm_eval_kernel_for(mode, wave_ok, general);
  for (int plant = 0; plant < 2; ++plant)
    for (int f = 0; f < RO_FEATURES; ++f) in.rollout[plant][f] = rollout_kernel_for(mode, wave_ok, general, plant, f == RO_SCRIPT, f == RO_MISSION);
  in.prepare = ipm_prepare_kernel_for(general);
  return in;
}

// A device allocation with one owner, move-only: what is resized or evicted while the handle lives, and a call's temporaries
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
  ~DevBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; }      // (hipFree waits for queued launches that still read it)
  hipError_t alloc(size_t bytes) { reset(); return hipMalloc(&p, bytes); }
};

// ---------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------
struct omgx_batch {
  int device = 0, n_agents = 0;
  omgx::Dims dims;
  omgx::Tables dev;               // device pointers
  omgx::Opts opts;
  int kkt_doubles = 0;
  size_t lds_bytes = 0;
  int ws_mode = 0, n_slabs = 0;        // workspace placement (omgx::WS_*), HBM slabs (= grid cap)
  Instances inst;                      // the kernels of this class (instances_for)
  int threads = kThreads;              // workgroup size of the solve kernel
  int per_cu = 1;                      // workgroups (agents in flight) per CU the workspace allows
  int prio_iter = 0, stagger = 0; // straggler priority / start offset of the second workgroup of a CU (two per CU only)
  size_t slab_doubles = 0;
  double* d_slabs = nullptr;
  double* d_dw = nullptr;          // per-agent inertia correction carried between warm-started solves
  // round 6: the setup of every solve as a kernel of its own ahead of the solve kernel (ipm_prepare_kernel): one record per agent
  double* d_prep = nullptr; size_t prep_doubles = 0; size_t prep_lds = 0; bool prepare_on = false;
  int order_dw = 1;                // omgx_batch_order_by_iters: ties of the iteration count broken by the carried inertia correction (OMGX_ORDER_DW=0: developer switch)
  const int32_t* d_order = nullptr; // optional launch order (device pointer owned by the caller)
  const int32_t* pend_iters = nullptr; int32_t* pend_order = nullptr;   // omgx_batch_order_by_iters not launched yet
  int* d_next = nullptr;            // spill modes: counter of the dynamic slot hand-out
  int* d_admm_done = nullptr;       // admm_update_kernel: finished workgroups (fleet sums by the last one)
  const double* d_x0_alt = nullptr; // restart guesses [n_alt][n_agents][n_var] (device, owned by the caller)
  int n_alt = 0;
  int32_t* d_attempts = nullptr;    // optional [n_agents] (device, owned by the caller): restarts each agent used
  int64_t* d_stats = nullptr;       // optional [stats_slots][4] launch statistics (device, owned by the caller)
  int stats_slots = 0; long long stats_launch = 0;
  StoreArgs store = {};             // trajectories written by the solve kernel (omgx_batch_set_store); out == nullptr: off
  SignalArgs signals = {};          // travelled trajectories appended by the solve and rollout kernels (omgx_batch_set_signals); log == nullptr: off
  StoreBlock store_host = {};       // the two as the kernels read them ...
  StoreBlock* d_store = nullptr;    // ... and their copy in device memory
  RolloutArgs* d_rollout = nullptr; int32_t* d_ro_perm = nullptr;      // omgx_batch_rollout
  DevBuf ro_steps; int ro_steps_cap = 0;      // (its step table grows with the longest rollout asked for)
  std::vector<int32_t> ro_perm_host;
  PlantBlock plant_host = {};       // omgx_batch_set_plant: the plant and its log as the rollout's plant instance reads them ...
  PlantBlock* d_plant = nullptr;    // ... their copy in device memory ...
  PlantBlock* d_plant_call = nullptr;      // ... and the copy of what a stand-alone omgx_batch_plant_simulate / _predict call was given
  bool plant_on = false;
  double *d_lag_tc = nullptr, *d_lag_decay = nullptr;      // omgx_batch_set_plant_lag: the handle's copies [n_agents] of time constant and decay ...
  double lag_sample_time = 0.0; bool lag_on = false;       // ... the sample time the decay was formed with, and whether the plant lags
  ObstacleScriptArgs script_host = {};      // omgx_batch_set_obstacle_script: the script as the rollout's script instances read it ...
  ObstacleScriptArgs* d_script = nullptr;   // ... its copy in device memory ...
  ObstacleScriptArgs* d_script_call = nullptr;      // ... and the copy of what a stand-alone omgx_batch_obstacles_advance call was given
  DevBuf script_t; int script_t_cap = 0;    // (t_abs of the script set: grows with the longest step list registered)
  bool script_on = false;
  MissionArgs mission_host = {};            // omgx_batch_set_mission: the mission as the rollout's mission instances read it ...
  MissionArgs* d_mission = nullptr;         // ... its copy in device memory ...
  double* d_x_reset = nullptr;              // ... and the handle's copy of the reset row [n_var]
  bool mission_on = false;
  FreeTArgs free_t_host = {};               // omgx_batch_set_free_t: the free-end-time glue as its kernels read it ...
  FreeTArgs* d_free_t = nullptr;            // ... its copy in device memory ...
  DevBuf free_t_tab;                        // ... and the fit / proj tables of its bases behind it (freed when it is switched off)
  bool free_t_on = false;
  StopArgs* d_stop = nullptr;     // omgx_batch_set_stop: device copy of the arguments
  StopArgs stop_host = {};          // (and the host copy: omgx_batch_rollout hands it to its kernel inside RolloutArgs)
  bool stop_on = false;
  int last_instance = 0;            // solve-kernel instance of the last omgx_batch_solve launch: 0 full, 1 lean (omgx_batch_last_instance)
  CenterArgs* d_center = nullptr;   // omgx_batch_set_center: device copy of the arguments (nullptr: off); the slot map behind it
  int32_t* d_pub_inv = nullptr;
  bool center_on = false;
  // Every device buffer that lives as long as the handle comes from dalloc and is freed by the loop over `allocs` in
  // omgx_batch_destroy, the lazily allocated ones (d_store, d_stop ...) included; what is resized or evicted is a DevBuf.
  // The plan's tables (`dev`) are not the handle's: it holds a reference to their image in the table cache (omgx_table_cache.h),
  // shared with every handle of the same template on this device, and only reads through it.
  std::vector<void*> allocs;
  const omgx::TableCache::Entry* tables = nullptr;      // taken by build_batch, released by omgx_batch_destroy
  hipStream_t own_stream = nullptr, stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ext_ev0 = nullptr, ext_ev1 = nullptr;   // caller's events for the next solve launch (one shot)
  bool timed = false;
  bool timing = true;              // bracket every solve kernel with events (omgx_batch_set_timing)
  // staging buffers for host-pointer calls
  double *d_p = nullptr, *d_x0 = nullptr, *d_lb = nullptr, *d_ub = nullptr, *d_x = nullptr, *d_lam = nullptr;
  // Two-sided rows lb < g < ub (`basics/optilayer.py:634-666`): the solve kernel knows one-sided rows, so the library hands it
  // the template with every such row twice -- row r as g <= ub, a copy behind the last row as g >= lb -- and maps bounds and
  // multipliers between the caller's n_con_user rows and the kernel's dims.n_con rows around every solve (range_* kernels).
  int n_con_user = 0, n_range = 0;
  int32_t *d_range_src = nullptr, *d_range_dup = nullptr;      // [n_range] source row of copy k; [n_con_user] copy of row r (-1: none)
  double *d_lam_user = nullptr, *d_lb_user = nullptr, *d_ub_user = nullptr;   // staging of the caller's arrays (host-pointer calls)
  int32_t *d_status = nullptr, *d_iters = nullptr;
  long long* d_prof = nullptr;
  // shift tables (entries + T matrices) live in the handle: uploaded when they change (a receding-horizon loop
  // passes the same ones at every knot crossing), so that a shift is one stream-ordered launch
  // (a receding-horizon loop passes the same few sets at every knot crossing -- an ADMM fleet four of them: x, p, z_ij,
  // l_ij --: each set is uploaded once and found again by content, so that a shift is stream-ordered launches only)
  struct ShiftSet { std::vector<int32_t> ent; std::vector<double> T; DevBuf d_ent, d_T; unsigned long long used = 0; };
  std::vector<ShiftSet> shift_sets; unsigned long long shift_clock = 0;
  int32_t* d_shift_ent = nullptr; double* d_shift_T = nullptr;      // the set the last staging call selected
  uint8_t* d_mask = nullptr;
  // omgx_batch_eval: Jacobian entry -> (row, variable), stored Hessian entry -> (address, variable a, variable b)
  std::vector<int32_t> ev_jrow, ev_jvar, ev_hess;
};

namespace {

// The ~60 tables of a plan live in one image (256-byte aligned pieces, one exact-size allocation) instead of sixty separately
// placed hipMalloc'ed buffers: every thread of every solve walks them.  build_batch lays the image out on the host (upload: a piece
// and the table pointer that will point at it), then takes its device copy from the table cache -- one per template and device,
// whoever asks first uploads it (bind_tables).  Nothing writes into it afterwards: the tables are const to every kernel.
struct TableImage {
  std::vector<char> bytes;
  std::vector<std::pair<const void**, size_t>> slots;      // (table pointer of the handle, offset of its piece)
};

template <typename T>
int upload(TableImage& img, const T* src, size_t n, const T** dst) {
  const size_t bytes = (n > 0 ? n : 1) * sizeof(T), off = img.bytes.size();
  img.bytes.resize(off + ((bytes + 255) & ~(size_t)255), 0);
  if (n > 0) memcpy(img.bytes.data() + off, src, n * sizeof(T));
  img.slots.emplace_back((const void**)dst, off);
  return OMGX_OK;
}

// the process-wide cache of table images (never destroyed: handles may outlive static destruction order)
omgx::TableCache& table_cache() {
  static const omgx::TableCacheOps ops = {
      [](void*, int, size_t bytes, void** out) -> int { return (int)hipMalloc(out, bytes); },
      [](void*, int, void* dst, const void* src, size_t bytes) -> int { return (int)hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); },
      [](void*, int, void* ptr) { (void)hipFree(ptr); },      // (hipFree waits for queued launches that still read it)
      nullptr};
  static omgx::TableCache* cache = new omgx::TableCache(ops);
  return *cache;
}

int bind_tables(omgx_batch* b, TableImage& img) {
  int err = 0, step = 0;
  b->tables = table_cache().take(b->device, img.bytes.data(), img.bytes.size(), &err, &step);
  if (!b->tables) {
    // (the texts are kept verbatim from the HIPCHK lines of the per-table upload this replaces: callers match on them)
    g_err = std::string(step == omgx::TableCache::STEP_COPY ? "hipMemcpy(ptr, src, n * sizeof(T), hipMemcpyHostToDevice): " : "hipMalloc(&ptr, cap): ") +
            hipGetErrorString((hipError_t)err);
    return OMGX_E_HIP;
  }
  for (auto& s : img.slots) *s.first = (const char*)b->tables->dev + s.second;
  return OMGX_OK;
}

template <typename T>
int dalloc(omgx_batch* b, size_t n, T** dst) {
  void* ptr = nullptr;
  HIPCHK(hipMalloc(&ptr, (n > 0 ? n : 1) * sizeof(T)));
  b->allocs.push_back(ptr);
  *dst = (T*)ptr;
  return OMGX_OK;
}

// Device copy of a host argument struct (StopArgs, CenterArgs, StoreBlock, RolloutArgs): allocated on first use, copied on the
// handle's stream behind the launches that still read the previous contents (pageable source: staged before the call returns)
template <typename T>
int push_args(omgx_batch* b, T** dev, const T& host) {
  if (!*dev) TRY(dalloc(b, (size_t)1, dev));
  HIPCHK(hipMemcpyAsync(*dev, &host, sizeof(T), hipMemcpyHostToDevice, b->stream));
  return OMGX_OK;
}

// The plan: which coefficients of x are the vehicle's splines and on which basis.  Every glue entry that reads it builds this one
// value from its arguments or its specification (plan_of), has it judged by check_plan / check_plan_in_x -- the one rule, written
// out above omgx_store_spec in include/omgx.h -- and copies it into its kernel-argument struct with put_plan.
struct Plan { int coeff_off, n_spl, degree, n_knots; double inv_T; const double* knots; };
template <class Spec> Plan plan_of(const Spec& sp) { return {sp.coeff_off, sp.n_spl, sp.degree, sp.n_knots, sp.inv_T, sp.knots}; }

constexpr int kAnySpl = 0x7fffffff, kOwnedSpl = 64;      // max_spl: unlimited / a thread of one wave owns a spline (plant, rollout)

// what can be judged without a handle (`who`: the entry, for the message)
int check_plan(const char* who, const Plan& pl, int min_degree = 1, int max_spl = kAnySpl, bool has_inv_T = true) {
  if (!pl.knots) return bad("%s: null knots", who);
  if (pl.degree < min_degree || pl.degree > 5) return bad("%s: degree = %d outside %d .. 5", who, pl.degree, min_degree);
  if (pl.n_knots < 2 * pl.degree + 2 || pl.n_knots > 40) return bad("%s: n_knots = %d outside %d .. 40", who, pl.n_knots, 2 * pl.degree + 2);
  if (pl.n_spl < 1) return bad("%s: n_spl = %d must be positive", who, pl.n_spl);
  if (pl.n_spl > max_spl) return bad("%s: n_spl = %d outside 1 .. %d", who, pl.n_spl, max_spl);
  if (pl.coeff_off < 0) return bad("%s: coeff_off = %d is negative", who, pl.coeff_off);
  if (has_inv_T && !(pl.inv_T > 0.0)) return bad("%s: inv_T = %g must be positive", who, pl.inv_T);
  return OMGX_OK;
}
// ... and what needs one: the n_spl splines of L = n_knots - degree - 1 coefficients lie inside x
int check_plan_in_x(const omgx_batch* b, const char* who, const Plan& pl) {
  const int L = pl.n_knots - pl.degree - 1;
  if (pl.coeff_off + (long long)pl.n_spl * L > b->dims.n_var)
    return bad("%s: coefficients outside x (coeff_off = %d, %d splines of %d, n_var = %d)", who, pl.coeff_off, pl.n_spl, L, b->dims.n_var);
  return OMGX_OK;
}
// `width` parameters from offset `off` lie inside p
bool in_p(const omgx_batch* b, int off, int width) { return off >= 0 && off + (long long)width <= b->dims.n_par; }

// a knot vector as the kernels take it by value (n_knots <= 40: check_plan)
void fill_knots(KnotArg& k, const double* knots, int n_knots) {
  for (int i = 0; i < 40; ++i) k.k[i] = i < n_knots ? knots[i] : 0.0;
}
template <class Args> void put_plan(Args& a, const Plan& pl) {
  a.coeff_off = pl.coeff_off; a.n_spl = pl.n_spl; a.degree = pl.degree; a.n_knots = pl.n_knots; a.inv_T = pl.inv_T;
  fill_knots(a.knots, pl.knots, pl.n_knots);
}
// two specifications or argument structs describe one plan (knot values apart)
template <class A, class B> bool same_plan(const A& a, const B& b) {
  return a.coeff_off == b.coeff_off && a.n_spl == b.n_spl && a.degree == b.degree && a.n_knots == b.n_knots;
}

#define UP(field, count)                                          \
  TRY(upload(img, H.field, (size_t)(count), &b->dev.field))

// smallest spill mode whose LDS part fits one CU (WS_MODES: none does)
int pick_mode(const omgx::Dims& d, int kkt_doubles, size_t* lds_doubles, size_t* hbm_doubles) {
  int mode = 0;
  for (; mode <= omgx::WS_ROWS_HBM; ++mode) {
    omgx::work_split(d, kkt_doubles, mode, lds_doubles, hbm_doubles);
    if (*lds_doubles * sizeof(double) <= (size_t)kLdsLimit) break;
  }
  if (mode <= omgx::WS_ROWS_HBM) return mode;
  // the root block alone is too large for LDS: it stays in the slab (mode 6; compiled for the general instance only -- the
  // templates that get here are the ones with lifted auxiliaries, hundreds of equality rows in the root)
  omgx::work_split(d, kkt_doubles, omgx::WS_ROOT_HBM, lds_doubles, hbm_doubles);
  return (d.general && *lds_doubles * sizeof(double) <= (size_t)kLdsLimit) ? (int)omgx::WS_ROOT_HBM : (int)omgx::WS_MODES;
}

// The plan of a template for the workspace mode it gets: the spill modes store the leaf panels by columns
// (omgx_plan.h `col_major`), so their plan is built a second time once the mode is known.
// Templates on the register-resident wave path get the compact store; when their workspace then fits half a CU -- all
// of it, or with the Jacobian values (WS_JAC_HV) and the row values hv (WS_JAC_ONLY) in a slab -- two agents share a CU: *per_cu = 2, workgroups
// of 256 threads (a solve is latency bound: four waves are as fast as eight, and the second agent fills the gaps).
bool plan_for_mode(omgx::HostPlan& plan, const omgx_template& t, int* mode, size_t* lds_doubles, size_t* hbm_doubles, int* per_cu) {
  *per_cu = 1;
  if (!plan.build(t)) return false;
  if (plan.dims.wave_ok && !getenv("OMGX_NO_COMPACT")) {
    // (built in place: HostPlan::tables points into the plan's own vectors)
    plan = omgx::HostPlan();
    plan.owners = 256;        // (the assembly records dealt to the 256 threads of a two-per-CU workgroup)
    if (!plan.build(t, false, true)) return false;
    const int cand[3] = {omgx::WS_LDS, omgx::WS_JAC_HV, omgx::WS_JAC_ONLY};
    // (two per CU = workgroups of four waves: the substitutions gather 64 doubles per wave in the scratch behind the
    // matrix descriptors, four of the eight blocks suffice)
    plan.dims.col_doubles -= 4 * 64;
    for (int k = 0; k < 3; ++k) {
      omgx::work_split(plan.dims, plan.kkt_doubles, cand[k], lds_doubles, hbm_doubles);
      if (*lds_doubles * sizeof(double) <= (size_t)kLdsHalf && !getenv("OMGX_ONE_PER_CU")) { *mode = cand[k]; *per_cu = 2; return true; }
    }
    plan = omgx::HostPlan();
    if (!plan.build(t, false, true)) return false;
    // one agent per CU: everything in LDS, or the Jacobian values in a slab (the register-resident factorisation either way)
    for (int k = 0; k < 3; ++k) {
      omgx::work_split(plan.dims, plan.kkt_doubles, cand[k], lds_doubles, hbm_doubles);
      if (*lds_doubles * sizeof(double) <= (size_t)kLdsLimit && !(k >= 1 && getenv("OMGX_NO_JAC_ONLY_FULL"))) { *mode = cand[k]; return true; }
    }
    plan = omgx::HostPlan();
    if (!plan.build(t)) return false;
  }
  plan.dims.wave_ok = 0;      // the blocked routines (dense panels)
  *mode = pick_mode(plan.dims, plan.kkt_doubles, lds_doubles, hbm_doubles);
  if (const char* e = getenv("OMGX_FORCE_MODE")) {      // (developer knob: a deeper spill mode than the class needs)
    const int fm = atoi(e);
    if (*mode != omgx::WS_MODES && fm > *mode && fm <= omgx::WS_ROWS_HBM) *mode = fm;
  }
  if (*mode != omgx::WS_LDS && *mode != omgx::WS_MODES) {
    plan = omgx::HostPlan();
    if (!plan.build(t, true)) return false;
    omgx::work_split(plan.dims, plan.kkt_doubles, *mode, lds_doubles, hbm_doubles);
    // a spill class is bound by dependent accesses to its slab: when the part that stays in LDS fits half a CU, two
    // agents share the CU and hide each other's round trips
    if (*lds_doubles * sizeof(double) <= (size_t)kLdsHalf && getenv("OMGX_SPILL_PER_CU") && atoi(getenv("OMGX_SPILL_PER_CU")) == 2) *per_cu = 2;
  }
  return true;
}

int check_template(const omgx_template* t) {
  if (!t || t->n_var <= 0 || t->n_par < 0 || t->n_con < 0 || t->n_terms < 0 || t->n_eq < 0 || t->n_root_vars < 0 ||
      !t->row_ptr || (t->n_terms > 0 && (!t->t_coef || !t->t_slot || !t->t_var)) || (t->n_eq > 0 && !t->eq_rows) ||
      (t->n_root_vars > 0 && !t->root_vars)) { g_err = "bad template"; return OMGX_E_INVALID; }
  if (t->n_lift < 0 || (t->n_lift > 0 && (t->n_lift > t->n_var || t->lift_row0 < 0 || t->lift_row0 + t->n_lift > t->n_con))) { g_err = "bad template: lifted rows outside the template"; return OMGX_E_INVALID; }
  // the block table (optional): every entry inside its flat vector -- callers fill p / x0 and read x through these offsets
  // (`Point2Point::fillParameterDict / extractData`, export/point2point/Point2Point.cpp:263-294)
  if (t->n_blocks > 0) {
    if (!t->block_kind || !t->block_off || !t->block_rows || !t->block_cols) { g_err = "bad template: block table without its arrays"; return OMGX_E_INVALID; }
    for (int i = 0; i < t->n_blocks; ++i) {
      const int k = t->block_kind[i];
      const long long n = k == OMGX_BLOCK_VAR ? t->n_var : (k == OMGX_BLOCK_PAR ? t->n_par : (k == OMGX_BLOCK_CON ? t->n_con : -1));
      const long long off = t->block_off[i], sz = (long long)t->block_rows[i] * t->block_cols[i];
      if (n < 0 || off < 0 || t->block_rows[i] < 0 || t->block_cols[i] < 0 || off + sz > n)
        return bad("bad template: block %d (kind %d, offset %lld, %d x %d) reaches outside its vector of %lld", i, k, off, t->block_rows[i],
                   t->block_cols[i], n);
    }
  }
  return OMGX_OK;
}

// The template with every two-sided row of its default bounds twice (see omgx_batch::n_range).  Host arrays owned by `own`.
struct ExpandedTemplate {
  omgx_template t;
  std::vector<int32_t> row_ptr, t_slot, t_var, src, dup;
  std::vector<double> t_coef, lb, ub;
};
static bool expand_range_rows(const omgx_template* in, ExpandedTemplate& e) {
  e.src.clear(); e.dup.assign(in->n_con, -1);
  if (!in->has_bounds || !in->lbg_def || !in->ubg_def) return false;
  std::vector<char> is_eq(in->n_con, 0);
  for (int k = 0; k < in->n_eq; ++k) if (in->eq_rows[k] >= 0 && in->eq_rows[k] < in->n_con) is_eq[in->eq_rows[k]] = 1;
  for (int r = 0; r < in->n_con; ++r)
    if (!is_eq[r] && std::isfinite(in->lbg_def[r]) && std::isfinite(in->ubg_def[r]) && in->lbg_def[r] < in->ubg_def[r]) {
      e.dup[r] = in->n_con + (int)e.src.size(); e.src.push_back(r);
    }
  if (e.src.empty()) return false;
  const int nu = in->n_con, ni = nu + (int)e.src.size(), W = OMGX_TERM_VARS;
  e.t = *in;
  e.row_ptr.assign(ni + 2, 0);
  auto put_row = [&](int from) {
    for (int i = in->row_ptr[from]; i < in->row_ptr[from + 1]; ++i) {
      e.t_coef.push_back(in->t_coef[i]); e.t_slot.push_back(in->t_slot[i]);
      for (int q = 0; q < W; ++q) e.t_var.push_back(in->t_var[(size_t)W * i + q]);
    }
  };
  int out = 0;
  for (int r = 0; r < nu; ++r) { put_row(r); e.row_ptr[++out] = (int)e.t_coef.size(); }
  for (int k = 0; k < (int)e.src.size(); ++k) { put_row(e.src[k]); e.row_ptr[++out] = (int)e.t_coef.size(); }
  put_row(nu); e.row_ptr[++out] = (int)e.t_coef.size();                 // the objective row stays last
  e.lb.resize(ni); e.ub.resize(ni);
  for (int r = 0; r < nu; ++r) { e.lb[r] = e.dup[r] >= 0 ? -INFINITY : in->lbg_def[r]; e.ub[r] = in->ubg_def[r]; }
  for (int k = 0; k < (int)e.src.size(); ++k) { e.lb[nu + k] = in->lbg_def[e.src[k]]; e.ub[nu + k] = INFINITY; }
  e.t_coef.push_back(0.0); e.t_slot.push_back(0); e.t_var.push_back(0);
  e.t.n_con = ni; e.t.n_terms = (int)e.t_coef.size() - 1;
  e.t.row_ptr = e.row_ptr.data(); e.t.t_coef = e.t_coef.data(); e.t.t_slot = e.t_slot.data(); e.t.t_var = e.t_var.data();
  e.t.lbg_def = e.lb.data(); e.t.ubg_def = e.ub.data();
  e.t.n_blocks = 0; e.t.block_names_len = 0;                            // (the block table describes the caller's rows)
  return true;
}

int build_batch(omgx_batch* b, const omgx_template* t) {
  omgx::HostPlan plan;
  size_t nl = 0, ng = 0;
  int mode = 0;
  if (!plan_for_mode(plan, *t, &mode, &nl, &ng, &b->per_cu)) { g_err = "inconsistent template: " + plan.error; return OMGX_E_INVALID; }
  b->dims = plan.dims;
  b->kkt_doubles = plan.kkt_doubles;
  if (mode == omgx::WS_MODES) return fail(OMGX_E_TOOLARGE, "per-agent O(n_var) vectors (%zu B) exceed the %d B LDS of one CU", nl * sizeof(double), kLdsLimit);
  b->ws_mode = mode; b->lds_bytes = nl * sizeof(double); b->slab_doubles = ng;
  b->threads = b->per_cu >= 2 ? 256 : kThreads;
  if (const char* e = getenv("OMGX_THREADS")) { const int t2 = atoi(e); if (t2 == 256 || (t2 == 512 && b->per_cu < 2)) b->threads = t2; }      // (developer knob; the workspace of two per CU is sized for four waves)
  if (b->per_cu >= 2) { b->prio_iter = 2; b->stagger = 0; }
  if (const char* e = getenv("OMGX_PRIO_ITER")) b->prio_iter = atoi(e);      // (developer knobs)
  if (const char* e = getenv("OMGX_STAGGER")) b->stagger = atoi(e);
  if (const char* e = getenv("OMGX_ORDER_DW")) b->order_dw = atoi(e);
  const omgx::Tables& H = plan.tables;
  const omgx::Dims& d = plan.dims;
  TableImage img;
  {
    b->ev_jrow.assign(plan.je_row.begin(), plan.je_row.begin() + d.nnz_j);
    b->ev_jvar.resize(d.nnz_j);
    for (int e = 0; e < d.nnz_j; ++e) b->ev_jvar[e] = plan.order[plan.jr_pos[e]];
    for (int q1 = 0; q1 + 1 < d.N; ++q1)          // (positions but the phase-I variable t, the last one)
      for (int q2 = 0; q2 <= q1; ++q2) {
        const int32_t ad = plan.kkt_addr(q1, q2);
        if (ad >= 0) { b->ev_hess.push_back(ad); b->ev_hess.push_back(plan.order[q1]); b->ev_hess.push_back(plan.order[q2]); }
      }
  }
  UP(prog, 6 * d.n_prog); UP(knots, t->n_knots); UP(pp_ptr, t->n_pp + 1); UP(pm_coef, t->n_mono);
  UP(pm_ptr, t->n_mono + 1); UP(pm_atom, t->n_matom); UP(slot_pp, d.n_slots);
  // (packed monomial records: 16-byte MonoRec or, with 5..8 atoms per monomial, 24-byte MonoRec8 behind the same pointers)
  if (d.mono_packed == 2) {
    // (the pointers are bound once the image is on the device: straight into the handle's table, the records' type apart)
    TRY(upload(img, plan.pm_rec8.data(), plan.pm_rec8.size(), (const omgx::MonoRec8**)&b->dev.pm_rec));
    TRY(upload(img, plan.sl_ell8.data(), plan.sl_ell8.size(), (const omgx::MonoRec8**)&b->dev.sl_ell));
  } else { UP(pm_rec, plan.pm_rec.size()); UP(sl_ell, plan.sl_ell.size()); }
  UP(row_ptr, d.n_con + 2); UP(t_coef, d.n_terms); UP(t_slot, d.n_terms); UP(t_var, OMGX_TERM_VARS * d.n_terms);
  UP(order, d.N); UP(leaf_off, d.n_leaf + 1); UP(leaf_bw, plan.leaf_bw.size()); UP(blk, d.N);
  UP(eq_rows, d.n_eq); UP(eq_index, d.n_con);
  UP(cpl_ptr, d.n_leaf + 1); UP(cpl_idx, plan.cpl_idx.size()); UP(cpl_map, plan.cpl_map.size());
  UP(d_off, d.n_leaf + 1); UP(b_off, plan.b_off.size());
  UP(lf_w, plan.lf_w.size()); UP(lf_ldb, plan.lf_ldb.size()); UP(lf_band, plan.lf_band.size()); UP(lf_kind, plan.lf_kind.size()); UP(dl_pos, plan.dl_pos.size());
  UP(bmat_img, plan.bmat_img.size());
  UP(pair4, plan.pair4.size()); UP(eqe3, plan.eqe3.size());
  UP(je_row, plan.je_row.size()); UP(diag_addr, d.N); UP(tq_addr, plan.tq_addr.size());
  UP(reg_w, d.N); UP(je_rp, plan.je_rp.size());
  UP(slot_rng, plan.slot_rng.size());
  UP(row_perm, plan.row_perm.size()); UP(cs_ptr, plan.cs_ptr.size()); UP(cs_rec, plan.cs_rec.size());
  UP(obj_ent, plan.obj_ent.size());
  UP(ka_rec, plan.ka_rec.size()); UP(kh_rec, plan.kh_rec.size()); UP(kg_rec, plan.kg_rec.size());
  UP(ka_fix, plan.ka_fix.size()); UP(kg_fix, plan.kg_fix.size()); UP(kh_fix, plan.kh_fix.size());
  UP(rt_ell, plan.rt_ell.size()); UP(rt_glen, plan.rt_glen.size()); UP(jp_ell, plan.jp_ell.size()); UP(jp_glen, plan.jp_glen.size());
  UP(cs_ell, plan.cs_ell.size()); UP(cs_glen, plan.cs_glen.size()); UP(cs_col, plan.cs_col.size()); UP(cs_own, plan.cs_own.size());
  UP(jv_ell, plan.jv_ell.size()); UP(jv_own, plan.jv_own.size()); UP(jv_glen, plan.jv_glen.size());
  UP(ja_ell, plan.ja_ell.size()); UP(ja_own, plan.ja_own.size()); UP(ja_glen, plan.ja_glen.size());
  UP(sl_list, plan.sl_list.size()); UP(sl_glen, plan.sl_glen.size());
  UP(lift_rec, plan.lift_rec.size()); UP(lift_lev, plan.lift_lev.size());
  return bind_tables(b, img);
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int omgx_version(void) { return OMGX_VERSION; }
const char* omgx_last_error(void) { return g_err.c_str(); }

const char* omgx_status_string(int32_t s) {
  switch (s) {
    case OMGX_SOLVE_SUCCEEDED: return "Solve_Succeeded";
    case OMGX_MAX_ITER_EXCEEDED: return "Maximum_Iterations_Exceeded";
    case OMGX_INFEASIBLE_DETECTED: return "Infeasible_Problem_Detected";
    case OMGX_UNSUPPORTED_BOUNDS: return "Unsupported_Bounds";
    case OMGX_NUMERICAL_FAILURE: return "Numerical_Failure";
    default: return "Unknown";
  }
}

int omgx_plan_describe(const omgx_template* tpl, omgx_plan_info* info, int32_t* order) {
  if (!info) { g_err = "null argument"; return OMGX_E_INVALID; }
  TRY(check_template(tpl));
  omgx::HostPlan plan;
  size_t nl = 0, ng = 0;
  int mode = 0, per_cu = 1;
  if (!plan_for_mode(plan, *tpl, &mode, &nl, &ng, &per_cu)) { g_err = "inconsistent template: " + plan.error; return OMGX_E_INVALID; }
  const omgx::Dims& d = plan.dims;
  memset(info, 0, sizeof *info);
  info->n_leaf = d.n_leaf; info->n_root = d.n_root; info->n_eq = d.n_eq; info->nnz_j = d.nnz_j;
  info->kkt_doubles = plan.kkt_doubles; info->wave_path = d.wave_ok;
  info->ws_mode = mode;
  info->lds_bytes = (int64_t)(nl * sizeof(double));
  for (int l = 0; l < d.n_leaf && l < OMGX_PLAN_MAX_LEAF; ++l) {
    info->leaf_size[l] = plan.leaf_off[l + 1] - plan.leaf_off[l];
    info->leaf_bw[l] = plan.leaf_bw[l];
    info->leaf_cpl[l] = plan.cpl_ptr[l + 1] - plan.cpl_ptr[l];
  }
  info->n_pairs = d.n_pairs; info->ka_len = d.ka_len; info->kh_len = d.kh_len; info->kg_len = d.kg_len;
  if (order) for (int q = 0; q < d.N; ++q) order[q] = plan.order[q];
  return OMGX_OK;
}

int omgx_plan_schur_tiles(const omgx_template* tpl, int32_t* n_banded) {
  if (!n_banded) { g_err = "null argument"; return OMGX_E_INVALID; }
  TRY(check_template(tpl));
  omgx::HostPlan plan;
  size_t nl = 0, ng = 0;
  int mode = 0, per_cu = 1;
  if (!plan_for_mode(plan, *tpl, &mode, &nl, &ng, &per_cu)) { g_err = "inconsistent template: " + plan.error; return OMGX_E_INVALID; }
  *n_banded = plan.dims.schur_tiles;
  return OMGX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Template files: the counts and arrays of omgx_template, written by the Python front end
// (omgtools.backend.save_template) once per problem class and read by C/C++ callers -- the role the
// generated nlp.so plays for the reference's C++ export (`export/export.py:236-262`, loaded in
// `Point2Point.cpp:80-91`).  Layout: "OMGXTPL4", 16 int32 counts (the last three: block-table entries, the length of
// their names, whether default bounds follow; "OMGXTPL5", written for templates with lifted auxiliaries: 18 counts, + n_lift and
// lift_row0), then the arrays in struct order, the block table last ("OMGXTPL3" files -- three variables per term -- and "OMGXTPL2" files -- 13 counts, no table -- are still read).
namespace {
struct TplField { int kind; size_t count; const void* const* src; void** dst; };     // kind 0 int32, 1 double, 2 char

size_t tpl_fields(const omgx_template& t, omgx_template* m, TplField* f, int term_vars = OMGX_TERM_VARS) {
  const omgx_template& s = t;
  size_t k = 0;
#define OMGX_F(KD, NAME, CNT) f[k].kind = KD; f[k].count = (size_t)(CNT); f[k].src = (const void* const*)&s.NAME; f[k].dst = m ? (void**)&m->NAME : nullptr; ++k;
  OMGX_F(0, prog, 6 * (size_t)t.n_prog)      OMGX_F(1, knots, t.n_knots)       OMGX_F(0, pp_ptr, t.n_pp + 1)
  OMGX_F(1, pm_coef, t.n_mono)               OMGX_F(0, pm_ptr, t.n_mono + 1)   OMGX_F(0, pm_atom, t.n_matom)
  OMGX_F(0, slot_pp, t.n_slots)              OMGX_F(0, row_ptr, t.n_con + 2)   OMGX_F(1, t_coef, t.n_terms)
  OMGX_F(0, t_slot, t.n_terms)               OMGX_F(0, t_var, (size_t)term_vars * t.n_terms)
  OMGX_F(0, eq_rows, t.n_eq)                 OMGX_F(0, root_vars, t.n_root_vars)
  OMGX_F(2, block_names, t.block_names_len)  OMGX_F(0, block_kind, t.n_blocks)        OMGX_F(0, block_off, t.n_blocks)
  OMGX_F(0, block_rows, t.n_blocks)          OMGX_F(0, block_cols, t.n_blocks)
  OMGX_F(1, lbg_def, t.has_bounds ? t.n_con : 0)  OMGX_F(1, ubg_def, t.has_bounds ? t.n_con : 0)
#undef OMGX_F
  return k;
}
}  // namespace

int omgx_template_write(const omgx_template* tpl, const char* path) {
  TRY(check_template(tpl));
  if (!path) { g_err = "null path"; return OMGX_E_INVALID; }
  FILE* fp = fopen(path, "wb");
  if (!fp) { g_err = std::string("cannot write ") + path; return OMGX_E_INVALID; }
  const int32_t counts[18] = {tpl->n_var, tpl->n_par, tpl->n_con, tpl->n_atoms, tpl->n_slots, tpl->n_terms, tpl->n_prog,
                              tpl->n_knots, tpl->n_pp, tpl->n_mono, tpl->n_matom, tpl->n_eq, tpl->n_root_vars,
                              tpl->n_blocks, tpl->block_names_len, tpl->has_bounds ? 1 : 0, tpl->n_lift, tpl->lift_row0};
  // (a template without lifted auxiliaries is written as before: "OMGXTPL4", 16 counts)
  const bool v5 = tpl->n_lift > 0;
  bool ok = fwrite(v5 ? "OMGXTPL5" : "OMGXTPL4", 1, 8, fp) == 8 && fwrite(counts, sizeof(int32_t), v5 ? 18 : 16, fp) == (size_t)(v5 ? 18 : 16);
  TplField f[24];
  const size_t nf = tpl_fields(*tpl, nullptr, f);
  for (size_t i = 0; i < nf && ok; ++i) {
    const size_t sz = f[i].kind == 1 ? sizeof(double) : (f[i].kind == 2 ? 1 : sizeof(int32_t));
    if (f[i].count && fwrite(*f[i].src, sz, f[i].count, fp) != f[i].count) ok = false;
  }
  if (fclose(fp) != 0) ok = false;
  if (!ok) { g_err = std::string("short write to ") + path; return OMGX_E_INVALID; }
  return OMGX_OK;
}

void omgx_template_free(omgx_template* t) {
  if (!t) return;
  TplField f[24];
  const size_t nf = tpl_fields(*t, t, f);
  for (size_t i = 0; i < nf; ++i) free(*f[i].dst);
  free(t);
}

int omgx_template_read(const char* path, omgx_template** out) {
  if (!path || !out) { g_err = "null argument"; return OMGX_E_INVALID; }
  *out = nullptr;
  FILE* fp = fopen(path, "rb");
  if (!fp) { g_err = std::string("cannot read ") + path; return OMGX_E_INVALID; }
  char magic[8];
  int32_t c[18] = {0};
  const bool head = fread(magic, 1, 8, fp) == 8;
  const int file_version = !head ? 0 : (memcmp(magic, "OMGXTPL5", 8) == 0 ? 5 : (memcmp(magic, "OMGXTPL4", 8) == 0 ? 4 : (memcmp(magic, "OMGXTPL3", 8) == 0 ? 3 : (memcmp(magic, "OMGXTPL2", 8) == 0 ? 2 : 0))));
  const int n_counts = file_version >= 5 ? 18 : (file_version >= 3 ? 16 : (file_version == 2 ? 13 : 0));
  const int file_tv = file_version >= 4 ? OMGX_TERM_VARS : 3;
  if (n_counts == 0 || fread(c, sizeof(int32_t), n_counts, fp) != (size_t)n_counts) {
    fclose(fp); g_err = std::string(path) + " is not an omgx template file"; return OMGX_E_INVALID;
  }
  for (int i = 0; i < 18; ++i) if (c[i] < 0 || c[i] > (1 << 26)) { fclose(fp); g_err = "template file: bad counts"; return OMGX_E_INVALID; }
  omgx_template* t = (omgx_template*)calloc(1, sizeof(omgx_template));
  if (!t) { fclose(fp); g_err = "out of memory"; return OMGX_E_INVALID; }
  t->n_var = c[0]; t->n_par = c[1]; t->n_con = c[2]; t->n_atoms = c[3]; t->n_slots = c[4]; t->n_terms = c[5]; t->n_prog = c[6];
  t->n_knots = c[7]; t->n_pp = c[8]; t->n_mono = c[9]; t->n_matom = c[10]; t->n_eq = c[11]; t->n_root_vars = c[12];
  t->n_blocks = c[13]; t->block_names_len = c[14]; t->has_bounds = c[15];
  t->n_lift = c[16]; t->lift_row0 = c[17];
  TplField f[24];
  const size_t nf = tpl_fields(*t, t, f, file_tv);
  bool ok = true;
  for (size_t i = 0; i < nf; ++i) {
    const size_t sz = f[i].kind == 1 ? sizeof(double) : (f[i].kind == 2 ? 1 : sizeof(int32_t));
    *f[i].dst = calloc(f[i].count + 1, sz);                  // (+1: an empty array still gets an address)
    if (!*f[i].dst) { ok = false; continue; }
    if (ok && f[i].count && fread(*f[i].dst, sz, f[i].count, fp) != f[i].count) ok = false;
  }
  fclose(fp);
  if (ok && file_tv != OMGX_TERM_VARS) {
    // an older file: three variables per term
    int32_t* wide = (int32_t*)calloc((size_t)OMGX_TERM_VARS * t->n_terms + 1, sizeof(int32_t));
    if (!wide) ok = false;
    else {
      for (int i = 0; i < t->n_terms; ++i)
        for (int k = 0; k < OMGX_TERM_VARS; ++k) wide[OMGX_TERM_VARS * i + k] = k < file_tv ? t->t_var[file_tv * i + k] : -1;
      free((void*)t->t_var);
      t->t_var = wide;
    }
  }
  if (!ok) { omgx_template_free(t); g_err = std::string("truncated template file ") + path; return OMGX_E_INVALID; }
  const int rc = check_template(t);
  if (rc != OMGX_OK) { omgx_template_free(t); return rc; }
  *out = t;
  return OMGX_OK;
}

// ---- block table -----------------------------------------------------------------------------------------
namespace {
// name of block i (its offset inside block_names), or nullptr when the table is malformed
const char* block_name(const omgx_template* t, int i) {
  if (!t->block_names || t->block_names_len <= 0 || t->block_names[t->block_names_len - 1] != 0) return nullptr;
  const char* p = t->block_names;
  const char* end = t->block_names + t->block_names_len;
  for (int k = 0; k < i; ++k) { p += strlen(p) + 1; if (p >= end) return nullptr; }
  return p < end ? p : nullptr;
}
}  // namespace

int omgx_template_n_blocks(const omgx_template* tpl, int32_t kind) {
  if (!tpl) { g_err = "null template"; return OMGX_E_INVALID; }
  int n = 0;
  for (int i = 0; i < tpl->n_blocks; ++i) if (tpl->block_kind[i] == kind) ++n;
  return n;
}

int omgx_template_block_at(const omgx_template* tpl, int32_t kind, int32_t i, const char** name, int32_t* off,
                           int32_t* rows, int32_t* cols) {
  if (!tpl || i < 0) { g_err = "bad argument"; return OMGX_E_INVALID; }
  int n = 0;
  for (int k = 0; k < tpl->n_blocks; ++k) {
    if (tpl->block_kind[k] != kind) continue;
    if (n++ == i) {
      const char* nm = block_name(tpl, k);
      if (!nm) { g_err = "malformed block table"; return OMGX_E_INVALID; }
      if (name) *name = nm;
      if (off) *off = tpl->block_off[k];
      if (rows) *rows = tpl->block_rows[k];
      if (cols) *cols = tpl->block_cols[k];
      return OMGX_OK;
    }
  }
  g_err = "block index out of range"; return OMGX_E_INVALID;
}

int omgx_template_block(const omgx_template* tpl, int32_t kind, const char* name, int32_t* off, int32_t* rows,
                        int32_t* cols) {
  if (!tpl || !name) { g_err = "null argument"; return OMGX_E_INVALID; }
  for (int k = 0; k < tpl->n_blocks; ++k) {
    const char* nm = tpl->block_kind[k] == kind ? block_name(tpl, k) : nullptr;
    if (nm && strcmp(nm, name) == 0) {
      if (off) *off = tpl->block_off[k];
      if (rows) *rows = tpl->block_rows[k];
      if (cols) *cols = tpl->block_cols[k];
      return OMGX_OK;
    }
  }
  g_err = std::string("the template has no entry named ") + name; return OMGX_E_INVALID;
}

void omgx_default_options(omgx_options* o) {
  o->tol = 1e-3; o->max_iter = 300; o->mu_init = 0.1; o->kappa_push = 1.0;
  o->nu_init = 100.0; o->scale_gmax = 100.0; o->warm_start = 0; o->kappa_warm = 1e-3;
  o->dw_leaf_ratio_cold = 1.0; o->warm_mu_factor = 1.0; o->warm_z_floor = 0.1; o->warm_z_cap = 0.01; o->max_soc = 1; o->hess_approx = 0; o->compl_inf_tol = 0.0; o->constr_viol_tol = 0.0; o->refine = 0;
}

namespace {
// the body of omgx_batch_create: any non-zero result makes the caller destroy the handle, whatever it holds by then
int create_batch(omgx_batch* b, const omgx_template* tpl) {
  const int n_agents = b->n_agents;
  omgx_options o; omgx_default_options(&o);
  (void)omgx_batch_set_options(b, &o);      // (the defaults pass its checks unchanged)
  ExpandedTemplate ex;
  const bool ranged = expand_range_rows(tpl, ex);
  b->n_con_user = tpl->n_con; b->n_range = ranged ? (int)ex.src.size() : 0;
  int rc = build_batch(b, ranged ? &ex.t : tpl);
  if (rc != OMGX_OK) return rc;
  const omgx::Dims& d = b->dims;
  b->inst = instances_for(b->ws_mode, d.wave_ok, d.general);
  if (ranged) {
    if (dalloc(b, ex.src.size(), &b->d_range_src) != OMGX_OK || dalloc(b, ex.dup.size(), &b->d_range_dup) != OMGX_OK ||
        hipMemcpy(b->d_range_src, ex.src.data(), ex.src.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b->d_range_dup, ex.dup.data(), ex.dup.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
      g_err = "hipMalloc failed"; return OMGX_E_HIP;
    }
    if ((rc = dalloc(b, (size_t)n_agents * b->n_con_user, &b->d_lam_user)) || (rc = dalloc(b, (size_t)n_agents * b->n_con_user, &b->d_lb_user)) ||
        (rc = dalloc(b, (size_t)n_agents * b->n_con_user, &b->d_ub_user))) return rc;
  }
  if ((rc = dalloc(b, (size_t)n_agents * d.n_par, &b->d_p)) || (rc = dalloc(b, (size_t)n_agents * d.n_var, &b->d_x0)) ||
      (rc = dalloc(b, (size_t)n_agents * d.n_con, &b->d_lb)) || (rc = dalloc(b, (size_t)n_agents * d.n_con, &b->d_ub)) ||
      (rc = dalloc(b, (size_t)n_agents * d.n_var, &b->d_x)) || (rc = dalloc(b, (size_t)n_agents * d.n_con, &b->d_lam)) ||
      (rc = dalloc(b, (size_t)n_agents, &b->d_status)) || (rc = dalloc(b, (size_t)n_agents, &b->d_iters)) ||
      (rc = dalloc(b, (size_t)n_agents * omgx::PH_COUNT, &b->d_prof)) || (rc = dalloc(b, (size_t)n_agents, &b->d_dw))) return rc;
  if (hipStreamCreate(&b->own_stream) != hipSuccess || hipEventCreate(&b->ev0) != hipSuccess ||
      hipEventCreate(&b->ev1) != hipSuccess) { g_err = "stream/event creation failed"; return OMGX_E_HIP; }
  b->stream = b->own_stream;
  if (hipMemset(b->d_dw, 0, (size_t)n_agents * sizeof(double)) != hipSuccess) { g_err = "hipMemset failed"; return OMGX_E_HIP; }
  // dynamic LDS of every instance this handle can launch (the attribute belongs to the kernel, not to the handle: keep the
  // largest request of the process)
  static int lds_reserved[4 * omgx::WS_MODES] = {0};
  int& reserved = lds_reserved[4 * b->ws_mode + (d.wave_ok ? 1 : 0) + (d.general ? 2 : 0)];
  if ((int)b->lds_bytes > reserved) reserved = (int)b->lds_bytes;
  for (const ipm_kernel_t k : {b->inst.full, b->inst.refine, b->inst.lean})
    if (k && hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, reserved) != hipSuccess) { g_err = "cannot reserve dynamic LDS for ipm_solve_kernel"; return OMGX_E_HIP; }
  for (const auto& row : b->inst.rollout)
    for (const ipm_rollout_t k : row)
      if (k && hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, reserved) != hipSuccess) { g_err = "cannot reserve dynamic LDS for ipm_rollout_kernel"; return OMGX_E_HIP; }
  {
    // Persistent workgroups, as many as fit the chip at once (one or two per CU), that take their agents from an atomic
    // counter -- in every mode: solves differ by a factor of several in their iteration counts.  The workgroups of the
    // spill modes own a slab each.
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, b->device) != hipSuccess) { g_err = "hipGetDeviceProperties failed"; return OMGX_E_HIP; }
    int per_cu = (int)((size_t)kLdsLimit / (b->lds_bytes > 0 ? b->lds_bytes : 1));
    per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);
    if (b->ws_mode == omgx::WS_LDS || b->ws_mode == omgx::WS_JAC_ONLY || b->ws_mode == omgx::WS_JAC_HV) per_cu = b->per_cu;      // (bound by the registers of 512-thread workgroups otherwise)
    int slabs = prop.multiProcessorCount * per_cu;
    if (slabs > n_agents) slabs = n_agents;
    b->n_slabs = slabs;
    if (b->slab_doubles > 0 && (rc = dalloc(b, (size_t)slabs * b->slab_doubles, &b->d_slabs))) return rc;
    if ((rc = dalloc(b, (size_t)2, &b->d_next))) return rc;
    if (hipMemset(b->d_next, 0, 2 * sizeof(int)) != hipSuccess) { g_err = "hipMemset failed"; return OMGX_E_HIP; }
  }
  // the setup kernel's records (omgx::prep_layout: ~43 KB per agent for config 2) and its LDS (atoms, knots, slots, x)
  b->prep_doubles = (size_t)omgx::prep_layout(d).total;
  b->prep_lds = prepare_lds_doubles(d) * sizeof(double);
  // OFF by default (omgx_batch_set_prepare / OMGX_PREPARE=1 switch it on).  Measured on the 1024-agent benchmark batch (round 6,
  // profiles/r06_prepare_ab.txt): the solve kernel drops from 341 k to 277 k cycles per warm-started solve (its setup phase 77 k ->
  // 6 k), but the setup kernel takes 64 us for the 1024 agents -- every workgroup walks the same chain of ~80 dependent table
  // loads whatever the occupancy, and at the head of the solve kernel that chain already overlaps with the agent that shares
  // the CU -- against 43 us saved: 1.73-1.74 M against 1.74-1.79 M solves/s with one launch per step.
  const char* env = getenv("OMGX_PREPARE");
  return env && env[0] == '1' ? omgx_batch_set_prepare(b, 1) : OMGX_OK;
}
}  // namespace

int omgx_batch_create(const omgx_template* tpl, int32_t n_agents, int32_t device, omgx_batch** out) {
  if (!tpl || !out || n_agents <= 0 || device < 0) { g_err = "bad argument"; return OMGX_E_INVALID; }
  TRY(check_template(tpl));
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device >= count) {
    g_err = "no usable HIP device (the solve path has no CPU fallback)";
    return OMGX_E_NODEVICE;
  }
  HIPCHK(hipSetDevice(device));
  omgx_batch* b = new omgx_batch();
  b->device = device; b->n_agents = n_agents;
  const int rc = create_batch(b, tpl);
  if (rc != OMGX_OK) { omgx_batch_destroy(b); return rc; }      // (the one failure path: destroy frees whatever exists by now)
  *out = b;
  return OMGX_OK;
}

int omgx_batch_set_prepare(omgx_batch* b, int32_t on) {
  if (!b) return OMGX_E_INVALID;
  if (!on) { b->prepare_on = false; return OMGX_OK; }
  if (b->prep_lds > (size_t)kLdsLimit) { g_err = "the setup kernel's LDS (atoms, knots, slots, x) does not fit one CU for this template"; return OMGX_E_INVALID; }
  if (!b->d_prep) {      // the records: allocated when the kernel is first asked for
    HIPCHK(hipSetDevice(b->device));
    TRY(dalloc(b, (size_t)b->n_agents * b->prep_doubles, &b->d_prep));
    static int prep_reserved[2] = {0, 0};
    int& res = prep_reserved[b->dims.general ? 1 : 0];
    if ((int)b->prep_lds > res) res = (int)b->prep_lds;
    if (hipFuncSetAttribute((const void*)b->inst.prepare, hipFuncAttributeMaxDynamicSharedMemorySize, res) != hipSuccess) { g_err = "cannot reserve dynamic LDS for ipm_prepare_kernel"; return OMGX_E_HIP; }
  }
  b->prepare_on = true;
  return OMGX_OK;
}

int omgx_batch_set_stop(omgx_batch* b, int32_t o_state0, int32_t o_input0, int32_t o_poseT, int32_t n_dim, double stop_tol, int32_t* under_way) {
  if (!b) { g_err = "bad argument"; return OMGX_E_INVALID; }
  if (!under_way) { b->stop_on = false; return OMGX_OK; }
  b->stop_on = false;      // (a failed registration leaves the rule OFF)
  const int np = b->dims.n_par;
  if (n_dim <= 0 || o_state0 < 0 || o_input0 < 0 || o_poseT < 0 || o_state0 + n_dim > np || o_input0 + n_dim > np || o_poseT + n_dim > np ||
      stop_tol != stop_tol) { g_err = "stop rule: parameter offsets out of range or a tolerance that is not a number"; return OMGX_E_INVALID; }      // (a negative tolerance is a rule that never holds: every agent is solved at every update)
  HIPCHK(hipSetDevice(b->device));
  StopArgs sa;
  sa.o_state = o_state0; sa.o_input = o_input0; sa.o_pose = o_poseT; sa.n_dim = n_dim; sa.tol = stop_tol; sa.under_way = under_way;
  TRY(push_args(b, &b->d_stop, sa));
  HIPCHK(hipStreamSynchronize(b->stream));
  b->stop_host = sa;
  b->stop_on = true;
  return OMGX_OK;
}

void omgx_batch_destroy(omgx_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  for (void* p : b->allocs) (void)hipFree(p);      // (everything dalloc handed out; the DevBufs go with `delete b`)
  table_cache().release(b->tables);                // (the last handle of the template on this device frees the image)
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
}

// the caller's options as the kernels take them
static omgx::Opts opts_of(const omgx_options* o) {
  return {o->tol, o->max_iter, o->mu_init, o->kappa_push, o->nu_init, o->scale_gmax, o->warm_start, o->kappa_warm,
             o->dw_leaf_ratio_cold > 0 ? o->dw_leaf_ratio_cold : 1.0, 0, o->warm_mu_factor >= 0 ? o->warm_mu_factor : 0.0,
             o->warm_z_floor >= 0 ? o->warm_z_floor : 0.0, o->warm_z_cap >= 0 ? o->warm_z_cap : 0.0, o->max_soc > 0 ? (o->max_soc > 8 ? 8 : o->max_soc) : 0, o->hess_approx > 0 ? 1 : 0,
             o->compl_inf_tol > 0 ? o->compl_inf_tol : 0.0, o->constr_viol_tol > 0 ? o->constr_viol_tol : 0.0, o->refine > 0 ? 1 : 0};
}

int omgx_batch_set_options(omgx_batch* b, const omgx_options* o) {
  if (!b || !o || !(o->tol > 0) || o->max_iter < 0) { g_err = "bad options"; return OMGX_E_INVALID; }
  b->opts = opts_of(o);
  return OMGX_OK;
}

int omgx_batch_set_stream(omgx_batch* b, void* s) {
  if (!b) return OMGX_E_INVALID;
  b->stream = s ? (hipStream_t)s : b->own_stream;
  return OMGX_OK;
}

static int flush_order(omgx_batch* b) {
  if (!b->pend_iters) return OMGX_OK;
  hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, b->stream, b->pend_iters, (const double*)(b->order_dw ? b->d_dw : nullptr), b->pend_order, b->n_agents);
  b->pend_iters = nullptr; b->pend_order = nullptr;
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_set_order(omgx_batch* b, const int32_t* order_device) {
  if (!b) return OMGX_E_INVALID;
  b->d_order = order_device;
  b->pend_iters = nullptr; b->pend_order = nullptr;
  return OMGX_OK;
}

int omgx_batch_set_restarts(omgx_batch* b, const double* x0_alt_device, int32_t n_alt, int32_t* attempts_device) {
  if (!b || n_alt < 0 || (n_alt > 0 && !x0_alt_device)) { g_err = "bad argument"; return OMGX_E_INVALID; }
  b->d_x0_alt = n_alt > 0 ? x0_alt_device : nullptr;
  b->n_alt = n_alt;
  b->d_attempts = attempts_device;
  return OMGX_OK;
}

int omgx_batch_order_by_iters(omgx_batch* b, const int32_t* iters_device, int32_t* order_device) {
  if (!b || !iters_device || !order_device) { g_err = "null argument"; return OMGX_E_INVALID; }
  // deferred: the next omgx_batch_predict(_ex) launch carries the ordering as one more workgroup; a solve that comes
  // first launches order_kernel itself (flush_order)
  b->pend_iters = iters_device; b->pend_order = order_device;
  b->d_order = order_device;
  return OMGX_OK;
}

int omgx_batch_lds_bytes(const omgx_batch* b) { return b ? (int)b->lds_bytes : OMGX_E_INVALID; }

int omgx_batch_last_instance(const omgx_batch* b) { return b ? b->last_instance : OMGX_E_INVALID; }

int omgx_batch_workspace(const omgx_batch* b, int32_t* mode, int64_t* lds_bytes, int64_t* hbm_bytes_per_slab, int32_t* n_slabs) {
  if (!b) return OMGX_E_INVALID;
  if (mode) *mode = b->ws_mode;
  if (lds_bytes) *lds_bytes = (int64_t)b->lds_bytes;
  if (hbm_bytes_per_slab) *hbm_bytes_per_slab = (int64_t)(b->slab_doubles * sizeof(double));
  if (n_slabs) *n_slabs = b->n_slabs;
  return OMGX_OK;
}

int omgx_batch_solve(omgx_batch* b, const double* p, const double* x0, const double* lbg, const double* ubg,
                     double* x, double* lam_g, int32_t* status, int32_t* iters, int32_t flags) {
  if (!b || !p || !x0 || !lbg || !ubg || !x || !lam_g || !status || !iters) { g_err = "null argument"; return OMGX_E_INVALID; }
  HIPCHK(hipSetDevice(b->device));
  const omgx::Dims& d = b->dims;
  const int B = b->n_agents;
  const bool dev = flags & OMGX_PTR_DEVICE, shared = flags & OMGX_BOUNDS_SHARED;
  const bool bdev = (flags & OMGX_BOUNDS_DEVICE) != 0;
  // (nu: rows of the caller's arrays; d.n_con: rows of the kernel's -- more when two-sided rows were doubled, omgx_batch::n_range)
  const int nu = b->n_con_user, ni = d.n_con;
  const bool ranged = b->n_range > 0;
  const size_t nb = (shared ? 1 : (size_t)B) * nu;
  const double *kp = p, *kx0 = x0, *klb = lbg, *kub = ubg;
  double *kx = x, *klam = lam_g; int32_t *kst = status, *kit = iters;
  const bool lam_in = b->opts.warm_start || (flags & OMGX_ONLY_FAILED);
  double* lam_user_dev = ranged ? (dev ? lam_g : b->d_lam_user) : nullptr;       // the caller's multipliers on the device
  if (!dev) {
    HIPCHK(hipMemcpyAsync(b->d_p, p, (size_t)B * d.n_par * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->d_x0, x0, (size_t)B * d.n_var * sizeof(double), hipMemcpyHostToDevice, b->stream));
    double* lam_to = ranged ? b->d_lam_user : b->d_lam;
    if (lam_in) {                         // a warm start or a restart pass reads the multipliers and the statuses
      HIPCHK(hipMemcpyAsync(lam_to, lam_g, (size_t)B * nu * sizeof(double), hipMemcpyHostToDevice, b->stream));
      HIPCHK(hipMemcpyAsync(b->d_status, status, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, b->stream));
    }
    if (flags & OMGX_ONLY_FAILED) {       // the skipped agents keep what the caller's buffers hold
      HIPCHK(hipMemcpyAsync(b->d_x, x, (size_t)B * d.n_var * sizeof(double), hipMemcpyHostToDevice, b->stream));
      HIPCHK(hipMemcpyAsync(b->d_iters, iters, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, b->stream));
    }
    kp = b->d_p; kx0 = b->d_x0; kx = b->d_x; klam = b->d_lam; kst = b->d_status; kit = b->d_iters;
  }
  if (ranged) {
    klam = b->d_lam;
    if (lam_in)
      hipLaunchKernelGGL(range_expand_lam, dim3((B * ni + 255) / 256), dim3(256), 0, b->stream, (const double*)lam_user_dev, b->d_lam, B, nu, ni,
                         (const int32_t*)b->d_range_src, (const int32_t*)b->d_range_dup);
  }
  if (!bdev) {
    double* lb_to = ranged ? b->d_lb_user : b->d_lb;
    double* ub_to = ranged ? b->d_ub_user : b->d_ub;
    HIPCHK(hipMemcpyAsync(lb_to, lbg, nb * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(ub_to, ubg, nb * sizeof(double), hipMemcpyHostToDevice, b->stream));
    klb = lb_to; kub = ub_to;
  }
  if (ranged) {
    const int sets = shared ? 1 : B;
    hipLaunchKernelGGL(range_expand_bounds, dim3((sets * ni + 255) / 256), dim3(256), 0, b->stream, klb, kub, b->d_lb, b->d_ub, sets, nu, ni,
                       (const int32_t*)b->d_range_src, (const int32_t*)b->d_range_dup);
    klb = b->d_lb; kub = b->d_ub;
  }
  TRY(flush_order(b));
  // Timing events ride on the dispatch packet of the solve kernel (hipExtLaunchKernelGGL: the packet's own begin / end
  // stamps) -- separate hipEventRecord calls around it cost two more packets, ~25 us of stream time per solve.
  // The caller's pair (omgx_batch_set_launch_events, one launch) goes first, else the handle's own when timing is on.
  hipEvent_t e0 = b->ext_ev0 ? b->ext_ev0 : (b->timing ? b->ev0 : nullptr);
  hipEvent_t e1 = b->ext_ev0 ? b->ext_ev1 : (b->timing ? b->ev1 : nullptr);
  b->timed = b->timing && !b->ext_ev0;
  b->ext_ev0 = b->ext_ev1 = nullptr;
  b->opts.prio_iter = b->prio_iter;
  const bool prepared = b->prepare_on && b->d_prep && !b->stop_on;      // (the stop rule is the solve kernel's: it does its own setup then)
  if (prepared) {
    // the setup of all B solves, many workgroups per CU; the begin stamp of the caller's / the handle's event pair rides on this
    // launch, the end stamp on the solve kernel's: the pair brackets both
    hipExtLaunchKernelGGL(b->inst.prepare, dim3(B), dim3(b->threads), (uint32_t)b->prep_lds, b->stream, e0, nullptr, 0u, d, b->dev, b->opts,
                          kp, kx0, klb, kub, shared ? 1 : 0, (const double*)klam, (const int32_t*)kst, B, b->d_prep, b->prep_doubles, (flags & OMGX_ONLY_FAILED) ? 1 : 0);
    HIPCHK(hipGetLastError());
    e0 = nullptr;
  }
  // What this launch hands to the optional blocks of the kernel; with all of it null or zero, both absolute tolerances off and no
  // refinement it runs the lean instance (LEAN of ipm_solve_kernel: those blocks compiled out).  Decided here, per launch, from the
  // handle's state: switching a feature on or off between two launches switches the instance, nothing else to call.
  const StoreArgs* k_stp = (b->store.out || b->signals.log) ? &b->d_store->st : nullptr;
  const int k_only_failed = (flags & OMGX_ONLY_FAILED) ? 1 : 0, k_n_alt = b->d_x0_alt ? b->n_alt : 0;
  const CenterArgs* k_ctr = b->center_on ? b->d_center : nullptr;
  double* k_prep = prepared ? b->d_prep : nullptr;
  const StopArgs* k_stop = b->stop_on ? b->d_stop : nullptr;
  const bool lean_launch = !k_stp && !k_only_failed && !k_n_alt && !b->d_attempts && !k_ctr && !k_prep && !k_stop &&
                           !(b->opts.compl_tol > 0.0) && !(b->opts.viol_tol > 0.0) && !b->opts.refine;
  const Instances& in = b->inst;
  b->last_instance = lean_launch && in.lean ? 1 : 0;      // (classes without a lean instance -- general, off the wave path, spill modes -- run the full one)
  const ipm_kernel_t kern = b->last_instance ? in.lean : (b->opts.refine && in.refine ? in.refine : in.full);
  // (the slot queue only where it decides something: with a workgroup per agent every fetch would return a slot past the end)
  int* const k_next = b->n_slabs >= B ? nullptr : b->d_next;
  hipExtLaunchKernelGGL(kern, dim3(b->n_slabs), dim3(b->threads), (uint32_t)b->lds_bytes, b->stream,
                        e0, e1, 0u, d, b->dev,
                        b->opts, b->kkt_doubles, kp, kx0, klb, kub, shared ? 1 : 0, kx, klam, kst, kit, B, b->d_prof,
                        b->d_slabs, b->slab_doubles, b->d_dw, b->d_order, k_stp, k_only_failed,
                        k_next, b->d_x0_alt, k_n_alt, b->d_attempts,
                        (unsigned long long*)(b->d_stats ? b->d_stats + 4 * (size_t)(b->stats_launch++ % b->stats_slots) : nullptr),
                        b->stagger, k_ctr, k_prep, b->prep_doubles, k_stop);
  HIPCHK(hipGetLastError());
  if (ranged)
    hipLaunchKernelGGL(range_contract_lam, dim3((B * nu + 255) / 256), dim3(256), 0, b->stream, (const double*)b->d_lam, lam_user_dev, B, nu, ni,
                       (const int32_t*)b->d_range_dup);
  if (!dev) {
    HIPCHK(hipMemcpyAsync(x, b->d_x, (size_t)B * d.n_var * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipMemcpyAsync(lam_g, ranged ? b->d_lam_user : b->d_lam, (size_t)B * nu * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipMemcpyAsync(status, b->d_status, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipMemcpyAsync(iters, b->d_iters, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  return OMGX_OK;
}

#ifdef OMGX_PROFILE
int omgx_batch_phase_cycles(omgx_batch* b, long long* out) {   // profiling build only
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(out, b->d_prof, (size_t)b->n_agents * omgx::PH_COUNT * sizeof(long long), hipMemcpyDeviceToHost));
  return OMGX_OK;
}
#endif

int omgx_batch_transfer(omgx_batch* b, int32_t n_seg, const void* const* src, void* const* dst, const int64_t* bytes) {
  if (!b || n_seg < 0 || n_seg > OMGX_TRANSFER_MAX || (n_seg > 0 && (!src || !dst || !bytes))) { g_err = "bad argument"; return OMGX_E_INVALID; }
  if (n_seg == 0) return OMGX_OK;
  TransferArgs a;
  memset(&a, 0, sizeof a);
  a.n_seg = n_seg;
  int blocks = 0;
  for (int i = 0; i < n_seg; ++i) {
    if (!src[i] || !dst[i] || bytes[i] < 0 || (bytes[i] & 7) || (((size_t)src[i] | (size_t)dst[i]) & 7)) { g_err = "transfer: segments are 8-byte aligned multiples of 8 bytes"; return OMGX_E_INVALID; }
    a.src[i] = (const double*)src[i]; a.dst[i] = (double*)dst[i]; a.n8[i] = bytes[i] / 8;
    a.blk0[i] = blocks;
    // (a workgroup per 16 KB, at least one, at most 256 per segment: enough requests in flight to fill the host link)
    long long nb = (bytes[i] + 16383) / 16384;
    blocks += (int)(nb < 1 ? 1 : (nb > 256 ? 256 : nb));
  }
  a.blk0[n_seg] = blocks;
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(transfer_kernel, dim3(blocks), dim3(256), 0, b->stream, a);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_sync(omgx_batch* b) {
  if (!b) return OMGX_E_INVALID;
  TRY(flush_order(b));      // (a deferred omgx_batch_order_by_iters)
  HIPCHK(hipStreamSynchronize(b->stream));
  return OMGX_OK;
}

int omgx_batch_eval(omgx_batch* b, const double* p, const double* x, const double* lam_g, double* g, double* f,
                    double* jac, double* hess) {
  if (!b || !p || !x || !lam_g) { g_err = "null argument"; return OMGX_E_INVALID; }
  if (b->n_range > 0) { g_err = "omgx_batch_eval: not available for a template with two-sided rows (the kernel's rows are not the caller's)"; return OMGX_E_INVALID; }
  HIPCHK(hipSetDevice(b->device));
  const omgx::Dims& d = b->dims;
  const int B = b->n_agents;
  const size_t stride = (size_t)d.n_con + 1 + d.nnz_j + b->kkt_doubles;
  DevBuf out_buf, lam_buf;      // temporaries of this call: freed on every way out
  HIPCHK(out_buf.alloc((size_t)B * stride * sizeof(double)));
  if (lam_buf.alloc((size_t)B * d.n_con * sizeof(double)) != hipSuccess) { g_err = "hipMalloc failed"; return OMGX_E_HIP; }
  double *d_out = (double*)out_buf.p, *d_lam = (double*)lam_buf.p;
  std::vector<double> out((size_t)B * stride);
  hipError_t e = hipMemcpyAsync(b->d_p, p, (size_t)B * d.n_par * sizeof(double), hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(b->d_x0, x, (size_t)B * d.n_var * sizeof(double), hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_lam, lam_g, (size_t)B * d.n_con * sizeof(double), hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(b->inst.eval, dim3(b->n_slabs), dim3(b->threads), (uint32_t)b->lds_bytes,
                       b->stream, d, b->dev, b->kkt_doubles, (const double*)b->d_p, (const double*)b->d_x0, (const double*)d_lam, B,
                       b->d_slabs, b->slab_doubles, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
  if (e != hipSuccess) { g_err = std::string("omgx_batch_eval: ") + hipGetErrorString(e); return OMGX_E_HIP; }
  const size_t nv = d.n_var, nc = d.n_con;
  for (int a = 0; a < B; ++a) {
    const double* o = out.data() + (size_t)a * stride;
    if (g) for (size_t r = 0; r < nc; ++r) g[a * nc + r] = o[r];
    if (f) f[a] = o[nc];
    if (jac) {
      double* J = jac + (size_t)a * (nc + 1) * nv;
      for (size_t i = 0; i < (nc + 1) * nv; ++i) J[i] = 0.0;
      for (int en = 0; en < d.nnz_j; ++en) J[(size_t)b->ev_jrow[en] * nv + b->ev_jvar[en]] = o[nc + 1 + en];
    }
    if (hess) {
      double* Hm = hess + (size_t)a * nv * nv;
      for (size_t i = 0; i < nv * nv; ++i) Hm[i] = 0.0;
      const double* kk = o + nc + 1 + d.nnz_j;
      for (size_t i = 0; i + 2 < b->ev_hess.size(); i += 3) {
        const int va = b->ev_hess[i + 1], vb = b->ev_hess[i + 2];
        Hm[(size_t)va * nv + vb] = kk[b->ev_hess[i]]; Hm[(size_t)vb * nv + va] = kk[b->ev_hess[i]];
      }
    }
  }
  return OMGX_OK;
}

int omgx_batch_set_stats(omgx_batch* b, int64_t* stats_device, int32_t n_slots) {
  if (!b || n_slots < 0 || (n_slots > 0 && !stats_device)) { g_err = "bad argument"; return OMGX_E_INVALID; }
  b->d_stats = n_slots > 0 ? stats_device : nullptr;
  b->stats_slots = n_slots; b->stats_launch = 0;
  return OMGX_OK;
}

int omgx_batch_set_launch_events(omgx_batch* b, void* start_event, void* stop_event) {
  if (!b || (!start_event) != (!stop_event)) { g_err = "bad argument"; return OMGX_E_INVALID; }
  b->ext_ev0 = (hipEvent_t)start_event; b->ext_ev1 = (hipEvent_t)stop_event;
  return OMGX_OK;
}

int omgx_batch_set_timing(omgx_batch* b, int32_t on) {
  if (!b) { g_err = "null handle"; return OMGX_E_INVALID; }
  b->timing = on != 0;
  if (!b->timing) b->timed = false;
  return OMGX_OK;
}

int omgx_batch_last_kernel_ms(omgx_batch* b, double* ms) {
  if (!b || !ms || !b->timed) { g_err = "no timed launch"; return OMGX_E_INVALID; }
  HIPCHK(hipEventSynchronize(b->ev1));
  float f = 0.f;
  HIPCHK(hipEventElapsedTime(&f, b->ev0, b->ev1));
  *ms = f;
  return OMGX_OK;
}

namespace {
// entries / T matrices of a shift into the handle's device buffers (no-op when unchanged); max_elems: LDS doubles
int stage_shift_tables(omgx_batch* b, const int32_t* entries, int32_t n_ent, const double* Tmats, int32_t n_tmat,
                       int limit, int* max_elems) {
  *max_elems = 0;
  for (int e = 0; e < n_ent; ++e) {
    const int32_t* q = entries + 4 * e;
    if (q[0] < 0 || q[1] <= 0 || q[2] <= 0 || q[3] < 0 || q[0] + q[1] * q[2] > limit || q[3] + q[1] * q[1] > n_tmat) {
      g_err = "shift entry outside the array / the matrices"; return OMGX_E_INVALID;
    }
    if (q[1] * q[2] > *max_elems) *max_elems = q[1] * q[2];
  }
  const size_t ne = 4 * (size_t)n_ent, nt = (size_t)n_tmat;
  ++b->shift_clock;
  for (auto& ss : b->shift_sets)
    if (ss.ent.size() == ne && ss.T.size() == nt && memcmp(ss.ent.data(), entries, ne * sizeof(int32_t)) == 0 &&
        memcmp(ss.T.data(), Tmats, nt * sizeof(double)) == 0) {
      ss.used = b->shift_clock; b->d_shift_ent = (int32_t*)ss.d_ent.p; b->d_shift_T = (double*)ss.d_T.p;
      return OMGX_OK;
    }
  const size_t kShiftSets = 16;
  if (b->shift_sets.size() >= kShiftSets) {       // the least recently used set goes (its buffers may still be read by a queued launch: hipFree waits)
    size_t old = 0;
    for (size_t i = 1; i < b->shift_sets.size(); ++i) if (b->shift_sets[i].used < b->shift_sets[old].used) old = i;
    b->shift_sets.erase(b->shift_sets.begin() + old);
  }
  omgx_batch::ShiftSet ss;
  ss.ent.assign(entries, entries + ne); ss.T.assign(Tmats, Tmats + nt); ss.used = b->shift_clock;
  HIPCHK(ss.d_ent.alloc(ne * sizeof(int32_t)));
  if (ss.d_T.alloc(nt * sizeof(double)) != hipSuccess) { g_err = "hipMalloc failed"; return OMGX_E_HIP; }
  // (fresh buffers nothing in flight reads: plain synchronous copies)
  if (hipMemcpy(ss.d_ent.p, ss.ent.data(), ne * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(ss.d_T.p, ss.T.data(), nt * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    g_err = "hipMemcpy failed"; return OMGX_E_HIP;
  }
  b->d_shift_ent = (int32_t*)ss.d_ent.p; b->d_shift_T = (double*)ss.d_T.p;
  b->shift_sets.push_back(std::move(ss));
  return OMGX_OK;
}
}  // namespace

int omgx_batch_shift(omgx_batch* b, double* x, const uint8_t* mask, const int32_t* entries, int32_t n_ent,
                     const double* Tmats, int32_t n_tmat, int32_t flags) {
  if (!b || !x || !entries || !Tmats || n_ent <= 0 || n_tmat <= 0) { g_err = "bad argument"; return OMGX_E_INVALID; }
  HIPCHK(hipSetDevice(b->device));
  const omgx::Dims& d = b->dims;
  const int B = b->n_agents;
  const bool dev = flags & OMGX_PTR_DEVICE;
  int max_elems = 0;
  TRY(stage_shift_tables(b, entries, n_ent, Tmats, n_tmat, d.n_var, &max_elems));
  const uint8_t* d_mask = mask; double* d_xx = x;
  if (!dev) {
    HIPCHK(hipMemcpyAsync(b->d_x, x, (size_t)B * d.n_var * sizeof(double), hipMemcpyHostToDevice, b->stream));
    d_xx = b->d_x;
    if (mask) {
      if (!b->d_mask) TRY(dalloc(b, (size_t)B, &b->d_mask));      // (one size for the life of the handle)
      HIPCHK(hipMemcpyAsync(b->d_mask, mask, B, hipMemcpyHostToDevice, b->stream));
      d_mask = b->d_mask;
    }
  }
  hipLaunchKernelGGL(shift_kernel, dim3(B), dim3(64), max_elems * sizeof(double), b->stream, d_xx, d.n_var,
                     d_mask, b->d_shift_ent, n_ent, b->d_shift_T);
  HIPCHK(hipGetLastError());
  if (!dev) {
    HIPCHK(hipMemcpyAsync(x, b->d_x, (size_t)B * d.n_var * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  return OMGX_OK;      // device pointers: stream-ordered, no host synchronisation
}

int omgx_batch_sample(omgx_batch* b, const double* x, int32_t coeff_off, int32_t n_spl, int32_t degree,
                      const double* knots, int32_t n_knots, int32_t n_der, const double* t0, double dt,
                      int32_t n_samp, void* out, int32_t as_f32, int32_t flags) {
  if (!x || !t0 || !out) return bad("sample: null x / t0 / out");
  const Plan pl{coeff_off, n_spl, degree, n_knots, 0.0, knots};
  TRY(check_plan("sample", pl, 0, kAnySpl, false));
  if (n_der < 1 || n_der > degree + 1) return bad("sample: n_der = %d outside 1 .. degree + 1 = %d", n_der, degree + 1);
  if (n_samp <= 0) return bad("sample: n_samp = %d must be positive", n_samp);
  if (!b) return bad("null handle");
  TRY(check_plan_in_x(b, "sample", pl));
  HIPCHK(hipSetDevice(b->device));
  const omgx::Dims& d = b->dims;
  const int B = b->n_agents;
  const bool dev = flags & OMGX_PTR_DEVICE;
  const size_t out_elems = (size_t)B * n_der * n_spl * n_samp, esz = as_f32 ? 4 : 8;
  KnotArg kn;
  fill_knots(kn, knots, n_knots);
  double* d_t0 = nullptr; void* d_out = out; const double* d_xx = x;
  DevBuf t0_buf, out_buf;                           // temporaries of the host-pointer path: freed on every way out
  if (!dev) {
    HIPCHK(hipMemcpyAsync(b->d_x, x, (size_t)B * d.n_var * sizeof(double), hipMemcpyHostToDevice, b->stream));
    d_xx = b->d_x;
    HIPCHK(t0_buf.alloc(B * sizeof(double)));
    d_t0 = (double*)t0_buf.p;
    HIPCHK(hipMemcpyAsync(d_t0, t0, B * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(out_buf.alloc(out_elems * esz));
    d_out = out_buf.p;
  } else {
    d_t0 = (double*)t0;
  }
  const dim3 grid((n_samp + OMGX_SAMPLE_CHUNK - 1) / OMGX_SAMPLE_CHUNK, B), block(256);
  const size_t lds = sample_scratch_doubles(n_spl, degree, n_knots, n_der) * sizeof(double);
  // (the caller's one-shot event pair of omgx_batch_set_launch_events stamps this launch as well: the duration of a
  // 20 us kernel cannot be taken with events recorded around the call)
  hipEvent_t e0 = b->ext_ev0, e1 = b->ext_ev1;
  b->ext_ev0 = b->ext_ev1 = nullptr;
  if (as_f32)
    hipExtLaunchKernelGGL(sample_kernel<float>, grid, block, lds, b->stream, e0, e1, 0, d_xx, d.n_var, coeff_off, n_spl, degree,
                          kn, n_knots, n_der, d_t0, dt, 1.0, n_samp, (float*)d_out, (float*)nullptr);
  else
    hipExtLaunchKernelGGL(sample_kernel<double>, grid, block, lds, b->stream, e0, e1, 0, d_xx, d.n_var, coeff_off, n_spl, degree,
                          kn, n_knots, n_der, d_t0, dt, 1.0, n_samp, (double*)d_out, (double*)nullptr);
  HIPCHK(hipGetLastError());
  if (!dev) {
    HIPCHK(hipMemcpyAsync(out, d_out, out_elems * esz, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  return OMGX_OK;      // device pointers: stream-ordered, the caller synchronises (omgx_batch_sync)
}

namespace {
int fill_store(const omgx_batch* b, const omgx_store_spec* sp, StoreArgs* st) {
  if (!sp->out || !sp->t0) return bad("store: null out / t0");
  const Plan pl = plan_of(*sp);
  TRY(check_plan("store", pl));
  if (sp->n_der < 1 || sp->n_der > sp->degree + 1) return bad("store: n_der = %d outside 1 .. degree + 1 = %d", sp->n_der, sp->degree + 1);
  if (sp->n_samp <= 0) return bad("store: n_samp = %d must be positive", sp->n_samp);
  if (sp->v_tot && sp->n_der < 2) return bad("store: v_tot needs n_der >= 2");
  if (!b) return bad("null handle");
  TRY(check_plan_in_x(b, "store", pl));
  put_plan(*st, pl);
  st->out = sp->out; st->v_tot = sp->v_tot; st->t0 = sp->t0; st->n_der = sp->n_der; st->n_samp = sp->n_samp; st->dt = sp->dt;
  return OMGX_OK;
}
}  // namespace

int omgx_batch_store(omgx_batch* b, const double* x, const omgx_store_spec* sp) {
  if (!x || !sp) return bad("null argument");
  StoreArgs st;
  TRY(fill_store(b, sp, &st));
  HIPCHK(hipSetDevice(b->device));
  const dim3 grid((st.n_samp + OMGX_SAMPLE_CHUNK - 1) / OMGX_SAMPLE_CHUNK, b->n_agents), block(256);
  const size_t lds = sample_scratch_doubles(st.n_spl, st.degree, st.n_knots, st.n_der) * sizeof(double);
  hipLaunchKernelGGL(sample_kernel<double>, grid, block, lds, b->stream, x, b->dims.n_var, st.coeff_off, st.n_spl,
                     st.degree, st.knots, st.n_knots, st.n_der, st.t0, st.dt, st.inv_T, st.n_samp, st.out, st.v_tot);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

namespace {
// the fused store and the fused log travel in one block of device memory (the kernels' `stp`): uploaded on the handle's stream,
// ordered behind the launches that still read the previous one (pageable source: staged before the call returns)
int upload_store_block(omgx_batch* b) {
  HIPCHK(hipSetDevice(b->device));
  b->store_host.st = b->store; b->store_host.sg = b->signals;
  return push_args(b, &b->d_store, b->store_host);
}

// the part of a log specification that can be judged without a handle
int check_signals_spec(const omgx_signals_spec* sp) {
  if (!sp->log || !sp->count) return bad("signals: null log / count");
  TRY(check_plan("signals", plan_of(*sp)));
  if (sp->n_der < 1 || sp->n_der > sp->degree + 1) return bad("signals: n_der = %d outside 1 .. degree + 1 = %d", sp->n_der, sp->degree + 1);
  if (sp->n_samp <= 0 || !(sp->sample_time > 0.0)) return bad("signals: n_samp and sample_time must be positive");
  if (sp->cap < sp->n_samp + 1) return bad("signals: cap = %d holds less than the first append (n_samp + 1 = %d columns)", sp->cap, sp->n_samp + 1);
  if (sp->p_t < 0) return bad("signals: p_t = %d is negative", sp->p_t);
  return OMGX_OK;
}

int fill_signals(const omgx_batch* b, const omgx_signals_spec* sp, SignalArgs* sg) {
  if (!sp) return bad("null argument");
  TRY(check_signals_spec(sp));
  if (!b) return bad("null handle");
  TRY(check_plan_in_x(b, "signals", plan_of(*sp)));
  if (!in_p(b, sp->p_t, 1)) return bad("signals: p_t = %d outside p", sp->p_t);
  put_plan(*sg, plan_of(*sp));
  sg->log = sp->log; sg->count = sp->count; sg->overflow = sp->overflow;
  sg->n_der = sp->n_der; sg->n_samp = sp->n_samp; sg->cap = sp->cap; sg->p_t = sp->p_t; sg->sample_time = sp->sample_time;
  return OMGX_OK;
}
}  // namespace

int omgx_batch_set_signals(omgx_batch* b, const omgx_signals_spec* sp) {
  if (!sp) {
    if (!b) return bad("null handle");
    b->signals = SignalArgs{};
    return b->store.out ? upload_store_block(b) : OMGX_OK;
  }
  SignalArgs sg;
  TRY(fill_signals(b, sp, &sg));
  if (sample_scratch_doubles(sg.n_spl, sg.degree, sg.n_knots, sg.n_der) > (size_t)b->kkt_doubles) return fail(OMGX_E_TOOLARGE, "signals: the per-agent scratch does not fit the KKT store");
  b->signals = sg;
  return upload_store_block(b);
}

int omgx_batch_signals_append(omgx_batch* b, const double* x, const double* p, const int32_t* under_way, const omgx_signals_spec* sp) {
  SignalArgs sg;
  TRY(fill_signals(b, sp, &sg));
  if (!x || !p) return bad("null argument");
  HIPCHK(hipSetDevice(b->device));
  const size_t lds = sample_scratch_doubles(sg.n_spl, sg.degree, sg.n_knots, sg.n_der) * sizeof(double);
  if (lds > 64 * 1024) { g_err = "signals: the per-agent scratch exceeds 64 KiB of LDS"; return OMGX_E_TOOLARGE; }
  hipLaunchKernelGGL(signals_append_kernel, dim3(b->n_agents), dim3(256), lds, b->stream, x, b->dims.n_var, p, b->dims.n_par, under_way, sg);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_signals_reduce(omgx_batch* b, const omgx_signals_spec* sp, const double* target, double* summary) {
  SignalArgs sg;
  TRY(fill_signals(b, sp, &sg));
  if (!target || !summary) return bad("null argument");
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(signals_reduce_kernel, dim3(b->n_agents), dim3(64), 0, b->stream, (const double*)sg.log, (const int32_t*)sg.count, target,
                     summary, sg.n_der, sg.n_spl, sg.cap, sg.sample_time);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

namespace {
// A plant specification and the log that goes with it -> the block the kernels read.  The checks that need no handle come first
// (null handle, n_knots, n_samp ... are refused without a device).
int fill_plant(const omgx_batch* b, const omgx_plant_spec* sp, const omgx_signals_spec* log_sp, PlantBlock* blk) {
  if (!sp) return bad("null argument");
  if (!sp->state || !sp->state_prev || !sp->input_last || !sp->n_upd) return bad("plant: null state / state_prev / input_last / n_upd");
  const Plan plan = plan_of(*sp);
  TRY(check_plan("plant", plan, 1, kOwnedSpl));
  if (sp->n_samp < 1) return bad("plant: n_samp = %d, at least one sample interval per update is needed", sp->n_samp);
  if (sp->max_updates < 1 || !(sp->sample_time > 0.0) || sp->stop_tol != sp->stop_tol)
    return bad("plant: max_updates and sample_time must be positive, stop_tol a number");
  if (log_sp) {
    TRY(check_signals_spec(log_sp));
    if (!same_plan(*log_sp, *sp) || log_sp->inv_T != sp->inv_T || log_sp->n_samp != sp->n_samp || log_sp->sample_time != sp->sample_time || log_sp->n_der < 2)
      return bad("plant: the log must be one of the plant's plan (coeff_off, n_spl, degree, n_knots, n_samp, sample_time, inv_T) with n_der >= 2");
  }
  if (!b) return bad("null handle");
  if (b->lag_on && sp->sample_time != b->lag_sample_time)
    return bad("plant: sample_time = %g is not the one the lag was set with (omgx_batch_set_plant_lag: %g)", sp->sample_time, b->lag_sample_time);
  TRY(check_plan_in_x(b, "plant", plan));
  if (!in_p(b, sp->p_state0, sp->n_spl) || !in_p(b, sp->p_input0, sp->n_spl) || !in_p(b, sp->p_poseT, sp->n_spl) || !in_p(b, sp->p_t, 1))
    return bad("plant: p_state0 / p_input0 / p_poseT / p_t outside p");
  PlantArgs& pl = blk->pl;
  put_plan(pl, plan);
  pl.state = sp->state; pl.state_prev = sp->state_prev; pl.input_last = sp->input_last; pl.dist = sp->dist; pl.n_upd = sp->n_upd;
  pl.overflow = sp->overflow; pl.under_way = sp->under_way; pl.n_samp = sp->n_samp; pl.max_updates = sp->max_updates;
  pl.p_t = sp->p_t; pl.p_state0 = sp->p_state0; pl.p_input0 = sp->p_input0; pl.p_poseT = sp->p_poseT;
  pl.sample_time = sp->sample_time; pl.stop_tol = sp->stop_tol;
  pl.lag_tc = b->lag_on ? b->d_lag_tc : nullptr; pl.lag_decay = b->lag_on ? b->d_lag_decay : nullptr;
  blk->sg = SignalArgs{};
  return log_sp ? fill_signals(b, log_sp, &blk->sg) : OMGX_OK;
}
// LDS doubles of a simulate: the log's sampling scratch (when there is a log) and the staged knots and plan behind it
size_t plant_lds_doubles(const PlantBlock& blk) {
  return (blk.sg.log ? sample_scratch_doubles(blk.sg.n_spl, blk.sg.degree, blk.sg.n_knots, blk.sg.n_der) : 0) +
         plant_stage_doubles(blk.pl.n_spl, blk.pl.degree, blk.pl.n_knots);
}
}  // namespace

int omgx_batch_set_plant(omgx_batch* b, const omgx_plant_spec* sp, const omgx_signals_spec* log_sp) {
  if (!sp) {
    if (!b) return bad("null handle");
    b->plant_on = false;
    return OMGX_OK;
  }
  PlantBlock blk;
  TRY(fill_plant(b, sp, log_sp, &blk));
  b->plant_on = false;      // (a failed registration leaves the plant OFF)
  if (plant_lds_doubles(blk) > (size_t)b->kkt_doubles) return fail(OMGX_E_TOOLARGE, "plant: the per-agent scratch (staged plan, log) does not fit the KKT store");
  HIPCHK(hipSetDevice(b->device));
  b->plant_host = blk;
  TRY(push_args(b, &b->d_plant, b->plant_host));
  b->plant_on = true;
  return OMGX_OK;
}

int omgx_batch_set_plant_lag(omgx_batch* b, const double* time_constant, const double* decay, int32_t n, double sample_time) {
  if (!time_constant) {      // the lag off; a registered plant block is pushed again without it
    if (!b) return bad("null handle");
    b->lag_on = false;
  } else {
    if (!decay) return bad("plant_lag: null decay");
    if (n < 1) return bad("plant_lag: n = %d must be positive", n);
    if (!(sample_time > 0.0) || !std::isfinite(sample_time)) return bad("plant_lag: sample_time = %g must be a positive number", sample_time);
    for (int i = 0; i < n; ++i)
      if (!(time_constant[i] > 0.0) || !std::isfinite(time_constant[i])) return bad("plant_lag: time_constant[%d] = %g must be positive and finite", i, time_constant[i]);
    for (int i = 0; i < n; ++i)
      if (!(decay[i] >= 0.0 && decay[i] < 1.0)) return bad("plant_lag: decay[%d] = %g outside [0, 1)", i, decay[i]);
    for (int i = 0; i < n; ++i)
      if (!(fabs(decay[i] - exp(-sample_time / time_constant[i])) <= 1e-12))
        return bad("plant_lag: decay[%d] = %.17g is not exp(-sample_time / time_constant[%d]) = %.17g", i, decay[i], i, exp(-sample_time / time_constant[i]));
    if (!b) return bad("null handle");
    if (n != b->n_agents) return bad("plant_lag: n = %d, the handle has %d agents", n, b->n_agents);
    HIPCHK(hipSetDevice(b->device));
    if (!b->d_lag_tc) TRY(dalloc(b, (size_t)n, &b->d_lag_tc));
    if (!b->d_lag_decay) TRY(dalloc(b, (size_t)n, &b->d_lag_decay));
    // (stream-ordered: a launch still running reads the previous values; pageable sources are staged before the calls return)
    HIPCHK(hipMemcpyAsync(b->d_lag_tc, time_constant, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->d_lag_decay, decay, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, b->stream));
    b->lag_sample_time = sample_time;
    b->lag_on = true;
  }
  if (b->plant_on && b->d_plant) {      // (the order of the two registrations does not matter)
    b->plant_host.pl.lag_tc = b->lag_on ? b->d_lag_tc : nullptr;
    b->plant_host.pl.lag_decay = b->lag_on ? b->d_lag_decay : nullptr;
    HIPCHK(hipSetDevice(b->device));
    TRY(push_args(b, &b->d_plant, b->plant_host));
  }
  return OMGX_OK;
}

int omgx_batch_plant_simulate(omgx_batch* b, const double* x, const double* p, const omgx_plant_spec* sp, const omgx_signals_spec* log_sp) {
  PlantBlock blk;
  TRY(fill_plant(b, sp, log_sp, &blk));
  if (!x || !p) return bad("null argument");
  const size_t lds = plant_lds_doubles(blk) * sizeof(double);
  if (lds > 64 * 1024) { g_err = "plant: the per-agent scratch (staged plan, log) exceeds 64 KiB of LDS"; return OMGX_E_TOOLARGE; }
  HIPCHK(hipSetDevice(b->device));
  TRY(push_args(b, &b->d_plant_call, blk));
  hipLaunchKernelGGL(plant_simulate_kernel, dim3(b->n_agents), dim3(256), lds, b->stream, x, b->dims.n_var, p, b->dims.n_par,
                     (const PlantBlock*)b->d_plant_call);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_plant_predict(omgx_batch* b, const double* x, double* p, double tau, double t_value, const omgx_plant_spec* sp) {
  PlantBlock blk;
  TRY(fill_plant(b, sp, nullptr, &blk));
  if (!x || !p || tau != tau) return bad("null argument");
  HIPCHK(hipSetDevice(b->device));
  TRY(push_args(b, &b->d_plant_call, blk));
  const int32_t* oi = b->pend_iters; int32_t* oo = b->pend_order;
  b->pend_iters = nullptr; b->pend_order = nullptr;
  hipLaunchKernelGGL(plant_predict_kernel, dim3(b->n_agents + (oi ? 1 : 0)), dim3(64), plant_stage_doubles(blk.pl.n_spl, blk.pl.degree, blk.pl.n_knots) * sizeof(double), b->stream, x, b->dims.n_var, p, b->dims.n_par, b->n_agents,
                     (const PlantBlock*)b->d_plant_call, tau, t_value, oi, oo, (const double*)(b->order_dw ? b->d_dw : nullptr));
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_set_store(omgx_batch* b, const omgx_store_spec* sp) {
  if (!sp) {
    if (!b) return bad("null handle");
    b->store = StoreArgs{};
    return b->signals.log ? upload_store_block(b) : OMGX_OK;
  }
  StoreArgs st;
  TRY(fill_store(b, sp, &st));
  if (sample_scratch_doubles(st.n_spl, st.degree, st.n_knots, st.n_der) > (size_t)b->kkt_doubles) return fail(OMGX_E_TOOLARGE, "store: the per-agent scratch does not fit the KKT store");
  b->store = st;
  return upload_store_block(b);
}

namespace {
// What the predict entries and the rollout share.  Without a handle: the plan and the outputs asked for ...
int check_predict(const char* who, const Plan& pl, int min_degree, int max_spl, const void* x, const void* p, const int32_t* p_off, int n_out) {
  if (!x || !p || !p_off) return bad("%s: null x / p / p_off", who);
  TRY(check_plan(who, pl, min_degree, max_spl));
  if (n_out < 1 || n_out > 4 || n_out > pl.degree + 1) return bad("%s: n_out = %d outside 1 .. min(4, degree + 1)", who, n_out);
  return OMGX_OK;
}
// ... with one: the plan inside x, the offsets inside p (n_spl parameters per output; a negative offset or p_t: skipped), into a.p_off
int check_predict_in_xp(const omgx_batch* b, const char* who, const Plan& pl, int n_out, const int32_t* p_off, int p_t, int* a_p_off) {
  TRY(check_plan_in_x(b, who, pl));
  if (p_t >= 0 && !in_p(b, p_t, 1)) return bad("%s: p_t = %d outside p", who, p_t);
  for (int o = 0; o < 4; ++o) {
    a_p_off[o] = o < n_out ? p_off[o] : -1;
    if (a_p_off[o] >= 0 && !in_p(b, a_p_off[o], pl.n_spl)) return bad("%s: p_off[%d] = %d outside p", who, o, a_p_off[o]);
  }
  return OMGX_OK;
}
int fill_predict(const omgx_batch* b, const char* who, PredictArgs& a, const Plan& pl, double tau, int n_out, const int32_t* p_off, int p_t,
                 double t_value, int mode, const double* state_in, int n_sub, double dtau) {
  if (!b) return bad("null handle");
  TRY(check_predict_in_xp(b, who, pl, n_out, p_off, p_t, a.p_off));
  put_plan(a, pl);
  a.n_out = n_out; a.tau = tau; a.p_t = p_t; a.t_value = t_value; a.mode = mode; a.state_in = state_in; a.n_sub = n_sub; a.dtau = dtau;
  return OMGX_OK;
}
}  // namespace

int omgx_batch_predict_quadrotor(omgx_batch* b, const double* x, double* p, int32_t coeff_off, int32_t degree, const double* knots,
                                 int32_t n_knots, double tau, double inv_T, int32_t n_out, const int32_t* p_off, int32_t p_t,
                                 double t_value, const double* state_in, double* state_out, int32_t n_sub, double dtau, double g) {
  const Plan pl{coeff_off, 2, degree, n_knots, inv_T, knots};
  TRY(check_predict("predict_quadrotor", pl, 3, kAnySpl, x, p, p_off, n_out));
  if (!state_in || n_sub < 1 || !(dtau > 0.0) || !(g > 0.0)) return bad("predict_quadrotor: state_in is null, or n_sub, dtau or g not positive");
  PredictArgs a;
  TRY(fill_predict(b, "predict_quadrotor", a, pl, tau, n_out, p_off, p_t, t_value, OMGX_PREDICT_RK4, state_in, n_sub, dtau));
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(predict_quadrotor_kernel, dim3((b->n_agents + 255) / 256), dim3(256), 0, b->stream, x, b->dims.n_var, p, b->dims.n_par, b->n_agents, a, g, state_out);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_rollout(omgx_batch* b, const omgx_rollout_spec* sp, double* p, double* x, const double* lbg, const double* ubg,
                       double* lam_g, int32_t* status, int32_t* iters, int32_t flags) {
  if (!sp || !lbg || !ubg || !lam_g || !status || !iters) return bad("null argument");
  const Plan pl = plan_of(*sp);
  TRY(check_predict("rollout", pl, 1, kOwnedSpl, x, p, sp->p_off, sp->n_out));
  if (!(flags & OMGX_PTR_DEVICE) || !(flags & OMGX_BOUNDS_DEVICE)) return bad("rollout: device pointers only (OMGX_PTR_DEVICE | OMGX_BOUNDS_DEVICE)");
  if (sp->n_steps <= 0 || !sp->tau || !sp->t_rel || !sp->crossed || sp->n_obst < 0 || sp->n_obst > 8 || (sp->n_obst > 0 && !sp->obst) || sp->n_ent < 0 ||
      (sp->n_ent > 0 && (!sp->shift_entries || !sp->shift_T || !sp->lam_perm)))
    return bad("rollout: bad specification (n_steps, tau / t_rel / crossed, at most 8 obstacles, shift tables with their multiplier map)");
  if (!b) return bad("null handle");
  const omgx::Dims& d = b->dims;
  if (!b->inst.rollout[0][RO_PLAIN] || b->n_range > 0 || !b->d_next)
    return bad("rollout: not available for this template class (spill modes, general instance, two-sided rows): step with omgx_batch_solve");
  if (b->plant_on && (!b->inst.rollout[1][RO_PLAIN] || !b->d_plant))
    return bad("rollout: a plant is set (omgx_batch_set_plant) but this template class has no plant instance of the rollout kernel: step with "
               "omgx_batch_plant_predict / omgx_batch_solve / omgx_batch_plant_simulate");
  if (b->plant_on && (!same_plan(*sp, b->plant_host.pl) || sp->p_t != b->plant_host.pl.p_t))
    return bad("rollout: the plan of the specification (coeff_off, n_spl, degree, n_knots, p_t) is not the one the plant was set with");
  if (b->plant_on && b->lag_on && b->plant_host.pl.sample_time != b->lag_sample_time)
    return bad("rollout: the plant's sample_time = %g is not the one the lag was set with (omgx_batch_set_plant_lag: %g)", b->plant_host.pl.sample_time, b->lag_sample_time);
  if (b->script_on) {
    const ObstacleScriptArgs& sc = b->script_host;
    if (!b->inst.rollout[b->plant_on ? 1 : 0][RO_SCRIPT] || !b->d_script)
      return bad("rollout: an obstacle script is set (omgx_batch_set_obstacle_script) but this template class has no script instance of the "
                 "rollout kernel: step with omgx_batch_obstacles_advance / omgx_batch_solve");
    if (sc.n_t < sp->n_steps + 1)
      return bad("rollout: t_abs of the obstacle script holds %d times, n_steps + 1 = %d are needed", sc.n_t, sp->n_steps + 1);
    bool same = sp->n_obst == sc.n_obst;
    for (int q = 0; same && q < sc.n_obst; ++q)
      for (int k = 0; k < 4; ++k) same = same && sp->obst[4 * q + k] == sc.obst[q][k];
    if (!same) return bad("rollout: the obstacle table of the specification is not the one the obstacle script was set with");
  }
  // with a mission the specification's step list is the TABLE of a leg's clock and the mission says how many steps an agent takes
  const int n_run = b->mission_on ? b->mission_host.K : sp->n_steps;
  if (b->mission_on) {
    const MissionArgs& ms = b->mission_host;
    if (b->script_on) return bad("rollout: a mission and an obstacle script are both set: the rollout kernel has no instance for the two");
    if (!b->inst.rollout[b->plant_on ? 1 : 0][RO_MISSION] || !b->d_mission)
      return bad("rollout: a mission is set (omgx_batch_set_mission) but this template class has no mission instance of the rollout kernel");
    if (!b->stop_on) return bad("rollout: a mission is set but the stop rule is off (omgx_batch_set_stop): arriving is that rule");
    if (ms.K > sp->n_steps) return bad("rollout: the mission runs %d steps per agent but the step table holds %d", ms.K, sp->n_steps);
    if (ms.coeff_off != sp->coeff_off || ms.n_spl != sp->n_spl || ms.L != sp->n_knots - sp->degree - 1 || ms.p_t != sp->p_t)
      return bad("rollout: the plan of the specification (coeff_off, n_spl, n_knots - degree - 1, p_t) is not the one the mission was set with");
    if (ms.o_state0 != b->stop_host.o_state || ms.o_input0 != b->stop_host.o_input || ms.o_poseT != b->stop_host.o_pose || ms.n_spl != b->stop_host.n_dim)
      return bad("rollout: o_state0 / o_input0 / o_poseT / n_spl of the mission are not those of the stop rule");
  }
  RolloutArgs a;
  memset(&a, 0, sizeof a);
  TRY(check_predict_in_xp(b, "rollout", pl, sp->n_out, sp->p_off, sp->p_t, a.p_off));
  HIPCHK(hipSetDevice(b->device));
  put_plan(a, pl);
  a.n_out = sp->n_out; a.p_t = sp->p_t; a.dt = sp->dt; a.n_obst = sp->n_obst;
  for (int q = 0; q < sp->n_obst; ++q) {
    for (int k = 0; k < 4; ++k) a.obst[q][k] = sp->obst[4 * q + k];
    const int nd = a.obst[q][3];
    if (nd <= 0 || nd > 64 || !in_p(b, a.obst[q][0], nd) || !in_p(b, a.obst[q][1], nd) || !in_p(b, a.obst[q][2], nd)) return bad("rollout: obstacle entries outside p");
  }
  // knot-crossing tables: the shift set (cached on the device by content) and the multiplier map
  a.n_ent = sp->n_ent;
  bool any_cross = false;
  for (int k = 0; k < sp->n_steps; ++k) any_cross = any_cross || sp->crossed[k] != 0;
  if (any_cross && sp->n_ent <= 0) { g_err = "rollout: a step crosses a knot but no shift tables were given"; return OMGX_E_INVALID; }
  if (sp->n_ent > 0) {
    int max_elems = 0;
    TRY(stage_shift_tables(b, sp->shift_entries, sp->n_ent, sp->shift_T, sp->n_tmat, d.n_var, &max_elems));
    if (max_elems > b->kkt_doubles || d.n_con > b->kkt_doubles) { g_err = "rollout: shift scratch exceeds the KKT store"; return OMGX_E_INVALID; }
    a.sh_ent = b->d_shift_ent; a.sh_T = b->d_shift_T;
    for (int i = 0; i < d.n_con; ++i) if (sp->lam_perm[i] >= d.n_con) { g_err = "rollout: multiplier map out of range"; return OMGX_E_INVALID; }
    if (b->ro_perm_host.size() != (size_t)d.n_con || memcmp(b->ro_perm_host.data(), sp->lam_perm, d.n_con * sizeof(int32_t)) != 0) {
      if (!b->d_ro_perm) TRY(dalloc(b, (size_t)d.n_con, &b->d_ro_perm));
      b->ro_perm_host.assign(sp->lam_perm, sp->lam_perm + d.n_con);
      // (stream-ordered like the two copies below: a rollout still running on a non-blocking caller stream reads the old map)
      HIPCHK(hipMemcpyAsync(b->d_ro_perm, b->ro_perm_host.data(), sizeof(int32_t) * (size_t)d.n_con, hipMemcpyHostToDevice, b->stream));
    }
    a.lam_perm = b->d_ro_perm;
  }
  if (sp->n_steps > b->ro_steps_cap) {
    b->ro_steps_cap = 0;
    HIPCHK(b->ro_steps.alloc(sizeof(RolloutStep) * (size_t)sp->n_steps));      // (frees the shorter table first)
    b->ro_steps_cap = sp->n_steps;
  }
  std::vector<RolloutStep> steps((size_t)sp->n_steps);
  for (int k = 0; k < sp->n_steps; ++k) { steps[k].tau = sp->tau[k]; steps[k].t_rel = sp->t_rel[k]; steps[k].crossed = sp->crossed[k] ? 1 : 0; steps[k].pad = 0; }
  a.steps = (const RolloutStep*)b->ro_steps.p; a.K = n_run; a.n_table = sp->n_steps;
  b->opts.prio_iter = b->prio_iter;
  a.o_cross = b->opts;
  if (sp->cross_options) {
    const omgx_options& co = *sp->cross_options;
    a.o_cross.kappa_warm = co.kappa_warm; a.o_cross.warm_mu_factor = co.warm_mu_factor; a.o_cross.warm_z_floor = co.warm_z_floor;
    a.o_cross.warm_z_cap = co.warm_z_cap; a.o_cross.max_iter = co.max_iter; a.o_cross.tol = co.tol; a.o_cross.max_soc = co.max_soc; a.o_cross.refine = co.refine > 0 ? 1 : 0;
  }
  // per-step statistics: the slots the next n_steps single launches would have taken (omgx_batch_set_stats)
  a.stop_on = b->stop_on ? 1 : 0; a.stop = b->stop_host;
  a.stats = nullptr;
  if (b->d_stats) {
    if (n_run > b->stats_slots - (int)(b->stats_launch % b->stats_slots)) { g_err = "rollout: the stats array has fewer free slots than steps"; return OMGX_E_INVALID; }
    a.stats = (unsigned long long*)b->d_stats + 4 * (size_t)(b->stats_launch % b->stats_slots);
    b->stats_launch += n_run;
  }
  a.iters_log = sp->iters_log; a.status_log = sp->status_log;
  a.plant = b->plant_on ? b->d_plant : nullptr;
  a.script = b->script_on ? b->d_script : nullptr;
  a.mission = b->mission_on ? b->d_mission : nullptr;
  const ipm_rollout_t kern = b->inst.rollout[b->plant_on ? 1 : 0][b->mission_on ? RO_MISSION : b->script_on ? RO_SCRIPT : RO_PLAIN];
  // Two small copies per call (one call is n_steps steps of the whole batch), ORDERED ON THE HANDLE'S STREAM: the persistent
  // kernel of a previous rollout reads these tables for its whole run, and on a non-blocking caller stream a null-stream
  // hipMemcpy would overwrite them under it (pageable sources: staged before the calls return, executed in stream order).
  HIPCHK(hipMemcpyAsync(b->ro_steps.p, steps.data(), sizeof(RolloutStep) * steps.size(), hipMemcpyHostToDevice, b->stream));
  TRY(push_args(b, &b->d_rollout, a));
  TRY(flush_order(b));
  const bool shared = flags & OMGX_BOUNDS_SHARED;
  hipEvent_t e0 = b->ext_ev0, e1 = b->ext_ev0 ? b->ext_ev1 : nullptr;
  b->ext_ev0 = b->ext_ev1 = nullptr;
  b->timed = false;
  hipExtLaunchKernelGGL(kern, dim3(b->n_slabs < b->n_agents ? b->n_slabs : b->n_agents), dim3(b->threads), (uint32_t)b->lds_bytes, b->stream, e0, e1, 0u,
                        d, b->dev, b->opts, b->kkt_doubles, p, x, lbg, ubg, shared ? 1 : 0, lam_g, status, iters, b->n_agents,
                        b->d_slabs, b->slab_doubles, b->d_dw, b->n_slabs >= b->n_agents ? nullptr : b->d_next, (const RolloutArgs*)b->d_rollout, b->stagger, b->d_order,
                        (const StoreArgs*)((b->store.out || b->signals.log) ? &b->d_store->st : nullptr));
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_predict_ex(omgx_batch* b, const double* x, double* p, int32_t coeff_off, int32_t n_spl, int32_t degree,
                          const double* knots, int32_t n_knots, double tau, double inv_T, int32_t n_out,
                          const int32_t* p_off, int32_t p_t, double t_value, int32_t mode, const double* state_in,
                          int32_t n_sub, double dtau) {
  const Plan pl{coeff_off, n_spl, degree, n_knots, inv_T, knots};
  TRY(check_predict("predict", pl, 1, kAnySpl, x, p, p_off, n_out));
  if (mode != OMGX_PREDICT_IDEAL && mode != OMGX_PREDICT_RK4) return bad("predict: mode = %d is neither OMGX_PREDICT_IDEAL nor OMGX_PREDICT_RK4", mode);
  if (mode == OMGX_PREDICT_RK4 && (!state_in || n_sub < 1 || !(dtau > 0.0) || n_out < 2))
    return bad("predict: OMGX_PREDICT_RK4 needs state_in, n_sub >= 1, dtau > 0 and n_out >= 2");
  PredictArgs a;
  TRY(fill_predict(b, "predict", a, pl, tau, n_out, p_off, p_t, t_value, mode, state_in, n_sub, dtau));
  const omgx::Dims& d = b->dims;
  HIPCHK(hipSetDevice(b->device));
  const int n = b->n_agents * n_spl;
  const int32_t* oi = b->pend_iters; int32_t* oo = b->pend_order;
  b->pend_iters = nullptr; b->pend_order = nullptr;
  hipLaunchKernelGGL(predict_kernel, dim3((n + 255) / 256 + (oi ? 1 : 0)), dim3(256), 0, b->stream, x, d.n_var, p, d.n_par, b->n_agents, a, oi, oo, (const double*)(b->order_dw ? b->d_dw : nullptr));
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_predict(omgx_batch* b, const double* x, double* p, int32_t coeff_off, int32_t n_spl, int32_t degree,
                       const double* knots, int32_t n_knots, double tau, double inv_T, int32_t p_state0,
                       int32_t p_input0, int32_t p_t, double t_value) {
  const int32_t off[2] = {p_state0, p_input0};
  return omgx_batch_predict_ex(b, x, p, coeff_off, n_spl, degree, knots, n_knots, tau, inv_T, 2, off, p_t, t_value,
                               OMGX_PREDICT_IDEAL, nullptr, 0, 0.0);
}

int omgx_batch_predict_measured(omgx_batch* b, const double* x, double* p, double tau, double t_value, const omgx_feedback_spec* sp) {
  if (!sp || !x || !p) return bad("predict_measured: null x / p / specification");
  if (!sp->state) return bad("predict_measured: null state");
  const Plan plan = plan_of(*sp);
  TRY(check_plan("predict_measured", plan, 1, kOwnedSpl));
  if (sp->n_samp < 1) return bad("predict_measured: n_samp = %d, at least one sample interval per update is needed", sp->n_samp);
  if (!(sp->sample_time > 0.0)) return bad("predict_measured: sample_time = %g must be positive", sp->sample_time);
  if (sp->n_out < 1 || sp->n_out > 4 || sp->n_out > sp->degree + 1) return bad("predict_measured: n_out = %d outside 1 .. min(4, degree + 1)", sp->n_out);
  if (sp->p_off[0] < 0) return bad("predict_measured: p_off[0] = %d, the state has no place in p", sp->p_off[0]);
  const size_t lds = feedback_lds_doubles(sp->n_spl, sp->degree, sp->n_knots, sp->n_samp) * sizeof(double);
  if (lds > 64 * 1024) return bad("predict_measured: n_samp = %d, the staged plan and n_spl * (n_samp + 1) input samples exceed 64 KiB of LDS", sp->n_samp);
  if (tau != tau || t_value != t_value) return bad("predict_measured: tau / t_value is not a number");
  if (!b) return bad("null handle");
  FeedbackArgs a;
  TRY(check_predict_in_xp(b, "predict_measured", plan, sp->n_out, sp->p_off, sp->p_t, a.p_off));
  if (sp->p_t < 0) return bad("predict_measured: p_t = %d outside p (the old t is read, the new one written)", sp->p_t);
  put_plan(a, plan);
  a.state = sp->state; a.input = sp->enforce ? sp->input : nullptr; a.fresh = sp->fresh;
  a.n_samp = sp->n_samp; a.n_out = sp->n_out; a.p_t = sp->p_t; a.enforce = sp->enforce ? 1 : 0; a.sample_time = sp->sample_time;
  HIPCHK(hipSetDevice(b->device));
  const int32_t* oi = b->pend_iters; int32_t* oo = b->pend_order;
  b->pend_iters = nullptr; b->pend_order = nullptr;
  hipLaunchKernelGGL(feedback_predict_kernel, dim3(b->n_agents + (oi ? 1 : 0)), dim3(64), lds, b->stream, x, b->dims.n_var, p, b->dims.n_par, b->n_agents,
                     a, tau, t_value, oi, oo, (const double*)(b->order_dw ? b->d_dw : nullptr));
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

namespace {
// A Quadrotor plant specification (and the log that goes with a simulate) -> the arguments the two kernels take by value.  `who`
// names the entry; with_plant: the plant's own arrays are read (not with measured states).  The checks that need no handle come first.
int fill_quad_plant(const omgx_batch* b, const char* who, const omgx_quad_plant_spec* sp, const omgx_signals_spec* log_sp, bool with_plant,
                    QuadPlantArgs* pl, SignalArgs* sg) {
  if (with_plant && (!sp->state || !sp->state_prev || !sp->input_last || !sp->dspl_last || !sp->n_upd))
    return bad("%s: null state / state_prev / input_last / dspl_last / n_upd", who);
  const Plan plan = plan_of(*sp);
  TRY(check_plan(who, plan, 3, kOwnedSpl));
  if (sp->n_spl != 2) return bad("%s: n_spl = %d, the Quadrotor's plan is the two splines x, y", who, sp->n_spl);
  if (sp->n_samp < 1 || sp->n_samp + 1 > 64) return bad("%s: n_samp = %d outside 1 .. 63 (a lane per sample, n_samp + 1 <= 64)", who, sp->n_samp);
  if (with_plant && sp->max_updates < 1) return bad("%s: max_updates = %d must be positive", who, sp->max_updates);
  if (!(sp->sample_time > 0.0)) return bad("%s: sample_time = %g must be positive", who, sp->sample_time);
  if (!(sp->g > 0.0)) return bad("%s: g = %g must be positive", who, sp->g);
  if (sp->stop_tol != sp->stop_tol) return bad("%s: stop_tol is not a number", who);
  if ((sp->log_state == nullptr) != (sp->log_input == nullptr) || (sp->log_state && !log_sp))
    return bad("%s: log_state / log_input go together, and with the log specification (count, cap)", who);
  size_t lds = quad_plant_lds_doubles(sp->degree, sp->n_knots, sp->n_samp);
  if (log_sp) {
    TRY(check_signals_spec(log_sp));
    if (!same_plan(*log_sp, *sp) || log_sp->inv_T != sp->inv_T || log_sp->n_samp != sp->n_samp || log_sp->sample_time != sp->sample_time)
      return bad("%s: the log must be one of the plant's plan (coeff_off, n_spl, degree, n_knots, n_samp, sample_time, inv_T)", who);
    lds += sample_scratch_doubles(log_sp->n_spl, log_sp->degree, log_sp->n_knots, log_sp->n_der);
  }
  if (lds * sizeof(double) > 64 * 1024) return bad("%s: the staged plan, samples and log scratch exceed 64 KiB of LDS", who);
  if (!b) return bad("null handle");
  TRY(check_plan_in_x(b, who, plan));
  for (int o = 0; o < 3; ++o)
    if (!in_p(b, sp->p_off[o], 2)) return bad("%s: p_off[%d] = %d outside p", who, o, sp->p_off[o]);
  if (with_plant && !in_p(b, sp->p_poseT, 2)) return bad("%s: p_poseT = %d outside p", who, sp->p_poseT);
  if (!in_p(b, sp->p_t, 1)) return bad("%s: p_t = %d outside p", who, sp->p_t);
  *pl = QuadPlantArgs{};
  put_plan(*pl, plan);
  pl->state = sp->state; pl->state_prev = sp->state_prev; pl->input_last = sp->input_last; pl->dspl_last = sp->dspl_last; pl->dist = sp->dist;
  pl->n_upd = sp->n_upd; pl->overflow = sp->overflow; pl->under_way = sp->under_way; pl->log_state = sp->log_state; pl->log_input = sp->log_input;
  pl->n_samp = sp->n_samp; pl->max_updates = sp->max_updates; pl->p_t = sp->p_t; pl->p_poseT = sp->p_poseT;
  for (int o = 0; o < 3; ++o) pl->p_off[o] = sp->p_off[o];
  pl->sample_time = sp->sample_time; pl->stop_tol = sp->stop_tol; pl->g = sp->g;
  *sg = SignalArgs{};
  return log_sp ? fill_signals(b, log_sp, sg) : OMGX_OK;
}
}  // namespace

int omgx_batch_plant_quadrotor_simulate(omgx_batch* b, const double* x, const double* p, const omgx_quad_plant_spec* sp,
                                        const omgx_signals_spec* log_sp) {
  if (!x || !p || !sp) return bad("plant_quadrotor_simulate: null x / p / specification");
  QuadPlantArgs pl; SignalArgs sg;
  TRY(fill_quad_plant(b, "plant_quadrotor_simulate", sp, log_sp, true, &pl, &sg));
  const size_t lds = (quad_plant_lds_doubles(pl.degree, pl.n_knots, pl.n_samp) +
                      (sg.log ? sample_scratch_doubles(sg.n_spl, sg.degree, sg.n_knots, sg.n_der) : 0)) * sizeof(double);
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(plant_quadrotor_simulate_kernel, dim3(b->n_agents), dim3(64), lds, b->stream, x, b->dims.n_var, p, b->dims.n_par, pl, sg);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_plant_quadrotor_predict(omgx_batch* b, const double* x, double* p, double tau, double t_value, const omgx_quad_plant_spec* sp,
                                       const double* states, const int32_t* fresh, int32_t enforce) {
  if (!x || !p || !sp) return bad("plant_quadrotor_predict: null x / p / specification");
  if (!states && (fresh || enforce)) return bad("plant_quadrotor_predict: fresh / enforce go with states");
  if (tau != tau || t_value != t_value) return bad("plant_quadrotor_predict: tau / t_value is not a number");
  omgx_quad_plant_spec spec = *sp;
  spec.log_state = spec.log_input = nullptr;      // (the simulate's: not read here)
  QuadPlantArgs pl; SignalArgs sg;
  TRY(fill_quad_plant(b, "plant_quadrotor_predict", &spec, nullptr, states == nullptr, &pl, &sg));
  HIPCHK(hipSetDevice(b->device));
  const int32_t* oi = b->pend_iters; int32_t* oo = b->pend_order;
  b->pend_iters = nullptr; b->pend_order = nullptr;
  hipLaunchKernelGGL(plant_quadrotor_predict_kernel, dim3(b->n_agents + (oi ? 1 : 0)), dim3(64),
                     quad_plant_lds_doubles(pl.degree, pl.n_knots, pl.n_samp) * sizeof(double), b->stream, x, b->dims.n_var, p, b->dims.n_par,
                     b->n_agents, pl, tau, t_value, states, fresh, enforce ? 1 : 0, oi, oo, (const double*)(b->order_dw ? b->d_dw : nullptr));
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

namespace {
// An obstacle script -> the block the kernels read.  The checks that need no handle come first; `who` names the entry.
int fill_script(const omgx_batch* b, const char* who, const omgx_obstacle_script* sp, ObstacleScriptArgs* a) {
  if (!sp->time || !sp->what || !sp->value || !sp->obst) return bad("%s: null time / what / value / obst", who);
  if (sp->n_ev < 1 || sp->n_ev > 32) return bad("%s: n_ev = %d outside 1 .. 32", who, sp->n_ev);
  if (sp->n_obst < 1 || sp->n_obst > 8) return bad("%s: n_obst = %d outside 1 .. 8", who, sp->n_obst);
  for (int q = 0; q < sp->n_obst; ++q)
    if (sp->obst[4 * q + 3] < 1 || sp->obst[4 * q + 3] > 3) return bad("%s: n_dim = %d of obstacle %d outside 1 .. 3", who, sp->obst[4 * q + 3], q);
  if (!b) return bad("null handle");
  if (sp->what_host)
    for (size_t i = 0; i < (size_t)b->n_agents * sp->n_ev; ++i)
      if (sp->what_host[i] < 0 || sp->what_host[i] >= 3 * sp->n_obst)
        return bad("%s: what = %d of agent %d, event %d outside 0 .. %d", who, sp->what_host[i], (int)(i / sp->n_ev), (int)(i % sp->n_ev), 3 * sp->n_obst - 1);
  *a = ObstacleScriptArgs{};
  for (int q = 0; q < sp->n_obst; ++q) {
    for (int k = 0; k < 4; ++k) a->obst[q][k] = sp->obst[4 * q + k];
    for (int k = 0; k < 3; ++k)
      if (!in_p(b, a->obst[q][k], a->obst[q][3])) return bad("%s: obst[%d][%d] = %d outside p", who, q, k, a->obst[q][k]);
  }
  a->time = sp->time; a->what = sp->what; a->value = sp->value; a->n_ev = sp->n_ev; a->n_obst = sp->n_obst;
  return OMGX_OK;
}
}  // namespace

int omgx_batch_obstacles_advance(omgx_batch* b, double* p, const omgx_obstacle_script* sp, double t_prev, double dt) {
  if (!sp || !p) return bad("obstacles_advance: null p / specification");
  if (!sp->time || !sp->what || !sp->value || !sp->obst) return bad("obstacles_advance: null time / what / value / obst");
  if (t_prev != t_prev || !(dt > 0.0) || dt - dt != 0.0) return bad("obstacles_advance: t_prev = %g is not a number or dt = %g not a positive number", t_prev, dt);
  ObstacleScriptArgs a;
  TRY(fill_script(b, "obstacles_advance", sp, &a));
  HIPCHK(hipSetDevice(b->device));
  TRY(push_args(b, &b->d_script_call, a));
  hipLaunchKernelGGL(obstacles_advance_kernel, dim3((b->n_agents + 7) / 8), dim3(256), 0, b->stream, p, b->dims.n_par, b->n_agents,
                     (const ObstacleScriptArgs*)b->d_script_call, t_prev, t_prev + dt, dt);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_set_obstacle_script(omgx_batch* b, const omgx_obstacle_script* sp, const double* t_abs, int32_t n_t) {
  if (!sp) {
    if (!b) return bad("null handle");
    b->script_on = false;
    return OMGX_OK;
  }
  if (!sp->time || !sp->what || !sp->value || !sp->obst) return bad("set_obstacle_script: null time / what / value / obst");
  if (!t_abs) return bad("set_obstacle_script: null t_abs");
  if (n_t < 2) return bad("set_obstacle_script: n_t = %d, the step boundaries of at least one step are needed", n_t);
  for (int k = 0; k < n_t; ++k)
    if (t_abs[k] - t_abs[k] != 0.0 || (k > 0 && !(t_abs[k] > t_abs[k - 1]))) return bad("set_obstacle_script: t_abs[%d] = %g is not a number above t_abs[%d]", k, t_abs[k], k - 1);
  ObstacleScriptArgs a;
  TRY(fill_script(b, "set_obstacle_script", sp, &a));
  b->script_on = false;      // (a failed registration leaves the script OFF)
  HIPCHK(hipSetDevice(b->device));
  if (n_t > b->script_t_cap) {
    b->script_t_cap = 0;
    HIPCHK(b->script_t.alloc(sizeof(double) * (size_t)n_t));      // (frees the shorter table first)
    b->script_t_cap = n_t;
  }
  // (stream-ordered, like the step table of omgx_batch_rollout: a rollout still running reads the previous times)
  HIPCHK(hipMemcpyAsync(b->script_t.p, t_abs, sizeof(double) * (size_t)n_t, hipMemcpyHostToDevice, b->stream));
  a.t_abs = (const double*)b->script_t.p; a.n_t = n_t;
  b->script_host = a;
  TRY(push_args(b, &b->d_script, b->script_host));
  b->script_on = true;
  return OMGX_OK;
}

int omgx_batch_set_mission(omgx_batch* b, const omgx_mission_spec* sp) {
  if (!sp) {
    if (!b) return bad("null handle");
    b->mission_on = false;
    return OMGX_OK;
  }
  if (!sp->goals || !sp->n_goals || !sp->leg || !sp->clock || !sp->arrivals || !sp->x_reset || !sp->cold)
    return bad("set_mission: null goals / n_goals / leg / clock / arrivals / x_reset / cold");
  if (sp->G < 1) return bad("set_mission: G = %d must be positive", sp->G);
  if (sp->n_spl < 1 || sp->n_spl > kOwnedSpl || sp->L < 2) return bad("set_mission: n_spl = %d outside 1 .. %d or L = %d below 2", sp->n_spl, kOwnedSpl, sp->L);
  if (sp->n_steps < 1 || sp->step_index < 0) return bad("set_mission: n_steps = %d must be positive and step_index = %d not negative", sp->n_steps, sp->step_index);
  if (!(sp->cold->tol > 0) || sp->cold->max_iter < 0) return bad("set_mission: bad cold options");
  if (!b) return bad("null handle");
  const omgx::Dims& d = b->dims;
  if (sp->coeff_off < 0 || sp->coeff_off + (long long)sp->n_spl * sp->L > d.n_var)
    return bad("set_mission: coefficients outside x (coeff_off = %d, %d splines of %d, n_var = %d)", sp->coeff_off, sp->n_spl, sp->L, d.n_var);
  if (!in_p(b, sp->o_state0, sp->n_spl) || !in_p(b, sp->o_input0, sp->n_spl) || !in_p(b, sp->o_poseT, sp->n_spl) || !in_p(b, sp->p_t, 1))
    return bad("set_mission: o_state0 / o_input0 / o_poseT / p_t outside p");
  b->mission_on = false;      // (a failed registration leaves the mission OFF)
  HIPCHK(hipSetDevice(b->device));
  if (!b->d_x_reset) TRY(dalloc(b, (size_t)d.n_var, &b->d_x_reset));
  // (stream-ordered: a rollout still running reads the previous row)
  HIPCHK(hipMemcpyAsync(b->d_x_reset, sp->x_reset, sizeof(double) * (size_t)d.n_var, hipMemcpyHostToDevice, b->stream));
  MissionArgs a = {};
  a.goals = sp->goals; a.n_goals = sp->n_goals; a.leg = sp->leg; a.clock = sp->clock; a.arrivals = sp->arrivals; a.x_reset = b->d_x_reset;
  a.G = sp->G; a.o_state0 = sp->o_state0; a.o_input0 = sp->o_input0; a.o_poseT = sp->o_poseT; a.p_t = sp->p_t;
  a.coeff_off = sp->coeff_off; a.n_spl = sp->n_spl; a.L = sp->L; a.n_var = d.n_var; a.n_con = d.n_con;
  a.K = sp->n_steps; a.step0 = sp->step_index;
  a.o_cold = opts_of(sp->cold);
  a.o_cold.warm_start = 0; a.o_cold.prio_iter = b->prio_iter;
  b->mission_host = a;
  TRY(push_args(b, &b->d_mission, b->mission_host));
  b->mission_on = true;
  return OMGX_OK;
}

int omgx_batch_mission_advance(omgx_batch* b, double* p, double* x, double* lam_g, int32_t step_index) {
  if (!p || !x || !lam_g) return bad("mission_advance: null p / x / lam_g");
  if (step_index < 0) return bad("mission_advance: step_index = %d is negative", step_index);
  if (!b) return bad("null handle");
  if (!b->mission_on || !b->d_mission) return bad("mission_advance: no mission is set (omgx_batch_set_mission)");
  if (!b->stop_on) return bad("mission_advance: the stop rule is off (omgx_batch_set_stop): arriving is that rule");
  if (b->n_range > 0) return bad("mission_advance: not with two-sided rows (the caller's multipliers are not the kernel's rows)");
  const MissionArgs& ms = b->mission_host;
  if (ms.o_state0 != b->stop_host.o_state || ms.o_input0 != b->stop_host.o_input || ms.o_poseT != b->stop_host.o_pose || ms.n_spl != b->stop_host.n_dim)
    return bad("mission_advance: o_state0 / o_input0 / o_poseT / n_spl of the mission are not those of the stop rule");
  if (b->plant_on && (b->plant_host.pl.n_spl != ms.n_spl || b->plant_host.pl.p_poseT != ms.o_poseT || !b->plant_host.pl.under_way))
    return bad("mission_advance: the plant set (omgx_batch_set_plant) is not one of the mission's splines and goal, or has no under_way");
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(mission_advance_kernel, dim3((b->n_agents + 3) / 4), dim3(256), 0, b->stream, p, x, lam_g, b->dims.n_par, b->n_agents,
                     (const MissionArgs*)b->d_mission, b->stop_host, (const PlantBlock*)(b->plant_on ? b->d_plant : nullptr), step_index);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_set_free_t(omgx_batch* b, const omgx_free_t_spec* sp) {
  if (!sp) {
    if (!b) return bad("null handle");
    b->free_t_on = false;
    HIPCHK(hipSetDevice(b->device));
    b->free_t_tab.reset();      // (waits for the launches that still read the tables)
    return OMGX_OK;
  }
  // without a handle: the plan, the limits, the tables
  if (!sp->p_off || !sp->entries || !sp->basis) return bad("set_free_t: null p_off / entries / basis");
  TRY(check_plan("set_free_t", Plan{sp->coeff_off, sp->n_spl, sp->degree, sp->n_knots, 0.0, sp->knots}, 1, kAnySpl, false));
  if (sp->n_out < 1 || sp->n_out > 4 || sp->n_out > sp->degree + 1) return bad("set_free_t: n_out = %d outside 1 .. min(4, degree + 1)", sp->n_out);
  if (!(sp->update_time > 0.0)) return bad("set_free_t: update_time = %g must be positive", sp->update_time);
  if (sp->o_T < 0) return bad("set_free_t: o_T = %d is negative", sp->o_T);
  if (sp->n_ent < 1 || sp->n_ent > OMGX_FREE_T_MAX_ENT) return bad("set_free_t: n_ent = %d outside 1 .. %d", sp->n_ent, OMGX_FREE_T_MAX_ENT);
  if (sp->n_basis < 1 || sp->n_basis > OMGX_FREE_T_MAX_BASIS) return bad("set_free_t: n_basis = %d outside 1 .. %d", sp->n_basis, OMGX_FREE_T_MAX_BASIS);
  size_t tab_doubles = 0;
  for (int i = 0; i < sp->n_basis; ++i) {
    const omgx_free_t_basis& bs = sp->basis[i];
    if (!bs.knots || !bs.fit || !bs.proj) return bad("set_free_t: basis[%d]: null knots / fit / proj", i);
    if (bs.degree < 1 || bs.degree > 5) return bad("set_free_t: basis[%d]: degree = %d outside 1 .. 5", i, bs.degree);
    if (bs.n_knots < 2 * bs.degree + 2 || bs.n_knots > 40) return bad("set_free_t: basis[%d]: n_knots = %d outside %d .. 40", i, bs.n_knots, 2 * bs.degree + 2);
    if (bs.n_knots - bs.degree - 1 > OMGX_FREE_T_MAX_ROWS) return bad("set_free_t: basis[%d]: rows = %d outside 1 .. %d", i, bs.n_knots - bs.degree - 1, OMGX_FREE_T_MAX_ROWS);
    if (bs.n_fit < 1 || bs.n_fit > OMGX_FREE_T_MAX_FIT) return bad("set_free_t: basis[%d]: n_fit = %d outside 1 .. %d", i, bs.n_fit, OMGX_FREE_T_MAX_FIT);
    tab_doubles += (size_t)bs.n_fit * (size_t)(1 + bs.n_knots - bs.degree - 1);
  }
  for (int e = 0; e < sp->n_ent; ++e) {
    const int32_t* en = sp->entries + 4 * e;
    if (en[1] < 1 || en[1] > OMGX_FREE_T_MAX_ROWS) return bad("set_free_t: entries[%d]: rows = %d outside 1 .. %d", e, en[1], OMGX_FREE_T_MAX_ROWS);
    if (en[3] < 0 || en[3] >= sp->n_basis) return bad("set_free_t: entries[%d]: basis = %d outside 0 .. %d", e, en[3], sp->n_basis - 1);
    const omgx_free_t_basis& bs = sp->basis[en[3]];
    if (en[1] != bs.n_knots - bs.degree - 1) return bad("set_free_t: entries[%d]: rows = %d, its basis has %d coefficients", e, en[1], bs.n_knots - bs.degree - 1);
    if (en[2] < 1) return bad("set_free_t: entries[%d]: cols = %d must be positive", e, en[2]);
    if (en[0] < 0) return bad("set_free_t: entries[%d]: offset = %d is negative", e, en[0]);
  }
  if (!b) return bad("null handle");
  const omgx::Dims& d = b->dims;
  FreeTArgs a = {};
  const Plan pl{sp->coeff_off, sp->n_spl, sp->degree, sp->n_knots, 0.0, sp->knots};
  TRY(check_predict_in_xp(b, "set_free_t", pl, sp->n_out, sp->p_off, sp->p_t, a.p_off));
  if (sp->o_T >= d.n_var) return bad("set_free_t: o_T = %d outside x (n_var = %d)", sp->o_T, d.n_var);
  for (int e = 0; e < sp->n_ent; ++e) {
    const int32_t* en = sp->entries + 4 * e;
    if (en[0] + (long long)en[1] * en[2] > d.n_var) return bad("set_free_t: entries[%d]: offset = %d, %d x %d coefficients outside x (n_var = %d)", e, en[0], en[1], en[2], d.n_var);
    for (int q = 0; q < 4; ++q) a.ent[e][q] = en[q];
  }
  b->free_t_on = false;      // (a failed registration leaves it OFF)
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(b->free_t_tab.alloc(sizeof(double) * tab_doubles));      // (frees the previous tables first: waits for the launches that read them)
  std::vector<double> tab;
  tab.reserve(tab_doubles);
  a.coeff_off = pl.coeff_off; a.n_spl = pl.n_spl; a.degree = pl.degree; a.n_knots = pl.n_knots;
  fill_knots(a.knots, pl.knots, pl.n_knots);
  a.n_out = sp->n_out; a.p_t = sp->p_t; a.o_T = sp->o_T; a.n_ent = sp->n_ent; a.n_basis = sp->n_basis; a.update_time = sp->update_time;
  for (int i = 0; i < sp->n_basis; ++i) {
    const omgx_free_t_basis& bs = sp->basis[i];
    FreeTBasis& o = a.basis[i];
    o.degree = bs.degree; o.n_knots = bs.n_knots; o.n_fit = bs.n_fit; o.rows = bs.n_knots - bs.degree - 1;
    fill_knots(o.knots, bs.knots, bs.n_knots);
    o.fit = (const double*)b->free_t_tab.p + tab.size();
    tab.insert(tab.end(), bs.fit, bs.fit + bs.n_fit);
    o.proj = (const double*)b->free_t_tab.p + tab.size();
    tab.insert(tab.end(), bs.proj, bs.proj + (size_t)o.rows * bs.n_fit);
  }
  // (a fresh allocation nothing reads yet; the copy is done when the call returns, so the host vector may go)
  HIPCHK(hipMemcpy(b->free_t_tab.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
  b->free_t_host = a;
  TRY(push_args(b, &b->d_free_t, b->free_t_host));
  b->free_t_on = true;
  return OMGX_OK;
}

int omgx_batch_free_t_advance(omgx_batch* b, double* x, double* p, double update_time, int32_t* under_way) {
  if (!x || !p) return bad("free_t_advance: null x / p");
  if (!(update_time > 0.0)) return bad("free_t_advance: update_time = %g must be positive", update_time);
  if (!b) return bad("null handle");
  if (!b->free_t_on || !b->d_free_t) return bad("free_t_advance: no free-end-time glue is set (omgx_batch_set_free_t)");
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(free_t_advance_kernel, dim3(b->n_agents), dim3(64), 0, b->stream, x, b->dims.n_var, p, b->dims.n_par,
                     (const FreeTArgs*)b->d_free_t, update_time, under_way);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_free_t_append(omgx_batch* b, const double* x, const int32_t* under_way, const omgx_signals_spec* sp) {
  if (!sp) return bad("null argument");
  omgx_signals_spec s = *sp;
  s.inv_T = 1.0; s.p_t = 0;      // (ignored by this entry: every agent has its own horizon, and t is 0)
  SignalArgs sg;
  TRY(check_signals_spec(&s));
  if (!b) return bad("null handle");
  if (!b->free_t_on) return bad("free_t_append: no free-end-time glue is set (omgx_batch_set_free_t)");
  TRY(check_plan_in_x(b, "free_t_append", plan_of(s)));
  if (!same_plan(s, b->free_t_host)) return bad("free_t_append: coeff_off / n_spl / degree / n_knots are not those given to omgx_batch_set_free_t");
  if (!x) return bad("null argument");
  put_plan(sg, plan_of(s));
  sg.log = s.log; sg.count = s.count; sg.overflow = s.overflow;
  sg.n_der = s.n_der; sg.n_samp = s.n_samp; sg.cap = s.cap; sg.p_t = 0; sg.sample_time = s.sample_time;
  HIPCHK(hipSetDevice(b->device));
  const size_t lds = sample_scratch_doubles(sg.n_spl, sg.degree, sg.n_knots, sg.n_der) * sizeof(double);
  if (lds > 64 * 1024) { g_err = "signals: the per-agent scratch exceeds 64 KiB of LDS"; return OMGX_E_TOOLARGE; }
  hipLaunchKernelGGL(free_t_append_kernel, dim3(b->n_agents), dim3(256), lds, b->stream, x, b->dims.n_var, under_way, sg, b->free_t_host.o_T,
                     b->free_t_host.update_time);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_admm_center(omgx_batch* b, const omgx_admm_layout* lay, const double* x, const double* p, double* x_i) {
  return omgx_admm_center_ex(b, lay, x, p, x_i, nullptr, 0, nullptr);
}

int omgx_admm_center_ex(omgx_batch* b, const omgx_admm_layout* lay, const double* x, const double* p, double* x_i,
                        const int32_t* pub_rows, int32_t n_pub, double* x_send) {
  if (!b || !lay || !x || !p || !x_i || n_pub < 0 || (n_pub > 0 && (!pub_rows || !x_send))) { g_err = "bad argument"; return OMGX_E_INVALID; }
  HIPCHK(hipSetDevice(b->device));
  const int n = (b->n_agents + n_pub) * lay->n_dim * lay->L;
  hipLaunchKernelGGL(admm_center_kernel, dim3((n + 255) / 256), dim3(256), 0, b->stream, *lay, x, b->dims.n_var,
                     p, b->dims.n_par, x_i, b->n_agents, pub_rows, n_pub, x_send);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_batch_set_center(omgx_batch* b, const omgx_admm_layout* lay, double* x_i, const int32_t* pub_rows, int32_t n_pub, double* x_send) {
  if (!b) { g_err = "bad argument"; return OMGX_E_INVALID; }
  if (!lay) { b->center_on = false; return OMGX_OK; }
  // (a failed registration leaves the epilogue OFF: the previous x_i may be a buffer the caller has released since)
  b->center_on = false;
  if (!x_i || n_pub < 0 || (n_pub > 0 && (!pub_rows || !x_send)) || lay->n_dim <= 0 || lay->L <= 0 ||
      lay->x_spl < 0 || lay->x_spl + lay->n_dim * lay->L > b->dims.n_var || lay->p_rel < 0 || lay->p_rel + lay->n_dim > b->dims.n_par) {
    g_err = "bad argument"; return OMGX_E_INVALID;
  }
  HIPCHK(hipSetDevice(b->device));
  std::vector<int32_t> inv((size_t)b->n_agents, -1);
  for (int i = 0; i < n_pub; ++i) {
    const int r = pub_rows[i];
    if (r < 0 || r >= b->n_agents) { g_err = "published row out of range"; return OMGX_E_INVALID; }
    if (inv[r] >= 0) { g_err = "a row published twice cannot ride on the solve (use omgx_admm_center_ex)"; return OMGX_E_INVALID; }
    inv[r] = i;
  }
  if (n_pub > 0 && !b->d_pub_inv) TRY(dalloc(b, (size_t)b->n_agents, &b->d_pub_inv));
  CenterArgs ca;
  ca.x_spl = lay->x_spl; ca.p_rel = lay->p_rel; ca.n_dim = lay->n_dim; ca.L = lay->L;
  ca.x_i = x_i; ca.pub_inv = n_pub > 0 ? b->d_pub_inv : nullptr; ca.x_send = x_send;
  // (pageable host memory: the copies are staged before the calls return)
  if (n_pub > 0) HIPCHK(hipMemcpyAsync(b->d_pub_inv, inv.data(), sizeof(int32_t) * inv.size(), hipMemcpyHostToDevice, b->stream));
  TRY(push_args(b, &b->d_center, ca));
  HIPCHK(hipStreamSynchronize(b->stream));
  b->center_on = true;
  return OMGX_OK;
}

int omgx_admm_update(omgx_batch* b, const omgx_admm_layout* lay, const double* x_ext, const int32_t* nbr,
                     const double* M, const double* F, double rho, double* p, double* z_ij, double* l_ij,
                     double* res) {
  return omgx_admm_update_sums(b, lay, x_ext, nbr, M, F, rho, p, z_ij, l_ij, res, nullptr);
}

int omgx_admm_update_sums(omgx_batch* b, const omgx_admm_layout* lay, const double* x_ext, const int32_t* nbr,
                          const double* M, const double* F, double rho, double* p, double* z_ij, double* l_ij,
                          double* res, double* sums) {
  if (!lay) { g_err = "bad argument"; return OMGX_E_INVALID; }
  return omgx_admm_update_ex(b, lay, x_ext, nbr, M, F, rho, p, z_ij, l_ij, lay->n_nghb * lay->n_dim * lay->L, res, sums,
                             nullptr, nullptr, 0);
}

int omgx_admm_update_ex(omgx_batch* b, const omgx_admm_layout* lay, const double* x_ext, const int32_t* nbr,
                        const double* M, const double* F, double rho, double* p, double* z_ij, double* l_ij,
                        int32_t zl_stride, double* res, double* sums, const int32_t* pub_slot, double* zl_send,
                        int32_t send_stride) {
  if (!b || !lay || !x_ext || !nbr || !M || !F || !p || !z_ij || !l_ij || !res || !(rho > 0) ||
      zl_stride < lay->n_nghb * lay->n_dim * lay->L || (pub_slot && (!zl_send || send_stride < 2 * lay->n_nghb * lay->n_dim * lay->L)) ||
      (pub_slot && sums && send_stride < 3)) {      // (sharded callers keep the three residual sums in a row of zl_send)
    g_err = "bad argument"; return OMGX_E_INVALID;
  }
  const int na = (1 + lay->n_nghb) * lay->n_dim * lay->L;
  if (na > 256) { g_err = "stacked consensus vector longer than 256"; return OMGX_E_TOOLARGE; }
  HIPCHK(hipSetDevice(b->device));
  if (sums && !b->d_admm_done) {
    TRY(dalloc(b, (size_t)1, &b->d_admm_done));
    HIPCHK(hipMemset(b->d_admm_done, 0, sizeof(int)));
  }
  const size_t lds_doubles = (size_t)std::max(6 * na + 16, sums ? 3 * 256 : 0);
  hipLaunchKernelGGL(admm_update_kernel, dim3(b->n_agents), dim3(256), lds_doubles * sizeof(double), b->stream,
                     *lay, x_ext, nbr, M, F, rho, p, b->dims.n_par, z_ij, l_ij, (int)zl_stride, res, sums, b->d_admm_done,
                     pub_slot, zl_send, (int)send_stride);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_admm_communicate(omgx_batch* b, const omgx_admm_layout* lay, const int32_t* nbr, const int32_t* slot,
                          const double* z_ij_ext, const double* l_ij_ext, double* p) {
  if (!lay) { g_err = "null argument"; return OMGX_E_INVALID; }
  return omgx_admm_communicate_ex(b, lay, nbr, slot, z_ij_ext, l_ij_ext, lay->n_nghb * lay->n_dim * lay->L, p, nullptr, 0, 0, nullptr);
}

int omgx_admm_communicate_ex(omgx_batch* b, const omgx_admm_layout* lay, const int32_t* nbr, const int32_t* slot,
                             const double* z_ij_ext, const double* l_ij_ext, int32_t zl_stride, double* p,
                             const double* sum_rows, int32_t n_sum_rows, int32_t sum_stride, double* sums_out) {
  if (!b || !lay || !nbr || !slot || !z_ij_ext || !l_ij_ext || !p || zl_stride < lay->n_nghb * lay->n_dim * lay->L ||
      (sums_out && (!sum_rows || n_sum_rows <= 0 || sum_stride < 3))) { g_err = "bad argument"; return OMGX_E_INVALID; }
  HIPCHK(hipSetDevice(b->device));
  const int n = std::max(3, b->n_agents * lay->n_nghb * lay->n_dim * lay->L);
  hipLaunchKernelGGL(admm_comm_kernel, dim3((n + 255) / 256), dim3(256), 0, b->stream, *lay, nbr, slot, z_ij_ext,
                     l_ij_ext, (int)zl_stride, p, b->dims.n_par, b->n_agents, sum_rows, (int)n_sum_rows, (int)sum_stride, sums_out);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

int omgx_shift_rows(omgx_batch* b, double* data, int32_t stride, int32_t n_rows, const uint8_t* mask,
                    const int32_t* entries, int32_t n_ent, const double* Tmats, int32_t n_tmat) {
  // device-pointer variant of omgx_batch_shift for arbitrary row-major arrays (p, z_ij, l_ij ...); stream-ordered
  if (!b || (!data && n_rows > 0) || !entries || !Tmats || n_ent <= 0 || n_rows < 0 || n_tmat <= 0 || stride <= 0) { g_err = "bad argument"; return OMGX_E_INVALID; }
  HIPCHK(hipSetDevice(b->device));
  int max_elems = 0;
  TRY(stage_shift_tables(b, entries, n_ent, Tmats, n_tmat, stride, &max_elems));
  if (n_rows == 0) return OMGX_OK;            // (tables uploaded ahead of the loop that will use them)
  hipLaunchKernelGGL(shift_kernel, dim3(n_rows), dim3(64), max_elems * sizeof(double), b->stream, data, stride,
                     mask, b->d_shift_ent, n_ent, b->d_shift_T);
  HIPCHK(hipGetLastError());
  return OMGX_OK;
}

}  // extern "C"
