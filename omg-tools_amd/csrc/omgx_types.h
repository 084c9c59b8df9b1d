// omgx_types.h -- what the host code of the library (omgx.hip, omgx_plan.h, omgx_device.h) and the solve (omgx_core.h) share as
// data: dimensions, table records, options, the workspace layout and its modes, the descriptors of the block-arrow KKT store,
// the record of a prepared solve, the result.  No execution context, no intrinsic, no thread index: compiles as plain C++
// (g++ -DOMGX_HOST_PORT), as host code and as device code.
#pragma once
#include <stdint.h>
#include <math.h>

#ifdef OMGX_HOST_PORT
#define OMGX_FN inline
#define OMGX_HD inline
#define OMGX_HDF inline
#else
#define OMGX_FN __device__ __forceinline__
#define OMGX_HD __host__ __device__ inline
#define OMGX_HDF __host__ __device__ __forceinline__      // OMGX_FN that the plan (host code of the library) may call too
#endif

namespace omgx {

enum { ROW_FREE = 0, ROW_UPPER = 1, ROW_LOWER = 2, ROW_EQ = 3, ROW_BAD = 4 };
enum { OP_DIV = 0, OP_BSPL = 1, OP_COS = 2, OP_SIN = 3 };

struct Dims {
  int n_var, n_par, n_con, n_atoms, n_slots, n_terms, n_prog;
  int N;        // n_var + 1 (phase-I variable t is variable index n_var)
  int n_leaf, n_root, n_eq, nnz_j, root_off;
  int nr;       // n_root + n_eq: order of the root block
  int n_pairs;  // Jacobian entry pairs contributing to J' Sigma J
  int n_eqe;    // Jacobian entries of the equality rows
  int max_leaf, max_cpl;
  int col_doubles;   // scratch for the blocked LDL' (staging + panel buffers)
  int col_small_noroot;   // col_small without the LDS copy of the root block (mode 6)
  int col_small;     // the same for the spill modes (left-looking leaf sweep only: inverse pivots + parked diagonal blocks per leaf): kept in LDS there
  int mono_packed;   // 1: every parameter monomial has <= 4 atoms, Tables::pm_rec / sl_ell hold MonoRec; 2: <= 8 atoms, MonoRec8; 0: CSR tables only
  int n_long;        // slots with more than OMGX_SLOT_CAP monomials (the first n_long entries of Tables::sl_list)
  int n_hess;        // number of terms with >= 2 factors
  int quartic;       // 1: some term has four factors
  int general;       // 1: quartic terms, cos / sin atoms or basis rows of degree > 5: the kernel instance that carries them
  int rp_packed;     // 1: rows and positions fit 16 bits each, Tables::je_rp is valid
  int n_knots;       // total length of the knot vectors of the atoms program (copied to LDS per solve)
  int atoms_alias;   // 1: atoms and knots live in the space of gbar | sol (they are dead once the slots are evaluated, gbar and sol
                     //    are first written inside the iteration): n_atoms + n_knots <= 2 N + n_eq
  int wave_ok;       // 1: every panel of the KKT store fits one wave (register-resident factorisation, omgx_wave.h)
  int n_jv;          // Jacobian entries whose value depends on x (the others are constant over a solve)
  int n_jv4, n_ja4;  // owners of the Jacobian item tables (four entries each): x-dependent entries, all entries
  int ka_len, kh_len, kg_len;   // records per owner bin (longest bin) of the pair / Hessian / Gershgorin passes
  int n_kafix, n_kgfix;         // targets whose run was cut (fix-up records)
  int n_khfix;                  // the same for the Hessian items
  int side_off, dump_off;       // side slots / per-lane dump slots behind the KKT store
  int n_cs_own;      // owner threads of the column sums J'w (chunks of the columns)
  int kg_side_dinv;  // 1: the side sums of the Gershgorin pass live in w.dinv, 0: in the side slots behind the KKT store
  int n_owner;       // owner bins in use (<= OMGX_NBIN, the stride of the record tables): the threads of the workgroup the plan was made for
  int n_lift, lift_depth;   // auxiliary variables of lifted products / quotients (omgx_template::n_lift) and the length of their longest chain
  // Schur phase by tile owners (wave path; HostPlan::schur_rule, kkt_factor_wave): schur_tiles = number of banded leaves (they all
  // couple to the same root positions in the same order), 0 = the round form.  The descriptor image then carries, as int32 behind
  // its (n_leaf + 1) descriptors: that coupling row at schur_row, the dl_pos slice of the diagonal leaf at schur_dl (offsets in ints
  // from the start of the image), schur_ints = length of the whole image
  int schur_tiles, schur_row, schur_dl, schur_ints;
};

// one parameter monomial coef * prod atoms[a_k] as a single 16-byte record (a_k = -1: unused): one
// load per monomial instead of the pointer chase pm_ptr -> pm_atom -> atoms of the CSR form
struct MonoRec { double coef; int16_t a0, a1, a2, a3; };
// the same with up to eight atoms (Dims::mono_packed == 2: ADMM objectives multiply rho, multipliers and basis values)
struct MonoRec8 { double coef; int16_t a0, a1, a2, a3, a4, a5, a6, a7; };

// Owner-computes records (omgx_plan.h): every sum of the solve has one owner thread and a fixed order.  A term is
// coef * slot * x_v0 x_v1 x_v2 x_v3 (OMGX_TERM_VARS = 4 factors, -1: unused; a repeated index is a power).
// JItem: one contribution coef * slot * x[va] * x[vb] * x[vc] (v = -1: factor 1) to a Jacobian entry: the term without
// one of its factors.
// HItem: one contribution of a nonlinear term to a KKT address (or, for the Gershgorin sums, to a position): the term
// without two of its factors, h = lambda_row * coef * slot * x[vthird] * x[vfourth]; kind 1 = the two factors that
// were taken out are the same variable (a diagonal entry: both orders of the pair land on it).
// (slot indices are 16 bit in the 16- and 24-byte records: the plan refuses templates with more than 32767 slots)
#define OMGX_TV 4
struct JItem { double coef; int16_t slot, va, vb, vc; };
// one term of a row for the row-value passes (24 bytes; padding records have coef 0)
struct RowTerm { double coef; int32_t slot; int16_t v0, v1, v2, v3; };
struct HItem { double coef; int32_t row, target; int16_t slot, vthird, vfourth, kind; };

struct Tables {   // read-only, shared by all agents (global memory)
  const int32_t* prog; const double* knots;
  const int32_t* pp_ptr; const double* pm_coef; const int32_t* pm_ptr; const int32_t* pm_atom;
  const int32_t* slot_pp;
  const MonoRec* pm_rec;    // [n_mono] packed form of (pm_coef, pm_ptr, pm_atom); valid if Dims::mono_packed
  const int32_t* slot_rng;  // [n_slots][2] monomial range of every slot (= pp_ptr[slot_pp[s]], pp_ptr[slot_pp[s] + 1])
  const int32_t* row_ptr; const double* t_coef; const int32_t* t_slot; const int32_t* t_var;
  const int32_t* order; const int32_t* leaf_off; const int32_t* blk;
  const int32_t* eq_rows; const int32_t* eq_index;
  const int32_t* cpl_ptr; const int32_t* cpl_idx; const int32_t* cpl_map;
  const int32_t* d_off; const int32_t* b_off;   // panel offsets / leading dimensions inside the KKT store
  // compact store of the wave path (omgx_plan.h `compact`): per leaf the offset of its carried rows (sparse diagonal
  // leaf: the number of coupling slots S), the row stride and width of its band, its kind (0 banded panel, 1 sparse
  // diagonal leaf); dl_pos[4 * leaf_off[l] + s * n_l + j]: root position coupled through slot s of variable j (-1: none)
  const int32_t* lf_w; const int32_t* lf_ldb; const int32_t* lf_band; const int32_t* lf_kind; const int32_t* dl_pos;
  const int32_t* bmat_img;  // compact store only: the matrix descriptors of a solve, [n_leaf + 1] BMat as the plan filled them (kkt_describe_fill)
  // precomputed KKT addresses (HostPlan): Jacobian pairs, t-column, diagonal, Hessian terms
  const int32_t* eqe3;      // [n_eqe][3] = {Jacobian entry, KKT address, row} of the equality-row entries
  const int32_t* pair4;     // [n_pairs][4] = {Jacobian entry a, entry b, KKT address, row}: one 16-byte record per pair
  const int32_t* je_row; const int32_t* diag_addr;
  const int32_t* je_rp;     // [nnz_j] (row << 16) | position of every Jacobian entry (valid if Dims::rp_packed)
  const double* reg_w;   // [N] position order: inertia-correction class (+1 nonlinear root variable, -1 nonlinear leaf variable, else the weight itself: OMGX_DW_LINEAR)
  const int32_t* leaf_bw;   // [n_leaf] half bandwidth of the leaf block in its (reverse Cuthill-McKee) order
  const int32_t* tq_addr;   // [n_var] KKT address of (t, q)
  // owner-computes tables
  const int32_t* row_perm;  // [n_con] rows, longest term list first
  // ELL tables of the row / column / entry owners: record `step` of owner i at index step * n_owner + i
  // (coalesced across the lanes), padded with null records; *_glen[i >> 6] = steps the 64 owners of a
  // group need (rounded up to the batch the loops load at a time)
  const RowTerm* rt_ell;    // [rt_steps][n_con] terms of row row_perm[i]
  const int32_t* rt_glen;
  const int32_t* jp_ell;    // [jp_steps][n_con][2] {Jacobian entry, position} of row row_perm[i] (padding: entry nnz_j = 0.0)
  const int32_t* jp_glen;
  const int32_t* cs_ell;    // [cs_steps][n_cs_own][2] {Jacobian entry, row} of column-sum owner o (padding: entry nnz_j = 0.0)
  const int32_t* cs_glen;
  const int32_t* cs_own;    // [n_var + 1] owners of the column in slot j: cs_own[j] .. cs_own[j + 1]
  const int32_t* cs_col;    // [n_var] column (position) of slot j (columns by decreasing length)
  // Jacobian items, four entries per owner (jac_entries4): the x-dependent entries (every iteration) and all entries (setup)
  const JItem* jv_ell;      // [jv_steps][4][n_jv4] items of the owner's k-th entry (entries by decreasing item count, four in a row per owner)
  const int32_t* jv_own;    // [4][n_jv4][2] {entry, row} (-1: the owner has no k-th entry)
  const int32_t* jv_glen;   // [n_jv4 / 64] items per entry the group walks (1 or even)
  const JItem* ja_ell;      // [ja_steps][4][n_ja4]
  const int32_t* ja_own;
  const int32_t* ja_glen;
  const int32_t* sl_list;   // [n_slots] slots by decreasing monomial count
  const MonoRec* sl_ell;    // [sl_steps][n_slots] monomials of slot sl_list[i] (padding: coef 0)
  const int32_t* sl_glen;
  // lifted auxiliaries (Dims::n_lift), level by level: lift_rec[k] = {ELL slot of the defining row, the auxiliary variable}; the records of
  // level L (rows that read auxiliaries of the levels below only) are lift_lev[L] .. lift_lev[L + 1]
  const int32_t* lift_rec; const int32_t* lift_lev;
  const int32_t* cs_ptr;    // [n_var + 1] column (position) -> its entries, row order
  const int32_t* cs_rec;    // [.][2] {Jacobian entry, row}
  const int32_t* obj_ent;   // [n_var] objective-row entry of the position (-1: none)
  // ELL layout: record r of owner bin b at index r * OMGX_NBIN + b (coalesced across the lanes), a bin's
  // records sorted by target; the target is stored only in the last record of its run (-1 in the others
  // and in the padding): the owner adds every record to a running sum and stores / restarts where it sees one
  const int32_t* ka_rec;    // [ka_len][OMGX_NBIN][4] pair records {entry a, entry b, KKT address, row}
  const HItem* kh_rec;      // [kh_len][OMGX_NBIN] Hessian items (target = KKT address)
  const HItem* kg_rec;      // [kg_len][OMGX_NBIN] Gershgorin items (target = position, N + k = side slot k)
  const int32_t* kh_fix;    // [n_khfix][3] the same for cut runs of Hessian items (after hess_bin)
  const int32_t* ka_fix;    // [n_kafix][3] {KKT address, first side slot, number of side slots}: address += the slots, in order
  const int32_t* kg_fix;    // [n_kgfix][3] the same for the Gershgorin sums (position)
};

struct Opts {
  double tol; int max_iter; double mu_init, kappa_push, nu_init, scale_gmax;
  int warm_start;      // 1: lam0 holds the multipliers of the previous solve (primal-dual warm start)
  double kappa_warm;   // kappa_push used for warm starts
  double dw_leaf_ratio_cold;   // cold starts: inertia-correction weight of nonlinear leaf variables (root: its inverse)
  int prio_iter;               // device: iteration from which a solve runs at raised wave priority (0: never)
  double warm_mu_factor;       // warm starts: mu_0 = clamp(warm_mu_factor * mean(s z), tol / 10, mu_init)
  double warm_z_floor;         // warm starts: multipliers lifted to max(OMGX_WARM_ZMIN, min(warm_z_floor * tol, warm_z_cap * tol / slack))
  double warm_z_cap;           // (0: no cap)
  int max_soc;                 // > 0: a rejected first trial of the line search is answered by up to max_soc second-order corrections (every template class: kkt_solve2_wave / kkt_solve2)
  int hess_approx;             // 1: no constraint curvature in the Hessian, damping driven by the accepted step length (general instances; include/omgx.h)  // (version 8) IPOPT's absolute tolerances on the UNSCALED problem beside `tol` (its documented defaults: compl_inf_tol = constr_viol_tol = 1e-4,
  // which the reference leaves in force when it sets ipopt.tol = 1e-3, `problems/problem.py:57`); 0: not tested (rounds 1-5).  The barrier
  // parameter ends at min(tol, compl_tol) / 10.
  double compl_tol, viol_tol;
  int refine;                  // (version 9) 1: iterative refinement of a regularised Newton step, from the second iteration of a solve on (default 0)
};

// fixed constants of the iteration (same values in oracle/ipm_numpy.py DEFAULTS)
#ifndef OMGX_KAPPA_EPS
#define OMGX_KAPPA_EPS   10.0
#endif
#define OMGX_KAPPA_MU    0.2
#define OMGX_THETA_MU    1.5
#define OMGX_TAU_MIN     0.99
#define OMGX_DELTA_C     1e-8    // regularisation of the equality block: delta_c = OMGX_DELTA_C * mu^(1/4) (IPOPT's delta_c_bar mu^kappa_c)
#define OMGX_ETA         1e-4
#define OMGX_PHI_NOISE   1e-10   // predicted merit decrease (relative) below which the Armijo test is skipped
#define OMGX_DW_FIRST    1e-4
#ifndef OMGX_DW_INC
#define OMGX_DW_INC      10.0
#endif
#ifndef OMGX_DW_DEC
#define OMGX_DW_DEC      (1.0 / 3.0)
#endif
#define OMGX_DW_MAX      1e10
#define OMGX_DW_ZERO     1e-9
#define OMGX_DW_HEAVY    10.0
#ifndef OMGX_KAPPA_EPS_HEAVY
#define OMGX_KAPPA_EPS_HEAVY 100.0    // (round 4 tried 30: same-box A/B, 4096 agents: config 2 cold 91.4k vs 90.0k solves/s -- noise -- but the Quadrotor class 12.2k vs 15.7k cold, 25.2 vs 21.7 ms per warm step: kept at 100)
#endif
#ifndef OMGX_DW_BACKOFF_MAX
#define OMGX_DW_BACKOFF_MAX 8
#endif
#ifndef OMGX_EXPAND_MAX
#define OMGX_EXPAND_MAX   16.0    // longest multiple of a regularised Newton step the line search offers
#endif
#ifndef OMGX_EXPAND_DW
#define OMGX_EXPAND_DW    1e-2    // ... when the inertia correction is at least this heavy
#endif
#ifndef OMGX_EXPAND_FROM
#define OMGX_EXPAND_FROM  2       // ... after this many iterations in a row that accepted their full step at the first trial
#endif
#define OMGX_LS_RETRY    3       // line-search failures in a row that are answered by a heavier inertia correction
#define OMGX_LS_RETRY_DW 100.0
#define OMGX_DW_CAP_FLOOR 0.03  // share of dw every nonlinear variable keeps under the Gershgorin cap
#ifndef OMGX_DW_CLAMP_FROM
#define OMGX_DW_CLAMP_FROM 1.0  // an inertia correction above this is compared with the Gershgorin guarantee (round 5, see the factorisation loop)
#endif
#define OMGX_DW_LINEAR   1e-8   // relative inertia correction of variables that only appear linearly
#ifndef OMGX_FTB_ACTUAL
#define OMGX_FTB_ACTUAL  0.5     // share of the linear fraction-to-boundary bound (1 - tau) s the slack of a row must really keep at an accepted trial point
#endif
#define OMGX_S_MAX       100.0
#define OMGX_KAPPA_SIGMA 1e10
#define OMGX_MAX_BACKTRACK 25
#define OMGX_NU_MAX      1e8
#ifndef OMGX_STALL_ITERS
#define OMGX_STALL_ITERS 20
#endif
#define OMGX_WARM_ZMIN   1e-8
#define OMGX_MAX_LEAF    16
#define OMGX_BMAT_DOUBLES 5      // sizeof(BMat) / 8
#define OMGX_PAN_LD 5      // panel buffer row stride: U[4] + pad (odd: conflict-free row-per-lane access)
#define OMGX_STAGE_LD 20   // per matrix: 4x4 block rows [16] + inverse pivots of the block [4]
#define OMGX_MIN_LEAF    8       // smaller components are gathered into one leaf
#define OMGX_NBIN        512     // owner bins of the assembly passes (= threads of the solve workgroup)
#define OMGX_SLOT_CAP    16      // monomials of a parameter slot one thread sums (setup); the rest of a longer slot: one wave
#define OMGX_REC_BATCH   8       // records an owner loads at a time (all in flight together)
#define OMGX_JE_OWN      4       // Jacobian entries per owner of the item tables (jac_entries4; the plan lays them out so)
#define OMGX_RUN_CAP     16      // longest run of records summed by one owner (longer runs are cut, see omgx_plan.h)
#define OMGX_RUN_CAP_H   64      // the same for the Hessian items (only templates with lifted auxiliaries have such runs)
#define OMGX_WAVE_ROWS   64      // register rows of a panel the wave-level routines take (lanes)
#define OMGX_WAVE_COLS   40      // columns (registers per lane)

// Per-agent work arrays (LDS on the device, heap on the host port).
struct Work {
  double *atoms, *slots, *knots;
  double *x, *xt;                 // [N] variable order, x[n_var] = t
  double *hv, *ht;                // [n_con] scaled row values (h for inequality, c for equality)
  double *rho, *vv;               // [n_con] row scale (signed), phase-I weights
  double *z, *ds;                 // [n_con] multiplier (y for equality rows), slack step
  // (the slack of an inequality row is not stored: every iterate keeps s = t v - h exactly -- `row_slack`; the bound of a
  // row is read from the caller's lbg / ubg where the line search needs it)
  double *jval;                   // [nnz_j] scaled Jacobian entries (objective row unscaled)
  double *gbar, *sol;             // [N], [N + n_eq]   position order
  double *kkt;                    // D_l (packed) | B_l | R (packed)
  double *col;                    // [col_doubles] blocked-LDL' staging + panel buffers
  double *root;                   // spill modes: LDS copy of the packed root block (+ its right-hand-side row) from the Schur step on (inside col)
  double *dinv;                   // [N] inverse leaf pivots
  int8_t *rtype;                  // [n_con]
  double *red;                    // reduction scratch [64]
};

// Workspace placement.  Mode 0 keeps every array in LDS (the fast path: cfg 1/2/4).  Problems
// whose arrays exceed the 160 KiB of one CU spill the largest ones to a per-workgroup slab in
// HBM (L2/MALL-cached), largest first:
//   mode 1  kkt                  mode 2  + jval
//   mode 3  + the six [n_con] row arrays and rtype (only the O(n_var) vectors stay in LDS)
// Mode 4 is the other direction: templates on the register-resident wave path whose workspace then fits HALF a CU --
// two workgroups (agents) per CU -- put the Jacobian values and the row values hv into the slab and keep the
// (compact) KKT store and every array the owner passes gather from in LDS.
// Mode 5 (round 4) is mode 4 with the row values hv back in LDS, for templates that still fit half a CU then (config 2: 80,280 B):
// hv is read by a dozen row passes per iteration, each a dependent global load per pass of the workgroup (+2 % solves/s).
// Mode 6 (round 5) is mode 3 with the root block left in the slab as well: templates whose root block (its variables + ALL
// equality rows: the classes with lifted auxiliaries carry hundreds, include/omgx.h n_lift) does not fit LDS even alone
// (Bicycle: order 439 = 773 KB).  Only the O(n_var) vectors, the descriptors and the panel buffers stay on chip.
enum { WS_LDS = 0, WS_KKT_HBM = 1, WS_JAC_HBM = 2, WS_ROWS_HBM = 3, WS_JAC_ONLY = 4, WS_JAC_HV = 5, WS_ROOT_HBM = 6, WS_MODES = 7 };
OMGX_HD constexpr bool ws_kkt_hbm(int mode) { return (mode >= WS_KKT_HBM && mode <= WS_ROWS_HBM) || mode == WS_ROOT_HBM; }
OMGX_HD constexpr bool ws_jac_hbm(int mode) { return mode >= WS_JAC_HBM; }
OMGX_HD constexpr bool ws_rows_hbm(int mode) { return mode == WS_ROWS_HBM || mode == WS_ROOT_HBM; }
OMGX_HD constexpr bool ws_hv_hbm(int mode) { return mode == WS_ROWS_HBM || mode == WS_JAC_ONLY || mode == WS_ROOT_HBM; }
OMGX_HD constexpr bool ws_root_lds(int mode) { return ws_kkt_hbm(mode) && mode != WS_ROOT_HBM; }      // spill modes 1-3: the root block is copied to LDS for its factorisation

OMGX_HD size_t root_doubles(const Dims& d) { return ((size_t)(d.nr + 1) * (d.nr + 2)) / 2; }

OMGX_HD void work_split(const Dims& d, int kkt_doubles, int mode, size_t* lds, size_t* hbm) {
  size_t nl = 0, ng = 0;
  nl += d.n_slots + (d.atoms_alias ? 0 : d.n_atoms + d.n_knots);
  nl += 2 * (size_t)d.N;
  nl += d.N + (d.N + d.n_eq);
  nl += d.N;                      // dinv
  nl += 64;                       // red
  const size_t rows = 5 * (size_t)d.n_con + (d.n_con + 7) / 8;
  (ws_rows_hbm(mode) ? ng : nl) += rows;
  (ws_hv_hbm(mode) ? ng : nl) += d.n_con;             // hv: only ever read by the thread that owns the row
  (ws_jac_hbm(mode) ? ng : nl) += d.nnz_j + 1;        // + one slot that stays 0.0 (padding records point at it)
  // (the spill modes keep the matrix descriptors and the small panel scratch of the leaf sweep in LDS: every row of
  // every block column reads them)
  if (ws_kkt_hbm(mode)) { ng += (size_t)kkt_doubles; nl += ws_root_lds(mode) ? d.col_small : d.col_small_noroot; } else nl += (size_t)kkt_doubles + d.col_doubles;
  *lds = nl; *hbm = ng;
}

OMGX_HD size_t work_doubles(const Dims& d, int kkt_doubles) {
  size_t nl, ng;
  work_split(d, kkt_doubles, WS_LDS, &nl, &ng);
  return nl;
}

// MODE is a compile-time constant so that every pointer keeps a provable address space
template <int MODE>
OMGX_HD void work_carve_split(Work& w, double* lds, double* hbm, const Dims& d, int kkt_doubles) {
  double* p = lds;
  double* g = hbm;
  w.slots = p; p += d.n_slots;
  if (!d.atoms_alias) { w.atoms = p; p += d.n_atoms; w.knots = p; p += d.n_knots; }
  w.x = p; p += d.N;             w.xt = p; p += d.N;
  w.gbar = p; p += d.N;          w.sol = p; p += d.N + d.n_eq;
  if (d.atoms_alias) { w.atoms = w.gbar; w.knots = w.gbar + d.n_atoms; }
  w.dinv = p; p += d.N;
  w.red = p; p += 64;
  if (ws_rows_hbm(MODE)) {
    w.ht = g; g += d.n_con;        w.rho = g; g += d.n_con;     w.vv = g; g += d.n_con;
    w.z = g; g += d.n_con;         w.ds = g; g += d.n_con;
    w.rtype = (int8_t*)g; g += (d.n_con + 7) / 8;
  } else {
    w.ht = p; p += d.n_con;        w.rho = p; p += d.n_con;     w.vv = p; p += d.n_con;
    w.z = p; p += d.n_con;         w.ds = p; p += d.n_con;
    w.rtype = (int8_t*)p; p += (d.n_con + 7) / 8;
  }
  if (ws_hv_hbm(MODE)) { w.hv = g; g += d.n_con; } else { w.hv = p; p += d.n_con; }
  if (ws_jac_hbm(MODE)) { w.jval = g; g += d.nnz_j + 1; } else { w.jval = p; p += d.nnz_j + 1; }
  if (ws_kkt_hbm(MODE)) { w.kkt = g; g += kkt_doubles; w.col = p; p += ws_root_lds(MODE) ? d.col_small : d.col_small_noroot; }
  else { w.kkt = p; p += kkt_doubles; w.col = p; p += d.col_doubles; }
  // spill modes: the root block is copied behind the root's panel buffer before the Schur updates -- over the leaf
  // sweep's scratch, which is dead by then (Dims::col_small covers both)
  w.root = ws_root_lds(MODE) ? w.col + (OMGX_BMAT_DOUBLES + OMGX_STAGE_LD) * (OMGX_MAX_LEAF + 1) + OMGX_PAN_LD * (d.nr + 1) : nullptr;
}

OMGX_HD void work_carve(Work& w, double* base, const Dims& d, int kkt_doubles) {
  work_carve_split<WS_LDS>(w, base, nullptr, d, kkt_doubles);
}

// ---------------------------------------------------------------------------
// block-arrow KKT store
// ---------------------------------------------------------------------------
OMGX_FN int tri(int i, int k) { return i * (i + 1) / 2 + k; }   // packed lower, row-major, i >= k

struct Kkt {
  // (copies of the few table pointers / dimensions it needs, not pointers to the structs: a struct whose address
  // escapes into a helper object cannot be kept in scalar registers -- the compiler copied all of Dims and
  // Tables into every lane's scratch memory at kernel entry)
  const int32_t *d_off, *b_off, *leaf_off, *leaf_bw, *cpl_ptr, *cpl_idx, *blk, *cpl_map, *lf_w, *lf_ldb, *lf_band, *lf_kind, *dl_pos;
  int n_leaf, n_root, root_off;
  double* a;
  OMGX_HDF void bind(const Dims& dd, const Tables& TT, double* store) {
    d_off = TT.d_off; b_off = TT.b_off; leaf_off = TT.leaf_off; leaf_bw = TT.leaf_bw; cpl_ptr = TT.cpl_ptr;
    cpl_idx = TT.cpl_idx; blk = TT.blk; cpl_map = TT.cpl_map;
    lf_w = TT.lf_w; lf_ldb = TT.lf_ldb; lf_band = TT.lf_band; lf_kind = TT.lf_kind; dl_pos = TT.dl_pos;
    n_leaf = dd.n_leaf; n_root = dd.n_root; root_off = dd.root_off; a = store;
  }
  // leaf l: panel of (n_l + nc_l + 1) rows with odd leading dimension ld_l; rows [0,n_l) hold the
  // leaf block D_l (lower part), rows [n_l, n_l+nc_l) the coupling rows B_l (one per coupled
  // root position), row n_l+nc_l the right-hand side of the leaf.  Root block R: packed lower,
  // row-major, nr rows + one more for its right-hand side.  The right-hand sides are carried through
  // the factorisation like coupling rows, so the forward substitutions L^{-1} r come out of it.
  OMGX_FN double* P(int l) const { return a + d_off[l]; }
  OMGX_HDF int ld(int l) const { return b_off[l]; }
  OMGX_FN double* R() const { return a + d_off[n_leaf]; }
  OMGX_HDF int nl(int l) const { return leaf_off[l + 1] - leaf_off[l]; }
  OMGX_HDF int nc(int l) const { return cpl_ptr[l + 1] - cpl_ptr[l]; }
};

// offsets (not pointers) so that every access stays a provable LDS access (ds_* instead of flat_*)
struct BMat { int a, ld, nfact, rows, npos, dinv, pan, cpl, bw, pad_; };   // cpl: offset of the leaf's coupling index list (cpl_ptr[l])   // a: offset in kkt; dinv: offset in w.dinv (-1: none); pan: offset in w.col
static_assert(sizeof(BMat) <= OMGX_BMAT_DOUBLES * sizeof(double), "BMat larger than its LDS slot");
#define OMGX_PAN_SMALL(n) (4 * (n) + 16)      // per leaf in the spill modes: ldl_left4 keeps n inverse pivots + 10 doubles per 4 columns there

// Matrix descriptors of the block-arrow store, at the head of w.col (shared by the workgroup), followed by the staging area
// and the panel buffers.  kkt_describe_fill is the one definition of their fields: a kernel runs it per workgroup
// (kkt_describe: the plan tables it reads are global memory, i.e. a chain of dependent loads per look-up), the plan runs it
// once per template for the instances on the wave path, whose descriptors depend on the template alone (HostPlan::bmat_img,
// Tables::bmat_img) and are then copied (kkt_descriptors).
template <bool WAVE_ONLY, bool HBM, bool ROOT_LDS>
OMGX_HDF void kkt_describe_fill(const Dims& d, const Kkt& K, BMat* Ms) {
  const int pan0 = (OMGX_BMAT_DOUBLES + OMGX_STAGE_LD) * (OMGX_MAX_LEAF + 1);      // (offset of the panel buffers in w.col)
  int pan = pan0;
  for (int l = 0; l < d.n_leaf; ++l) {
    BMat& M = Ms[l];
    if constexpr (WAVE_ONLY) {
      // compact store: a = band of the leaf block (sparse diagonal leaf: its arrays), pan = its carried rows
      // (sparse: number of coupling slots), pad_ = row stride of the band, bw = stored band (-1: sparse leaf)
      M.a = K.d_off[l]; M.ld = K.ld(l); M.nfact = K.nl(l); M.rows = K.nl(l) + K.nc(l) + 1; M.npos = M.nfact;
      M.dinv = K.leaf_off[l]; M.pan = K.lf_w[l]; M.cpl = K.cpl_ptr[l]; M.bw = K.lf_kind[l] ? -1 : K.lf_band[l]; M.pad_ = K.lf_ldb[l];
      continue;
    }
    M.a = K.d_off[l]; M.ld = K.ld(l); M.nfact = K.nl(l); M.rows = K.nl(l) + K.nc(l) + 1; M.npos = M.nfact;   // + the rhs row
    M.dinv = K.leaf_off[l]; M.pan = pan; pan += HBM ? OMGX_PAN_SMALL(M.nfact) : OMGX_PAN_LD * M.rows; M.cpl = K.cpl_ptr[l]; M.bw = K.leaf_bw[l];
  }
  BMat& Mr = Ms[d.n_leaf];
  Mr.a = ROOT_LDS ? 0 : K.d_off[d.n_leaf]; Mr.ld = 0; Mr.nfact = d.nr; Mr.rows = d.nr + 1; Mr.npos = d.n_root; Mr.dinv = -1; Mr.pan = pan0; Mr.cpl = 0; Mr.bw = d.nr;
  Mr.pad_ = K.d_off[d.n_leaf];      // where the assembly writes the root block (Mr.a: where the factorisation reads it)
}

// optional per-phase cycle counters (profiling build only, -DOMGX_PROFILE)
enum { PH_JAC = 0, PH_RESID, PH_ASSEMBLE, PH_FACTOR, PH_SOLVE, PH_STEP, PH_LINESEARCH, PH_UPDATE, PH_F_LEAF, PH_F_SCHUR, PH_F_ROOT, PH_LA, PH_LS, PH_LB, PH_SETUP, PH_TOTAL,
       PH_S_DESC, PH_S_PARAMS, PH_S_JAC0, PH_S_CLASS, PH_S_INIT, PH_A_ZERO, PH_A_PAIRS, PH_A_REST, PH_A_DIAG,
       PH_K_FWD, PH_K_ROOTRHS, PH_K_ROOT, PH_K_LEAFRHS, PH_K_BWD, PH_L_TERMS, PH_L_ROWS,
       PH_F_PARK, PH_F_SWEEP, PH_F_SCALE, PH_A_TCOL, PH_A_HESS, PH_P_LOAD, PH_P_DIV, PH_P_BSPL, PH_P_SLOTS,
       PH_WG_HEAD, PH_WG_TAIL,      // outside PH_TOTAL: kernel entry (or the workgroup's previous solve) to the start of a solve; its last solve to its exit
       PH_F_SCHUR_MFMA, PH_F_SCHUR_SUB,      // PH_F_SCHUR split by wave 0's clock: forming the tiles of S_l on the matrix pipe; subtracting them from the root (with its barriers)
       PH_K_PRELOAD,      // wave 1's clock: loading the operands of its leaf's substitutions while wave 0 has the root (kkt_root_solve_wave)
       PH_COUNT };

// ---------------------------------------------------------------------------
// the solve: its result, what its setup hands to its iteration, the record of a prepared solve
// ---------------------------------------------------------------------------
struct Result { int status, iters; double f, mu, t, dw; };

// The reference's stop criterion of the point-mass classes on an agent's parameter vector (`problems/point2point.py:98-102` ->
// `vehicles/holonomic.py:145-151`, `holonomic3d.py`: |state0 - poseT| <= tol and |input0| <= tol, Euclidean norms): what ends a
// vehicle's loop in `execution/simulator.py:39-62`.  One statement for the solve kernel's stop rule and the host build's.
OMGX_HD bool stop_criterium(const double* p, int o_state, int o_input, int o_pose, int n_dim, double tol) {
  double e2 = 0.0, u2 = 0.0;
  for (int k = 0; k < n_dim; ++k) {
    const double e = p[o_state + k] - p[o_pose + k], u = p[o_input + k];
    e2 += e * e; u2 += u * u;
  }
  return sqrt(e2) <= tol && sqrt(u2) <= tol;
}

// What the setup of a solve hands to its iteration (beside the work arrays): status 1 = go on, 3 = invalid rows / start point
struct Start { int status, warm, use_t; double mu, zt, f; };

// Record of a prepared solve (one per agent, global memory; written by ipm_prepare_kernel, read by the solve kernel): offsets
// in doubles.  sc: {status, warm, use_t, mu, zt, f, -, -}; x: [N] start point (lifted auxiliaries on their rows, x[n_var] = t);
// the row arrays; rtype bytes; the scaled Jacobian values (+ the padding slot).
struct PrepLayout { int sc, x, slots, hv, rho, vv, z, rtype, jval, total; };
OMGX_HD PrepLayout prep_layout(const Dims& d) {
  PrepLayout L; int o = 0;
  L.sc = o; o += 8;
  L.x = o; o += d.N;
  L.slots = o; o += d.n_slots;
  L.hv = o; o += d.n_con; L.rho = o; o += d.n_con; L.vv = o; o += d.n_con; L.z = o; o += d.n_con;
  L.rtype = o; o += (d.n_con + 7) / 8;
  o = (o + 1) & ~1;                       // (the Jacobian values 16-byte aligned)
  L.jval = o; o += d.nnz_j + 1;
  L.total = (o + 1) & ~1;
  return L;
}

}  // namespace omgx
