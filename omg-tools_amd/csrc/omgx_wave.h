// omgx_wave.h -- wave-level, register-resident linear algebra for the block-arrow KKT solve (gfx950 only).
//
// One wave owns one small symmetric matrix (a leaf panel or the root block of the KKT store): lane i
// holds row i in registers, a column is a register index.  The right-looking LDL' needs, per pair
// (j, k > j), the entry u_kj of the pivot column in every lane -- a v_readlane broadcast from lane k --
// and one fp64 FMA on the whole wave; there is no LDS traffic and no barrier inside the factorisation
// (the LDS-resident routines it replaces, ldl_left4 / ldl_blocked, re-read every operand from LDS for
// every block step and were bound by LDS issue: 61 k + 69 k cycles for four 36-column leaves and the
// 39-column root of config 2).  All register indices are compile-time constants (full unrolling), the
// run-time order n only cuts the loops short through wave-uniform branches.
//
// Storage convention (same as the routines replaced): factorised rows hold U = L D
// (u_ij = l_ij d_j, the pivot d_i on the diagonal), carried rows hold W = B L^{-T}, inverse pivots in a
// side array.  "Vector rows" are carried rows kept as one value per lane (lane k = column k) instead of
// one row per lane: the phase-I coupling row and the right-hand side of a leaf, the right-hand side of
// the root -- so that config 2's 36 + 28 register rows fill the 64 lanes exactly.
#pragma once

namespace omgx {

// (lane: any wave-uniform value)
__device__ __forceinline__ double readlane_d(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sign test of a pivot on its two words -- integer arithmetic, so that a wave-uniform pivot (v_readlane leaves it in
// scalar registers) is judged by the scalar unit, and the flag kept in a scalar register.  The same decision as
// !(pos ? d > 0.0 : d < 0.0) for every double (+-0, denormals, +-inf and NaN included): with the sign bit flipped where
// a negative pivot is wanted, d passes iff its sign bit is clear and its magnitude lies in (0, inf] -- k = high word |
// (low word != 0) orders the magnitudes the way the doubles are ordered wherever it matters (0 -> 0, inf -> 0x7ff00000,
// every NaN above, a set sign bit above all): wrong iff k - 1 > 0x7fefffff (unsigned).
//   j, npos, n: column, number of positive pivots, order (pos = j < npos; columns j >= n are padding and raise no flag:
//   their bound is 0xffffffff, which nothing exceeds).
// Returns `bad`, set to 1 if the pivot of a live column has the wrong sign.
// On the device the six instructions are written out: from C the compiler turns every form tried (selects, or compare-free
// shifts and adds) back into wave-uniform booleans, which it keeps as lane masks and combines on the vector pipe (v_cndmask /
// v_or / v_cmp around v_rcp_f64, the masks spilled across the column).
__host__ __device__ __forceinline__ unsigned pivot_wrong_sign(unsigned bad, int hi, int lo, int j, int npos, int n) {
  const unsigned flip = (unsigned)(npos - 1 - j) & 0x80000000u;          // j >= npos: a negative pivot is wanted
  const unsigned lim = j < n ? 0x7fefffffu : 0xffffffffu;
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned w, t;
  // (both are wave-uniform; where the compiler has them in a vector register all the same, an "s" operand is not moved for us)
  const unsigned flip_s = __builtin_amdgcn_readfirstlane(flip), lim_s = __builtin_amdgcn_readfirstlane(lim);
  asm("s_min_u32 %2, %4, 1\n\t"               // low word != 0
      "s_xor_b32 %1, %3, %5\n\t"
      "s_or_b32 %1, %1, %2\n\t"               // k
      "s_add_u32 %1, %1, -1\n\t"
      "s_cmp_gt_u32 %1, %6\n\t"
      "s_cselect_b32 %0, 1, %0"
      : "+s"(bad), "=&s"(w), "=&s"(t) : "s"(hi), "s"(lo), "s"(flip_s), "s"(lim_s) : "scc");
  return bad;
#else
  const unsigned k = ((unsigned)hi ^ flip) | (lo != 0 ? 1u : 0u);
  return (k - 1u > lim) ? 1u : bad;
#endif
}

// A panel of the KKT store as one wave sees it.  Rows [0, n): the symmetric block (lower part stored);
// rows [n, nreg): carried rows held one per lane; rows [nreg, nreg + nvec): carried rows held as lane
// vectors (nvec <= the NVEC of the wave_ldl instance the panel goes through: a leaf has two, the root one).
// Pivots j < npos must be positive, the others negative.  Two storage forms:
//   packed (root block, band < 0): row r starts at base + r (r + 1) / 2;
//   banded (leaf panels, band >= 0): row i of the symmetric block keeps its entries (i, i - band) .. (i, i) at
//     base + i * ldb (a leaf in reverse Cuthill-McKee order has no fill outside its band), the carried rows are
//     dense rows of n entries at wbase + (r - n) * ld.
struct WPanel { int base, ld, n, nreg, nvec, npos, bw, vrow, band, ldb, wbase; };    // bw: half bandwidth the factorisation works with (n - 1: dense); vrow: index of the first vector row

// The descriptor fields are the same in every lane but come from LDS (per-lane loads): without this the
// compiler has to treat every loop bound of the routines below as divergent (exec-masked regions
// instead of scalar branches, broadcast values spilled across them).
__device__ __forceinline__ WPanel wpanel_uniform(const WPanel& Q) {
  WPanel P;
  P.base = __builtin_amdgcn_readfirstlane(Q.base); P.ld = __builtin_amdgcn_readfirstlane(Q.ld);
  P.n = __builtin_amdgcn_readfirstlane(Q.n);
  P.nreg = __builtin_amdgcn_readfirstlane(Q.nreg); P.nvec = __builtin_amdgcn_readfirstlane(Q.nvec);
  P.npos = __builtin_amdgcn_readfirstlane(Q.npos); P.bw = __builtin_amdgcn_readfirstlane(Q.bw);
  P.vrow = __builtin_amdgcn_readfirstlane(Q.vrow); P.band = __builtin_amdgcn_readfirstlane(Q.band);
  P.ldb = __builtin_amdgcn_readfirstlane(Q.ldb); P.wbase = __builtin_amdgcn_readfirstlane(Q.wbase);
  return P;
}

// The leaf instances sized to the hyperplane leaves of the headline class (order 36, half bandwidth 5 in reverse
// Cuthill-McKee order): a leaf takes them iff it fits both bounds (n, bw: wave-uniform descriptor fields).
#define OMGX_LEAF_COLS_SMALL 36
#define OMGX_LEAF_BW_SMALL   5
__host__ __device__ __forceinline__ bool wave_leaf_small(int n, int bw) { return n <= OMGX_LEAF_COLS_SMALL && bw <= OMGX_LEAF_BW_SMALL; }

// start of carried row r >= n (a dense row of n entries)
template <bool BANDED>
__device__ __forceinline__ int wcarried(const WPanel& P, int r) {
  return BANDED ? P.wbase + (r - P.n) * P.ld : P.base + ((r * (r + 1)) >> 1);
}
// offset such that entry (i, k) of the symmetric block sits at wsym(P, i) + k (banded: only i - band <= k <= i exist)
template <bool BANDED>
__device__ __forceinline__ int wsym(const WPanel& P, int i) {
  return BANDED ? P.base + i * P.ldb + P.band - i : P.base + ((i * (i + 1)) >> 1);
}

// All dynamic LDS of the workgroup (HIP: every `extern __shared__` array starts at the same address): the
// out-of-line routines below take offsets into it, so that their accesses stay ds_* instructions (a
// pointer argument would be a generic pointer: flat_* instructions).
extern __shared__ double omgx_lds[];

// In-place LDL' of a panel by one wave, the matrix in registers: lane i holds row i, a[k] = A[i][k].
// Straight-line code: all NC columns are processed whatever the order n is (the columns >= n work on
// garbage that is never stored and raise no flag), the half bandwidth BW is a compile-time bound (columns further than
// BW right of the pivot are skipped: u_kj = 0 there, nothing to subtract from any row), so all register
// indices and all broadcast lanes are constants and there is no branch inside the factorisation --
// every run-time loop bound tried (uniform scalar branches per chunk, rolled block loops with a shifting
// register window and run-time broadcast lanes) made the compiler hoist, spill or relocate the chunks,
// at 30-40 cycles per broadcast-and-FMA instead of the 12 of this form (tools/micro/bcast.hip: two
// v_readlane + one fp64 FMA).  Details that matter (each measured on the device):
//   * the descriptor must be provably wave-uniform (wpanel_uniform);
//   * the four FMAs of a chunk are pinned behind their broadcasts by an empty volatile asm: without it
//     the compiler issues the broadcasts of a whole column first and spills their SGPRs (v_writelane);
//   * lane masks are formed from a laundered lane id where they are used, otherwise all NC of them are
//     hoisted to the top and spilled;
//   * a pivot of the wrong sign is only recorded; the caller looks at the flag at the end (the panel is
//     garbage then, but nothing traps).
// On return the panel holds U = L D (rows < n, lower part and diagonal) / W = B L^{-T} (carried rows), the
// vector rows are stored forward-substituted.  Returns 1 if a pivot had the wrong sign.  `off`: offset of
// the KKT store in the dynamic LDS (doubles).  BANDED: storage form of the panel (WPanel).  NVEC: vector rows the instance
// carries (1: the root, which has its right-hand side alone; 2: a leaf) -- a row it does not carry costs nothing.
// Instances: <40, 40, false, 1> the root; <40, 40, true, 2> and <40, 8, true, 2> leaves of any order / of half bandwidth
// <= 8; <36, 5, true, 2> hyperplane leaves of order <= 36 and half bandwidth <= 5 (wave_leaf_small: the headline class --
// four columns, and three broadcast-and-FMA pairs per pivot, fewer than <40, 8>; the entries skipped are exact zeros of
// the band, so every stored entry sees the same operands in the same order).
template <int NC, int BW, bool BANDED, int NVEC>
__device__ __forceinline__ int wave_ldl(int off, const WPanel Pin) {
  static_assert(NC % 4 == 0 && NVEC >= 1 && NVEC <= 2, "columns go in chunks of four; one or two vector rows");
  const double* A = omgx_lds + off;
  double* Aw = omgx_lds + off;
  const WPanel P = wpanel_uniform(Pin);
  const int lane = threadIdx.x & 63;
  const int n = P.n;
  const bool has_row = lane < P.nreg;
  const bool sym_row = lane < n;                       // a row of the symmetric block: only its lower part is stored
  const int rl = has_row ? lane : 0;
  const int ra = rl < n ? wsym<BANDED>(P, rl) : wcarried<BANDED>(P, rl);
  // stored columns of this lane's row: [klo, khi]
  const int klo = (BANDED && rl < n && rl > P.band) ? rl - P.band : 0;
  const int khi = rl < n ? rl : n - 1;
  double a[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {                       // unconditional loads (all in flight), masked afterwards
    const int kk = k < klo ? klo : (k > khi ? khi : k);
    const double v = A[ra + kk];
    a[k] = (has_row && k >= klo && k <= khi) ? v : 0.0;
  }
  const int v0a = wcarried<BANDED>(P, P.vrow), v1a = wcarried<BANDED>(P, P.vrow + (NVEC > 1 && P.nvec > 1 ? 1 : 0));
  double yv0, yv1 = 0.0;
  {
    const int c = sym_row ? lane : 0;
    const double v0 = A[v0a + c];
    yv0 = (P.nvec > 0 && sym_row) ? v0 : 0.0;
    if (NVEC > 1) {
      const double v1 = A[v1a + c];
      yv1 = (P.nvec > 1 && sym_row) ? v1 : 0.0;
    }
  }
  unsigned bad = 0;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    // the pivot as the two scalar words the broadcast leaves: its sign is tested on the scalar unit, beside the chain
    // (rcp -> l_ij -> the FMAs of the column) and not in front of it
    const int dlo = __builtin_amdgcn_readlane(__double2loint(a[j]), j), dhi = __builtin_amdgcn_readlane(__double2hiint(a[j]), j);
    const double dj = __hiloint2double(dhi, dlo);
    bad = pivot_wrong_sign(bad, dhi, dlo, j, P.npos, n);      // (columns >= n: padding, whatever they compute is never stored)
    const double inv = rcp_pivot(dj);
    const double li = a[j] * inv;                      // l_ij of every row i > j (lanes <= j: unused upper part)
    {
      // the vector rows live on the lanes of the block rows: only rows below the pivot take part
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const double lm = ln > j ? li : 0.0;
      // (columns >= n broadcast zero: their garbage may hold NaN, and 0 * NaN would reach the real lanes)
      const double y0j = readlane_d(yv0, j);
      yv0 = fma(-lm, j < n ? y0j : 0.0, yv0);
      if (NVEC > 1) {
        const double y1j = readlane_d(yv1, j);
        yv1 = fma(-lm, j < n ? y1j : 0.0, yv1);
      }
    }
#pragma unroll
    for (int c = j / 4; c < NC / 4; ++c) {             // columns in chunks of four
      if (4 * c > j + BW) continue;                    // (compile time)
      double s[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] = readlane_d(a[j], 4 * c + q);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = 4 * c + q;
        if (k > j && k <= j + BW) a[k] = fma(-li, s[q], a[k]);
      }
      asm volatile("" : "+v"(a[4 * c]), "+v"(a[4 * c + 1]), "+v"(a[4 * c + 2]), "+v"(a[4 * c + 3]));
    }
  }
  if (!bad) {
    if (has_row) {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        // (a row of the symmetric block: its stored part [klo, lane]; a carried row: all n columns -- [klo, khi] either
        // way, so the order n takes no part in the decision: no wave-uniform k < n kept as a lane mask per column)
        const int kh = sym_row ? ln : khi;
        if (k >= klo && k <= kh) Aw[ra + k] = a[k];
      }
    }
    if (sym_row) {
      if (P.nvec > 0) Aw[v0a + lane] = yv0;
      if (NVEC > 1 && P.nvec > 1) Aw[v1a + lane] = yv1;
    }
  }
  return (int)bad;
}

// inverse pivot of column `lane`, read back from the stored diagonal (after wave_ldl + wave_fence)
template <bool BANDED>
__device__ __forceinline__ double wave_dinv(const double* A, const WPanel P) {
  const int lane = threadIdx.x & 63;
  const int c = lane < P.n ? lane : 0;
  const double d = A[wsym<BANDED>(P, c) + c];
  return lane < P.n ? rcp_pivot(d) : 0.0;
}

// x <- L^{-T} z for the factor stored in the panel (U = L D in LDS, left by wave_ldl): lane j reads
// column j (u_ij, i > j), scales it by its own inverse pivot and the wave substitutes backwards with one
// broadcast per row.  z: component `lane` (lanes >= n ignored); returns x_lane.
// The two halves are routines of their own: the operands (column `lane` of L', scaled) depend on the factor alone, so a wave
// may hold them in registers before z exists (kkt_root_solve_wave, omgx_core.h: a leaf wave loads them while wave 0 has the
// root).  P: wave-uniform (wpanel_uniform).  lt: NA >= NC registers, the first NC are written / read.
template <int NC, bool BANDED, int NA>
__device__ __forceinline__ void wave_bwd_load(int off, const WPanel& P, double dinvl, double (&lt)[NA]) {
  static_assert(NA >= NC, "room for NC operands");
  const double* A = omgx_lds + off;
  const int lane = threadIdx.x & 63;
  const int n = P.n;
  const int c = lane < n ? lane : 0;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int ic = i < n ? i : n - 1;
    // (banded: entry (i, c) exists for i - c <= band; outside the band the factor is zero)
    const bool in = !BANDED || ic - c <= P.band;
    const int cc = in ? c : ic - P.band;
    const double v = A[wsym<BANDED>(P, ic) + cc];
    lt[i] = (i < n && lane < i && in) ? v * dinvl : 0.0;
  }
}
template <int NC, int NA>
__device__ __forceinline__ double wave_bwd_chain(int n, const double (&lt)[NA], double z) {
  const int lane = threadIdx.x & 63;
  double x = lane < n ? z : 0.0;
#pragma unroll
  for (int i = NC - 1; i >= 1; --i) {
    if (i < n) x = fma(-lt[i], readlane_d(x, i), x);
  }
  return x;
}
template <int NC, bool BANDED>
__device__ __forceinline__ double wave_bwd(int off, const WPanel Pin, double dinvl, double z) {
  const WPanel P = wpanel_uniform(Pin);
  double lt[NC];
  wave_bwd_load<NC, BANDED>(off, P, dinvl, lt);
  return wave_bwd_chain<NC>(P.n, lt, z);
}

// Substitutions for a right-hand side that did NOT ride through the factorisation (second-order correction of a trial
// step: one more solve with the factors of the iteration).  Rolled forms -- a run-time loop over chunks of eight columns,
// the broadcast lane a scalar register -- on purpose: they are called from inside the line search, where the scalars of
// the step are alive on top of the iteration's, and n steps of ~15 cycles do not need the straight-line treatment of the
// n^2 / 2 steps of wave_ldl (a second fully unrolled instance of wave_bwd there cost 35 KB of code and spilled).
//
// wave_fwd_r: y <- L^{-1} r.  Lane i reads row i of the symmetric block (u_ij, j < i), scales column j by the inverse
// pivot of lane j (dinvl: lane c holds 1 / d_c).  r: component `lane` (lanes >= n ignored); returns y_lane.
template <bool BANDED>
__device__ __forceinline__ double wave_fwd_r(int off, const WPanel Pin, double dinvl, double r) {
  const double* A = omgx_lds + off;
  const WPanel P = wpanel_uniform(Pin);
  const int lane = threadIdx.x & 63;
  const int n = P.n;
  const int rl = lane < n ? lane : 0;
  const int ra = wsym<BANDED>(P, rl);
  const int klo = (BANDED && rl > P.band) ? rl - P.band : 0;
  double y = lane < n ? r : 0.0;
  for (int j0 = 0; j0 < n; j0 += 8) {
    double l[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {                      // unconditional loads on clamped addresses, masked afterwards
      const int j = j0 + q;
      const int kk = j < klo ? klo : (j > rl ? rl : j);
      const double v = A[ra + kk];
      const double dk = readlane_d(dinvl, j);          // (j < 48: n <= OMGX_WAVE_COLS)
      l[q] = (lane < n && j >= klo && j < rl) ? v * dk : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int j = j0 + q;
      const double yj = readlane_d(y, j);
      y = fma(-l[q], j < n ? yj : 0.0, y);
    }
  }
  return y;
}

// wave_bwd_r: x <- L^{-T} z, the rolled twin of wave_bwd (lane j reads column j and scales it by its own inverse pivot)
template <bool BANDED>
__device__ __forceinline__ double wave_bwd_r(int off, const WPanel Pin, double dinvl, double z) {
  const double* A = omgx_lds + off;
  const WPanel P = wpanel_uniform(Pin);
  const int lane = threadIdx.x & 63;
  const int n = P.n;
  const int c = lane < n ? lane : 0;
  double x = lane < n ? z : 0.0;
  for (int i0 = ((n + 7) & ~7) - 8; i0 >= 0; i0 -= 8) {
    double l[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = i0 + q;
      const int ic = i < n ? i : n - 1;
      const bool in = !BANDED || ic - c <= P.band;     // (banded: entry (i, c) exists for i - c <= band)
      const int cc = in ? c : ic - P.band;
      const double v = A[wsym<BANDED>(P, ic) + cc];
      l[q] = (i < n && lane < i && in) ? v * dinvl : 0.0;
    }
#pragma unroll
    for (int q = 7; q >= 0; --q) {
      const int i = i0 + q;
      const double xi = readlane_d(x, i);
      x = fma(-l[q], i < n ? xi : 0.0, x);
    }
  }
  return x;
}

}  // namespace omgx
