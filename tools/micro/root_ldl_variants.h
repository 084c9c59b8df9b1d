// Developer experiment (round 5, NOT part of the product; profiles/r05_micro_root_ldl.txt): the packed root block in panels of
// 16 columns -- each factorised in registers like wave_ldl, the rank-16 update of the columns right of it on the matrix pipe
// (v_mfma_f64_16x16x4), operands and result tiles changing layout through 240 doubles of LDS scratch at `soff`:
//   [0, 96)     the current four panel columns of the rows below the panel, row-major (stride 4)
//   [96, 112)   inverse pivots of the panel's columns
//   [112, 240)  half a result tile (8 rows x 16)
// Same contract as wave_ldl<NC, NC, false>.  Correct (<= 3e-15 against a host LDL'), and no faster: kept for the record.
#pragma once
namespace omgx {
// wave_ldl as it stood before the instances sized to the plan (all NC columns whatever the order, two vector rows in every
// instance, the pivot's sign tested with fp64 compares on the vector pipe): what the instances of omgx_wave.h must
// reproduce to the bit.  Same contract as wave_ldl<NC, BW, BANDED, 2>.
template <int NC, int BW, bool BANDED>
__device__ __forceinline__ int wave_ldl_ref(int off, const WPanel Pin) {
  const double* A = omgx_lds + off;
  double* Aw = omgx_lds + off;
  const WPanel P = wpanel_uniform(Pin);
  const int lane = threadIdx.x & 63;
  const int n = P.n;
  const bool has_row = lane < P.nreg;
  const bool sym_row = lane < n;
  const int rl = has_row ? lane : 0;
  const int ra = rl < n ? wsym<BANDED>(P, rl) : wcarried<BANDED>(P, rl);
  const int klo = (BANDED && rl < n && rl > P.band) ? rl - P.band : 0;
  const int khi = rl < n ? rl : n - 1;
  double a[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int kk = k < klo ? klo : (k > khi ? khi : k);
    const double v = A[ra + kk];
    a[k] = (has_row && k >= klo && k <= khi) ? v : 0.0;
  }
  const int v0a = wcarried<BANDED>(P, P.vrow), v1a = wcarried<BANDED>(P, P.vrow + (P.nvec > 1 ? 1 : 0));
  double yv0, yv1;
  {
    const int c = sym_row ? lane : 0;
    const double v0 = A[v0a + c], v1 = A[v1a + c];
    yv0 = (P.nvec > 0 && sym_row) ? v0 : 0.0;
    yv1 = (P.nvec > 1 && sym_row) ? v1 : 0.0;
  }
  int bad = 0;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const double dj = readlane_d(a[j], j);
    const bool okp = (j < P.npos) ? (dj > 0.0) : (dj < 0.0);
    bad |= (j < n && !okp) ? 1 : 0;
    const double inv = rcp_pivot(dj);
    const double li = a[j] * inv;
    {
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const double lm = ln > j ? li : 0.0;
      const double y0j = readlane_d(yv0, j), y1j = readlane_d(yv1, j);
      yv0 = fma(-lm, j < n ? y0j : 0.0, yv0);
      yv1 = fma(-lm, j < n ? y1j : 0.0, yv1);
    }
#pragma unroll
    for (int c = j / 4; c < NC / 4; ++c) {
      if (4 * c > j + BW) continue;
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
        if (k < n && (sym_row ? (k <= ln && k >= klo) : true)) Aw[ra + k] = a[k];
      }
    }
    if (sym_row) {
      if (P.nvec > 0) Aw[v0a + lane] = yv0;
      if (P.nvec > 1) Aw[v1a + lane] = yv1;
    }
  }
  return bad;
}

template <int NC>
__device__ __forceinline__ int wave_ldl_packed16(int off, const WPanel Pin, int soff) {
  typedef double v4d __attribute__((ext_vector_type(4)));
  const double* A = omgx_lds + off;
  double* Aw = omgx_lds + off;
  double* S = omgx_lds + soff;
  const WPanel P = wpanel_uniform(Pin);
  const int lane = threadIdx.x & 63;
  const int n = P.n;
  const bool has_row = lane < P.nreg;
  const int rl = has_row ? lane : 0;
  const int ra = wsym<false>(P, rl < n ? rl : 0);
  const int khi = rl < n ? rl : n - 1;
  double a[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int kk = k > khi ? khi : k;
    const double v = A[ra + kk];
    a[k] = (has_row && rl < n && k <= khi) ? v : 0.0;
  }
  const int v0a = wcarried<false>(P, P.vrow);
  double yv0;
  {
    const int c = lane < n ? lane : 0;
    const double v0 = A[v0a + c];
    yv0 = (P.nvec > 0 && lane < n) ? v0 : 0.0;
  }
  int bad = 0;
#pragma unroll
  for (int c0 = 0; c0 < NC; c0 += 16) {
    const int c1 = c0 + 16 < NC ? c0 + 16 : NC;
#pragma unroll
    for (int j = c0; j < c1; ++j) {
      const double dj = readlane_d(a[j], j);
      const bool okp = (j < P.npos) ? (dj > 0.0) : (dj < 0.0);
      bad |= (j < n && !okp) ? 1 : 0;
      const double inv = rcp_pivot(dj);
      const double li = a[j] * inv;
      {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const double lm = ln > j ? li : 0.0;
        const double y0j = readlane_d(yv0, j);
        yv0 = fma(-lm, j < n ? y0j : 0.0, yv0);
        if (ln == 0) S[96 + (j - c0)] = (j < n) ? inv : 0.0;
      }
#pragma unroll
      for (int c = j / 4; c < (c1 + 3) / 4; ++c) {
        double s[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = readlane_d(a[j], 4 * c + q);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = 4 * c + q;
          if (k > j && k < c1) a[k] = fma(-li, s[q], a[k]);
        }
        asm volatile("" : "+v"(a[4 * c]), "+v"(a[4 * c + 1]), "+v"(a[4 * c + 2]), "+v"(a[4 * c + 3]));
      }
    }
#ifndef OMGX_DBG_SKIP_TRAIL
    if (c1 < NC) {
      const int NT = (NC - c1 + 15) / 16;
      v4d acc[3];
#pragma unroll
      for (int t = 0; t < 3; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
      const int r16 = lane & 15, kq = lane >> 4;
#pragma unroll
      for (int kb = 0; kb < (c1 - c0) / 4; ++kb) {
        wave_fence();
        {
          int ln = lane;
          asm volatile("" : "+v"(ln));
          const int row = ln - c1;
          if (row >= 0 && ln < n) {
#pragma unroll
            for (int q = 0; q < 4; ++q) S[row * 4 + q] = a[c0 + 4 * kb + q];
          }
        }
        wave_fence();
        const double dk = S[96 + 4 * kb + kq];
        double u[2], l[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int row = 16 * b + r16;
          const bool on = b < NT && c1 + row < n;
          const double v = S[(on ? row : 0) * 4 + kq];
          u[b] = on ? v : 0.0;
          l[b] = u[b] * dk;
        }
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(l[0], u[0], acc[0], 0, 0, 0);
        if (NT > 1) {
          acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(l[1], u[0], acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(l[1], u[1], acc[2], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        if (t > 0 && NT < 2) continue;
        const int rb = t == 0 ? 0 : 1, cb = t == 2 ? 1 : 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (c1 + 16 * rb + 8 * h >= NC) continue;
          wave_fence();
          S[112 + (kq + 0) * 16 + r16] = acc[t][2 * h];
          S[112 + (kq + 4) * 16 + r16] = acc[t][2 * h + 1];
          wave_fence();
          int ln = lane;
          asm volatile("" : "+v"(ln));
          const int rr = ln - (c1 + 16 * rb + 8 * h);
          const bool mine = rr >= 0 && rr < 8 && ln < n;
          const double* Drow = S + 112 + (mine ? rr : 0) * 16;
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            const int k = c1 + 16 * cb + c;
            if (k < NC) {
              const double dv = Drow[c];
              a[k] = (mine && k <= ln) ? a[k] - dv : a[k];
            }
          }
        }
      }
    }
#endif
  }
  if (!bad) {
    if (has_row && rl < n) {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        if (k < n && k <= ln) Aw[ra + k] = a[k];
      }
    }
    if (lane < n && P.nvec > 0) Aw[v0a + lane] = yv0;
  }
  return bad;
}

// Round 6: the packed root block by FOUR waves.  wave_ldl<40, 40, false> on one wave is a chain of 39 pivots at ~770 cycles each (two
// v_readlane + one FMA per pair, 741 pairs, three waves parked: 35 k of the 76 k factorisation cycles of a solve).  Here the columns are
// dealt round-robin to the waves (wave w holds columns w, w + 4, ...: NC / 4 registers per lane, lane i = row i as before); per pivot
// the owner publishes its column and the reciprocal of its pivot in LDS (double-buffered: ONE workgroup barrier per pivot), every wave reads its
// row's entry and the reciprocal, and the entries u_jk of its own columns as broadcast reads (all lanes one address: no v_readlane, no scalar-register traffic),
// and updates its <= NC / 4 columns.  The arithmetic of every stored entry is that of wave_ldl -- a_ik <- fma(-(a_ij / d_j), u_kj, a_ik), the
// pivots in the same order, the right-hand-side row as a lane vector updated with the same operands (kept by every wave) -- so the
// factor is the SAME BITS.  All threads of the workgroup call it (waves beyond the fourth only take part in the barriers); `xoff`:
// offset of 145 doubles of exchange buffer in the dynamic LDS; returns 1 (in every thread) if a pivot had the wrong sign -- nothing is
// stored then -- and ends with a barrier (the factor is visible to the workgroup).
// (W: this wave's index as a compile-time constant -- which columns it holds, whether it publishes the next one: nothing is decided at
// run time but k < n; with the wave index in a register every pivot was a thicket of scalar branches, 730 cycles instead of 600 for the
// un-pipelined form.  W = 4: a wave beyond the fourth, barriers only.)
template <int NC, int W>
__device__ __forceinline__ int root_ldl_4w_wave(int off, const WPanel P, int xoff) {
  constexpr int NL = NC / 4;
  constexpr int BS = 72;                               // a buffer: [0, 64) the column, [64] the reciprocal of its pivot
  constexpr bool act = W < 4;
  const double* A = omgx_lds + off;
  double* Aw = omgx_lds + off;
  double* X = omgx_lds + xoff;
  const int lane = threadIdx.x & 63;
  const int n = P.n;
  const bool has_row = lane < n;                       // (the root has no carried register rows: nreg == n)
  const int rl = has_row ? lane : 0;
  const int ra = wsym<false>(P, rl);
  double a[NL];
#pragma unroll
  for (int c = 0; c < NL; ++c) {                       // unconditional loads (all in flight), masked afterwards
    const int j = 4 * c + (act ? W : 0);
    const int jj = j > rl ? rl : j;
    const double v = A[ra + jj];
    a[c] = (has_row && j <= rl) ? v : 0.0;
  }
  const int v0a = wcarried<false>(P, P.vrow);
  double yv0;
  {
    const double v0 = A[v0a + rl];
    yv0 = (P.nvec > 0 && has_row) ? v0 : 0.0;
  }
  int bad = 0;
  if (W == 0) {
    X[lane] = a[0];
    const double d0 = readlane_d(a[0], 0);
    if (lane == 0) X[64] = rcp_pivot(d0);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    if (k < n) {                                        // (wave-uniform; the only run-time decision)
      const double* buf = X + (k & 1) * BS;
      double* nxt = X + ((k + 1) & 1) * BS;
      if (act) {
        const bool pub = (k + 1 < NC) && (((k + 1) & 3) == W);      // (compile time) this wave owns column k + 1
        const int c1 = pub ? (k + 1) >> 2 : 0;
        const double colk = buf[lane], inv = buf[64], s1 = buf[pub ? k + 1 : 0], dk = buf[k];
        const double li = colk * inv;
        if (pub) {                                      // the next pivot's column first, published at once (with the reciprocal of its pivot)
          a[c1] = fma(-li, s1, a[c1]);
          nxt[lane] = a[c1];
          const double d1 = readlane_d(a[c1], k + 1);
          if (lane == 0) nxt[64] = rcp_pivot(d1);
        }
        const bool okp = (k < P.npos) ? (dk > 0.0) : (dk < 0.0);
        bad |= okp ? 0 : 1;
        {
          int ln = lane;
          asm volatile("" : "+v"(ln));
          const double lm = ln > k ? li : 0.0;
          const double y0k = readlane_d(yv0, k);
          yv0 = fma(-lm, y0k, yv0);
        }
#pragma unroll
        for (int c = k >> 2; c < NL; ++c) {
          const int j = 4 * c + W;
          if (j > k + 1) {                              // (compile time; column k + 1: done above by its owner)
            const double s = buf[j];                    // u_jk: every lane reads the same address
            a[c] = fma(-li, s, a[c]);
          }
        }
      }
      __syncthreads();
    }
  }
  if (!bad && act) {
    if (has_row) {
#pragma unroll
      for (int c = 0; c < NL; ++c) {
        const int j = 4 * c + W;
        if (j < n && j <= lane) Aw[ra + j] = a[c];
      }
    }
    if (W == 0 && has_row && P.nvec > 0) Aw[v0a + lane] = yv0;
  }
  // (every wave saw the same pivots: `bad` is the same in all of them; waves beyond the fourth learn it through the buffer)
  if (W == 0 && lane == 0) X[2 * BS] = bad ? 1.0 : 0.0;
  __syncthreads();
  const int bad_all = X[2 * BS] != 0.0 ? 1 : 0;
  __syncthreads();
  return bad_all;
}

template <int NC>
__device__ __forceinline__ int root_ldl_4w(int off, const WPanel Pin, int xoff) {
  static_assert(NC % 4 == 0, "columns are dealt to four waves");
  const WPanel P = wpanel_uniform(Pin);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  switch (wv) {
    case 0: return root_ldl_4w_wave<NC, 0>(off, P, xoff);
    case 1: return root_ldl_4w_wave<NC, 1>(off, P, xoff);
    case 2: return root_ldl_4w_wave<NC, 2>(off, P, xoff);
    case 3: return root_ldl_4w_wave<NC, 3>(off, P, xoff);
    default: return root_ldl_4w_wave<NC, 4>(off, P, xoff);
  }
}
}  // namespace omgx
