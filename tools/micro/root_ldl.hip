// Developer micro-benchmark (not part of the product): the packed root block of the KKT store factorised by one wave --
// wave_ldl<40, 40, false> (column by column in registers) against wave_ldl_packed16<40> (panels of 16, trailing updates on the
// matrix pipe) -- on random quasi-definite matrices of run-time order n <= 40 with a right-hand-side row, checked against a
// plain host LDL' and timed alone and with a second workgroup on the CU (256 threads each, like the solve kernel).
// The root instance carries one vector row (wave_ldl<40, 40, false, 1>) and tests the pivots' signs on the scalar unit; "two
// vector rows (before)" is the routine as it stood (wave_ldl_ref, root_ldl_variants.h), whose bits it must reproduce.
// The leaf case (k_leaf, leaf_cases): banded panels of order 8 .. 36, half bandwidth 1 and 5, with 0 and 28 carried rows and two
// vector rows, through the instance of 40 columns and band 8 as it stood, the same with the scalar sign test, and the instance
// of 36 columns and band 5 -- cycles of factorisation + inverse pivots + backward substitution, "same bits: yes / no" against
// the first, and a pivot of the wrong sign, a zero pivot and a NaN pivot, which every instance must flag without storing.
// Exits non-zero on any "no".
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "../../omg-tools_amd/csrc/omgx_core.h"
#include "root_ldl_variants.h"
using namespace omgx;

__global__ __launch_bounds__(256) void k_root(const double* in, double* out, long long* cyc, int reps, int n, int npos, int blocked) {
  extern __shared__ double lds[];
  const int total = (n + 1) * (n + 2) / 2;
  double* kkt = lds;                       // offset 0 of the dynamic LDS
  const int soff = 1024;                   // scratch behind the block
  const int wave = threadIdx.x >> 6;
  long long t_sum = 0; int bad_any = 0;
  for (int rep = 0; rep < reps; ++rep) {
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += blockDim.x) kkt[i] = in[i];
    __syncthreads();
    const long long t0 = clock64();
    WPanel P; P.base = 0; P.ld = 0; P.n = n; P.nreg = n; P.nvec = 1; P.npos = npos; P.bw = n; P.vrow = n; P.band = -1; P.ldb = 0; P.wbase = 0;
    if (blocked == 2) bad_any |= root_ldl_4w<OMGX_WAVE_COLS>(0, P, soff);      // (round 6: all four waves)
    else if (wave == 0) {
      // (3: the root instance as it stood with two vector rows and the fp64 sign test, root_ldl_variants.h)
      bad_any |= blocked == 3 ? wave_ldl_ref<OMGX_WAVE_COLS, OMGX_WAVE_COLS, false>(0, P)
                 : (blocked ? wave_ldl_packed16<OMGX_WAVE_COLS>(0, P, soff) : wave_ldl<OMGX_WAVE_COLS, OMGX_WAVE_COLS, false, 1>(0, P));
      wave_fence();
    }
    const long long t1 = clock64();
    __syncthreads();
    if (rep >= reps / 2) t_sum += t1 - t0;
  }
  if (blockIdx.x == 0) for (int i = threadIdx.x; i < total; i += blockDim.x) out[i] = kkt[i];
  if (threadIdx.x == 0) { cyc[2 * blockIdx.x] = t_sum / (reps - reps / 2); cyc[2 * blockIdx.x + 1] = bad_any; }
}

// The leaf case: a banded panel (half bandwidth `band`, row stride band + 1) with `ncar` carried register rows and two vector rows,
// one copy per wave (four waves factorise at once, as the leaf waves of a solve do), through
//   which 0: wave_ldl_ref<40, 8, true> (the routine as it stood), backward substitution on 40 positions
//   which 1: wave_ldl<40, 8, true, 2>, backward substitution on 40 positions
//   which 2: wave_ldl<36, 5, true, 2>, backward substitution on 36 positions        (n <= 36, band <= 5)
// followed by wave_dinv and wave_bwd on the factor.  out: the panel of wave 0 and the substituted vector behind it.
#define LEAF_STRIDE 1536
__global__ __launch_bounds__(256) void k_leaf(const double* in, double* out, long long* cyc, int reps, int n, int band, int ncar, int npos, int which) {
  extern __shared__ double lds[];
  const int ldb = band + 1, total = n * ldb + (ncar + 2) * n;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int off = wave * LEAF_STRIDE;
  long long t_sum = 0; int bad_any = 0;
  double x = 0.0;
  for (int rep = 0; rep < reps; ++rep) {
    __syncthreads();
    for (int i = lane; i < total; i += 64) lds[off + i] = in[i];
    __syncthreads();
    const long long t0 = clock64();
    WPanel P; P.base = 0; P.ld = n; P.n = n; P.nreg = n + ncar; P.nvec = 2; P.npos = npos; P.bw = band; P.vrow = n + ncar; P.band = band; P.ldb = ldb; P.wbase = n * ldb;
    int bad;
    if (which == 0) bad = wave_ldl_ref<OMGX_WAVE_COLS, 8, true>(off, P);
    else if (which == 1) bad = wave_ldl<OMGX_WAVE_COLS, 8, true, 2>(off, P);
    else bad = wave_ldl<OMGX_LEAF_COLS_SMALL, OMGX_LEAF_BW_SMALL, true, 2>(off, P);
    wave_fence();
    const double dl = wave_dinv<true>(lds + off, P);
    const double z = lds[off + wcarried<true>(P, P.vrow + 1) + (lane < n ? lane : 0)] * dl;
    x = which == 2 ? wave_bwd<OMGX_LEAF_COLS_SMALL, true>(off, P, dl, z) : wave_bwd<OMGX_WAVE_COLS, true>(off, P, dl, z);
    const long long t1 = clock64();
    bad_any |= bad;
    __syncthreads();
    if (rep >= reps / 2) t_sum += t1 - t0;
  }
  if (blockIdx.x == 0 && wave == 0) {
    for (int i = lane; i < total; i += 64) out[i] = lds[i];
    out[total + lane] = (lane < n && !bad_any) ? x : 0.0;
  }
  if (threadIdx.x == 0) { cyc[2 * blockIdx.x] = t_sum / (reps - reps / 2); cyc[2 * blockIdx.x + 1] = bad_any; }
}

// the integer sign test of omgx_wave.h against the fp64 compares it replaces, on the host: the edge cases and random bit patterns
static int check_sign_test() {
  long bad = 0;
  unsigned long long s = 88172645463325252ull;
  auto check = [&](unsigned long long b) {
    double d; memcpy(&d, &b, 8);
    for (int j = 0; j < 3; ++j) for (int npos = 0; npos < 3; ++npos) for (int n = 0; n < 4; ++n) {
      const bool okp = (j < npos) ? (d > 0.0) : (d < 0.0);
      if ((j < n && !okp) != (pivot_wrong_sign(0u, (int)(b >> 32), (int)(b & 0xffffffffu), j, npos, n) != 0)) ++bad;
    }
  };
  const unsigned long long edge[] = {0ull, 1ull, 0xffffffffull, 0x100000000ull, 0x000fffffffffffffull, 0x0010000000000000ull, 0x3ff0000000000000ull,
                                     0x7fefffffffffffffull, 0x7ff0000000000000ull, 0x7ff0000000000001ull, 0x7ff0000100000000ull, 0x7ff8000000000000ull, 0x7fffffffffffffffull};
  for (unsigned long long e : edge) { check(e); check(e | 0x8000000000000000ull); }
  for (int i = 0; i < 1000000; ++i) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    check(s); check((s & 0x800fffffffffffffull) | 0x7ff0000000000000ull); check(s & 0x800fffffffffffffull); check(s & 0xffffffff00000000ull);
  }
  printf("integer sign test against (j < npos ? d > 0 : d < 0), +-0, denormals, +-inf, NaN and 4 M random patterns: %ld mismatches\n", bad);
  return bad ? 1 : 0;
}

static int leaf_cases() {
  int rc = 0;
  const int ns[5] = {8, 9, 33, 35, 36}, bands[2] = {1, 5}, ncars[2] = {0, 28};
  const int nb_max = 512, cap = LEAF_STRIDE + 64;
  double *d_in, *d_out; long long* d_cyc;
  hipMalloc(&d_in, cap * 8); hipMalloc(&d_out, cap * 8); hipMalloc(&d_cyc, nb_max * 2 * sizeof(long long));
  const size_t lds = 4 * LEAF_STRIDE * 8;
  hipFuncSetAttribute((const void*)k_leaf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  for (int in_ = 0; in_ < 5; ++in_) for (int ib = 0; ib < 2; ++ib) for (int ic = 0; ic < 2; ++ic) {
    const int n = ns[in_], band = bands[ib], ncar = ncars[ic], ldb = band + 1, npos = n - 2;
    const int total = n * ldb + (ncar + 2) * n;
    unsigned s = 4242 + 97 * n + 7 * band + ncar;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0 - 0.5; };
    std::vector<double> in(total, 0.0);
    for (int i = 0; i < n; ++i) for (int k = (i > band ? i - band : 0); k <= i; ++k)
      in[i * ldb + band - i + k] = (i == k) ? ((i < npos) ? 7.0 + rnd() : -(7.0 + rnd())) : 0.4 * rnd();
    for (int i = n * ldb; i < total; ++i) in[i] = rnd();
    // pivot cases: the panel as it is, then its first pivot (the stored diagonal of column 0) of the wrong sign, zero, NaN:
    // every instance must raise the flag and leave the store as it was
    for (int pc = 0; pc < 4; ++pc) {
      std::vector<double> inp = in;
      if (pc == 1) inp[band] = -3.0;
      if (pc == 2) inp[band] = 0.0;
      if (pc == 3) inp[band] = nan("");
      hipMemcpy(d_in, inp.data(), total * 8, hipMemcpyHostToDevice);
      std::vector<double> first;
      long long bad_first = 0;
      for (int which = 0; which < 3; ++which) {
        for (int nb = 256; nb <= (pc == 0 ? 512 : 256); nb += 256) {
          hipMemset(d_out, 0, cap * 8);
          hipLaunchKernelGGL(k_leaf, dim3(nb), dim3(256), lds, 0, d_in, d_out, d_cyc, pc == 0 ? 16 : 2, n, band, ncar, npos, which);
          const hipError_t e = hipDeviceSynchronize();
          std::vector<double> out(total + 64); std::vector<long long> cyc(nb * 2);
          hipMemcpy(out.data(), d_out, (total + 64) * 8, hipMemcpyDeviceToHost);
          hipMemcpy(cyc.data(), d_cyc, nb * 2 * sizeof(long long), hipMemcpyDeviceToHost);
          double c = 0; long long bad = 0;
          for (int i = 0; i < nb; ++i) { c += cyc[2 * i]; bad |= cyc[2 * i + 1]; }
          if (which == 0 && nb == 256) { first = out; bad_first = bad; }
          const bool same_bits = memcmp(out.data(), first.data(), (total + 64) * 8) == 0 && (bad != 0) == (bad_first != 0);
          const bool untouched = memcmp(out.data(), inp.data(), total * 8) == 0;
          const bool flag_ok = (pc == 0) ? bad == 0 && !untouched : bad != 0 && untouched;
          printf("leaf n %2d band %d carried %2d %-10s %-22s %d workgroup(s) per CU  %6.0f cycles  bad %lld%s  same bits: %s (%s)\n", n, band, ncar,
                 pc == 0 ? "" : (pc == 1 ? "wrong sign" : (pc == 2 ? "zero pivot" : "NaN pivot")),
                 which == 0 ? "<40, 8> before" : (which == 1 ? "<40, 8, true, 2>" : "<36, 5, true, 2>"), nb / 256, c / nb, bad,
                 pc == 0 ? "" : (untouched ? ", store untouched" : ", STORE TOUCHED"), same_bits ? "yes" : "no", hipGetErrorString(e));
          if (!same_bits || !flag_ok || e != hipSuccess) rc = 1;
          if (e != hipSuccess) return rc;          // (nothing more on a device that reported an error)
        }
      }
    }
  }
  hipFree(d_in); hipFree(d_out); hipFree(d_cyc);
  return rc;
}

static void host_ldl(std::vector<double>& M, int n) {   // (n + 1) x n, lower part + the right-hand-side row; U = L D convention
  for (int j = 0; j < n; ++j) {
    const double d = M[j * n + j];
    for (int i = j + 1; i <= n; ++i) {
      const double l = M[i * n + j] / d;
      const int kmax = i < n ? i : n - 1;
      for (int k = j + 1; k <= kmax; ++k) M[i * n + k] -= l * M[k * n + j];
    }
  }
}

int main() {
  int rc = check_sign_test();
  rc |= leaf_cases();
  const int cases[4][2] = {{40, 30}, {39, 29}, {30, 24}, {17, 12}};
  for (int cs = 0; cs < 4; ++cs) {
    const int n = cases[cs][0], npos = cases[cs][1], total = (n + 1) * (n + 2) / 2;
    std::vector<double> in(total, 0.0);
    unsigned s = 777 + cs;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0 - 0.5; };
    for (int i = 0; i <= n; ++i) for (int k = 0; k <= i && k < n; ++k) {
      double v = 0.4 * rnd();
      if (i == k) v = (i < npos) ? 7.0 + rnd() : -(7.0 + rnd());
      if (i == n) v = rnd();
      in[i * (i + 1) / 2 + k] = v;
    }
    std::vector<double> M((n + 1) * n, 0.0);
    for (int i = 0; i <= n; ++i) for (int k = 0; k < n && k <= i; ++k) M[i * n + k] = in[i * (i + 1) / 2 + k];
    host_ldl(M, n);
    double *d_in, *d_out; long long* d_cyc;
    const int nb_max = 512;
    hipMalloc(&d_in, total * 8); hipMalloc(&d_out, total * 8); hipMalloc(&d_cyc, nb_max * 2 * sizeof(long long));
    hipMemcpy(d_in, in.data(), total * 8, hipMemcpyHostToDevice);
    const size_t lds = (1024 + 256) * 8;
    hipFuncSetAttribute((const void*)k_root, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    std::vector<double> first;
    for (int blocked = 0; blocked < 4; ++blocked) {
      for (int nb = 256; nb <= 512; nb += 256) {           // one / two workgroups per CU
        hipMemset(d_out, 0, total * 8);
        hipLaunchKernelGGL(k_root, dim3(nb), dim3(256), lds, 0, d_in, d_out, d_cyc, 16, n, npos, blocked);
        hipDeviceSynchronize();
        std::vector<double> out(total); std::vector<long long> cyc(nb * 2);
        hipMemcpy(out.data(), d_out, total * 8, hipMemcpyDeviceToHost);
        hipMemcpy(cyc.data(), d_cyc, nb * 2 * sizeof(long long), hipMemcpyDeviceToHost);
        double c = 0; long long bad = 0;
        for (int i = 0; i < nb; ++i) { c += cyc[2 * i]; bad |= cyc[2 * i + 1]; }
        double err = 0.0, mag = 0.0;
        for (int i = 0; i <= n; ++i) for (int k = 0; k < n && k <= i; ++k) {
          err = fmax(err, fabs(M[i * n + k] - out[i * (i + 1) / 2 + k])); mag = fmax(mag, fabs(M[i * n + k]));
        }
        if (blocked == 0) first = out;
        bool same_bits = true;
        for (int i = 0; i < total; ++i) same_bits = same_bits && out[i] == first[i];
        printf("n %2d (%2d positive pivots)  %-22s %d workgroup(s) per CU  %6.0f cycles  bad %lld  max |device - host| %.2e (max |entry| %.1f) %s, same bits as column by column: %s (%s)\n",
               n, npos, blocked == 3 ? "two vector rows (before)" : blocked == 2 ? "four waves through LDS" : (blocked ? "panels of 16 + MFMA" : "column by column"), nb / 256, c / nb, bad, err, mag, err < 1e-11 ? "OK" : "MISMATCH", same_bits ? "yes" : "no", hipGetErrorString(hipGetLastError()));
        if ((blocked == 2 || blocked == 3) && !same_bits) rc = 1;
        if (!(err < 1e-11) || bad) rc = 1;
      }
    }
    // a pivot of the wrong sign must be reported and nothing stored
    in[(npos - 1) * npos / 2 + npos - 1] = -3.0;
    hipMemcpy(d_in, in.data(), total * 8, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_root, dim3(1), dim3(256), lds, 0, d_in, d_out, d_cyc, 2, n, npos, 2);
    hipDeviceSynchronize();
    std::vector<double> out(total); long long cyc[2];
    hipMemcpy(out.data(), d_out, total * 8, hipMemcpyDeviceToHost);
    hipMemcpy(cyc, d_cyc, sizeof cyc, hipMemcpyDeviceToHost);
    bool untouched = true;
    for (int i = 0; i < total; ++i) untouched = untouched && out[i] == in[i];
    printf("n %2d wrong-sign pivot: bad %lld, store untouched: %s\n", n, cyc[1], untouched ? "yes" : "NO");
    if (!cyc[1] || !untouched) rc = 1;
    hipFree(d_in); hipFree(d_out); hipFree(d_cyc);
  }
  return rc;
}
