// Developer micro-benchmark (not part of the product): factorisation plus solve of the wave path on one KKT store, in the form the
// kernels had before kkt_root_solve_wave -- wave 0 factorises the root, c.rmax publishes the inertia, kkt_solve_wave substitutes the
// root behind one barrier and the leaves behind the next; kept here as old_factor_wave / old_solve_wave -- against kkt_factor_wave
// of omgx_core.h as it stands (the factorisation ends in the solution).  Random banded leaves (half bandwidth 5, diagonally
// dominant) of order 36 / 33 / 24 with nc + 1 = 30 / 16 / 9 carried rows, 3 / 6 / 10 of them, one sparse diagonal leaf of two slots
// behind them, a packed root; workgroups of 4 and of 8 waves; the root as it is (inertia right: both forms return 0 and leave the
// step in `sol`) and with one diagonal entry made negative (both return 2, the root and `sol` untouched).  Prints the cycles of each
// form alone on a CU and, where two images fit the LDS, with a second workgroup on it, and "same bits: yes / no" of the new form
// against the old one on the return code, the solution, the inverse pivots and the whole store.  Exits non-zero on any "no".
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o tools/micro/solve_handoff tools/micro/solve_handoff.hip && ./tools/micro/solve_handoff
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "../../omg-tools_amd/csrc/omgx_core.h"
using namespace omgx;

// LDS image of a case, in doubles: descriptor image and the waves' gather scratch (w.col) | inverse pivots | reduction scratch | sol | KKT store
enum { IMG_OFF = 0, IMG_DOUBLES = OMGX_BMAT_DOUBLES * (OMGX_MAX_LEAF + 1) + 8 * 64 + 3, DINV_OFF = IMG_OFF + IMG_DOUBLES, DINV_DOUBLES = 400,
       RED_OFF = DINV_OFF + DINV_DOUBLES, SOL_OFF = RED_OFF + 64, SOL_DOUBLES = 448, KKT_OFF = SOL_OFF + SOL_DOUBLES, LDS_CAP = 20000 };

// ---- the form before kkt_root_solve_wave (statements as they were; profiling lines left out) ----
template <class C>
OMGX_FN int old_factor_wave(const C& c, const Dims& d, const Kkt& K, Work& w) {
  const BMat* Ms = (const BMat*)w.col;
  const int lane = c.lane(), wave = c.wave(), nw = c.nwaves();
  const int koff = (int)(w.kkt - omgx_lds);
  int badl = 0;
  for (int l = wave; l < d.n_leaf; l += nw) {
    const int kind_bw = __builtin_amdgcn_readfirstlane(Ms[l].bw);
    if (kind_bw < 0) {
      const DiagLeaf L = diag_leaf(Ms[l]);
      const double dj = w.kkt[L.base + (lane < L.n ? lane : 0)];
      if (lane < L.n) { w.dinv[L.dinv + lane] = rcp_pivot(dj); if (!(dj > 0.0)) badl = 1; }
      continue;
    }
    const WPanel P = wpanel_leaf(Ms[l]);
    const int leaf_n = __builtin_amdgcn_readfirstlane(Ms[l].nfact);
    if (wave_leaf_small(leaf_n, kind_bw)) badl |= wave_ldl<OMGX_LEAF_COLS_SMALL, OMGX_LEAF_BW_SMALL, true, 2>(koff, P);
    else badl |= (kind_bw <= 8) ? wave_ldl<OMGX_WAVE_COLS, 8, true, 2>(koff, P) : wave_ldl<OMGX_WAVE_COLS, OMGX_WAVE_COLS, true, 2>(koff, P);
    wave_fence();
    const double dl = wave_dinv<true>(w.kkt, P);
    if (lane < P.n) w.dinv[Ms[l].dinv + lane] = dl;
  }
  if (c.rmax(badl ? 1.0 : 0.0) > 0.0) return 1;
  long long ts0_ = 0, tm_ = 0;
  kkt_schur_wave(c, d, K, w, ts0_, tm_);
  int badr = 0;
  if (wave == 0) badr = wave_ldl<OMGX_WAVE_COLS, OMGX_WAVE_COLS, false, 1>(koff, wpanel_root(Ms[d.n_leaf], d.n_root));
  return c.rmax(badr ? 1.0 : 0.0) > 0.0 ? 2 : 0;
}

template <class C>
OMGX_FN void old_solve_wave(const C& c, const Dims& d, const Kkt& K, Work& w, double* sol) {
  const BMat* Ms = (const BMat*)w.col;
  const int lane = c.lane(), wave = c.wave(), nw = c.nwaves();
  const int koff = (int)(w.kkt - omgx_lds);
  if (wave == 0) {
    const WPanel P = wpanel_root(Ms[d.n_leaf], d.n_root);
    const double dl = wave_dinv<false>(w.kkt, P);
    const double y = w.kkt[wcarried<false>(P, P.n) + (lane < P.n ? lane : 0)];
    const double x = wave_bwd<OMGX_WAVE_COLS, false>(koff, P, dl, y * dl);
    if (lane < P.n) sol[d.root_off + lane] = x;
  }
  c.sync();
  double* xg = w.col + OMGX_BMAT_DOUBLES * (OMGX_MAX_LEAF + 1) + wave * 64;
  for (int l = wave; l < d.n_leaf; l += nw) {
    const BMat M = Ms[l];
    if (__builtin_amdgcn_readfirstlane(M.bw) < 0) {
      const DiagLeaf L = diag_leaf(M);
      const int j = lane < L.n ? lane : 0;
      const double* A = w.kkt + L.base + j;
      double acc = A[(2 + L.S) * L.n] - A[(1 + L.S) * L.n] * sol[d.root_off + d.n_root - 1];
      for (int s = 0; s < L.S; ++s) {
        const int ps = diag_leaf_pos(d, K, w, L, s, j);
        acc = fma(-A[(1 + s) * L.n], sol[d.root_off + (ps < 0 ? 0 : ps)] * (ps < 0 ? 0.0 : 1.0), acc);
      }
      if (lane < L.n) sol[L.dinv + lane] = acc * w.dinv[L.dinv + j];
      continue;
    }
    const WPanel P = wpanel_uniform(wpanel_leaf(M));
    const int n = P.n, nc = P.nreg + 1 - P.n, ld = P.ld;
    if (lane < nc) xg[lane] = sol[d.root_off + leaf_cpl_at(d, K, w, M.cpl, lane)];
    wave_fence();
    const int j = lane < n ? lane : 0;
    const double* Wt = w.kkt + P.wbase + j;
    double acc = Wt[nc * ld];
#pragma unroll 4
    for (int a = 0; a < nc; ++a) acc = fma(-Wt[a * ld], xg[a], acc);
    const int dv = __builtin_amdgcn_readfirstlane(M.dinv);
    const double dl = w.dinv[dv + j];
    const double x = wave_leaf_small(n, P.bw) ? wave_bwd<OMGX_LEAF_COLS_SMALL, true>(koff, P, dl, acc * dl)
                                              : wave_bwd<OMGX_WAVE_COLS, true>(koff, P, dl, acc * dl);
    if (lane < n) sol[dv + lane] = x;
    wave_fence();
  }
  c.sync();
}

template <int FORM>
__global__ __launch_bounds__(512) void k_solve(const double* in, double* out, long long* cyc, int* ret, int reps, int total, Dims d, Kkt K) {
  double* lds = omgx_lds;
  CtxT<WaveToolFlags> c; c.red = lds + RED_OFF; c.prof = nullptr;
  Work w; w.col = lds + IMG_OFF; w.dinv = lds + DINV_OFF; w.red = lds + RED_OFF; w.sol = lds + SOL_OFF; w.kkt = lds + KKT_OFF; w.root = nullptr;
  K.a = w.kkt;
  long long t_sum = 0;
  int bad = 0;
  for (int rep = 0; rep < reps; ++rep) {
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += blockDim.x) lds[i] = in[i];
    __syncthreads();
    const long long t0 = clock64();
    if (FORM == 0) { bad = old_factor_wave(c, d, K, w); if (!bad) old_solve_wave(c, d, K, w, w.sol); }
    else bad = kkt_factor_wave(c, d, K, w, w.sol);
    __syncthreads();
    const long long t1 = clock64();
    if (rep >= reps / 2) t_sum += t1 - t0;
  }
  if (blockIdx.x == 0) for (int i = threadIdx.x; i < total; i += blockDim.x) out[i] = lds[i];
  if (threadIdx.x == 0) { cyc[blockIdx.x] = t_sum / (reps - reps / 2); ret[blockIdx.x] = bad; }
}

static int tri_h(int i, int k) { return i * (i + 1) / 2 + k; }

int main() {
  int rc = 0;
  const int orders[3] = {36, 33, 24}, nc1s[3] = {30, 16, 9}, nbs[3] = {3, 6, 10};
  const int n_cu = 256;
  double *d_in, *d_out; long long* d_cyc; int* d_ret; int32_t *d_cpl, *d_dl, *d_doff;
  const int dl_cap = 4 * DINV_DOUBLES + 64;
  hipMalloc(&d_in, LDS_CAP * 8); hipMalloc(&d_out, LDS_CAP * 8); hipMalloc(&d_cyc, 2 * n_cu * sizeof(long long)); hipMalloc(&d_ret, 2 * n_cu * sizeof(int));
  hipMalloc(&d_cpl, 16 * 32 * 4); hipMalloc(&d_dl, dl_cap * 4); hipMalloc(&d_doff, 32 * 4);
  hipFuncSetAttribute((const void*)k_solve<0>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_CAP * 8);
  hipFuncSetAttribute((const void*)k_solve<1>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_CAP * 8);
  for (int io = 0; io < 3; ++io) for (int ic = 0; ic < 3; ++ic) for (int ib = 0; ib < 3; ++ib) for (int wrong = 0; wrong < 2; ++wrong) {
    const int n = orders[io], nb = nbs[ib], nc1 = nc1s[ic], nc = nc1 - 1, n_leaf = nb + 1, n_root = nc + 2, nr = n_root;
    const int nd = nc / 2, S = 2, bw = 5, ldb = 6, ld = n | 1;
    unsigned s = 4201 + 131 * io + 17 * ic + ib;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0 - 0.5; };
    std::vector<int> ci(nc), ps(S * nd);
    for (int i = 0; i < nc; ++i) ci[i] = i + (i >= 3 ? 1 : 0);                 // increasing, below the position of t (n_root - 1)
    for (int j = 0; j < nd; ++j) { ps[j] = j; ps[nd + j] = (j % 3 == 0) ? -1 : nd + j; }
    std::vector<double> img(LDS_CAP, 0.0);
    std::vector<BMat> Ms(n_leaf + 1);
    std::vector<int32_t> cpl(nb * nc), dl(dl_cap, -1), doff(n_leaf + 1, 0);
    int ko = 0, dvo = 0;
    for (int l = 0; l < nb; ++l) {
      BMat& M = Ms[l];
      M.a = ko; M.ld = ld; M.nfact = n; M.rows = n + nc1; M.npos = n; M.dinv = dvo; M.pan = ko + n * ldb; M.cpl = l * nc; M.bw = bw; M.pad_ = ldb;
      for (int i = 0; i < n; ++i) for (int k = (i > bw ? i - bw : 0); k <= i; ++k)
        img[KKT_OFF + M.a + i * ldb + bw - i + k] = i == k ? 7.0 + rnd() : 0.5 * rnd();
      for (int i = 0; i < nc1 * ld; ++i) img[KKT_OFF + M.pan + i] = rnd();
      for (int i = 0; i < nc; ++i) cpl[l * nc + i] = ci[i];
      ko += n * ldb + nc1 * ld; dvo += n;
    }
    {
      BMat& M = Ms[nb];
      M.a = ko; M.ld = 0; M.nfact = nd; M.rows = nd; M.npos = nd; M.dinv = dvo; M.pan = S; M.cpl = 0; M.bw = -1; M.pad_ = 0;
      for (int i = 0; i < (3 + S) * nd; ++i) img[KKT_OFF + ko + i] = rnd();
      for (int j = 0; j < nd; ++j) img[KKT_OFF + ko + j] = 5.0 + rnd();
      for (int i = 0; i < S * nd; ++i) dl[4 * dvo + i] = ps[i];
      ko += (3 + S) * nd; dvo += nd;
    }
    const int root_off = ko, root_len = (nr + 1) * (nr + 2) / 2;
    for (int i = 0; i <= nr; ++i) for (int k = 0; k <= i && k < nr; ++k) img[KKT_OFF + root_off + tri_h(i, k)] = (i == k ? 40.0 + 12.0 * nb : 0.0) + rnd();
    if (wrong) img[KKT_OFF + root_off + tri_h(5, 5)] = -60.0;
    ko += root_len;
    { BMat& M = Ms[n_leaf]; M.a = root_off; M.ld = 0; M.nfact = nr; M.rows = nr + 1; M.npos = n_root; M.dinv = -1; M.pan = 0; M.cpl = 0; M.bw = nr; M.pad_ = 0; }
    doff[n_leaf] = root_off;
    const int total = KKT_OFF + ko, n_var = dvo + n_root;
    std::vector<int32_t> ints((n_leaf + 1) * 10);
    memcpy(ints.data(), Ms.data(), ints.size() * 4);
    Dims d; memset(&d, 0, sizeof d);
    d.n_leaf = n_leaf; d.n_root = n_root; d.n_eq = 0; d.nr = nr; d.wave_ok = 1; d.root_off = dvo;
    // the plan's rule (schur_rule, omgx_plan.h): coupling row and diagonal-leaf positions ride in the descriptor image where they fit
    // its free slots -- tile owners in the Schur phase, the diagonal leaf's substitution on wave 0 --, else the round form with
    // the global tables and the plain rotation (10 banded leaves with nc + 1 = 30)
    const bool tiles = (int)ints.size() + nc + S * nd <= 2 * OMGX_BMAT_DOUBLES * (OMGX_MAX_LEAF + 1);
    if (tiles) {
      d.schur_tiles = nb; d.schur_row = (int)ints.size(); ints.insert(ints.end(), ci.begin(), ci.end());
      d.schur_dl = (int)ints.size(); ints.insert(ints.end(), ps.begin(), ps.end());
      d.schur_ints = (int)ints.size();
    }
    if (total > LDS_CAP || (int)ints.size() > 2 * OMGX_BMAT_DOUBLES * (OMGX_MAX_LEAF + 1) || dvo > DINV_DOUBLES || n_var > SOL_DOUBLES || 4 * dvo > dl_cap ||
        nb * nc > 16 * 32 || n + nc1 - 2 > 64 || nr > OMGX_WAVE_COLS) { printf("case does not fit\n"); return 1; }
    memcpy(&img[IMG_OFF], ints.data(), ints.size() * 4);
    for (int q = 0; q < n_var; ++q) img[SOL_OFF + q] = 1000.0 + q;             // stands for the phase-I column: untouched on a wrong-sign root
    hipMemcpy(d_in, img.data(), total * 8, hipMemcpyHostToDevice);
    hipMemcpy(d_cpl, cpl.data(), cpl.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(d_dl, dl.data(), dl.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(d_doff, doff.data(), doff.size() * 4, hipMemcpyHostToDevice);
    Kkt K; memset(&K, 0, sizeof K);
    K.d_off = d_doff; K.cpl_idx = d_cpl; K.dl_pos = d_dl; K.n_leaf = n_leaf; K.n_root = n_root; K.root_off = 0;
    const int lds_bytes = total * 8;
    const int max_per_cu = 2 * lds_bytes <= 160 * 1024 ? 2 : 1;
    for (int threads = 256; threads <= 512; threads += 256) {
      std::vector<double> first; int first_ret = -1;
      for (int form = 0; form < 2; ++form) for (int per_cu = 1; per_cu <= max_per_cu; ++per_cu) {
        const int nblk = n_cu * per_cu;
        hipMemset(d_out, 0, total * 8);
        if (form == 0) hipLaunchKernelGGL(k_solve<0>, dim3(nblk), dim3(threads), lds_bytes, 0, d_in, d_out, d_cyc, d_ret, 12, total, d, K);
        else hipLaunchKernelGGL(k_solve<1>, dim3(nblk), dim3(threads), lds_bytes, 0, d_in, d_out, d_cyc, d_ret, 12, total, d, K);
        const hipError_t e = hipDeviceSynchronize();
        std::vector<double> out(total); std::vector<long long> cyc(nblk); std::vector<int> ret(nblk);
        hipMemcpy(out.data(), d_out, total * 8, hipMemcpyDeviceToHost);
        hipMemcpy(cyc.data(), d_cyc, nblk * sizeof(long long), hipMemcpyDeviceToHost);
        hipMemcpy(ret.data(), d_ret, nblk * sizeof(int), hipMemcpyDeviceToHost);
        double cs = 0;
        for (int i = 0; i < nblk; ++i) cs += cyc[i];
        if (form == 0 && per_cu == 1) { first = out; first_ret = ret[0]; }
        // the solution, the inverse pivots, the whole store (not the waves' gather scratch: the leaves changed waves)
        bool same = ret[0] == first_ret && e == hipSuccess;
        same = same && memcmp(&out[SOL_OFF], &first[SOL_OFF], n_var * 8) == 0 && memcmp(&out[DINV_OFF], &first[DINV_OFF], dvo * 8) == 0 &&
               memcmp(&out[KKT_OFF], &first[KKT_OFF], ko * 8) == 0;
        bool expect = ret[0] == (wrong ? 2 : 0);
        if (wrong) expect = expect && memcmp(&out[SOL_OFF], &img[SOL_OFF], n_var * 8) == 0;      // (sol untouched)
        else { double mx = 0; for (int q = 0; q < n_var; ++q) { expect = expect && out[SOL_OFF + q] != img[SOL_OFF + q] && isfinite(out[SOL_OFF + q]); mx = fmax(mx, fabs(out[SOL_OFF + q])); } expect = expect && mx < 100.0; }
        printf("leaf order %2d  nc+1 %2d  %2d banded + 1 diagonal (%s)  %d waves  root %-10s %-3s %d workgroup(s) per CU  %6.0f cycles  returns %d (%s)  same bits: %s (%s)\n",
               n, nc1, nb, tiles ? "tiles" : "rounds", threads / 64, wrong ? "wrong sign" : "as it is", form ? "new" : "old", per_cu, cs / nblk, ret[0], expect ? "as expected" : "UNEXPECTED",
               same ? "yes" : "no", hipGetErrorString(e));
        if (!same || !expect) rc = 1;
        if (e != hipSuccess) return rc;          // (nothing more on a device that reported an error)
      }
    }
  }
  hipFree(d_in); hipFree(d_out); hipFree(d_cyc); hipFree(d_ret); hipFree(d_cpl); hipFree(d_dl); hipFree(d_doff);
  return rc;
}
