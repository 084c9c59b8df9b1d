// Developer micro-benchmark (not part of the product): the Schur phase of the wave-path factorisation, kkt_schur_wave of
// omgx_core.h, alone -- the round form (one leaf per barrier-separated round, coupling indices from the global tables) against the
// tile form (waves 0 / 1 / 2 own a root tile each, one subtraction in leaf order, indices from the descriptor image in LDS) -- on
// random factorised leaves (carried rows Wt, inverse pivots) and a random packed root with its right-hand-side row, in a workgroup
// of 256 threads like the solve kernel's.  Banded leaves of order 36 / 33 / 24 and of mixed order (36, 33, 24 in one group of
// three: the tail loop of schur_tile_group with leaves shorter than the longest), nc + 1 = 30, 22, 16, 9 coupling rows with the
// right-hand-side row, 1, 3 and 5 banded leaves, always followed by one sparse diagonal leaf of two slots.  The coupling row skips
// root position 3, so tile entries do not sit at their own index.  Prints the cycles of each form alone and with a second
// workgroup on the CU, the largest difference to a plain host computation, and "same bits: yes / no" of the tile form against
// the round form on the whole root including its right-hand-side row.  Exits non-zero on any "no".
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o tools/micro/schur_tiles tools/micro/schur_tiles.hip && ./tools/micro/schur_tiles
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "../../omg-tools_amd/csrc/omgx_core.h"
using namespace omgx;

// LDS image of a case, in doubles: descriptor image (ints) | inverse pivots | reduction scratch | KKT store
enum { IMG_OFF = 0, IMG_DOUBLES = 160, DINV_OFF = IMG_OFF + IMG_DOUBLES, DINV_DOUBLES = 256, RED_OFF = DINV_OFF + DINV_DOUBLES,
       KKT_OFF = RED_OFF + 64, LDS_CAP = 8192 };

__global__ __launch_bounds__(256) void k_schur(const double* in, double* out, long long* cyc, int reps, int total, Dims d, Kkt K,
                                               int root_off, int root_len) {
  extern __shared__ double lds[];
  CtxT<WaveToolFlags> c; c.red = lds + RED_OFF; c.prof = nullptr;
  Work w; w.col = lds + IMG_OFF; w.dinv = lds + DINV_OFF; w.red = lds + RED_OFF; w.kkt = lds + KKT_OFF; w.root = nullptr;
  K.a = w.kkt;
  long long t_sum = 0, tm = 0;
  for (int rep = 0; rep < reps; ++rep) {
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += blockDim.x) lds[i] = in[i];
    __syncthreads();
    const long long t0 = clock64();
    kkt_schur_wave(c, d, K, w, t0, tm);      // (either form ends in a barrier)
    const long long t1 = clock64();
    if (rep >= reps / 2) t_sum += t1 - t0;
  }
  __syncthreads();
  if (blockIdx.x == 0) for (int i = threadIdx.x; i < root_len; i += blockDim.x) out[i] = lds[KKT_OFF + root_off + i];
  if (threadIdx.x == 0) cyc[blockIdx.x] = t_sum / (reps - reps / 2);
}

static int tri_h(int i, int k) { return i * (i + 1) / 2 + k; }

int main() {
  int rc = 0;
  const int order_sets[4][3] = {{36, 36, 36}, {33, 33, 33}, {24, 24, 24}, {36, 33, 24}};
  const int nc1s[4] = {30, 22, 16, 9}, nbs[3] = {1, 3, 5};
  const int nb_max = 512;
  double *d_in, *d_out; long long* d_cyc; int32_t *d_cpl, *d_dl, *d_doff;
  const int dl_cap = 4 * DINV_DOUBLES + 64;
  hipMalloc(&d_in, LDS_CAP * 8); hipMalloc(&d_out, LDS_CAP * 8); hipMalloc(&d_cyc, nb_max * sizeof(long long));
  hipMalloc(&d_cpl, 8 * 32 * 4); hipMalloc(&d_dl, dl_cap * 4); hipMalloc(&d_doff, 16 * 4);
  hipFuncSetAttribute((const void*)k_schur, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_CAP * 8);
  for (int io = 0; io < 4; ++io) for (int ic = 0; ic < 4; ++ic) for (int ib = 0; ib < 3; ++ib) {
    const int nb = nbs[ib], nc1 = nc1s[ic], nc = nc1 - 1, n_leaf = nb + 1, n_root = nc + 2, nr = n_root, pt = n_root - 1;
    const int nd = nc / 2, S = 2;
    unsigned s = 9001 + 131 * io + 17 * ic + ib;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0 - 0.5; };
    std::vector<int> ci(nc), ps(S * nd);
    for (int i = 0; i < nc; ++i) ci[i] = i + (i >= 3 ? 1 : 0);                 // increasing, below pt
    for (int j = 0; j < nd; ++j) { ps[j] = j; ps[nd + j] = (j % 3 == 0) ? -1 : nd + j; }      // no root position twice, all below pt
    // the store: carried rows of the banded leaves (odd leading dimension) | the diagonal leaf's arrays | the packed root
    std::vector<double> img(LDS_CAP, 0.0);
    std::vector<BMat> Ms(n_leaf + 1);
    std::vector<int32_t> cpl(nb * nc), dl(dl_cap, -1), doff(n_leaf + 1, 0);
    int ko = 0, dvo = 0;
    for (int l = 0; l < nb; ++l) {
      const int n = order_sets[io][l % 3], ld = n | 1;
      BMat& M = Ms[l];
      M.a = 0; M.ld = ld; M.nfact = n; M.rows = n + nc1; M.npos = n; M.dinv = dvo; M.pan = ko; M.cpl = l * nc; M.bw = 5; M.pad_ = 6;
      for (int i = 0; i < nc1 * ld; ++i) img[KKT_OFF + ko + i] = rnd();
      for (int j = 0; j < n; ++j) img[DINV_OFF + dvo + j] = 1.0 / (7.0 + rnd());
      for (int i = 0; i < nc; ++i) cpl[l * nc + i] = ci[i];
      ko += nc1 * ld; dvo += n;
    }
    {
      BMat& M = Ms[nb];
      M.a = ko; M.ld = 0; M.nfact = nd; M.rows = nd; M.npos = nd; M.dinv = dvo; M.pan = S; M.cpl = 0; M.bw = -1; M.pad_ = 0;
      for (int i = 0; i < (3 + S) * nd; ++i) img[KKT_OFF + ko + i] = rnd();
      for (int j = 0; j < nd; ++j) { img[KKT_OFF + ko + j] = 5.0 + rnd(); img[DINV_OFF + dvo + j] = 1.0 / img[KKT_OFF + ko + j]; }
      for (int i = 0; i < S * nd; ++i) dl[4 * dvo + i] = ps[i];
      ko += (3 + S) * nd; dvo += nd;
    }
    const int root_off = ko, root_len = (nr + 1) * (nr + 2) / 2;
    for (int i = 0; i <= nr; ++i) for (int k = 0; k <= i && k < nr; ++k) img[KKT_OFF + root_off + tri_h(i, k)] = (i == k ? 9.0 : 0.0) + rnd();
    ko += root_len;
    { BMat& M = Ms[n_leaf]; M.a = root_off; M.ld = 0; M.nfact = nr; M.rows = nr + 1; M.npos = n_root; M.dinv = -1; M.pan = 0; M.cpl = 0; M.bw = nr; M.pad_ = 0; }
    doff[n_leaf] = root_off;
    const int total = KKT_OFF + ko;
    // the descriptor image: descriptors | the one coupling row | the diagonal leaf's positions
    std::vector<int32_t> ints((n_leaf + 1) * 10);
    memcpy(ints.data(), Ms.data(), ints.size() * 4);
    Dims dr; memset(&dr, 0, sizeof dr);
    dr.n_leaf = n_leaf; dr.n_root = n_root; dr.n_eq = 0; dr.nr = nr; dr.wave_ok = 1;
    Dims dt = dr;
    dt.schur_tiles = nb; dt.schur_row = (int)ints.size(); ints.insert(ints.end(), ci.begin(), ci.end());
    dt.schur_dl = (int)ints.size(); ints.insert(ints.end(), ps.begin(), ps.end());
    dt.schur_ints = (int)ints.size();
    if (total > LDS_CAP || (int)ints.size() > 2 * IMG_DOUBLES || dvo > DINV_DOUBLES || 4 * dvo > dl_cap || nb * nc > 8 * 32) { printf("case does not fit\n"); return 1; }
    memcpy(&img[IMG_OFF], ints.data(), ints.size() * 4);
    // plain host computation of the same root
    std::vector<double> H(img.begin() + KKT_OFF + root_off, img.begin() + KKT_OFF + root_off + root_len);
    for (int l = 0; l < nb; ++l) {
      const BMat& M = Ms[l];
      const double *W = &img[KKT_OFF + M.pan], *di = &img[DINV_OFF + M.dinv];
      for (int a = 0; a < nc1; ++a) for (int b = 0; b <= a && b < nc; ++b) {
        double sum = 0.0;
        for (int j = 0; j < M.nfact; ++j) sum += W[a * M.ld + j] * di[j] * W[b * M.ld + j];
        H[tri_h(a < nc ? ci[a] : nr, ci[b])] -= sum;
      }
    }
    {
      const BMat& M = Ms[nb];
      const double *A = &img[KKT_OFF + M.a], *di = &img[DINV_OFF + M.dinv];
      for (int j = 0; j < nd; ++j) {
        const double vt = A[(1 + S) * nd + j], rj = A[(2 + S) * nd + j];
        for (int q = 0; q < S; ++q) {
          if (ps[q * nd + j] < 0) continue;
          const int p = ps[q * nd + j];
          const double u = A[(1 + q) * nd + j] * di[j];
          for (int q2 = 0; q2 <= q; ++q2) {
            const int p2 = ps[q2 * nd + j];
            if (p2 >= 0) H[tri_h(p > p2 ? p : p2, p > p2 ? p2 : p)] -= u * A[(1 + q2) * nd + j];
          }
          H[tri_h(pt, p)] -= u * vt; H[tri_h(nr, p)] -= u * rj;
        }
        H[tri_h(pt, pt)] -= vt * di[j] * vt; H[tri_h(nr, pt)] -= rj * di[j] * vt;
      }
    }
    hipMemcpy(d_in, img.data(), total * 8, hipMemcpyHostToDevice);
    hipMemcpy(d_cpl, cpl.data(), cpl.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(d_dl, dl.data(), dl.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(d_doff, doff.data(), doff.size() * 4, hipMemcpyHostToDevice);
    Kkt K; memset(&K, 0, sizeof K);
    K.d_off = d_doff; K.cpl_idx = d_cpl; K.dl_pos = d_dl; K.n_leaf = n_leaf; K.n_root = n_root; K.root_off = 0;
    std::vector<double> first;
    for (int form = 0; form < 2; ++form) for (int nblk = 256; nblk <= 512; nblk += 256) {       // one / two workgroups per CU
      hipMemset(d_out, 0, root_len * 8);
      hipLaunchKernelGGL(k_schur, dim3(nblk), dim3(256), LDS_CAP * 8, 0, d_in, d_out, d_cyc, 16, total, form ? dt : dr, K, root_off, root_len);
      const hipError_t e = hipDeviceSynchronize();
      std::vector<double> out(root_len); std::vector<long long> cyc(nblk);
      hipMemcpy(out.data(), d_out, root_len * 8, hipMemcpyDeviceToHost);
      hipMemcpy(cyc.data(), d_cyc, nblk * sizeof(long long), hipMemcpyDeviceToHost);
      double cs = 0, err = 0;
      for (int i = 0; i < nblk; ++i) cs += cyc[i];
      for (int i = 0; i < root_len; ++i) err = fmax(err, fabs(out[i] - H[i]));
      if (form == 0 && nblk == 256) first = out;
      const bool same_bits = memcmp(out.data(), first.data(), root_len * 8) == 0;
      printf("leaf order %2d/%2d/%2d  nc+1 %2d  %d banded + 1 diagonal  %-6s %d workgroup(s) per CU  %6.0f cycles  max |device - host| %.1e %s  same bits: %s (%s)\n",
             order_sets[io][0], order_sets[io][1], order_sets[io][2], nc1, nb, form ? "tiles" : "rounds", nblk / 256, cs / nblk, err,
             err < 1e-12 ? "OK" : "MISMATCH", same_bits ? "yes" : "no", hipGetErrorString(e));
      if (!same_bits || !(err < 1e-12) || e != hipSuccess) rc = 1;
      if (e != hipSuccess) return rc;          // (nothing more on a device that reported an error)
    }
  }
  hipFree(d_in); hipFree(d_out); hipFree(d_cyc); hipFree(d_cpl); hipFree(d_dl); hipFree(d_doff);
  return rc;
}
