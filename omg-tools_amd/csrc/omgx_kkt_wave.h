// omgx_kkt_wave.h -- the linear solve of the wave path (device only, gfx950): factorisation, Schur phase, root and
// substitutions on the register-resident routines of omgx_wave.h.  The blocked path and the host twin are not in here: it
// reads without them.  Included by omgx_core.h, in device builds, behind the data layout, the execution context and
// rcp_pivot that it uses; not meant to be included alone.
#pragma once
#include "omgx_wave.h"      // register-resident wave-level LDL'

namespace omgx {

// ---------------------------------------------------------------------------
// Wave path (every panel of the store fits one wave, Dims::wave_ok): register-resident factorisation
// (omgx_wave.h).  Leaf l is factorised by wave l % nwaves -- all leaves at once, no workgroup barrier inside
// --, the Schur complements S_l = Wt Delta^{-1} Wt' are formed on the matrix pipe (16x16x4 fp64 MFMA tiles)
// and subtracted from the root in leaf order (fixed order of the sums): by tile owners where the plan allows
// it (Dims::schur_tiles), else by the wave that factorised the leaf, one leaf per barrier-separated round;
// the root is factorised by wave 0.
// ---------------------------------------------------------------------------
OMGX_FN WPanel wpanel_leaf(const BMat& M) {
  WPanel P; P.base = M.a; P.ld = M.ld; P.n = M.nfact; P.nreg = M.rows - 2; P.nvec = 2; P.npos = M.nfact; P.bw = M.bw;
  P.vrow = M.rows - 2; P.band = M.bw; P.ldb = M.pad_; P.wbase = M.pan;
  return P;
}
OMGX_FN WPanel wpanel_root(const BMat& M, int n_root) {
  WPanel P; P.base = M.a; P.ld = 0; P.n = M.nfact; P.nreg = M.nfact; P.nvec = 1; P.npos = n_root; P.bw = M.nfact;
  P.vrow = M.nfact; P.band = -1; P.ldb = 0; P.wbase = 0;
  return P;
}

// Sparse diagonal leaf (the terminal slacks g*: every variable alone on its diagonal, coupled to one trajectory
// coefficient and to t): arrays of n entries each -- diagonal | S coupling slots | t coupling | right-hand side.
// Nothing to factorise; its Schur complement has one owner per target (the plan checked that no root position is
// coupled to two of its variables), the two entries every variable shares -- (t, t) and (rhs, t) -- are wave sums.
struct DiagLeaf { int base, n, S, dinv, dl; };
OMGX_FN DiagLeaf diag_leaf(const BMat& M) {
  DiagLeaf L;
  L.base = __builtin_amdgcn_readfirstlane(M.a); L.n = __builtin_amdgcn_readfirstlane(M.nfact);
  L.S = __builtin_amdgcn_readfirstlane(M.pan); L.dinv = __builtin_amdgcn_readfirstlane(M.dinv); L.dl = 4 * L.dinv;
  return L;
}
// slot s of variable j of the diagonal leaf: the root position it is coupled to (-1: none).  From the LDS copy of the table
// behind the descriptors where the plan put one (Dims::schur_tiles), from the global table otherwise.
OMGX_FN int diag_leaf_pos(const Dims& d, const Kkt& K, const Work& w, const DiagLeaf& L, int s, int j) {
  if (d.schur_tiles) return ((const int32_t*)w.col)[d.schur_dl + s * L.n + j];
  return K.dl_pos[L.dl + s * L.n + j];
}
// entry i of the coupling index list of a banded leaf (BMat::cpl): of the one row every banded leaf has, in LDS, or of the global table
OMGX_FN int leaf_cpl_at(const Dims& d, const Kkt& K, const Work& w, int cpl, int i) {
  if (d.schur_tiles) return ((const int32_t*)w.col)[d.schur_row + i];
  return K.cpl_idx[__builtin_amdgcn_readfirstlane(cpl) + i];
}

// Schur complement of the sparse diagonal leaf: lane j owns variable j.  v_0 .. v_{S-1} at root positions p_0 .. p_{S-1},
// v_t at the position of t (n_root - 1), the right-hand side r_j at row nr of the root.  load() reads the leaf (and forms
// the two wave sums every variable shares), apply() subtracts from the root: a caller may put a barrier between them.
struct DiagSchur {
  double vs[4], di, vt, rj, stt, srt;
  int ps[4], S;
  bool on;
  template <class C>
  OMGX_FN void load(const C& c, const Dims& d, const Kkt& K, const Work& w, const BMat& M) {
    const DiagLeaf L = diag_leaf(M);
    const int lane = c.lane(), j = lane < L.n ? lane : 0;
    on = lane < L.n; S = L.S;
    const double* A = w.kkt + L.base + j;
    di = w.dinv[L.dinv + j];
    vt = A[(1 + L.S) * L.n]; rj = A[(2 + L.S) * L.n];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bool has = s < L.S;
      ps[s] = has ? diag_leaf_pos(d, K, w, L, s, j) : -1;
      const double v = A[(1 + (has ? s : 0)) * L.n];
      vs[s] = (has && on && ps[s] >= 0) ? v : 0.0;
    }
    // shared targets: fixed-order wave sums
    stt = c.wave_sum(on ? vt * di * vt : 0.0); srt = c.wave_sum(on ? rj * di * vt : 0.0);
  }
  template <class C>
  OMGX_FN void apply(const C& c, const Dims& d, double* R) const {
    const int pt = d.n_root - 1;
    if (on) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (ps[s] < 0 || s >= S) continue;
        const double u = vs[s] * di;
#pragma unroll
        for (int s2 = 0; s2 <= s; ++s2) {
          if (ps[s2] < 0) continue;
          const int pa = ps[s] > ps[s2] ? ps[s] : ps[s2], pb = ps[s] > ps[s2] ? ps[s2] : ps[s];
          R[tri(pa, pb)] -= u * vs[s2];
        }
        R[tri(pt, ps[s])] -= u * vt;                  // (t is the last root variable: pt > every p_s)
        R[tri(d.nr, ps[s])] -= u * rj;
      }
    }
    if (c.lane() == 0) { R[tri(pt, pt)] -= stt; R[tri(d.nr, pt)] -= srt; }
  }
};

// One tile of the Schur complements S_l = W_l D_l^-1 W_l' of CNT banded leaves (descriptors Ms[0 .. CNT-1]), formed side by side on
// the matrix pipe -- rows ra of W_l against rows cb, four columns j0 .. j0+3 of the leaf per MFMA, a zero accumulator per leaf: per
// entry the products and the j0 order of the round form in kkt_factor_wave -- and subtracted from r in leaf order.
// No branch inside the loops, so the loads of the CNT leaves go out together, and the operands of the next four columns are
// requested before the MFMAs of these four (the loads clamp their index: the request behind the last columns is harmless).
// Whole blocks of four columns need no predicate; behind the end of a leaf (its order is no multiple of four, or it is shorter
// than the longest of the group) both operands are zero as in the round form (acc + 0 * 0: the same bits).  Rows at or beyond
// nc1 read the last row instead of zeros: entry (a, b) of a tile is a sum over row a and row b alone, and the caller never stores
// such a row.
template <int CNT>
OMGX_FN void schur_tile_group(const Work& w, const BMat* Ms, int ra, int cb, int nc1, int q, double (&r)[4]) {
  typedef double v4d __attribute__((ext_vector_type(4)));
  const int rac = ra < nc1 ? ra : nc1 - 1, cbc = cb < nc1 ? cb : nc1 - 1;
  v4d acc[CNT];
  int n[CNT], ao[CNT], bo[CNT], dv[CNT], nmax = 0, nfull = OMGX_WAVE_ROWS;
#pragma unroll
  for (int k = 0; k < CNT; ++k) {
    const int ld = __builtin_amdgcn_readfirstlane(Ms[k].ld), wo = __builtin_amdgcn_readfirstlane(Ms[k].pan);
    acc[k] = (v4d){0.0, 0.0, 0.0, 0.0};
    n[k] = __builtin_amdgcn_readfirstlane(Ms[k].nfact); dv[k] = __builtin_amdgcn_readfirstlane(Ms[k].dinv);
    ao[k] = wo + rac * ld; bo[k] = wo + cbc * ld;
    nmax = n[k] > nmax ? n[k] : nmax; nfull = (n[k] & ~3) < nfull ? (n[k] & ~3) : nfull;
  }
  double wa[CNT], wb[CNT], dj[CNT];
  auto request = [&](int j) {
#pragma unroll
    for (int k = 0; k < CNT; ++k) {
      const int jc = j < n[k] ? j : n[k] - 1;
      wa[k] = w.kkt[ao[k] + jc]; wb[k] = w.kkt[bo[k] + jc]; dj[k] = w.dinv[dv[k] + jc];       // unconditional loads
    }
  };
  request(q);
  int j0 = 0;
  for (; j0 < nfull; j0 += 4) {
    double a[CNT], b[CNT];
#pragma unroll
    for (int k = 0; k < CNT; ++k) { a[k] = wa[k] * dj[k]; b[k] = wb[k]; }
    request(j0 + 4 + q);
#pragma unroll
    for (int k = 0; k < CNT; ++k) acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[k], b[k], acc[k], 0, 0, 0);
  }
  for (; j0 < nmax; j0 += 4) {
    const int j = j0 + q;
    double a[CNT], b[CNT];
#pragma unroll
    for (int k = 0; k < CNT; ++k) { const bool in = j < n[k]; a[k] = (in ? wa[k] : 0.0) * dj[k]; b[k] = in ? wb[k] : 0.0; }
    request(j + 4);
#pragma unroll
    for (int k = 0; k < CNT; ++k) acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[k], b[k], acc[k], 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < CNT; ++k) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] -= acc[k][i];
  }
}

// The Schur phase of kkt_factor_wave: the leaves are factorised (Wt = B L^-T in their carried rows, inverse pivots in w.dinv), the
// packed root R -= sum_l S_l.  Every wave of the workgroup calls it and passes the same number of barriers whichever form
// runs; the last statement of either form is a barrier.  ts0_ / tm_: wave 0's clock at the start of the phase and its cycles
// up to the end of its MFMA loops (profiling build; dead otherwise).  A routine of its own so that tools/micro/schur_tiles.hip
// can run the two forms against each other.
template <class C>
OMGX_FN void kkt_schur_wave(const C& c, const Dims& d, const Kkt& K, Work& w, [[maybe_unused]] long long ts0_, [[maybe_unused]] long long& tm_) {
  typedef double v4d __attribute__((ext_vector_type(4)));
  const BMat* Ms = (const BMat*)w.col;
  const int lane = c.lane(), wave = c.wave(), nw = c.nwaves();
  double* R = K.R();
  if (d.schur_tiles && nw >= 3) {
    // Tile owners: the banded leaves (0 .. nb-1, in front of the diagonal leaf) all couple to the same root positions in the same
    // order, so tile (row block, column block) of every S_l lands on the same root entries.  Wave T = 0, 1, 2 owns tile (0,0),
    // (1,0), (1,1): it forms that tile for every leaf (the statements and the j0 order of the round form below, a zero
    // accumulator per leaf, three leaves in flight) and subtracts them in leaf order from a register copy of its root entries
    // -- per root entry the operands and the order of the round form, hence its bits -- and stores once.  Then the diagonal
    // leaf, read by its wave while the tiles are formed.  Two barriers, whatever the wave and whatever it had to do.
    const int nb = d.schur_tiles;
    const int32_t* si = (const int32_t*)w.col + d.schur_row;
    const int nc1 = __builtin_amdgcn_readfirstlane(Ms[0].rows) - __builtin_amdgcn_readfirstlane(Ms[0].nfact);      // coupling rows + the right-hand-side row (last)
    if (wave == 0 || (wave < 3 && nc1 > 16)) {
      const int rb = wave >= 1 ? 16 : 0, kb = wave == 2 ? 16 : 0;
      const int cb = kb + (lane & 15), ci_b = si[cb < nc1 - 1 ? cb : 0];
      int ad[4]; bool ok[4]; double r[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ca = rb + (lane >> 4) + 4 * i;
        const int ci_a = ca < nc1 - 1 ? si[ca] : d.nr;
        ok[i] = ca < nc1 && cb < nc1 - 1 && (rb != kb || cb <= ca);
        ad[i] = ok[i] ? tri(ci_a, ci_b) : 0;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = R[ad[i]];
      const int ra = rb + (lane & 15), q = lane >> 4;
      for (int l0 = 0; l0 < nb; l0 += 3) {
        const int cnt = nb - l0;
        if (cnt >= 3) schur_tile_group<3>(w, Ms + l0, ra, cb, nc1, q, r);
        else if (cnt == 2) schur_tile_group<2>(w, Ms + l0, ra, cb, nc1, q, r);
        else schur_tile_group<1>(w, Ms + l0, ra, cb, nc1, q, r);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) if (ok[i]) R[ad[i]] = r[i];
    }
#ifdef OMGX_PROFILE
    tm_ = clock64() - ts0_;
#endif
    const int dw = nw > 3 ? 3 : 0;
    const bool diag = nb < d.n_leaf && wave == dw;
    DiagSchur D;
    if (diag) D.load(c, d, K, w, Ms[nb]);
    c.sync();
    if (diag) D.apply(c, d, R);
    c.sync();
  } else for (int base = 0; base < d.n_leaf; base += nw) {      // the round form
    const int l = base + wave;
#ifdef OMGX_PROFILE
    const long long tb_ = clock64();
#endif
    v4d acc00 = {0.0, 0.0, 0.0, 0.0}, acc10 = acc00, acc11 = acc00;
    int nc1 = 0, ci_b0 = 0, ci_b1 = 0, ci_a[8];
    bool sparse = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) ci_a[i] = 0;
    if (l < d.n_leaf) {
      const BMat M = Ms[l];
      sparse = __builtin_amdgcn_readfirstlane(M.bw) < 0;
      if (!sparse) {
      const int n = __builtin_amdgcn_readfirstlane(M.nfact), ld = __builtin_amdgcn_readfirstlane(M.ld);
      nc1 = __builtin_amdgcn_readfirstlane(M.rows) - n;            // coupling rows + the right-hand-side row (last)
      const double* Wt = w.kkt + __builtin_amdgcn_readfirstlane(M.pan);
      const double* di = w.dinv + __builtin_amdgcn_readfirstlane(M.dinv);
      // root positions of this lane's rows / columns (global table, or its LDS copy: requested before the MFMA loop)
      const int cb0 = lane & 15, cb1 = 16 + (lane & 15);
      ci_b0 = leaf_cpl_at(d, K, w, M.cpl, cb0 < nc1 - 1 ? cb0 : 0); ci_b1 = leaf_cpl_at(d, K, w, M.cpl, cb1 < nc1 - 1 ? cb1 : 0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int ca = 16 * (i >> 2) + (lane >> 4) + 4 * (i & 3);
        ci_a[i] = ca < nc1 - 1 ? leaf_cpl_at(d, K, w, M.cpl, ca) : d.nr;
      }
      const int r0 = lane & 15, r1 = 16 + (lane & 15), q = lane >> 4;
      const int r0c = r0 < nc1 ? r0 : nc1 - 1, r1c = r1 < nc1 ? r1 : nc1 - 1;
      const bool two = nc1 > 16;
      for (int j0 = 0; j0 < n; j0 += 4) {
        const int j = j0 + q, jc = j < n ? j : n - 1;
        const double w0 = Wt[r0c * ld + jc], w1 = Wt[r1c * ld + jc], dj = di[jc];       // unconditional loads
        const double b0 = (r0 < nc1 && j < n) ? w0 : 0.0, b1 = (r1 < nc1 && j < n) ? w1 : 0.0;
        acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(b0 * dj, b0, acc00, 0, 0, 0);
        if (two) {
          acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(b1 * dj, b0, acc10, 0, 0, 0);
          acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(b1 * dj, b1, acc11, 0, 0, 0);
        }
      }
      }
    }
#ifdef OMGX_PROFILE
    tm_ += clock64() - tb_;
#endif
    // subtract from the root, one leaf per round
    const int lend = base + nw < d.n_leaf ? base + nw : d.n_leaf;
    for (int lr = base; lr < lend; ++lr) {
      if (l == lr && !sparse) {
        const int cb0 = lane & 15, cb1 = 16 + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ca0 = (lane >> 4) + 4 * i, ca1 = 16 + ca0;
          if (ca0 < nc1 && cb0 < nc1 - 1 && cb0 <= ca0) R[tri(ci_a[i], ci_b0)] -= acc00[i];
          if (ca1 < nc1 && cb0 < nc1 - 1) R[tri(ci_a[4 + i], ci_b0)] -= acc10[i];
          if (ca1 < nc1 && cb1 < nc1 - 1 && cb1 <= ca1) R[tri(ci_a[4 + i], ci_b1)] -= acc11[i];
        }
      } else if (l == lr) {
        DiagSchur D;
        D.load(c, d, K, w, Ms[l]);
        D.apply(c, d, R);
      }
      c.sync();
    }
  }
}

// One bit from any wave to every wave: a slot of the reduction scratch per wave and the barrier the caller needs anyway, instead
// of a reduction of doubles (c.rmax: a DPP ladder in every wave, two barriers).  `flag`: any lane of the wave may raise it.  A
// caller that goes on to write c.red without another barrier in between has to put one there (the readers of this exchange).
template <class C>
OMGX_FN int wave_flags_any(const C& c, int flag) {
  const int mine = __builtin_amdgcn_ballot_w64(flag != 0) != 0 ? 1 : 0;
  if (c.lane() == 0) c.red[c.wave()] = mine ? 1.0 : 0.0;
  c.sync();
  int any = 0;
  for (int i = 0; i < c.nwaves(); ++i) any |= c.red[i] != 0.0 ? 1 : 0;
  return __builtin_amdgcn_readfirstlane(any);
}

// A banded leaf's share of the solve, in two parts.  load(): what does not depend on the root -- the carried right-hand side
// L^{-1} r_l, the inverse pivot, and column `lane` of L' scaled by it (wave_bwd_load: 36 or 40 registers of doubles) -- and may
// therefore run as soon as the leaf factors are final; finish(): the gather of the root solution from `sol`, the chain over the
// coupling rows, the backward chain, the store.  The statements and their order are those the solve always had, whoever calls
// the two parts when: the same bits.
// (The coupling rows Wt[a * ld] stay in the store.  Held in registers as well -- 2 x 30 more -- the lean headline instance
// spills 71 vector registers, 288 B of scratch for 64; held instead of the L' column they keep 48 B and measure 1.9 % below
// this form on the bench, which is 0.7 % below the kernel as it was before this routine: profiles/solve_handoff_ab.txt.)
struct LeafSolveOps {
  double lt[OMGX_WAVE_COLS], acc0, dl;
  WPanel P;
  int nc, dv, cpl;
  bool small;
  template <class C>
  OMGX_FN void load(const C& c, const Work& w, const BMat& M, int koff) {
    const int lane = c.lane();
    P = wpanel_uniform(wpanel_leaf(M));
    nc = P.nreg + 1 - P.n;                               // (wave-uniform values: scalar loop bounds)
    dv = __builtin_amdgcn_readfirstlane(M.dinv); cpl = M.cpl;
    const int j = lane < P.n ? lane : 0;
    acc0 = w.kkt[P.wbase + j + nc * P.ld];               // L^{-1} r_l
    dl = w.dinv[dv + j];
    // (the leaf instance that factorised it, kkt_factor_wave: 36 positions instead of 40 where the leaf has no more)
    small = wave_leaf_small(P.n, P.bw);
    if (small) wave_bwd_load<OMGX_LEAF_COLS_SMALL, true>(koff, P, dl, lt);
    else wave_bwd_load<OMGX_WAVE_COLS, true>(koff, P, dl, lt);
  }
  template <class C>
  OMGX_FN void finish(const C& c, const Dims& d, const Kkt& K, const Work& w, double* xg, double* sol) const {
    const int lane = c.lane();
    if (lane < nc) xg[lane] = sol[d.root_off + leaf_cpl_at(d, K, w, cpl, lane)];
    wave_fence();
    const double* Wt = w.kkt + P.wbase + (lane < P.n ? lane : 0);
    double acc = acc0;
#pragma unroll 4
    for (int a = 0; a < nc; ++a) acc = fma(-Wt[a * P.ld], xg[a], acc);
    const double x = small ? wave_bwd_chain<OMGX_LEAF_COLS_SMALL>(P.n, lt, acc * dl) : wave_bwd_chain<OMGX_WAVE_COLS>(P.n, lt, acc * dl);
    if (lane < P.n) sol[dv + lane] = x;
    wave_fence();
  }
};

// The root block and everything behind it: wave 0 factorises the root (its Schur complements are in) and, the inertia being
// right, substitutes it backwards at once -- the right-hand side rode through wave_ldl --; meanwhile every other wave loads
// the operands of its first banded leaf (LeafSolveOps::load).  One barrier publishes the root solution and the inertia flag
// (a slot of the reduction scratch) together.  Wrong inertia: 2 is returned, nothing was stored by wave_ldl and `sol` is
// untouched -- it still holds the phase-I column the next assembly of this iteration reads.  Right inertia: no assembly of
// this iteration can follow any more (ipm_iterate leaves its factorisation loop on 0), the leaf waves gather, run their two
// chains and store: `sol` holds the Newton step on return, 0.
// Who substitutes which leaf: leaf l goes to wave (l + 1) % nw -- wave 0 has the root and comes last --, and under the tile
// rule (Dims::schur_tiles) the diagonal leaf, which has nothing to preload, to wave 0.  Only the substitution rotates: the
// factorisation keeps l % nw.  A wave's later leaves (more leaves than waves) and wave 0's go through the same statements
// behind the barrier.  Every wave passes the same barriers: one, a second one on either way out.
template <class C>
OMGX_FN int kkt_root_solve_wave(const C& c, const Dims& d, const Kkt& K, Work& w, double* sol) {
  const BMat* Ms = (const BMat*)w.col;
  const int lane = c.lane(), wave = c.wave(), nw = c.nwaves();
  const int koff = (int)(w.kkt - omgx_lds);            // the out-of-line wave routines address the LDS by offset
  OMGX_TIC();
  [[maybe_unused]] long long tr_ = 0;                  // (thread 0's clock behind the root factorisation)
  const int diag = (d.schur_tiles > 0 && d.schur_tiles < d.n_leaf) ? d.schur_tiles : -1;      // (tile rule: the last leaf)
  const int n_rr = diag >= 0 ? diag : d.n_leaf;        // leaves dealt round-robin
  const int l_done = 1 << 20;
  double* xg = w.col + OMGX_BMAT_DOUBLES * (OMGX_MAX_LEAF + 1) + wave * 64;      // gathered root solution of this wave's leaf
  int l = wave ? wave - 1 : nw - 1;
  LeafSolveOps Q;
  const bool pre = wave != 0 && l < n_rr && __builtin_amdgcn_readfirstlane(Ms[l < n_rr ? l : 0].bw) >= 0;
  if (wave == 0) {
    const WPanel P = wpanel_root(Ms[d.n_leaf], d.n_root);
#ifdef OMGX_PROFILE
    const long long tr0_ = clock64();
#endif
    // (The root on the four waves of the workgroup -- root_ldl_4w, tools/micro/root_ldl_variants.h: the same bits, 30.2 k -> 22.1 k cycles alone on a CU --
    // was measured twice and not adopted.  Round 6, for every iteration, one launch per step: f_root drops by 3.4 k only while the
    // agent that shares the CU loses what the three parked waves left it, 342 k -> 349 k cycles per solve
    // (profiles/r06_micro_root_ldl.txt).  With this routine, out of line and for iterations >= 1 only -- the solves a launch of the
    // per-step path waits for --, the leaf waves preloading behind it: +0.7 % on the default bench line against a spread of 3.6 % of
    // the parent's own runs, lean scratch 64 -> 80 B: taken out again (profiles/solve_handoff_ab.txt section 9).)
    const int badr = wave_ldl<OMGX_WAVE_COLS, OMGX_WAVE_COLS, false, 1>(koff, P);
#ifdef OMGX_PROFILE
    tr_ = clock64();
    if (c.tid() == 0) c.prof[PH_F_SWEEP] += tr_ - tr0_;      // raw root time
#endif
    if (!badr) {
      wave_fence();
      const double dl = wave_dinv<false>(w.kkt, P);
      const double y = w.kkt[wcarried<false>(P, P.n) + (lane < P.n ? lane : 0)];           // L^{-1} r: the carried vector row
      const double x = wave_bwd<OMGX_WAVE_COLS, false>(koff, P, dl, y * dl);
      if (lane < P.n) sol[d.root_off + lane] = x;
    }
    if (lane == 0) c.red[0] = badr ? 1.0 : 0.0;
  } else if (pre) {
#ifdef OMGX_PROFILE
    const long long tp0_ = clock64();
#endif
    Q.load(c, w, Ms[l], koff);
#ifdef OMGX_PROFILE
    if (c.tid() == 64) c.prof[PH_K_PRELOAD] += clock64() - tp0_;      // the preload as wave 1 sees it
#endif
  }
  c.sync();
  const int badr = __builtin_amdgcn_readfirstlane(c.red[0] != 0.0 ? 1 : 0);
#ifdef OMGX_PROFILE
  // f_root: up to the end of wave 0's factorisation; k_root: its substitution and the barrier
  { const long long now_ = clock64(); if (c.tid() == 0) { c.prof[PH_F_ROOT] += tr_ - tic_; c.prof[PH_K_ROOT] += now_ - tr_; } tic_ = now_; }
#endif
  if (badr) { c.sync(); return 2; }                  // 2: the leaves are fine, the root has the wrong inertia  (the barrier: c.red is free again)
  bool have = pre;                                   // (the operands of leaf l are in Q)
  for (;;) {                                         // the preloaded leaf, a wave's later leaves, and wave 0's
    if (wave == 0 && diag >= 0 && l >= n_rr && l < l_done) l = diag;
    if (!(l < d.n_leaf && (l < n_rr || wave == 0))) break;
    if (__builtin_amdgcn_readfirstlane(Ms[l].bw) >= 0) {
      if (!have) Q.load(c, w, Ms[l], koff);
      have = false;
      Q.finish(c, d, K, w, xg, sol);
    } else {
      // sparse diagonal leaf: x_j = (r_j - sum_s v_s x_r[p_s] - v_t x_t) / d_j
      const DiagLeaf L = diag_leaf(Ms[l]);
      const int j = lane < L.n ? lane : 0;
      const double* A = w.kkt + L.base + j;
      double acc = A[(2 + L.S) * L.n] - A[(1 + L.S) * L.n] * sol[d.root_off + d.n_root - 1];
      for (int s = 0; s < L.S; ++s) {
        const int ps = diag_leaf_pos(d, K, w, L, s, j);
        acc = fma(-A[(1 + s) * L.n], sol[d.root_off + (ps < 0 ? 0 : ps)] * (ps < 0 ? 0.0 : 1.0), acc);
      }
      if (lane < L.n) sol[L.dinv + lane] = acc * w.dinv[L.dinv + j];
    }
    l = l == diag ? l_done : l + nw;
  }
  c.sync();
  OMGX_TOC(PH_K_BWD);                                  // what is left behind the root: gather, two chains, store
  return 0;
}

// Leaves, Schur complements, root -- and, the inertia being right, the Newton step in `sol` (kkt_root_solve_wave).
template <class C>
OMGX_FN int kkt_factor_wave(const C& c, const Dims& d, const Kkt& K, Work& w, double* sol) {
  const BMat* Ms = (const BMat*)w.col;
  const int lane = c.lane(), wave = c.wave(), nw = c.nwaves();
  const int koff = (int)(w.kkt - omgx_lds);            // the out-of-line wave routines address the LDS by offset
  OMGX_TIC();
  int badl = 0;
#ifdef OMGX_PROFILE
  const long long tw0_ = clock64();
#endif
  for (int l = wave; l < d.n_leaf; l += nw) {
    const int kind_bw = __builtin_amdgcn_readfirstlane(Ms[l].bw);
    if (kind_bw < 0) {
      const DiagLeaf L = diag_leaf(Ms[l]);
      const double dj = w.kkt[L.base + (lane < L.n ? lane : 0)];
      if (lane < L.n) { w.dinv[L.dinv + lane] = rcp_pivot(dj); if (!(dj > 0.0)) badl = 1; }
      continue;
    }
    const WPanel P = wpanel_leaf(Ms[l]);
    // hyperplane leaves are banded (half bandwidth 5 in reverse Cuthill-McKee order): the instance of 36 columns and band 5
    // where the leaf fits it, a compile-time band of 8 on 40 columns for the other banded ones
    const int leaf_n = __builtin_amdgcn_readfirstlane(Ms[l].nfact);
    if (wave_leaf_small(leaf_n, kind_bw)) badl |= wave_ldl<OMGX_LEAF_COLS_SMALL, OMGX_LEAF_BW_SMALL, true, 2>(koff, P);
    else badl |= (kind_bw <= 8) ? wave_ldl<OMGX_WAVE_COLS, 8, true, 2>(koff, P) : wave_ldl<OMGX_WAVE_COLS, OMGX_WAVE_COLS, true, 2>(koff, P);
    wave_fence();
    const double dl = wave_dinv<true>(w.kkt, P);
    if (lane < P.n) w.dinv[Ms[l].dinv + lane] = dl;
  }
#ifdef OMGX_PROFILE
  if (c.tid() == 0) { c.prof[PH_F_SCALE] += clock64() - tw0_; c.prof[PH_F_PARK] += 1; }      // raw leaf time of wave 0, number of factorisations
#endif
  if (wave_flags_any(c, badl)) { c.sync(); return 1; }       // (its barrier: the panels and inverse pivots are visible)
  OMGX_TOC(PH_F_LEAF);
  [[maybe_unused]] long long ts0_ = 0, tm_ = 0;      // (wave 0's own clock: start of the Schur phase, cycles up to the end of its MFMA loops)
#ifdef OMGX_PROFILE
  ts0_ = clock64();
#endif
  kkt_schur_wave(c, d, K, w, ts0_, tm_);
  OMGX_TOC(PH_F_SCHUR);
#ifdef OMGX_PROFILE
  // (the split of f_schur by wave 0's clock: up to the end of its MFMA loops, and the rest -- subtraction and barriers)
  if (c.tid() == 0) { c.prof[PH_F_SCHUR_MFMA] += tm_; c.prof[PH_F_SCHUR_SUB] += tic_ - ts0_ - tm_; }
#endif
  return kkt_root_solve_wave(c, d, K, w, sol);
}

// One more solve with the factors kkt_factor_wave left in the store (the factorisation carries the right-hand side of the
// Newton system along; a second-order correction solves once more with the same factors).  In: the raw right-hand side
// where kkt_rhs writes it (last carried row of every leaf, row nr of the root).  Leaf waves substitute forwards in
// registers (wave_fwd_r) and form their share W Delta^{-1} y of the root's right-hand side; wave 0 subtracts the shares in
// leaf order (fixed order of the sums), substitutes the root forwards and backwards; the leaves finish as in
// kkt_root_solve_wave.  out [N]: the solution in position order (the equality multipliers of this solve are dropped).
template <class C>
OMGX_FN void kkt_solve2_wave(const C& c, const Dims& d, const Kkt& K, Work& w, double* out, bool with_y = false) {
  const BMat* Ms = (const BMat*)w.col;
  const int lane = c.lane(), wave = c.wave(), nw = c.nwaves();
  const int koff = (int)(w.kkt - omgx_lds);
  double* xg0 = w.col + OMGX_BMAT_DOUBLES * (OMGX_MAX_LEAF + 1);
  double* R = K.R();
  const int rrow = tri(d.nr, 0);
  for (int base = 0; base < d.n_leaf; base += nw) {
    const int l = base + wave;
    double* xg = xg0 + wave * 64;
    if (l < d.n_leaf && __builtin_amdgcn_readfirstlane(Ms[l].bw) >= 0) {
      const BMat M = Ms[l];
      const WPanel P = wpanel_uniform(wpanel_leaf(M));
      const int n = P.n, nc = P.nreg + 1 - P.n, ld = P.ld;
      const int j = lane < n ? lane : 0;
      double* Wt = w.kkt + P.wbase;
      const int dv = __builtin_amdgcn_readfirstlane(M.dinv);
      const double dl = w.dinv[dv + j];
      const double y = wave_fwd_r<true>(koff, P, dl, Wt[nc * ld + j]);
      if (lane < n) { Wt[nc * ld + lane] = y; xg[lane] = y * dl; }
      wave_fence();
      // share of coupling row a: sum_j W_aj y_j / d_j
      const int a = lane < nc ? lane : 0;
      double acc = 0.0;
#pragma unroll 4
      for (int q = 0; q < n; ++q) acc = fma(Wt[a * ld + q], xg[q], acc);
      wave_fence();
      if (lane < nc) xg[lane] = acc;
    }
    c.sync();
    if (wave == 0) {
      const int lend = base + nw < d.n_leaf ? base + nw : d.n_leaf;
      for (int lr = base; lr < lend; ++lr) {
        const BMat M = Ms[lr];
        if (__builtin_amdgcn_readfirstlane(M.bw) >= 0) {
          const int nc = __builtin_amdgcn_readfirstlane(M.rows) - 1 - __builtin_amdgcn_readfirstlane(M.nfact);
          const double* xs = xg0 + (lr - base) * 64;
          if (lane < nc) R[rrow + leaf_cpl_at(d, K, w, M.cpl, lane)] -= xs[lane];
        } else {
          // sparse diagonal leaf: y = r; lane j owns variable j and the root positions it is coupled to
          const DiagLeaf L = diag_leaf(M);
          const int j = lane < L.n ? lane : 0;
          const bool on = lane < L.n;
          const double* A = w.kkt + L.base + j;
          const double u = A[(2 + L.S) * L.n] * w.dinv[L.dinv + j];
          for (int s = 0; s < L.S; ++s) {
            const int ps = diag_leaf_pos(d, K, w, L, s, j);
            if (on && ps >= 0) R[rrow + ps] -= A[(1 + s) * L.n] * u;
          }
          const double st = c.wave_sum(on ? A[(1 + L.S) * L.n] * u : 0.0);
          if (lane == 0) R[rrow + d.n_root - 1] -= st;
        }
        wave_fence();
      }
    }
    c.sync();
  }
  if (wave == 0) {
    const WPanel P = wpanel_root(Ms[d.n_leaf], d.n_root);
    const double dl = wave_dinv<false>(w.kkt, P);
    const int j = lane < P.n ? lane : 0;
    const double y = wave_fwd_r<false>(koff, P, dl, w.kkt[wcarried<false>(P, P.n) + j]);
    const double x = wave_bwd_r<false>(koff, P, dl, y * dl);
    if (lane < (with_y ? P.n : d.n_root)) out[d.root_off + lane] = x;      // (with_y: the equality multipliers behind the N positions)
  }
  c.sync();
  double* xg = xg0 + wave * 64;
  for (int l = wave; l < d.n_leaf; l += nw) {
    const BMat M = Ms[l];
    if (__builtin_amdgcn_readfirstlane(M.bw) < 0) {
      const DiagLeaf L = diag_leaf(M);
      const int j = lane < L.n ? lane : 0;
      const double* A = w.kkt + L.base + j;
      double acc = A[(2 + L.S) * L.n] - A[(1 + L.S) * L.n] * out[d.root_off + d.n_root - 1];
      for (int s = 0; s < L.S; ++s) {
        const int ps = diag_leaf_pos(d, K, w, L, s, j);
        acc = fma(-A[(1 + s) * L.n], out[d.root_off + (ps < 0 ? 0 : ps)] * (ps < 0 ? 0.0 : 1.0), acc);
      }
      if (lane < L.n) out[L.dinv + lane] = acc * w.dinv[L.dinv + j];
      continue;
    }
    const WPanel P = wpanel_uniform(wpanel_leaf(M));
    const int n = P.n, nc = P.nreg + 1 - P.n, ld = P.ld;
    if (lane < nc) xg[lane] = out[d.root_off + leaf_cpl_at(d, K, w, M.cpl, lane)];
    wave_fence();
    const int j = lane < n ? lane : 0;
    const double* Wt = w.kkt + P.wbase + j;
    double acc = Wt[nc * ld];
#pragma unroll 4
    for (int a = 0; a < nc; ++a) acc = fma(-Wt[a * ld], xg[a], acc);
    const int dv = __builtin_amdgcn_readfirstlane(M.dinv);
    const double dl = w.dinv[dv + j];
    const double x = wave_bwd_r<true>(koff, P, dl, acc * dl);
    if (lane < n) out[dv + lane] = x;
    wave_fence();
  }
  c.sync();
}

}  // namespace omgx
