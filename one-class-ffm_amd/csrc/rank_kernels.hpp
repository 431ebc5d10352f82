// rank_kernels.hpp — the serving kernels: top-N recommendation, ranking
// evaluation, top-N and label ranks among candidate lists.  Included through rank_driver.hpp
// by solver.hip (the block Newton-CG problem: REC_PLAIN), by sgd.hip (the SGD
// trainer's model: REC_NORM) and by model.hip (REC_PLAIN, and REC_SIM for the
// item-item similarities: sim_kernels.hpp), after kernels.hpp.
#pragma once

#include "kernels.hpp"

namespace ocffm {

// ---------------------------------------------------- recommendation ---
// Top-N items per query row (ocffm_problem_recommend): the score product
// fused with the selection, so no rows x n score matrix ever exists.
//
// k_rec_topn: a block owns REC_RT query rows (a row tile) and one item slice,
// which it walks REC_IT items at a time.  Each wave takes 16 of the tile's
// items and both 16-row halves of the row tile: two chains of C KP / 4
// v_mfma_{f32,f64}_16x16x4 over the whole depth (lane l holds 4 consecutive
// depth elements of row / item l & 15 starting at 16 j + 4 (l >> 4), one per
// MFMA of the chunk: TMma's operand layout), operands straight from global
// memory into registers, two groups of chunks in flight (the row tile stays
// in the vector L1; an item row is read once per row tile).  The tile's scores s = acc + b_j + a_i go to LDS
// as fp64 (exact for either precision), then each wave selects for 8 of the
// rows, one candidate per lane: a candidate that beats the row's current
// N-th entry, is inside the slice and is not among the row's sorted labels
// is inserted into the row's sorted list.  The list (REC_MAX entries, score
// descending, equal scores by ascending item) lives in LDS, entries p and
// p + 64 owned by lane p: a lane reads and writes only its own two entries
// and gets its neighbour's through a DPP wave shift, so the list needs no
// barrier; each row's current N-th entry is also kept in LDS, written by the
// row's wave and read only after the next tile's barriers.
// Selection is on the strict total order (score, item), hence independent of
// tiling, slicing and the row's place in the call.  Cold rows (no kept
// feature node) rank popular[j], j < npop (ffm.cpp:975-977).
// Ragged edges: rows >= R and items >= n are neither read nor selected.
constexpr int REC_RT = 32, REC_IT = 64, REC_MAX = 128;
constexpr uint32_t REC_NONE = 0xffffffffu;
constexpr double REC_NEG_INF = -__builtin_huge_val();

// How a chain's sum becomes a score (rec_score)
enum RecMode : int {
  REC_PLAIN = 0,  // (acc + b_j) + a_i; cold rows rank the popularity
  REC_NORM = 1,   // the SGD model: the same times 1 / (su_i + sv_j)
  REC_SIM = 2,    // item-item similarity: acc (inv_i inv_j), the inverse norms in the su / sv slots
};

// What a sweep over the items needs (rec_sweep); k_rec_topn and k_eval_count
// add their own.
template <typename real> struct SweepArgs {
  uint64_t R, p0;              // query rows of this launch; their first row in the P tables
  uint64_t n, npop, per;       // items, popularity entries, items per slice (multiple of REC_IT)
  int C, exclude;
  uint32_t S, rt;              // item slices; row tiles of this launch (work items: slice-major)
  const real *const *P;        // C user-side cross tables of the query rows (R x KP)
  const real *const *Q;        // C item-side cross tables (n x KP)
  const real *a, *b;           // a_i of the query rows, b_j
  const uint8_t *cold;         // per query row
  const double *popular;
  const int64_t *lptr;         // sorted, distinct items < n of each query row to leave out (exclude)
  const uint32_t *lcol;
  const real *su, *sv;         // REC_NORM: squared norms of the query rows, of the items;
                               // REC_SIM: their inverse norms (both null: 1, the inner product)
};
template <typename real> struct RecArgs : SweepArgs<real> {
  int topn;
  double *part_v;              // R x slices x topn
  uint32_t *part_j;
};

// a before b in the ranking
__device__ __forceinline__ bool rec_better(double av, uint32_t aj, double bv, uint32_t bj) {
  return av > bv || (av == bv && aj < bj);
}

// x of lane l (wave-uniform l): v_readlane, no LDS-pipe shuffle
__device__ __forceinline__ uint32_t rec_lane(uint32_t x, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)x, l);
}
__device__ __forceinline__ double rec_lane(double x, int l) {
  W2 w = __builtin_bit_cast(W2, x);
  w.lo = rec_lane(w.lo, l);
  w.hi = rec_lane(w.hi, l);
  return __builtin_bit_cast(double, w);
}

// Insert (v, j) into the sorted list whose entries lane and lane + 64 this
// lane holds in (v0, j0), (v1, j1); the last entry falls off.  Wave-uniform
// call.  The shift is a DPP wave_shr:1 (0x138: lane l takes lane l - 1's).
__device__ __forceinline__ void rec_insert(double v, uint32_t j, double &v0, uint32_t &j0, double &v1, uint32_t &j1,
                                           int lane) {
  const bool k0 = rec_better(v0, j0, v, j), k1 = rec_better(v1, j1, v, j);
  const int pos = __popcll(__ballot(k0)) + __popcll(__ballot(k1));
  const double u0 = dpp<0x138>(v0), u1 = dpp<0x138>(v1), w0 = rec_lane(v0, 63);
  const uint32_t i0 = dpp<0x138>(j0), i1 = dpp<0x138>(j1), x0 = rec_lane(j0, 63);
  const int p0 = lane, p1 = lane + 64;
  if (p0 == pos) {
    v0 = v;
    j0 = j;
  } else if (p0 > pos) {
    v0 = u0;
    j0 = i0;
  }
  if (p1 == pos) {
    v1 = v;
    j1 = j;
  } else if (p1 > pos) {
    v1 = lane == 0 ? w0 : u1;
    j1 = lane == 0 ? x0 : i1;
  }
}

// Offer the candidates of the lanes in mask (score v, item j) to the sorted
// list in (v0, j0), (v1, j1), whose topn-th entry is (tv, tj).  Wave-uniform.
// DUP: the offered items may repeat (candidate lists); a sweep's are distinct
// and skip that ballot.
template <bool DUP>
__device__ __forceinline__ void rec_offer(uint64_t mask, double v, uint32_t j, double &v0, uint32_t &j0, double &v1,
                                          uint32_t &j1, double &tv, uint32_t &tj, int topn, int lane) {
  const int tl = (topn - 1) & 63;
  const bool hi = topn > 64;
  while (mask) {
    const int src = __ffsll((unsigned long long)mask) - 1;
    mask &= mask - 1;
    const double cv = rec_lane(v, src);
    const uint32_t cj = rec_lane(j, src);
    if (!rec_better(cv, cj, tv, tj)) continue;   // the threshold has moved past it (or it is a copy below it)
    if (DUP && __ballot(j0 == cj || j1 == cj)) continue;  // a copy that is in the list
    rec_insert(cv, cj, v0, j0, v1, j1, lane);
    tv = hi ? rec_lane(v1, tl) : rec_lane(v0, tl);
    tj = hi ? rec_lane(j1, tl) : rec_lane(j0, tl);
  }
}

// j among the sorted distinct col[lo, hi)
__device__ __forceinline__ bool rec_in_sorted(const uint32_t *col, int64_t lo, int64_t hi, uint32_t j) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (col[mid] < j) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && col[lo] == j;
}

// A pair's score from its chain's sum acc: (acc + b_j) + a_i; REC_NORM (the SGD
// model, sgd.hip): times rn = 1 / (su_i + sv_j), the instance's squared norm
// (rn = 1 where that is 0: no node, or a model trained without the
// normalisation, whose su and sv are zero).  REC_SIM (ocffm_similar.h): su and
// sv are the two inverse norms and the score is acc (su sv); their product
// comes first and commutes, so the score of (x, y) has the bits of (y, x); a_i
// and b_j play no part.  The one text of the sweep and of
// k_eval_label_scores, so a pair has the same bits in both.  The division is
// correctly rounded: its result does not depend on the code around it.
template <RecMode MODE, typename real>
__device__ __forceinline__ real rec_score(real acc, real bj, real ai, real su, real sv) {
  if constexpr (MODE == REC_SIM) {
    return acc * (su * sv);
  } else {
    const real s = (acc + bj) + ai;
    if constexpr (MODE == REC_NORM) {
      const real d = su + sv;
      return s * (d > (real)0 ? (real)1 / d : (real)1);
    } else {
      return s;
    }
  }
}
// REC_SIM: an inverse norm from its array (null: the inner product, 1)
template <typename real> __device__ __forceinline__ real rec_inv(const real *inv, uint64_t i) {
  return inv ? inv[i] : (real)1;
}

// 4 consecutive depth elements of a row, and the MFMA of one of them
template <typename real> struct RecMma;
template <> struct RecMma<float> {
  using V = f4v;
  static constexpr int GR = 4;  // chunks per load group (two groups in flight)
  static __device__ __forceinline__ V ld(const float *p) { return gvld<float>(p); }
  static __device__ __forceinline__ V mma(float a, float b, V c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // output row of D register r in lane group q = l >> 4 (column l & 15)
  static __device__ __forceinline__ int drow(int q, int r) { return 4 * q + r; }
};
template <> struct RecMma<double> {
  using V = d4v;
  static constexpr int GR = 2;
  static __device__ __forceinline__ V ld(const double *p) {
    typedef const __attribute__((address_space(1))) d2v *gp;
    const d2v lo = *(gp)p, hi = *(gp)(p + 2);
    return V{lo[0], lo[1], hi[0], hi[1]};
  }
  static __device__ __forceinline__ V mma(double a, double b, V c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int drow(int q, int r) { return q + 4 * r; }
};

// Lane group q's 4 depth elements of chunk c (from 16 c + 4 q) of row `row`
// of the tables T; zero past the depth and where !ok (nothing is read)
template <typename real, int KP>
__device__ __forceinline__ typename RecMma<real>::V rec_ld(const real *const *T, uint64_t row, int c, int q,
                                                           int depth, bool ok) {
  const int d = 16 * c + 4 * q;
  const bool in = d < depth;
  const int tb = in ? d / KP : 0, el = d % KP;
  return (in && ok) ? RecMma<real>::ld(T[tb] + row * KP + el) : typename RecMma<real>::V{0, 0, 0, 0};
}

// The sweep of a block's work item: row tile L % rt (first row r0) against
// item slice sl = L / rt.  Work items are slice-major: the row tiles of one
// slice run side by side and read its Q rows at about the same time.
// (XCD-contiguous work items, xcd_work_item, measured no different at the
// kkbox shape: 5.49 against 5.43 ms fp32, 7.61 against 7.60 ms fp64.)
// Every tile's scores go through sc; then consume(il, i, j, v, cand) runs once
// per row of this wave (row il of the tile, i of the launch) with the lane's
// item j, its score v and whether it is a candidate so far: inside the slice
// and, for a cold row, below npop (REC_NORM and REC_SIM: no row is cold, g.cold
// and g.popular are not read; REC_SIM reads neither g.a nor g.b).  Block-uniform call, after a barrier that
// covers the caller's own LDS set-up; what consume writes to LDS for another
// tile's call of the same row needs no barrier of its own.
template <typename real, int KP, RecMode MODE, typename F>
__device__ __forceinline__ void rec_sweep(const SweepArgs<real> &g, uint64_t r0, uint64_t sl,
                                          double (&sc)[REC_RT][REC_IT + 1], F &&consume) {
  using M = RecMma<real>;
  using V = typename M::V;
  constexpr int GR = M::GR;
  constexpr bool NORM = MODE == REC_NORM, SIM = MODE == REC_SIM;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int m = lane & 15, q = lane >> 4;
  const uint64_t jb = sl * g.per < g.n ? sl * g.per : g.n;
  const uint64_t je = jb + g.per < g.n ? jb + g.per : g.n;
  const int depth = g.C * KP, nch = (depth + 15) / 16;
  // this lane's A rows (row m of each half); the side terms of its D rows
  const uint64_t ra0 = r0 + m, ra1 = r0 + 16 + m;
  const bool ha0 = ra0 < g.R, ha1 = ra1 < g.R;
  real ai[2][4], sui[2][4];
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint64_t i = r0 + 16 * h + M::drow(q, r);
      ai[h][r] = (!SIM && i < g.R) ? g.a[i] : (real)0;
      if constexpr (SIM) sui[h][r] = i < g.R ? rec_inv(g.su, i) : (real)0;
      else sui[h][r] = (NORM && i < g.R) ? g.su[i] : (real)0;
    }
  // the selection's rows of this wave: REC_RT / 4 of them, cold flags as bits
  unsigned coldbits = 0;
  if constexpr (MODE == REC_PLAIN)
    for (int rr = 0; rr < REC_RT / 4; rr++) {
      const uint64_t i = r0 + w * (REC_RT / 4) + rr;
      if (i < g.R && g.cold[i]) coldbits |= 1u << rr;
    }
  const V zero = {(real)0, (real)0, (real)0, (real)0};
  uint64_t jq = jb + (uint64_t)w * 16 + m;  // this lane's B row (item) of the tile being loaded
  bool hb = jq < je;
  V bq[2][GR], a0q[2][GR], a1q[2][GR];
  auto load = [&](auto SB_, int c0) {
    constexpr int sb = decltype(SB_)::value;
#pragma unroll
    for (int u = 0; u < GR; u++) {
      const int d = 16 * (c0 + u) + 4 * q;  // (rec_ld here costs fp32 KP 16 / 32 up to 12 VGPRs)
      const bool in = d < depth;
      const int tb = in ? d / KP : 0, e = d % KP;
      bq[sb][u] = (in && hb) ? M::ld(g.Q[tb] + jq * KP + e) : zero;
      a0q[sb][u] = (in && ha0) ? M::ld(g.P[tb] + (g.p0 + ra0) * KP + e) : zero;
      a1q[sb][u] = (in && ha1) ? M::ld(g.P[tb] + (g.p0 + ra1) * KP + e) : zero;
    }
  };
  // one chain per output tile, chunks in order: a score's bits do not
  // depend on where its row and item sit
  auto mma = [&](auto SB_, int c0, V &acc0, V &acc1) {
    constexpr int sb = decltype(SB_)::value;
#pragma unroll
    for (int u = 0; u < GR; u++)
      if (c0 + u < nch) {
#pragma unroll
        for (int s = 0; s < 4; s++) {
          acc0 = M::mma(a0q[sb][u][s], bq[sb][u][s], acc0);
          acc1 = M::mma(a1q[sb][u][s], bq[sb][u][s], acc1);
        }
      }
  };
  load(std::integral_constant<int, 0>(), 0);
  for (uint64_t t0 = jb; t0 < je; t0 += REC_IT) {
    V acc0 = zero, acc1 = zero;
    const real bj = (!SIM && hb) ? g.b[jq] : (real)0;
    real svj = (real)0;
    if constexpr (SIM) svj = hb ? rec_inv(g.sv, jq) : (real)0;
    else if constexpr (NORM) svj = hb ? g.sv[jq] : (real)0;
    for (int c0 = 0; c0 < nch; c0 += 2 * GR) {
      load(std::integral_constant<int, 1>(), c0 + GR);
      mma(std::integral_constant<int, 0>(), c0, acc0, acc1);
      if (c0 + GR >= nch) break;
      load(std::integral_constant<int, 0>(), c0 + 2 * GR);
      mma(std::integral_constant<int, 1>(), c0 + GR, acc0, acc1);
    }
    // the next tile's first group is on its way during the selection
    jq += REC_IT;
    hb = jq < je;
    if (t0 + REC_IT < je) load(std::integral_constant<int, 0>(), 0);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i0 = M::drow(q, r);
      sc[i0][w * 16 + m] = (double)rec_score<MODE>(acc0[r], bj, ai[0][r], sui[0][r], svj);
      sc[16 + i0][w * 16 + m] = (double)rec_score<MODE>(acc1[r], bj, ai[1][r], sui[1][r], svj);
    }
    __syncthreads();
    // wave w takes rows 8 w .. 8 w + 7, lane = the tile's item
    const uint64_t j = t0 + lane;
    for (int rr = 0; rr < REC_RT / 4; rr++) {
      const int il = w * (REC_RT / 4) + rr;
      const uint64_t i = r0 + il;
      if (i >= g.R) break;  // (wave-uniform)
      double v = REC_NEG_INF;
      bool cand = j < je;
      if (coldbits >> rr & 1) {
        cand = cand && j < g.npop;
        if (cand) v = g.popular[j];
      } else {
        v = sc[il][lane];
      }
      consume(il, i, j, v, cand);
    }
    __syncthreads();
  }
}

template <typename real, int KP, RecMode MODE = REC_PLAIN>
__global__ __launch_bounds__(BLOCK) void k_rec_topn(RecArgs<real> g) {
  __shared__ double sc[REC_RT][REC_IT + 1];
  __shared__ double lv[REC_RT][REC_MAX];
  __shared__ uint32_t lj[REC_RT][REC_MAX];
  __shared__ double thr_v[REC_RT];  // each row's current topn-th entry (written by the row's wave)
  __shared__ uint32_t thr_j[REC_RT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned L = blockIdx.x;
  if (L >= g.rt * g.S) return;
  const uint64_t r0 = (uint64_t)(L % g.rt) * REC_RT, sl = L / g.rt;
  for (int t = threadIdx.x; t < REC_RT * REC_MAX; t += BLOCK) {
    lv[t / REC_MAX][t % REC_MAX] = REC_NEG_INF;
    lj[t / REC_MAX][t % REC_MAX] = REC_NONE;
  }
  if (threadIdx.x < REC_RT) {
    thr_v[threadIdx.x] = REC_NEG_INF;
    thr_j[threadIdx.x] = REC_NONE;
  }
  __syncthreads();
  // selection: the threshold first, so the search runs on few candidates
  rec_sweep<real, KP, MODE>(g, r0, sl, sc, [&](int il, uint64_t i, uint64_t j, double v, bool cand) {
    double tv = thr_v[il];
    uint32_t tj = thr_j[il];
    cand = cand && rec_better(v, (uint32_t)j, tv, tj);
    if (cand && g.exclude && rec_in_sorted(g.lcol, g.lptr[i], g.lptr[i + 1], (uint32_t)j)) cand = false;
    const uint64_t mask = __ballot(cand);
    if (!mask) return;
    double v0 = lv[il][lane], v1 = lv[il][lane + 64];
    uint32_t j0 = lj[il][lane], j1 = lj[il][lane + 64];
    rec_offer<false>(mask, v, (uint32_t)j, v0, j0, v1, j1, tv, tj, g.topn, lane);
    lv[il][lane] = v0;
    lv[il][lane + 64] = v1;
    lj[il][lane] = j0;
    lj[il][lane + 64] = j1;
    if (lane == 0) {  // (read again only after the next tile's barriers)
      thr_v[il] = tv;
      thr_j[il] = tj;
    }
  });
  // the slice's list of each row
  for (int rr = 0; rr < REC_RT / 4; rr++) {
    const int il = w * (REC_RT / 4) + rr;
    const uint64_t i = r0 + il;
    if (i >= g.R) break;
    const uint64_t o = (i * g.S + sl) * (uint64_t)g.topn;
    for (int p = lane; p < g.topn; p += 64) {
      g.part_v[o + p] = lv[il][p];
      g.part_j[o + p] = lj[il][p];
    }
  }
}

// The slices' lists of a row merged under the same order: one block per row;
// entry e's final place is the number of entries, over every slice's sorted
// list, that rank before it (a binary search per list; items are distinct
// across slices, so places are distinct).  Places past the candidates hold
// OCFFM_REC_NONE and -inf.
static __global__ __launch_bounds__(BLOCK) void k_rec_merge(uint64_t R, int S, int topn,
                                                            const double *__restrict__ part_v,
                                                            const uint32_t *__restrict__ part_j,
                                                            uint32_t *__restrict__ items, double *__restrict__ scores) {
  const uint64_t i = blockIdx.x;
  if (i >= R) return;
  const double *pv = part_v + i * (uint64_t)S * topn;
  const uint32_t *pj = part_j + i * (uint64_t)S * topn;
  for (int p = threadIdx.x; p < topn; p += BLOCK) {
    items[i * topn + p] = REC_NONE;
    scores[i * topn + p] = REC_NEG_INF;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < S * topn; e += BLOCK) {
    const double v = pv[e];
    const uint32_t j = pj[e];
    if (j == REC_NONE) continue;
    const int own = e / topn;
    int place = e % topn;  // (its own list is sorted: the entries before it)
    for (int s = 0; s < S && place < topn; s++) {
      if (s == own) continue;
      int lo = 0, hi = topn;  // entries of list s ranking before (v, j); unfilled ones rank last
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t mj = pj[s * topn + mid];
        if (mj != REC_NONE && rec_better(pv[s * topn + mid], mj, v, j)) lo = mid + 1;
        else hi = mid;
      }
      place += lo;
    }
    if (place < topn) {
      items[i * topn + place] = j;
      scores[i * topn + place] = v;
    }
  }
}

// ------------------------------------------------- ranking evaluation ---
// Exact rank of every label among its row's candidates
// (ocffm_problem_label_ranks): the label's own score is computed first, then
// one sweep over all items counts, per label, the candidates that come before
// it.  No rows x n array and no top-N list exists.
//
// k_eval_label_scores: a wave takes 16 (row, item) pairs; lane l holds the
// operands of pair l & 15 on both sides of the MFMA and runs k_rec_topn's
// chain (chunks of 16 depth elements in order, then rec_score), so the
// diagonal of the 16 x 16 product holds each pair's score with the bits the
// sweep gives it: an output element depends only on its own row and item.
template <typename real, int KP, RecMode MODE = REC_PLAIN>
__global__ __launch_bounds__(BLOCK) void k_eval_label_scores(uint64_t L, int C, const real *const *__restrict__ P,
                                                             const real *const *__restrict__ Q,
                                                             const real *__restrict__ a, const real *__restrict__ b,
                                                             const uint8_t *__restrict__ cold,
                                                             const double *__restrict__ popular,
                                                             const uint32_t *__restrict__ lrow,
                                                             const uint32_t *__restrict__ litem,
                                                             double *__restrict__ out,
                                                             const real *__restrict__ su,
                                                             const real *__restrict__ sv) {
  using M = RecMma<real>;
  using V = typename M::V;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int m = lane & 15, q = lane >> 4;
  const uint64_t e = ((uint64_t)blockIdx.x * (BLOCK / 64) + w) * 16 + m;
  const bool have = e < L;
  const uint64_t row = have ? lrow[e] : 0, item = have ? litem[e] : 0;
  const int depth = C * KP, nch = (depth + 15) / 16;
  V acc = {(real)0, (real)0, (real)0, (real)0};
  for (int c = 0; c < nch; c++) {
    const V av = rec_ld<real, KP>(P, row, c, q, depth, have), bv = rec_ld<real, KP>(Q, item, c, q, depth, have);
#pragma unroll
    for (int s = 0; s < 4; s++) acc = M::mma(av[s], bv[s], acc);
  }
  if (!have) return;
#pragma unroll
  for (int r = 0; r < 4; r++)
    if (M::drow(q, r) == m) {
      if constexpr (MODE == REC_SIM)
        out[e] = (double)rec_score<REC_SIM>(acc[r], (real)0, (real)0, rec_inv(su, row), rec_inv(sv, item));
      else if constexpr (MODE == REC_NORM)
        out[e] = (double)rec_score<REC_NORM>(acc[r], b[item], a[row], su[row], sv[item]);
      else out[e] = cold[row] ? popular[item] : (double)rec_score<REC_PLAIN>(acc[r], b[item], a[row], (real)0, (real)0);
    }
}

// k_eval_count: k_rec_topn's sweep (rec_sweep: one text, hence the same bits
// for the same (row, item)) with counters in place of the lists.  A
// candidate (s_ij, j) of row i that is inside the slice, a candidate at all
// (j < n; cold rows: j < npop, score popular[j]) and not in the row's sorted
// seen list is located among the row's labels, which are sorted by the same
// order (score descending, item ascending): it adds one to the counter of the
// first label it ranks strictly before; one compare against the row's last
// label drops a candidate that ranks before none.  The prefix sum of a row's
// counters is then each label's rank.  The labels of a row with at most
// EV_LC of them are searched in LDS.  Counters of a row with at most
// EV_CAP labels are kept in LDS and added to the global ones once per block;
// a longer row adds to the global counters directly.  Adds from one tile to
// one counter are merged into one.  Integer adds commute: the result does
// not depend on slicing or scheduling.
constexpr int EV_CAP = 128;
constexpr int EV_LC = 16;  // labels of a row that are also searched in LDS

template <typename real> struct EvalArgs : SweepArgs<real> {  // (lptr / lcol: the seen items)
  const int64_t *kptr;         // each query row's labels in kv / kj / cnt
  const double *kv;            // label scores and items, each row's sorted by the ranking order
  const uint32_t *kj;
  uint32_t *cnt;               // per label: candidates between the label before it and itself
};

template <typename real, int KP, RecMode MODE = REC_PLAIN>
__global__ __launch_bounds__(BLOCK) void k_eval_count(EvalArgs<real> g) {
  __shared__ double sc[REC_RT][REC_IT + 1];
  __shared__ uint32_t cnt[REC_RT][EV_CAP];
  __shared__ double last_v[REC_RT];  // each row's last label
  __shared__ uint32_t last_j[REC_RT];
  __shared__ int64_t k0[REC_RT];
  __shared__ int kn[REC_RT];
  __shared__ double lkv[REC_RT][EV_LC];  // the labels of a row with at most EV_LC of them
  __shared__ uint32_t lkj[REC_RT][EV_LC];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned L = blockIdx.x;
  if (L >= g.rt * g.S) return;
  const uint64_t r0 = (uint64_t)(L % g.rt) * REC_RT, sl = L / g.rt;
  for (int t = threadIdx.x; t < REC_RT * EV_CAP; t += BLOCK) cnt[t / EV_CAP][t % EV_CAP] = 0;
  for (int t = threadIdx.x; t < REC_RT * EV_LC; t += BLOCK) {
    const uint64_t i = r0 + t / EV_LC;
    const int p = t % EV_LC;
    const int64_t b0 = i < g.R ? g.kptr[i] : 0, b1 = i < g.R ? g.kptr[i + 1] : 0;
    const bool in = b1 - b0 <= EV_LC && p < b1 - b0;
    lkv[t / EV_LC][p] = in ? g.kv[b0 + p] : 0.0;
    lkj[t / EV_LC][p] = in ? g.kj[b0 + p] : 0u;
  }
  if (threadIdx.x < REC_RT) {
    const uint64_t i = r0 + threadIdx.x;
    const int64_t b0 = i < g.R ? g.kptr[i] : 0, b1 = i < g.R ? g.kptr[i + 1] : 0;
    k0[threadIdx.x] = b0;
    kn[threadIdx.x] = (int)(b1 - b0);
    last_v[threadIdx.x] = b1 > b0 ? g.kv[b1 - 1] : 0.0;
    last_j[threadIdx.x] = b1 > b0 ? g.kj[b1 - 1] : 0u;
  }
  __syncthreads();
  {  // a row tile without labels has nothing to count (block-uniform)
    int any = 0;
    for (int t = 0; t < REC_RT; t++) any |= kn[t];
    if (!any) return;
  }
  // counting: the last label first, so the search runs on few candidates
  rec_sweep<real, KP, MODE>(g, r0, sl, sc, [&](int il, uint64_t i, uint64_t j, double v, bool cand) {
    const int np = kn[il];
    if (np == 0) return;
    cand = cand && rec_better(v, (uint32_t)j, last_v[il], last_j[il]);
    if (cand && g.exclude && rec_in_sorted(g.lcol, g.lptr[i], g.lptr[i + 1], (uint32_t)j)) cand = false;
    const uint64_t mask = __ballot(cand);
    if (!mask) return;
    const int64_t kb = k0[il];
    int t = 0;
    if (cand) {  // the first label it ranks before (it ranks before the last one)
      int lo = 0, hi = np - 1;
      if (np <= EV_LC) {
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (rec_better(v, (uint32_t)j, lkv[il][mid], lkj[il][mid])) hi = mid;
          else lo = mid + 1;
        }
      } else {
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (rec_better(v, (uint32_t)j, g.kv[kb + mid], g.kj[kb + mid])) hi = mid;
          else lo = mid + 1;
        }
      }
      t = lo;
    }
    const int first = __ffsll((unsigned long long)mask) - 1;
    const int tf = (int)rec_lane((uint32_t)t, first);
    const bool one = __ballot(cand && t != tf) == 0;  // the whole tile before the same label
    const uint32_t add = one ? (uint32_t)__popcll(mask) : 1u;
    if (one ? lane == first : cand) {
      if (np <= EV_CAP) atomicAdd(&cnt[il][t], add);
      else atomicAdd(g.cnt + kb + t, add);
    }
  });
  // (a row's LDS counters are written by the row's wave only)
  for (int rr = 0; rr < REC_RT / 4; rr++) {
    const int il = w * (REC_RT / 4) + rr;
    const int np = kn[il];
    if (np == 0 || np > EV_CAP) continue;
    for (int p = lane; p < np; p += 64) {
      const uint32_t c = cnt[il][p];
      if (c) atomicAdd(g.cnt + k0[il] + p, c);
    }
  }
}

// ------------------------------------------- top-N among candidate lists ---
// Top-N of each query row's own candidate list
// (ocffm_problem_recommend_among).  The work is a gather of item rows, not a
// dense product: no two rows share an item tile, so k_rec_topn's tiling does
// not apply.
//
// k_rerank: one wave owns one work item, a segment of one row's list, and
// walks it 16 candidates at a time.  Lane l holds 4 consecutive depth
// elements (starting at 16 c + 4 (l >> 4) of chunk c) of the wave's one query
// row on the A side and of candidate l & 15's item row on the B side
// (k_eval_label_scores's operand layout with one row for all 16 pairs), and
// runs k_rec_topn's chain: chunks in order, four MFMAs per chunk, then
// rec_score.  Every row of the 16 x 16 product is the query row, so
// each lane reads candidate l & 15's score from its first D register; an
// output element depends only on its own row and item, hence the bits are
// those of recommend.  The query row's first RR_NA chunks stay in registers
// for the whole segment (the kkbox depth, 6 x 32, is exactly RR_NA chunks);
// chunks past them re-read it (it stays in the vector L1).  The item rows of
// those chunks are all requested before the first MFMA: up to RR_NA 16- or
// 32-byte loads per lane in flight.
// Selection: rec_insert's sorted list (two entries per lane) and the row's
// N-th entry live in registers for the whole segment: no LDS, no barrier.  A
// candidate is an entry < n (cold rows: < npop, score popular[j]) that is not
// among the row's sorted labels (exclude).  A copy of an entry already seen
// is either still in the list (one ballot on item equality) or no better than
// the N-th entry (equal items have equal scores), so a duplicate counts once.
// A row with one work item writes its result; the others write partial lists
// that k_rerank_merge offers, in work item order, to one list per row under
// the same rules, so copies in different segments count once as well.
// Selection is on the strict total order (score, item) over distinct items,
// hence independent of the list's order and of how it was split.
// Ragged edges: list entries outside a work item's range are never read, nor
// are item rows of entries that are no candidates.
constexpr int RR_NA = 12;

template <typename real> struct RerankArgs {
  uint64_t W, w0;              // work items of this launch; the first one's index in wrow / wbeg / wlen
  uint64_t r0, c0;             // first row of this launch (out is relative to it); first list entry in ccol
  uint64_t n, npop;
  int C, topn, exclude;
  const real *const *P;        // C user-side cross tables of the call's rows
  const real *const *Q;        // C item-side cross tables (n x KP)
  const real *a, *b;           // a_i of the call's rows, b_j
  const uint8_t *cold;         // per row of the call
  const double *popular;
  const int64_t *lptr;         // sorted, distinct labels < n of each row of the call (exclude)
  const uint32_t *lcol;
  const real *su, *sv;         // REC_NORM: squared norms of the call's rows, of the items
  const int64_t *wptr;         // per row of the call: its work items [wptr[i], wptr[i + 1])
  const uint32_t *wrow;        // work item -> row of the call
  const uint64_t *wbeg;        // work item -> its first list entry (an index of the call's ccol)
  const uint32_t *wlen;        // work item -> entries
  const uint32_t *ccol;        // this launch's list entries (entry c0 first)
  double *part_v, *out_v;      // W x topn partial lists; rows x topn results
  uint32_t *part_j, *out_j;
};

template <typename real, int KP, RecMode MODE = REC_PLAIN>
__global__ __launch_bounds__(BLOCK) void k_rerank(RerankArgs<real> g) {
  static_assert(MODE != REC_SIM, "the list kernels have no similarity mode");
  constexpr bool NORM = MODE == REC_NORM;
  using M = RecMma<real>;
  using V = typename M::V;
  const int lane = threadIdx.x & 63;
  const int m = lane & 15, q = lane >> 4;
  const uint64_t wl = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if (wl >= g.W) return;  // (wave-uniform)
  const uint64_t w = g.w0 + wl;
  const uint64_t i = g.wrow[w];
  const uint64_t cb = g.wbeg[w] - g.c0;
  const uint32_t len = g.wlen[w];
  const bool cold = g.cold[i] != 0;
  const uint64_t lim = cold ? g.npop : g.n;
  const int depth = g.C * KP, nch = (depth + 15) / 16;
  V aq[RR_NA];
#pragma unroll
  for (int c = 0; c < RR_NA; c++) aq[c] = rec_ld<real, KP>(g.P, i, c, q, depth, !cold);
  const real ai = g.a[i];
  const real sui = NORM ? g.su[i] : (real)0;
  const int64_t lb = g.exclude ? g.lptr[i] : 0, le = g.exclude ? g.lptr[i + 1] : 0;
  double v0 = REC_NEG_INF, v1 = REC_NEG_INF, tv = REC_NEG_INF;
  uint32_t j0 = REC_NONE, j1 = REC_NONE, tj = REC_NONE;
  uint32_t jn = (uint32_t)m < len ? g.ccol[cb + m] : REC_NONE;
  for (uint32_t t0 = 0; t0 < len; t0 += 16) {
    const bool have = t0 + m < len;
    const uint32_t j = jn;
    // the next 16 entries are on their way while these are scored
    jn = (uint64_t)t0 + 16 + m < len ? g.ccol[cb + t0 + 16 + m] : REC_NONE;
    bool valid = have && j < lim;
    if (valid && rec_in_sorted(g.lcol, lb, le, j)) valid = false;
    double v = REC_NEG_INF;
    if (cold) {
      if (valid) v = g.popular[j];
    } else {
      V bq[RR_NA];
#pragma unroll
      for (int c = 0; c < RR_NA; c++) bq[c] = rec_ld<real, KP>(g.Q, j, c, q, depth, valid);
      V acc = {(real)0, (real)0, (real)0, (real)0};
#pragma unroll
      for (int c = 0; c < RR_NA; c++)
        if (c < nch) {
#pragma unroll
          for (int s = 0; s < 4; s++) acc = M::mma(aq[c][s], bq[c][s], acc);
        }
      for (int c = RR_NA; c < nch; c++) {
        const V av = rec_ld<real, KP>(g.P, i, c, q, depth, true), bv = rec_ld<real, KP>(g.Q, j, c, q, depth, valid);
#pragma unroll
        for (int s = 0; s < 4; s++) acc = M::mma(av[s], bv[s], acc);
      }
      if (valid) v = (double)rec_score<MODE>(acc[0], g.b[j], ai, sui, NORM ? g.sv[j] : (real)0);
    }
    const bool cand = valid && q == 0 && rec_better(v, j, tv, tj);
    rec_offer<true>(__ballot(cand), v, j, v0, j0, v1, j1, tv, tj, g.topn, lane);
  }
  const bool whole = g.wptr[i + 1] - g.wptr[i] == 1;  // the row's only work item: its list is the result
  double *dv = whole ? g.out_v + (i - g.r0) * (uint64_t)g.topn : g.part_v + wl * (uint64_t)g.topn;
  uint32_t *dj = whole ? g.out_j + (i - g.r0) * (uint64_t)g.topn : g.part_j + wl * (uint64_t)g.topn;
  if (lane < g.topn) {
    dv[lane] = v0;
    dj[lane] = j0;
  }
  if (lane + 64 < g.topn) {
    dv[lane + 64] = v1;
    dj[lane + 64] = j1;
  }
}

// The partial lists of a row's work items merged into its result: one wave
// per row offers every entry, in work item order, to one list (rec_offer<true>:
// a copy counts once).  A row with one work item already has its result; a
// row with none gets OCFFM_REC_NONE and -inf.
static __global__ __launch_bounds__(BLOCK) void k_rerank_merge(uint64_t R, uint64_t r0, uint64_t w0, int topn,
                                                               const int64_t *__restrict__ wptr,
                                                               const double *__restrict__ part_v,
                                                               const uint32_t *__restrict__ part_j,
                                                               uint32_t *__restrict__ items,
                                                               double *__restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const uint64_t il = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if (il >= R) return;  // (wave-uniform)
  const int64_t wb = wptr[r0 + il], we = wptr[r0 + il + 1];
  if (we - wb == 1) return;
  double v0 = REC_NEG_INF, v1 = REC_NEG_INF, tv = REC_NEG_INF;
  uint32_t j0 = REC_NONE, j1 = REC_NONE, tj = REC_NONE;
  const uint64_t eb = (uint64_t)(wb - (int64_t)w0) * topn, ee = (uint64_t)(we - (int64_t)w0) * topn;
  for (uint64_t e0 = eb; e0 < ee; e0 += 64) {
    const bool have = e0 + lane < ee;
    const uint32_t j = have ? part_j[e0 + lane] : REC_NONE;
    const double v = have ? part_v[e0 + lane] : REC_NEG_INF;
    const bool cand = j != REC_NONE && rec_better(v, j, tv, tj);
    rec_offer<true>(__ballot(cand), v, j, v0, j0, v1, j1, tv, tj, topn, lane);
  }
  if (lane < topn) {
    scores[il * topn + lane] = v0;
    items[il * topn + lane] = j0;
  }
  if (lane + 64 < topn) {
    scores[il * topn + lane + 64] = v1;
    items[il * topn + lane + 64] = j1;
  }
}

// ------------------------------------- label ranks among candidate lists ---
// Exact rank of every label among its row's own candidate set
// (ocffm_problem_label_ranks_among): k_rerank's gather with k_eval_count's
// counters in place of the list.
//
// k_rerank_count: one wave owns one work item, a segment of one row's
// candidate set K_i, and walks it 16 entries at a time with k_rerank's
// operand layout, resident query chunks (RR_NA) and chain, then rec_score: an
// entry's score has recommend's bits.  The host hands over K_i itself (the
// distinct list entries that are candidates, united with the row's candidate
// labels: rank_driver.hpp), so every entry counts, once.  An entry (s_ij, j)
// is located among the row's labels, which are sorted by the ranking order
// (kv / kj): one compare against the row's last label drops an entry that
// ranks before none, a binary search finds the first label the others rank
// strictly before, and that label's counter gets one more.  The prefix sum of
// a row's counters is then each label's rank.  Adds of one step to one
// counter are merged, and a run of steps that all go to the same counter (the
// usual case: one positive per row) is held in a wave-uniform register and
// added once.  Cold rows take popular[j] and gather nothing.  Integer adds
// commute: the result does not depend on the list's order, on how it was cut
// into segments or on scheduling.
// Ragged edges: entries outside a work item's range are never read, nor are
// item rows of lanes past the segment's end.
template <typename real> struct RerankCountArgs {
  uint64_t W, w0;              // work items of this launch; the first one's index in wrow / wbeg / wlen
  uint64_t c0;                 // first entry of this launch in the call's sets (ccol is relative to it)
  int C;
  const real *const *P;        // C user-side cross tables of the call's rows
  const real *const *Q;        // C item-side cross tables (n x KP)
  const real *a, *b;           // a_i of the call's rows, b_j
  const uint8_t *cold;         // per row of the call
  const double *popular;
  const real *su, *sv;         // REC_NORM: squared norms of the call's rows, of the items
  const uint32_t *wrow;        // work item -> row of the call
  const uint64_t *wbeg;        // work item -> its first entry (an index of the call's sets)
  const uint32_t *wlen;        // work item -> entries
  const uint32_t *ccol;        // this launch's entries (entry c0 first): distinct candidates of their row
  const int64_t *kptr;         // each row's labels in kv / kj / cnt (a row with work items has some)
  const double *kv;            // label scores and items, each row's sorted by the ranking order
  const uint32_t *kj;
  uint32_t *cnt;               // per label: candidates between the label before it and itself
};

template <typename real, int KP, RecMode MODE = REC_PLAIN>
__global__ __launch_bounds__(BLOCK) void k_rerank_count(RerankCountArgs<real> g) {
  static_assert(MODE != REC_SIM, "the list kernels have no similarity mode");
  constexpr bool NORM = MODE == REC_NORM;
  using M = RecMma<real>;
  using V = typename M::V;
  const int lane = threadIdx.x & 63;
  const int m = lane & 15, q = lane >> 4;
  const uint64_t wl = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if (wl >= g.W) return;  // (wave-uniform)
  const uint64_t w = g.w0 + wl;
  const uint64_t i = g.wrow[w];
  const uint64_t cb = g.wbeg[w] - g.c0;
  const uint32_t len = g.wlen[w];
  const int64_t kb = g.kptr[i];
  const int np = (int)(g.kptr[i + 1] - kb);
  if (np <= 0 || len == 0) return;  // (wave-uniform; the host makes no such work item)
  const bool cold = g.cold[i] != 0;
  const int depth = g.C * KP, nch = (depth + 15) / 16;
  V aq[RR_NA];
#pragma unroll
  for (int c = 0; c < RR_NA; c++) aq[c] = rec_ld<real, KP>(g.P, i, c, q, depth, !cold);
  const real ai = g.a[i];
  const real sui = NORM ? g.su[i] : (real)0;
  const double last_v = g.kv[kb + np - 1];
  const uint32_t last_j = g.kj[kb + np - 1];
  int pt = -1;      // the counter the pending adds go to (wave-uniform)
  uint32_t pn = 0;  // pending adds
  uint32_t jn = (uint32_t)m < len ? g.ccol[cb + m] : REC_NONE;
  for (uint32_t t0 = 0; t0 < len; t0 += 16) {
    const bool have = t0 + m < len;
    const uint32_t j = jn;
    // the next 16 entries are on their way while these are scored
    jn = (uint64_t)t0 + 16 + m < len ? g.ccol[cb + t0 + 16 + m] : REC_NONE;
    double v = REC_NEG_INF;
    if (cold) {
      if (have) v = g.popular[j];
    } else {
      V bq[RR_NA];
#pragma unroll
      for (int c = 0; c < RR_NA; c++) bq[c] = rec_ld<real, KP>(g.Q, j, c, q, depth, have);
      V acc = {(real)0, (real)0, (real)0, (real)0};
#pragma unroll
      for (int c = 0; c < RR_NA; c++)
        if (c < nch) {
#pragma unroll
          for (int s = 0; s < 4; s++) acc = M::mma(aq[c][s], bq[c][s], acc);
        }
      for (int c = RR_NA; c < nch; c++) {
        const V av = rec_ld<real, KP>(g.P, i, c, q, depth, true), bv = rec_ld<real, KP>(g.Q, j, c, q, depth, have);
#pragma unroll
        for (int s = 0; s < 4; s++) acc = M::mma(av[s], bv[s], acc);
      }
      if (have) v = (double)rec_score<MODE>(acc[0], g.b[j], ai, sui, NORM ? g.sv[j] : (real)0);
    }
    // counting: the last label first, so the search runs on few entries
    const bool cand = have && q == 0 && rec_better(v, j, last_v, last_j);
    const uint64_t mask = __ballot(cand);
    if (!mask) continue;
    int t = 0;
    if (cand) {  // the first label it ranks before (it ranks before the last one)
      int lo = 0, hi = np - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rec_better(v, j, g.kv[kb + mid], g.kj[kb + mid])) hi = mid;
        else lo = mid + 1;
      }
      t = lo;
    }
    const int first = __ffsll((unsigned long long)mask) - 1;
    const int tf = (int)rec_lane((uint32_t)t, first);
    const bool one = __ballot(cand && t != tf) == 0;  // the whole step before the same label
    if (one) {
      if (tf != pt) {
        if (pn && lane == 0) atomicAdd(g.cnt + kb + pt, pn);
        pt = tf;
        pn = 0;
      }
      pn += (uint32_t)__popcll(mask);
    } else if (cand) {
      atomicAdd(g.cnt + kb + t, 1u);
    }
  }
  if (pn && lane == 0) atomicAdd(g.cnt + kb + pt, pn);
}

}  // namespace ocffm
