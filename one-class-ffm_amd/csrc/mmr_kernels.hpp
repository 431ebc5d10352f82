// mmr_kernels.hpp — diversified top-N (ocffm_diverse.h): greedy
// maximal-marginal-relevance re-ranking of each row's pool, the top-`pool`
// list the serving sweep (or the list path) has just left on the device.
// Included by model.hip.
#pragma once

#include "rank_kernels.hpp"

namespace ocffm {

// What k_mmr needs: a chunk's pool lists and where its selection goes
template <typename real> struct MmrArgs {
  uint64_t R;                  // rows of the chunk (one workgroup each)
  int C, pool, topn, ld;       // cross tables; pool entries per row; picks per row; row stride of sim in LDS
  const real *const *Q;        // C item-side cross tables (n x KP)
  const real *inv;             // the items' inverse norms (n)
  const uint32_t *pool_j;      // R x pool: each row's pool, filled slots first
  const double *pool_v;        // their scores, descending
  double w, theta;             // w = 1 - theta (the host's)
  uint32_t *items, *pos;       // R x topn
  double *scores, *mmr;
};

// Rows of sim in LDS are ld reals apart: the padded pool plus one, so the
// mirrored stores of a tile (a lane group's 16 lanes walk a column) spread
// over the banks
inline int mmr_ld(uint32_t pool) { return (int)((pool + 15) / 16 * 16 + 1); }
template <typename real> inline size_t mmr_lds_bytes(uint32_t pool) {
  return (size_t)((pool + 15) / 16 * 16) * (size_t)mmr_ld(pool) * sizeof(real);
}

// v = w rel - theta ms: two products and a difference, each rounded on its own
__device__ __forceinline__ double mmr_value(double w, double rel, double theta, double ms) {
#pragma clang fp contract(off)
  const double a = w * rel;
  const double b = theta * ms;
  return a - b;
}
// rel = (s - last) / range, 0 where the pool's scores are all equal
__device__ __forceinline__ double mmr_rel(double s, double last, double range) {
#pragma clang fp contract(off)
  const double d = s - last;
  return range == 0.0 ? 0.0 : d / range;
}

// k_mmr: one workgroup per query row of the chunk.
// Load: the row's pool items, their scores and inverse norms go to LDS; c is
// the number of filled slots (they come first).
// Similarities: the 16 x 16 tiles (ti <= tj) of the c x c matrix are dealt to
// the four waves in turn.  A lane holds the A operand of pool row 16 ti +
// (lane & 15) and the B operand of pool row 16 tj + (lane & 15), both straight
// from the catalogue tables (rec_ld), and runs k_eval_label_scores's chain:
// chunks of 16 depth elements in order, four MFMAs per chunk, the loads of
// RecMma::GR chunks requested together.  D register r of lane (q, m) is
// element (16 ti + drow(q, r), 16 tj + m); rec_score<REC_SIM> with the two
// items' inverse norms gives ocffm_model_item_similarity's bits, since an
// MFMA output element depends only on its own row and column.  The value is
// stored at (row, column) and, off the diagonal tiles, at (column, row): sim is
// symmetric bit for bit.  Pool rows >= c are neither loaded nor stored.
// Greedy: wave 0 alone, after the one barrier; lane l owns pool positions l
// and l + 64 (rec_insert's layout) and keeps their rel, max-sim and taken
// flags in registers; each step reads the newly taken row of sim from LDS,
// forms v (mmr_value) and finds the pick by a wave arg-max on (v descending,
// position ascending).  Lane 0 writes the step's outputs.  No barrier inside
// the loop, no floating-point atomics, no scratch.
// Algorithmic bytes: a row's c item rows of C KP reals (re-read per tile out
// of L2), 12 pool B read and 24 topn B written.
template <typename real, int KP>
__global__ __launch_bounds__(BLOCK) void k_mmr(MmrArgs<real> g) {
  using M = RecMma<real>;
  using V = typename M::V;
  constexpr int GR = M::GR;
  extern __shared__ __attribute__((aligned(16))) unsigned char mmr_lds[];
  real *sim = reinterpret_cast<real *>(mmr_lds);
  __shared__ uint32_t sj[REC_MAX];
  __shared__ double ss[REC_MAX];
  __shared__ real sinv[REC_MAX];
  __shared__ int cnt;
  const uint64_t row = blockIdx.x;
  if (row >= g.R) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int m = lane & 15, q = lane >> 4;
  // ---- load
  if (tid == 0) cnt = g.pool;
  __syncthreads();
  if (tid < g.pool) {
    const uint32_t j = g.pool_j[row * g.pool + tid];
    sj[tid] = j;
    ss[tid] = g.pool_v[row * g.pool + tid];
    sinv[tid] = j != REC_NONE ? g.inv[j] : (real)0;
    if (j == REC_NONE) atomicMin(&cnt, tid);
  }
  __syncthreads();
  const int c = cnt;  // (block-uniform)
  // ---- similarities
  const int nt = (c + 15) / 16, depth = g.C * KP, nch = (depth + 15) / 16;
  int t = 0;
  for (int ti = 0; ti < nt; ti++)
    for (int tj = ti; tj < nt; tj++, t++) {
      if ((t & (BLOCK / 64 - 1)) != w) continue;  // (wave-uniform)
      const int ra = 16 * ti + m, rb = 16 * tj + m;
      const bool oka = ra < c, okb = rb < c;
      const uint64_t ja = oka ? sj[ra] : 0, jb = okb ? sj[rb] : 0;
      V acc = {(real)0, (real)0, (real)0, (real)0};
      for (int c0 = 0; c0 < nch; c0 += GR) {
        V av[GR], bv[GR];
#pragma unroll
        for (int u = 0; u < GR; u++) {
          av[u] = rec_ld<real, KP>(g.Q, ja, c0 + u, q, depth, oka);
          bv[u] = rec_ld<real, KP>(g.Q, jb, c0 + u, q, depth, okb);
        }
#pragma unroll
        for (int u = 0; u < GR; u++)
          if (c0 + u < nch) {
#pragma unroll
            for (int s = 0; s < 4; s++) acc = M::mma(av[u][s], bv[u][s], acc);
          }
      }
      if (okb) {
        const real ib = sinv[rb];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int pa = 16 * ti + M::drow(q, r);
          if (pa >= c) continue;
          const real s = rec_score<REC_SIM>(acc[r], (real)0, (real)0, sinv[pa], ib);
          sim[pa * g.ld + rb] = s;
          if (ti != tj) sim[rb * g.ld + pa] = s;
        }
      }
    }
  __syncthreads();
  if (w != 0) return;
  // ---- greedy selection
  const int npick = c < g.topn ? c : g.topn;
  uint32_t *oi = g.items + row * g.topn, *op = g.pos + row * g.topn;
  double *os = g.scores + row * g.topn, *om = g.mmr + row * g.topn;
  for (int e = npick + lane; e < g.topn; e += 64) {
    oi[e] = REC_NONE;
    op[e] = REC_NONE;
    os[e] = REC_NEG_INF;
    om[e] = REC_NEG_INF;
  }
  if (npick == 0) return;
  const int p0 = lane, p1 = lane + 64;
  bool f0 = p0 < c, f1 = p1 < c;  // still to be taken
  const double last = ss[c - 1], range = ss[0] - last;  // (a difference alone: nothing to contract)
  const double rel0 = f0 ? mmr_rel(ss[p0], last, range) : 0.0, rel1 = f1 ? mmr_rel(ss[p1], last, range) : 0.0;
  double ms0 = REC_NEG_INF, ms1 = REC_NEG_INF;
  int u = 0;  // the position just taken (wave-uniform)
  if (lane == 0) {
    oi[0] = sj[0];
    op[0] = 0;
    os[0] = ss[0];
    om[0] = g.w * rel0;
    f0 = false;
  }
  for (int step = 1; step < npick; step++) {
    double v = REC_NEG_INF;
    int p = 0x7fffffff;
    if (f1) {  // (the higher position first: an equal v at p0 replaces it)
      const double s = (double)sim[u * g.ld + p1];
      ms1 = s > ms1 ? s : ms1;
      v = mmr_value(g.w, rel1, g.theta, ms1);
      p = p1;
    }
    if (f0) {
      const double s = (double)sim[u * g.ld + p0];
      ms0 = s > ms0 ? s : ms0;
      const double v0 = mmr_value(g.w, rel0, g.theta, ms0);
      if (!f1 || v0 >= v) {
        v = v0;
        p = p0;
      }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double ov = __shfl_xor(v, d, 64);
      const int opp = __shfl_xor(p, d, 64);
      if (ov > v || (ov == v && opp < p)) {
        v = ov;
        p = opp;
      }
    }
    u = __builtin_amdgcn_readfirstlane(p);
    if ((unsigned)u >= (unsigned)c) {  // no position compares (a NaN score or table): the rest stays empty
      for (int e = step + lane; e < npick; e += 64) {
        oi[e] = REC_NONE;
        op[e] = REC_NONE;
        os[e] = REC_NEG_INF;
        om[e] = REC_NEG_INF;
      }
      return;
    }
    if (p0 == u) f0 = false;
    if (p1 == u) f1 = false;
    if (lane == 0) {
      oi[step] = sj[u];
      op[step] = (uint32_t)u;
      os[step] = ss[u];
      om[step] = v;
    }
  }
}

}  // namespace ocffm
