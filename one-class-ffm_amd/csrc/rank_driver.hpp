// rank_driver.hpp — the host driver of the serving kernels (rank_kernels.hpp):
// row chunking and item slicing, the sweeps' arguments, recommend's partial
// lists and merge, label_ranks' bookkeeping, per-row sort, count step (the
// sweep, or the gather over per-row candidate sets) and prefix sums, the
// scores of given pairs, and the list path: segments, chunks, scratch and
// merge of recommend_among.  It works on a view of a model
// (RankModel) and of the query rows (RankRows), so the block Newton-CG
// problem (solver.hip) and the SGD trainer (sgd.hip) run the same text.
//
// Host: what the driver needs of its caller:
//   launch(kernel, grid, block, smem, args...)   a launch on the model's stream
//   prof_launch(family, bytes, body, flops)      the timing hook around body's launches
//   flush_prof()                                 after the last launch of a call
//   resident(kernel, smem)                       blocks of kernel resident on the GPU
//   sync()                                       wait for the stream
//   rank_setup_done(counter)                     the call's host set-up ends here
// MODE (rank_kernels.hpp RecMode, rec_score): REC_PLAIN for the Newton
// problem and the model handle, REC_NORM for the normalised scores of the SGD
// model, REC_SIM for the model handle's item-item similarities, which use
// recommend() and score_pairs() alone (the other entries' kernels have no such
// instantiation).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <limits>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.hpp"
#include "rank_kernels.hpp"

namespace ocffm {

// OCFFM_EXP_KP32 (experiment builds only, tools/build_variant.sh): fp32 at
// KP = 32 instantiated alone, so a kernel experiment compiles in a fraction
// of the full build's time.
template <class F> static void with_kp(uint32_t kp, F &&f) {
#ifdef OCFFM_EXP_KP32
  if (kp != 32) throw Error(OCFFM_E_ARG, "experiment build: k must pad to 32");
  f(std::integral_constant<int, 32>());
  return;
#endif
  switch (kp) {
    case 4: f(std::integral_constant<int, 4>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 32: f(std::integral_constant<int, 32>()); break;
    case 64: f(std::integral_constant<int, 64>()); break;
    case 128: f(std::integral_constant<int, 128>()); break;
    default: throw Error(OCFFM_E_ARG, "k must be in 1..128");
  }
}

// The list arguments of the *_among calls: rows + 1 non-decreasing offsets from 0
inline void check_lists(const uint64_t *cptr, const uint32_t *ccol, uint64_t rows) {
  if (!cptr) throw Error(OCFFM_E_ARG, "null cptr");
  if (cptr[0] != 0) throw Error(OCFFM_E_ARG, "cptr[0] must be 0");
  for (uint64_t i = 0; i < rows; i++)
    if (cptr[i + 1] < cptr[i]) throw Error(OCFFM_E_ARG, "cptr must not decrease");
  if (cptr[rows] > 0 && !ccol) throw Error(OCFFM_E_ARG, "null ccol");
}

// The item side of a model and how its sweeps and lists are cut
template <typename real> struct RankModel {
  const real *const *Q = nullptr;    // C item-side cross tables (n x kp)
  const real *b = nullptr;           // b_j
  const real *sv = nullptr;          // REC_NORM: the items' squared norms; REC_SIM: their inverse norms (null: 1)
  const double *popular = nullptr;   // cold rows' scores (no cold rows: null)
  uint64_t n = 0, npop = 0;          // items; popularity entries (<= n)
  uint32_t C = 0, kp = 0;
  unsigned slices = 0;               // OCFFM_REC_SLICES (0: from n, the rows and the CU count)
  uint64_t chunk_rows = 0;           // OCFFM_REC_ROWS (0: 4096 rows per chunk)
  uint64_t rec_seg = 0;              // OCFFM_REC_SEG (0: from the call's entries and the resident waves)
  hipStream_t stream = nullptr;

  // OCFFM_REC_SEG as the hosts read it at create: a multiple of 16 entries
  static uint64_t seg_from_env() {
    const char *e = std::getenv("OCFFM_REC_SEG");
    return e ? (std::clamp<uint64_t>(std::strtoull(e, nullptr, 10), 1, 1u << 30) + 15) / 16 * 16 : 0;
  }
};

// The query rows of a call: their side of the model, the cold flags and the
// sorted distinct items < n of each row to leave out
template <typename real> struct RankRows {
  const real *const *P = nullptr;    // C user-side cross tables of the rows (rows x kp)
  const real *a = nullptr;           // a_i
  const real *su = nullptr;          // REC_NORM: the rows' squared norms; REC_SIM: their inverse norms (null: 1)
  std::vector<uint8_t> cold;         // (all zero without cold rows)
  DevBuf<uint8_t> dcold;
  std::vector<int64_t> lptr;
  std::vector<uint32_t> lcol;
  DevBuf<int64_t> dlptr;
  DevBuf<uint32_t> dlcol;

  // the labels < n of rows [row0, row0 + rows) of lab (NULL: none), sorted and distinct
  void exclusions(const HostData *lab, uint64_t row0, uint64_t rows, uint64_t n) {
    lptr.assign(rows + 1, 0);
    lcol.clear();
    if (lab)
      for (uint64_t i = 0; i < rows; i++) {
        const size_t b = lcol.size();
        for (uint64_t p = lab->yptr[row0 + i]; p < lab->yptr[row0 + i + 1]; p++)
          if (lab->ycol[p] < n) lcol.push_back((uint32_t)lab->ycol[p]);
        std::sort(lcol.begin() + b, lcol.end());
        lcol.erase(std::unique(lcol.begin() + b, lcol.end()), lcol.end());
        lptr[i + 1] = (int64_t)lcol.size();
      }
    if (lcol.empty()) lcol.push_back(0);
    dlptr.upload(lptr);
    dlcol.upload(lcol);
  }
};

// Row chunk and item slices of a sweep (k_rec_topn, k_eval_count)
struct RankPlan {
  uint64_t chunk, S, per;  // rows per launch; item slices; items per slice (multiple of REC_IT)
};

// The post-chunk hook of recommend / rerank: post(c0, cr, out_j, out_v) runs
// inside the chunk's timed launches, after its last launch, with the chunk's
// device lists (cr x topn items and scores, rows c0.. of the call); it adds its
// own launches and returns the device-to-host copies that take the place of
// copy_back (a null dst is skipped).  RankNoPost: no hook, copy_back as ever.
struct RankCopy {
  const void *src;
  void *dst;
  size_t bytes;
};
struct RankNoPost {};

template <typename real, RecMode MODE, class Host> struct RankDriver {
  Host &h;
  const RankModel<real> &m;

  uint64_t chunk(uint64_t rows) const { return std::min<uint64_t>(rows, m.chunk_rows ? m.chunk_rows : 4096); }
  // Resident blocks of a kernel with a KP parameter (kernel_of(K): its instantiation)
  template <class KOf> unsigned resident(KOf &&kernel_of) {
    unsigned slots = 0;
    with_kp(m.kp, [&](auto K) { slots = h.resident(kernel_of(K), 0); });
    return slots;
  }
  template <class KOf> RankPlan plan(uint64_t rows, KOf &&kernel_of) {
    RankPlan p;
    p.chunk = chunk(rows);
    p.S = m.slices;
    if (!p.S) {
      // one resident wave of blocks: every slice costs each row its own
      // list warm-up (~topn inserts), so as few slices as fill the machine;
      // at least 4 item tiles per slice
      p.S = std::max<uint64_t>(1, resident(kernel_of) / ((p.chunk + REC_RT - 1) / REC_RT));
      p.S = std::min<uint64_t>(p.S, (m.n + 4 * REC_IT - 1) / (4 * REC_IT));
      p.S = std::clamp<uint64_t>(p.S, 1, 64);
    }
    p.per = ((m.n + p.S - 1) / p.S + REC_IT - 1) / REC_IT * REC_IT;
    return p;
  }
  // A sweep's arguments for rows [c0, c0 + cr) of L
  void sweep_args(SweepArgs<real> &g, const RankRows<real> &L, uint64_t c0, uint64_t cr, const RankPlan &p,
                  bool exclude) {
    g.R = cr;
    g.p0 = c0;
    g.n = m.n;
    g.npop = m.npop;
    g.per = p.per;
    g.C = (int)m.C;
    g.exclude = exclude ? 1 : 0;
    g.S = (uint32_t)p.S;
    g.rt = (uint32_t)((cr + REC_RT - 1) / REC_RT);
    g.P = L.P;
    g.Q = m.Q;
    g.a = L.a + c0;
    g.b = m.b;
    g.cold = L.dcold.p + c0;
    g.popular = m.popular;
    g.lptr = L.dlptr.p + c0;
    g.lcol = L.dlcol.p;
    g.su = (MODE != REC_PLAIN && L.su) ? L.su + c0 : nullptr;
    g.sv = m.sv;
  }
  // Scores of the pairs (krow[e] of L, kitem[e]), every one a candidate, timed under `family`
  std::vector<double> score_pairs(const RankRows<real> &L, const std::vector<uint32_t> &krow,
                                  const std::vector<uint32_t> &kitem, const char *family) {
    const uint64_t nk = kitem.size();
    DevBuf<uint32_t> dkrow, dkitem;
    DevBuf<double> dkv;
    dkrow.upload(krow);
    dkitem.upload(kitem);
    dkv.alloc(nk, false);
    const double depth = (double)m.C * m.kp;
    h.prof_launch(family, (double)nk * (2 * depth * sizeof(real) + sizeof(double) + 2 * sizeof(uint32_t)), [&] {
      with_kp(m.kp, [&](auto K) {
        constexpr int KP = decltype(K)::value;
        h.launch(k_eval_label_scores<real, KP, MODE>, (unsigned)((nk + 63) / 64), BLOCK, 0, nk, (int)m.C,
                 (const real *const *)L.P, (const real *const *)m.Q, (const real *)L.a, (const real *)m.b,
                 (const uint8_t *)L.dcold.p, (const double *)m.popular, (const uint32_t *)dkrow.p,
                 (const uint32_t *)dkitem.p, dkv.p, (const real *)L.su, (const real *)m.sv);
      });
    }, 2.0 * (double)nk * depth);
    std::vector<double> kv(nk);
    HIPCHK(hipMemcpyAsync(kv.data(), dkv.p, nk * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    h.sync();
    return kv;
  }
  // A chunk's results (rows c0.. of the call) to the caller's arrays
  void copy_back(uint64_t c0, uint64_t cr, uint32_t topn, const DevBuf<uint32_t> &out_j, const DevBuf<double> &out_v,
                 uint32_t *items, double *scores) {
    HIPCHK(hipMemcpyAsync(items + c0 * topn, out_j.p, cr * topn * sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream));
    if (scores)
      HIPCHK(hipMemcpyAsync(scores + c0 * topn, out_v.p, cr * topn * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    h.sync();
  }

  // A hook's copies (RankCopy) in copy_back's place
  void copy_back(const std::vector<RankCopy> &cp) {
    for (const RankCopy &c : cp)
      if (c.dst && c.bytes) HIPCHK(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, m.stream));
    h.sync();
  }
  // The end of a chunk: the hook's launches (call this inside the timed body) ...
  template <class Post>
  std::vector<RankCopy> run_post(Post &&post, uint64_t c0, uint64_t cr, const DevBuf<uint32_t> &out_j,
                                 const DevBuf<double> &out_v) {
    if constexpr (std::is_same<std::decay_t<Post>, RankNoPost>::value) return {};
    else return post(c0, cr, (const uint32_t *)out_j.p, (const double *)out_v.p);
  }
  // ... and the chunk's results to the host
  template <class Post>
  void finish_chunk(const std::vector<RankCopy> &cp, uint64_t c0, uint64_t cr, uint32_t topn,
                    const DevBuf<uint32_t> &out_j, const DevBuf<double> &out_v, uint32_t *items, double *scores) {
    if constexpr (std::is_same<std::decay_t<Post>, RankNoPost>::value) copy_back(c0, cr, topn, out_j, out_v, items, scores);
    else copy_back(cp);
  }

  // ---------------------------------------------------- recommendation
  // Top-N items of the rows of L.  The rows are scored in chunks: scratch is
  // chunk x slices x topn partial entries, never rows x n.
  // prep(g, c0, cr), inside the chunk's timed launches and before its sweep:
  // the caller's own launches for rows [c0, c0 + cr) and changes to the
  // sweep's arguments (similar_items gathers the chunk's query rows there).
  void recommend(const RankRows<real> &L, uint64_t rows, uint32_t topn, bool excl, uint32_t *items, double *scores,
                 const char *setup_counter) {
    recommend(L, rows, topn, excl, items, scores, setup_counter, "recommend", [](RecArgs<real> &, uint64_t, uint64_t) {});
  }
  template <class Prep>
  void recommend(const RankRows<real> &L, uint64_t rows, uint32_t topn, bool excl, uint32_t *items, double *scores,
                 const char *setup_counter, const char *family, Prep &&prep) {
    recommend(L, rows, topn, excl, items, scores, setup_counter, family, prep, RankNoPost{});
  }
  // post: the post-chunk hook (RankCopy above); items / scores are then unused
  template <class Prep, class Post>
  void recommend(const RankRows<real> &L, uint64_t rows, uint32_t topn, bool excl, uint32_t *items, double *scores,
                 const char *setup_counter, const char *family, Prep &&prep, Post &&post) {
    const RankPlan pl = plan(rows, [](auto K) { return k_rec_topn<real, decltype(K)::value, MODE>; });
    const uint64_t chunk = pl.chunk, S = pl.S;
    DevBuf<double> part_v, out_v;
    DevBuf<uint32_t> part_j, out_j;
    part_v.alloc(chunk * S * topn, false);
    part_j.alloc(chunk * S * topn, false);
    out_v.alloc(chunk * topn, false);
    out_j.alloc(chunk * topn, false);
    h.sync();
    h.rank_setup_done(setup_counter);
    for (uint64_t c0 = 0; c0 < rows; c0 += chunk) {
      const uint64_t cr = std::min(chunk, rows - c0);
      RecArgs<real> g{};
      sweep_args(g, L, c0, cr, pl, excl);
      g.topn = (int)topn;
      g.part_v = part_v.p;
      g.part_j = part_j.p;
      const double depth = (double)m.C * m.kp;
      const double bytes = ((double)cr + (double)m.n) * depth * sizeof(real) + (double)m.n * sizeof(real) +
                           (double)cr * topn * (sizeof(double) + sizeof(uint32_t));
      std::vector<RankCopy> cp;
      h.prof_launch(family, bytes, [&] {
        prep(g, c0, cr);
        with_kp(m.kp, [&](auto K) {
          constexpr int KP = decltype(K)::value;
          h.launch(k_rec_topn<real, KP, MODE>, (unsigned)((uint64_t)g.rt * g.S), BLOCK, 0, g);
        });
        h.launch(k_rec_merge, (unsigned)cr, BLOCK, 0, cr, (int)S, (int)topn, (const double *)part_v.p,
                 (const uint32_t *)part_j.p, out_j.p, out_v.p);
        cp = run_post(post, c0, cr, out_j, out_v);
      }, 2.0 * (double)cr * (double)m.n * depth);
      finish_chunk<Post>(cp, c0, cr, topn, out_j, out_v, items, scores);
    }
    h.flush_prof();
  }

  // ------------------------------------------------ scores of given pairs
  // Scores of the pairs (prow[e] of L, pitem[e]): those that are candidates
  // go through k_eval_label_scores, the others are -inf.
  void score(const RankRows<real> &L, uint64_t npairs, const uint32_t *prow, const uint32_t *pitem, double *out,
             const char *setup_counter) {
    std::vector<uint32_t> krow, kitem;
    std::vector<uint64_t> where;
    for (uint64_t e = 0; e < npairs; e++) {
      out[e] = -std::numeric_limits<double>::infinity();
      if (pitem[e] >= (L.cold[prow[e]] ? m.npop : m.n)) continue;
      krow.push_back(prow[e]);
      kitem.push_back(pitem[e]);
      where.push_back(e);
    }
    h.sync();
    h.rank_setup_done(setup_counter);
    if (kitem.empty()) return;
    const std::vector<double> kv = score_pairs(L, krow, kitem, "rerank");
    h.flush_prof();
    for (size_t t = 0; t < kv.size(); t++) out[where[t]] = kv[t];
  }

  // ------------------------------------------ top-N among candidate lists
  // Work items of per-row lists (k_rerank, k_rerank_count): row-major, a row's
  // segments in list order, one wave each, so a long list does not serialise
  // on one wave.
  struct ListPlan {
    std::vector<int64_t> wptr;  // per row: its work items
    std::vector<uint32_t> wrow, wlen;
    std::vector<uint64_t> wbeg;
    uint64_t chunk = 0, maxw = 0, maxc = 0;  // rows per launch; the most work items and entries of one
    DevBuf<int64_t> dwptr;
    DevBuf<uint32_t> dwrow, dwlen, dccol;
    DevBuf<uint64_t> dwbeg;
  };
  // Segment length (OCFFM_REC_SEG forces it): every k_rerank segment pays its
  // own list warm-up (about topn (1 + ln(len / topn)) inserts), so as few
  // segments as fill the machine: the call's entries over the resident waves,
  // within REC_SEG_MIN..REC_SEG_MAX.  Measured at the kkbox shape (3,075 rows,
  // fp32, family ms at 1,000 / 10,000 entries per row): 128: 1.44 / 8.49,
  // 256: 1.28 / 7.36, 512: 1.07 / 6.61, 1024: 0.87 / 6.07, 2048: 0.86 / 6.01.
  // Below 256 the one-wave merge of a row's partial lists takes over (64 rows
  // x 10,000 entries: 0.88 ms at 64, 0.61 at 128, 0.33 at 256, 0.39 at 512).
  // k_rerank_count has no warm-up and no merge; it takes the same rule.
  static constexpr uint64_t REC_SEG_MIN = 256, REC_SEG_MAX = 2048;
  template <class KOf> void plan_lists(ListPlan &p, uint64_t rows, const uint64_t *cptr, KOf &&kernel_of) {
    uint64_t seg = m.rec_seg;
    if (!seg) {
      const unsigned slots = resident(kernel_of);
      seg = cptr[rows] / ((uint64_t)slots * (BLOCK / 64)) + 1;
      seg = (std::clamp(seg, REC_SEG_MIN, REC_SEG_MAX) + 15) / 16 * 16;
    }
    p.wptr.assign(rows + 1, 0);
    for (uint64_t i = 0; i < rows; i++) {
      for (uint64_t b = cptr[i]; b < cptr[i + 1]; b += seg) {
        p.wrow.push_back((uint32_t)i);
        p.wbeg.push_back(b);
        p.wlen.push_back((uint32_t)std::min<uint64_t>(seg, cptr[i + 1] - b));
      }
      p.wptr[i + 1] = (int64_t)p.wrow.size();
    }
    p.chunk = chunk(rows);
    for (uint64_t c0 = 0; c0 < rows; c0 += p.chunk) {
      const uint64_t c1 = std::min(rows, c0 + p.chunk);
      p.maxw = std::max<uint64_t>(p.maxw, (uint64_t)(p.wptr[c1] - p.wptr[c0]));
      p.maxc = std::max<uint64_t>(p.maxc, cptr[c1] - cptr[c0]);
    }
    p.dwptr.upload(p.wptr);
    if (p.wrow.empty()) {  // (a pointer for a call without list entries)
      p.wrow.push_back(0);
      p.wbeg.push_back(0);
      p.wlen.push_back(0);
    }
    p.dwrow.upload(p.wrow);
    p.dwbeg.upload(p.wbeg);
    p.dwlen.upload(p.wlen);
    p.dccol.alloc(std::max<uint64_t>(p.maxc, 1), false);
  }
  // Algorithmic bytes of a list launch: gathered Q rows and b_j (an upper
  // bound: every entry taken as a warm candidate), the rows' P, the lists and
  // work items
  double list_bytes(uint64_t nc, uint64_t cr, uint64_t W) const {
    const double depth = (double)m.C * m.kp;
    return (double)nc * (depth * sizeof(real) + sizeof(real) + sizeof(uint32_t)) + (double)cr * depth * sizeof(real) +
           (double)W * 20.0;
  }
  // Top-N of each row's own candidate list (ocffm.h
  // ocffm_problem_recommend_among): row i of L has ccol[cptr[i] .. cptr[i + 1]).
  // Nothing is sorted on the host.  The rows go in chunks: scratch is a
  // chunk's work items x topn partial entries.
  void rerank(const RankRows<real> &L, uint64_t rows, const uint64_t *cptr, const uint32_t *ccol, uint32_t topn,
              bool excl, uint32_t *items, double *scores, const char *setup_counter) {
    rerank(L, rows, cptr, ccol, topn, excl, items, scores, setup_counter, "rerank", RankNoPost{});
  }
  // post: the post-chunk hook, as in recommend
  template <class Post>
  void rerank(const RankRows<real> &L, uint64_t rows, const uint64_t *cptr, const uint32_t *ccol, uint32_t topn,
              bool excl, uint32_t *items, double *scores, const char *setup_counter, const char *family, Post &&post) {
    ListPlan p;
    plan_lists(p, rows, cptr, [](auto K) { return k_rerank<real, decltype(K)::value, MODE>; });
    const uint64_t chunk = p.chunk;
    DevBuf<uint32_t> part_j, out_j;
    DevBuf<double> part_v, out_v;
    part_v.alloc(std::max<uint64_t>(p.maxw, 1) * topn, false);
    part_j.alloc(std::max<uint64_t>(p.maxw, 1) * topn, false);
    out_v.alloc(chunk * topn, false);
    out_j.alloc(chunk * topn, false);
    h.sync();
    h.rank_setup_done(setup_counter);
    for (uint64_t c0 = 0; c0 < rows; c0 += chunk) {
      const uint64_t cr = std::min(chunk, rows - c0);
      const uint64_t nc = cptr[c0 + cr] - cptr[c0];
      if (nc)
        HIPCHK(hipMemcpyAsync(p.dccol.p, ccol + cptr[c0], nc * sizeof(uint32_t), hipMemcpyHostToDevice, m.stream));
      RerankArgs<real> g{};
      g.W = (uint64_t)(p.wptr[c0 + cr] - p.wptr[c0]);
      g.w0 = (uint64_t)p.wptr[c0];
      g.r0 = c0;
      g.c0 = cptr[c0];
      g.n = m.n;
      g.npop = m.npop;
      g.C = (int)m.C;
      g.topn = (int)topn;
      g.exclude = excl ? 1 : 0;
      g.P = L.P;
      g.Q = m.Q;
      g.a = L.a;
      g.b = m.b;
      g.cold = L.dcold.p;
      g.popular = m.popular;
      g.lptr = L.dlptr.p;
      g.lcol = L.dlcol.p;
      g.su = L.su;
      g.sv = m.sv;
      g.wptr = p.dwptr.p;
      g.wrow = p.dwrow.p;
      g.wbeg = p.dwbeg.p;
      g.wlen = p.dwlen.p;
      g.ccol = p.dccol.p;
      g.part_v = part_v.p;
      g.part_j = part_j.p;
      g.out_v = out_v.p;
      g.out_j = out_j.p;
      const double depth = (double)m.C * m.kp;
      // list_bytes, the partial lists written and read back, the results
      const double bytes = list_bytes(nc, cr, g.W) +
                           (double)g.W * 2.0 * topn * (sizeof(double) + sizeof(uint32_t)) +
                           (double)cr * topn * (sizeof(double) + sizeof(uint32_t));
      std::vector<RankCopy> cp;
      h.prof_launch(family, bytes, [&] {
        if (g.W)
          with_kp(m.kp, [&](auto K) {
            constexpr int KP = decltype(K)::value;
            h.launch(k_rerank<real, KP, MODE>, (unsigned)((g.W + BLOCK / 64 - 1) / (BLOCK / 64)), BLOCK, 0, g);
          });
        h.launch(k_rerank_merge, (unsigned)((cr + BLOCK / 64 - 1) / (BLOCK / 64)), BLOCK, 0, cr, c0, g.w0, (int)topn,
                 (const int64_t *)p.dwptr.p, (const double *)part_v.p, (const uint32_t *)part_j.p, out_j.p, out_v.p);
        cp = run_post(post, c0, cr, out_j, out_v);
      }, 2.0 * (double)nc * depth);
      finish_chunk<Post>(cp, c0, cr, topn, out_j, out_v, items, scores);
    }
    h.flush_prof();
  }

  // ------------------------------------------------- ranking evaluation
  // Exact rank of every label of X (its rows are those of L) among its row's
  // candidates.  The bookkeeping is shared by the two ways of counting
  // (label_ranks: every item; label_ranks_among: the row's own list): the
  // distinct candidate labels of every row (candidate_labels) are scored on
  // their own (k_eval_label_scores), sorted per row on the host by the ranking
  // order, a count step fills one counter per label with the candidates that
  // fall between the label before it and itself, and the prefix sums are the
  // ranks (rank_labels).  L's exclusion lists are the seen items.
  struct Labels {
    std::vector<int64_t> kptr;         // per row: its distinct candidate labels in krow / kitem
    std::vector<uint32_t> krow, kitem;
    std::vector<int64_t> where;        // label entry of X -> its kept label (-1: not a candidate)
  };
  // (also fills ranks / scores with what a label that is no candidate gets)
  Labels candidate_labels(const RankRows<real> &L, const HostData &X, uint32_t *ranks, double *scores) {
    const uint64_t rows = X.m, ny = X.yptr[rows];
    Labels lb;
    lb.kptr.assign(rows + 1, 0);
    lb.where.assign(ny, -1);
    std::vector<std::pair<uint32_t, uint64_t>> tmp;
    for (uint64_t i = 0; i < rows; i++) {
      const uint64_t lim = L.cold[i] ? m.npop : m.n;
      const uint32_t *sb = L.lcol.data() + L.lptr[i], *se = L.lcol.data() + L.lptr[i + 1];
      tmp.clear();
      for (uint64_t p = X.yptr[i]; p < X.yptr[i + 1]; p++) {
        const uint64_t j = X.ycol[p];
        if (j < lim && !std::binary_search(sb, se, (uint32_t)j)) tmp.push_back({(uint32_t)j, p});
      }
      std::sort(tmp.begin(), tmp.end());
      for (size_t t = 0; t < tmp.size(); t++) {
        if (t == 0 || tmp[t].first != tmp[t - 1].first) {
          lb.krow.push_back((uint32_t)i);
          lb.kitem.push_back(tmp[t].first);
        }
        lb.where[tmp[t].second] = (int64_t)lb.kitem.size() - 1;
      }
      lb.kptr[i + 1] = (int64_t)lb.kitem.size();
    }
    for (uint64_t p = 0; p < ny; p++) {
      ranks[p] = OCFFM_RANK_NONE;
      if (scores) scores[p] = -std::numeric_limits<double>::infinity();
    }
    return lb;
  }
  // count(dkptr, dsv, dsj, dcnt): the launches that fill the counters dcnt of
  // the labels (dsv, dsj: each row's sorted by the ranking order; dkptr: the
  // rows' offsets).  Called with at least one label.
  template <class Count>
  void rank_labels(const RankRows<real> &L, const HostData &X, const Labels &lb, uint32_t *ranks, double *scores,
                   Count &&count) {
    const uint64_t rows = X.m, ny = X.yptr[rows], nk = lb.kitem.size();
    const std::vector<int64_t> &kptr = lb.kptr;
    DevBuf<uint32_t> dcnt;
    DevBuf<int64_t> dkptr;
    dkptr.upload(kptr);
    dcnt.alloc(nk);
    // the labels' own scores
    const std::vector<double> kv = score_pairs(L, lb.krow, lb.kitem, "evaluate");
    // each row's labels in ranking order
    std::vector<uint32_t> ord(nk);
    for (uint64_t e = 0; e < nk; e++) ord[e] = (uint32_t)e;
    for (uint64_t i = 0; i < rows; i++)
      std::sort(ord.begin() + kptr[i], ord.begin() + kptr[i + 1], [&](uint32_t x, uint32_t y) {
        return kv[x] > kv[y] || (kv[x] == kv[y] && lb.kitem[x] < lb.kitem[y]);
      });
    std::vector<double> sv(nk);
    std::vector<uint32_t> sj(nk);
    for (uint64_t e = 0; e < nk; e++) {
      sv[e] = kv[ord[e]];
      sj[e] = lb.kitem[ord[e]];
    }
    DevBuf<double> dsv;
    DevBuf<uint32_t> dsj;
    dsv.upload(sv);
    dsj.upload(sj);
    count(dkptr, dsv, dsj, dcnt);
    std::vector<uint32_t> cnt(nk);
    HIPCHK(hipMemcpyAsync(cnt.data(), dcnt.p, nk * sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream));
    h.sync();
    h.flush_prof();
    // ranks: the prefix sums of each row's counters, back in label order
    std::vector<uint32_t> krank(nk);
    for (uint64_t i = 0; i < rows; i++) {
      uint32_t run = 0;
      for (int64_t e = kptr[i]; e < kptr[i + 1]; e++) {
        run += cnt[e];
        krank[ord[e]] = run;
      }
    }
    for (uint64_t p = 0; p < ny; p++)
      if (lb.where[p] >= 0) {
        ranks[p] = krank[lb.where[p]];
        if (scores) scores[p] = kv[lb.where[p]];
      }
  }
  // Among every item: one sweep over the items (k_eval_count, rows in chunks,
  // items in slices as in recommend) counts.  excl: there are seen items.
  void label_ranks(const RankRows<real> &L, const HostData &X, bool excl, uint32_t *ranks, double *scores,
                   uint32_t *ncand, const char *setup_counter) {
    const uint64_t rows = X.m;
    if (ncand)
      for (uint64_t i = 0; i < rows; i++) {
        const uint64_t lim = L.cold[i] ? m.npop : m.n;
        const uint32_t *sb = L.lcol.data() + L.lptr[i], *se = L.lcol.data() + L.lptr[i + 1];
        ncand[i] = (uint32_t)(lim - (uint64_t)(std::lower_bound(sb, se, (uint32_t)lim) - sb));
      }
    const Labels lb = candidate_labels(L, X, ranks, scores);
    if (lb.kitem.empty()) {
      h.rank_setup_done(setup_counter);
      return;
    }
    const RankPlan pl = plan(rows, [](auto K) { return k_eval_count<real, decltype(K)::value, MODE>; });
    const uint64_t chunk = pl.chunk;
    h.sync();
    h.rank_setup_done(setup_counter);
    const double depth = (double)m.C * m.kp;
    const std::vector<int64_t> &kptr = lb.kptr;
    rank_labels(L, X, lb, ranks, scores, [&](const DevBuf<int64_t> &dkptr, const DevBuf<double> &dsv,
                                             const DevBuf<uint32_t> &dsj, const DevBuf<uint32_t> &dcnt) {
      for (uint64_t c0 = 0; c0 < rows; c0 += chunk) {
        const uint64_t cr = std::min(chunk, rows - c0);
        if (kptr[c0 + cr] == kptr[c0]) continue;  // no label in these rows
        EvalArgs<real> g{};
        sweep_args(g, L, c0, cr, pl, excl);
        g.kptr = dkptr.p + c0;
        g.kv = dsv.p;
        g.kj = dsj.p;
        g.cnt = dcnt.p;
        const double bytes = ((double)cr + (double)m.n) * depth * sizeof(real) + (double)m.n * sizeof(real) +
                             (double)(kptr[c0 + cr] - kptr[c0]) * (sizeof(double) + 2 * sizeof(uint32_t));
        h.prof_launch("evaluate", bytes, [&] {
          with_kp(m.kp, [&](auto K) {
            constexpr int KP = decltype(K)::value;
            h.launch(k_eval_count<real, KP, MODE>, (unsigned)((uint64_t)g.rt * g.S), BLOCK, 0, g);
          });
        }, 2.0 * (double)cr * (double)m.n * depth);
      }
    });
  }
  // Among each row's own list (ocffm.h ocffm_problem_label_ranks_among): row
  // i's candidate set K_i is the distinct entries of ccol[cptr[i] ..
  // cptr[i + 1]) that are candidates, united with the row's candidate labels.
  // K_i is built here in one pass over the entries with an n-long stamp array
  // (an item's stamp is the last row that took or excluded it), exact and
  // O(entries + seen items + labels); ncand[i] = |K_i| comes out of the same
  // pass.  k_rerank_count then counts over K_i, cut into segments and row
  // chunks as recommend_among's lists are.  A row without candidate labels is
  // only counted: it gets no work item.
  void label_ranks_among(const RankRows<real> &L, const HostData &X, const uint64_t *cptr, const uint32_t *ccol,
                         uint32_t *ranks, double *scores, uint32_t *ncand, const char *setup_counter) {
    const uint64_t rows = X.m;
    const Labels lb = candidate_labels(L, X, ranks, scores);
    std::vector<uint64_t> dptr(rows + 1, 0);
    std::vector<uint32_t> dcol;
    {
      std::vector<uint32_t> stamp(m.n, 0);  // (rows < 2^32 - 1: i + 1 is no stamp of an earlier call's)
      for (uint64_t i = 0; i < rows; i++) {
        const uint32_t mark = (uint32_t)(i + 1);
        const uint64_t lim = L.cold[i] ? m.npop : m.n;
        const bool work = lb.kptr[i + 1] > lb.kptr[i];
        for (int64_t p = L.lptr[i]; p < L.lptr[i + 1]; p++) stamp[L.lcol[p]] = mark;  // seen: never taken
        uint64_t cnt = (uint64_t)(lb.kptr[i + 1] - lb.kptr[i]);
        for (int64_t e = lb.kptr[i]; e < lb.kptr[i + 1]; e++) {
          stamp[lb.kitem[e]] = mark;
          dcol.push_back(lb.kitem[e]);
        }
        for (uint64_t p = cptr[i]; p < cptr[i + 1]; p++) {
          const uint32_t j = ccol[p];
          if (j >= lim || stamp[j] == mark) continue;
          stamp[j] = mark;
          cnt++;
          if (work) dcol.push_back(j);
        }
        if (ncand) ncand[i] = (uint32_t)cnt;
        dptr[i + 1] = dcol.size();
      }
    }
    if (lb.kitem.empty()) {
      h.rank_setup_done(setup_counter);
      return;
    }
    ListPlan p;
    plan_lists(p, rows, dptr.data(), [](auto K) { return k_rerank_count<real, decltype(K)::value, MODE>; });
    const uint64_t chunk = p.chunk;
    h.sync();
    h.rank_setup_done(setup_counter);
    const double depth = (double)m.C * m.kp;
    rank_labels(L, X, lb, ranks, scores, [&](const DevBuf<int64_t> &dkptr, const DevBuf<double> &dsv,
                                             const DevBuf<uint32_t> &dsj, const DevBuf<uint32_t> &dcnt) {
      for (uint64_t c0 = 0; c0 < rows; c0 += chunk) {
        const uint64_t cr = std::min(chunk, rows - c0);
        const uint64_t nc = dptr[c0 + cr] - dptr[c0];
        if (!nc) continue;  // no label in these rows
        HIPCHK(hipMemcpyAsync(p.dccol.p, dcol.data() + dptr[c0], nc * sizeof(uint32_t), hipMemcpyHostToDevice,
                              m.stream));
        RerankCountArgs<real> g{};
        g.W = (uint64_t)(p.wptr[c0 + cr] - p.wptr[c0]);
        g.w0 = (uint64_t)p.wptr[c0];
        g.c0 = dptr[c0];
        g.C = (int)m.C;
        g.P = L.P;
        g.Q = m.Q;
        g.a = L.a;
        g.b = m.b;
        g.cold = L.dcold.p;
        g.popular = m.popular;
        g.su = L.su;
        g.sv = m.sv;
        g.wrow = p.dwrow.p;
        g.wbeg = p.dwbeg.p;
        g.wlen = p.dwlen.p;
        g.ccol = p.dccol.p;
        g.kptr = dkptr.p;
        g.kv = dsv.p;
        g.kj = dsj.p;
        g.cnt = dcnt.p;
        // list_bytes, the labels searched and their counters
        const double bytes = list_bytes(nc, cr, g.W) +
                             (double)(lb.kptr[c0 + cr] - lb.kptr[c0]) * (sizeof(double) + 2 * sizeof(uint32_t));
        h.prof_launch("evaluate", bytes, [&] {
          with_kp(m.kp, [&](auto K) {
            constexpr int KP = decltype(K)::value;
            h.launch(k_rerank_count<real, KP, MODE>, (unsigned)((g.W + BLOCK / 64 - 1) / (BLOCK / 64)), BLOCK, 0, g);
          });
        }, 2.0 * (double)nc * depth);
        // (the next chunk's entries overwrite dccol: the copy is ordered after this launch on the stream)
      }
    });
  }
};

}  // namespace ocffm
