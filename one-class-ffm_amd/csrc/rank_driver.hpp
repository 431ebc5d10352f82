// rank_driver.hpp — the host driver of the serving sweeps (rank_kernels.hpp):
// row chunking and item slicing, the sweeps' arguments, recommend's partial
// lists and merge, label_ranks' bookkeeping, per-row sort, count launch and
// prefix sums, and the scores of given pairs.  It works on a view of a model
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
// NORM: the normalised scores of the SGD model (rank_kernels.hpp rec_score);
// the Newton problem's instantiations are NORM = false.
#pragma once

#include <algorithm>
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

// The item side of a model and how its sweeps are cut
template <typename real> struct RankModel {
  const real *const *Q = nullptr;    // C item-side cross tables (n x kp)
  const real *b = nullptr;           // b_j
  const real *sv = nullptr;          // NORM: the items' squared norms
  const double *popular = nullptr;   // cold rows' scores (no cold rows: null)
  uint64_t n = 0, npop = 0;          // items; popularity entries (<= n)
  uint32_t C = 0, kp = 0;
  unsigned slices = 0;               // OCFFM_REC_SLICES (0: from n, the rows and the CU count)
  uint64_t chunk_rows = 0;           // OCFFM_REC_ROWS (0: 4096 rows per chunk)
  hipStream_t stream = nullptr;
};

// The query rows of a call: their side of the model, the cold flags and the
// sorted distinct items < n of each row to leave out
template <typename real> struct RankRows {
  const real *const *P = nullptr;    // C user-side cross tables of the rows (rows x kp)
  const real *a = nullptr;           // a_i
  const real *su = nullptr;          // NORM: the rows' squared norms
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

template <typename real, bool NORM, class Host> struct RankDriver {
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
    g.su = NORM ? L.su + c0 : nullptr;
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
        h.launch(k_eval_label_scores<real, KP, NORM>, (unsigned)((nk + 63) / 64), BLOCK, 0, nk, (int)m.C,
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

  // ---------------------------------------------------- recommendation
  // Top-N items of the rows of L.  The rows are scored in chunks: scratch is
  // chunk x slices x topn partial entries, never rows x n.
  void recommend(const RankRows<real> &L, uint64_t rows, uint32_t topn, bool excl, uint32_t *items, double *scores,
                 const char *setup_counter) {
    const RankPlan pl = plan(rows, [](auto K) { return k_rec_topn<real, decltype(K)::value, NORM>; });
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
      h.prof_launch("recommend", bytes, [&] {
        with_kp(m.kp, [&](auto K) {
          constexpr int KP = decltype(K)::value;
          h.launch(k_rec_topn<real, KP, NORM>, (unsigned)((uint64_t)g.rt * g.S), BLOCK, 0, g);
        });
        h.launch(k_rec_merge, (unsigned)cr, BLOCK, 0, cr, (int)S, (int)topn, (const double *)part_v.p,
                 (const uint32_t *)part_j.p, out_j.p, out_v.p);
      }, 2.0 * (double)cr * (double)m.n * depth);
      copy_back(c0, cr, topn, out_j, out_v, items, scores);
    }
    h.flush_prof();
  }

  // ------------------------------------------------- ranking evaluation
  // Exact rank of every label of X (its rows are those of L) among its row's
  // candidates.  The distinct candidate labels of every row are scored on
  // their own (k_eval_label_scores), sorted per row on the host by the ranking
  // order, and one sweep over the items (k_eval_count, rows in chunks, items
  // in slices as in recommend) counts the candidates that fall between
  // consecutive labels; the prefix sums are the ranks.  L's exclusion lists
  // are the seen items (excl: there are some).
  void label_ranks(const RankRows<real> &L, const HostData &X, bool excl, uint32_t *ranks, double *scores,
                   uint32_t *ncand, const char *setup_counter) {
    const uint64_t rows = X.m;
    // each row's distinct candidate labels; every label's place among them
    const uint64_t ny = X.yptr[rows];
    std::vector<int64_t> kptr(rows + 1, 0);
    std::vector<uint32_t> krow, kitem;
    std::vector<int64_t> where(ny, -1);  // label entry -> its kept label (-1: not a candidate)
    {
      std::vector<std::pair<uint32_t, uint64_t>> tmp;
      for (uint64_t i = 0; i < rows; i++) {
        const uint64_t lim = L.cold[i] ? m.npop : m.n;
        const uint32_t *sb = L.lcol.data() + L.lptr[i], *se = L.lcol.data() + L.lptr[i + 1];
        if (ncand) ncand[i] = (uint32_t)(lim - (uint64_t)(std::lower_bound(sb, se, (uint32_t)lim) - sb));
        tmp.clear();
        for (uint64_t p = X.yptr[i]; p < X.yptr[i + 1]; p++) {
          const uint64_t j = X.ycol[p];
          if (j < lim && !std::binary_search(sb, se, (uint32_t)j)) tmp.push_back({(uint32_t)j, p});
        }
        std::sort(tmp.begin(), tmp.end());
        for (size_t t = 0; t < tmp.size(); t++) {
          if (t == 0 || tmp[t].first != tmp[t - 1].first) {
            krow.push_back((uint32_t)i);
            kitem.push_back(tmp[t].first);
          }
          where[tmp[t].second] = (int64_t)kitem.size() - 1;
        }
        kptr[i + 1] = (int64_t)kitem.size();
      }
    }
    const uint64_t nk = kitem.size();
    for (uint64_t p = 0; p < ny; p++) {
      ranks[p] = OCFFM_RANK_NONE;
      if (scores) scores[p] = -std::numeric_limits<double>::infinity();
    }
    if (nk == 0) {
      h.rank_setup_done(setup_counter);
      return;
    }
    DevBuf<uint32_t> dcnt;
    DevBuf<int64_t> dkptr;
    dkptr.upload(kptr);
    dcnt.alloc(nk);
    const RankPlan pl = plan(rows, [](auto K) { return k_eval_count<real, decltype(K)::value, NORM>; });
    const uint64_t chunk = pl.chunk;
    h.sync();
    h.rank_setup_done(setup_counter);
    const double depth = (double)m.C * m.kp;
    // the labels' own scores
    const std::vector<double> kv = score_pairs(L, krow, kitem, "evaluate");
    // each row's labels in ranking order
    std::vector<uint32_t> ord(nk);
    for (uint64_t e = 0; e < nk; e++) ord[e] = (uint32_t)e;
    for (uint64_t i = 0; i < rows; i++)
      std::sort(ord.begin() + kptr[i], ord.begin() + kptr[i + 1], [&](uint32_t x, uint32_t y) {
        return kv[x] > kv[y] || (kv[x] == kv[y] && kitem[x] < kitem[y]);
      });
    std::vector<double> sv(nk);
    std::vector<uint32_t> sj(nk);
    for (uint64_t e = 0; e < nk; e++) {
      sv[e] = kv[ord[e]];
      sj[e] = kitem[ord[e]];
    }
    DevBuf<double> dsv;
    DevBuf<uint32_t> dsj;
    dsv.upload(sv);
    dsj.upload(sj);
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
          h.launch(k_eval_count<real, KP, NORM>, (unsigned)((uint64_t)g.rt * g.S), BLOCK, 0, g);
        });
      }, 2.0 * (double)cr * (double)m.n * depth);
    }
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
      if (where[p] >= 0) {
        ranks[p] = krank[where[p]];
        if (scores) scores[p] = kv[where[p]];
      }
  }
};

}  // namespace ocffm
