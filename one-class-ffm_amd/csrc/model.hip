// model.hip — the stand-alone model handle (ocffm.h ocffm_model): W / H of a
// saved or trained model, an item catalogue in the serving sweeps' form, and
// the serving entries on it, the item-item similarities (ocffm_similar.h,
// sim_kernels.hpp) and the diversified top-N (ocffm_diverse.h,
// mmr_kernels.hpp) among them.  A third host of the serving driver
// (rank_driver.hpp) beside the Newton-CG problem (solver.hip) and the SGD
// trainer (sgd.hip): the files are read on the host (model_file.cpp), any rows
// are projected through W / H by one launch (k_project_side), and the sweeps,
// lists and merges are the driver's.  Single GPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ocffm.h"
#include "common.hpp"
#include "fold_kernels.hpp"
#include "kernels.hpp"
#include "model_file.h"
#include "mmr_kernels.hpp"
#include "model_source.hpp"
#include "rank_driver.hpp"
#include "sim_kernels.hpp"

namespace ocffm {

// ------------------------------------------------------- projection ---
// One field's CSR over the rows of a side (split_fields' layout: file order
// within a row)
template <typename real> struct ProjField {
  const int64_t *xptr;
  const uint32_t *xidx;
  const real *xval;
};

// The rows of one side and the model's tables they go through.  Cross job c
// (block order: f1 fv + f2 - fu) reads the rows' field cfld[c] and the table
// ctab[c] (W_b for user rows, H_b for item rows) and writes out[c] (R x KP);
// the side job reads the side's nside used blocks (f1 <= f2) in (f1, f2) order.
template <typename real> struct ProjSideArgs {
  uint64_t R;
  uint32_t C, nside;
  const ProjField<real> *fld;  // the side's fields
  const uint32_t *cfld;
  const real *const *ctab;
  real *const *out;
  const uint32_t *sf1, *sf2;   // the side blocks' fields (within the side)
  const real *const *sW, *const *sH;
  real *bias;                  // a_i or b_j
};

// sum over the row's nodes of one field of val * T[idx], from zero in CSR
// order: k_utx's chain (kernels.hpp)
template <typename real, int KP>
__device__ __forceinline__ vec_t<real> proj_row(const ProjField<real> F, const real *T, uint64_t row, int li) {
  using G = Geo<real, KP>;
  vec_t<real> acc = vzero<real>();
  for (int64_t p = F.xptr[row]; p < F.xptr[row + 1]; p++)
    acc += vsplat<real>(F.xval[p]) * gvld<real>(T + (size_t)F.xidx[p] * KP + li * G::VE);
  return acc;
}

// k_project_side: one launch turns the per-field CSR of a side's rows into
// everything the serving sweeps read for them: the C cross-table rows (Q_c[j]
// and b_j for item rows, P_c[i] and a_i for user rows) and the side term.
// One subgroup of LPR lanes per (row, job), job <= C, 16 B (fp64: 32 B) of a
// table row per lane; the row's node lists are walked, not held in lanes, so
// rows of any width work.  job < C: the cross-table row, k_utx's chain.
// job == C: the side term, from zero over the side's used blocks in (f1, f2)
// order: p1 = X_f1 W_b and p2 = X_f2 H_b by the same chain, d =
// sg_sum(hsum(p1 * p2)), bias += d: k_rowdot_add applied in calc_side's order,
// without the round trip of p1 / p2 through memory (which changes no bit).
// The arithmetic is pinned: the results are the problem's block-by-block
// projection's, bit for bit.  A (row, job) is one subgroup's, summed in the
// row's own order: it does not depend on the row's place in the launch nor on
// the grid (subgroups stride over the (row, job) pairs).
// Algorithmic bytes: the side's CSR once per job that reads the field (12 or
// 16 B a node and the row pointers), one KP-real table row per (node, job of
// its field), C KP + 1 reals written per row.
template <typename real, int KP>
__global__ __launch_bounds__(BLOCK) void k_project_side(ProjSideArgs<real> d) {
  using G = Geo<real, KP>;
  const int li = threadIdx.x % G::LPR;
  const uint64_t jobs = (uint64_t)d.C + 1, total = d.R * jobs;
  const uint64_t nsg = (uint64_t)gridDim.x * BLOCK / G::LPR;
  for (uint64_t s = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) / G::LPR; s < total; s += nsg) {
    const uint64_t row = s / jobs;
    const uint32_t c = (uint32_t)(s % jobs);
    if (c < d.C) {
      const vec_t<real> acc = proj_row<real, KP>(d.fld[d.cfld[c]], d.ctab[c], row, li);
      vst<real>(d.out[c] + row * KP + li * G::VE, acc);
    } else {
      real bias = (real)0;
      for (uint32_t q = 0; q < d.nside; q++) {
        const vec_t<real> p1 = proj_row<real, KP>(d.fld[d.sf1[q]], d.sW[q], row, li);
        const vec_t<real> p2 = proj_row<real, KP>(d.fld[d.sf2[q]], d.sH[q], row, li);
        const real dd = sg_sum<G::LPR>(hsum<real>(p1 * p2));
        bias += dd;
      }
      if (li == 0) d.bias[row] = bias;
    }
  }
}

static uint32_t model_pad_k(uint32_t k) {
  uint32_t kp = 4;
  while (kp < k) kp <<= 1;
  return kp;
}

static void model_check_cuts(const uint32_t *cuts, uint32_t ncut) {
  if (!cuts || ncut < 1 || ncut > OCFFM_EVAL_MAX_CUTS) throw Error(OCFFM_E_ARG, "ncut must be in 1..OCFFM_EVAL_MAX_CUTS");
  for (uint32_t s = 0; s < ncut; s++)
    if (cuts[s] < 1 || (s && cuts[s] <= cuts[s - 1])) throw Error(OCFFM_E_ARG, "cuts must be >= 1 and strictly increasing");
}

// ------------------------------------------------------------------ model
// A fold request of a serving call (ocffm_model_fold_in): the history rows and
// the parameters; delta / nhist (fold_in alone) take the corrections and |H_i|
// of the call's rows.
struct FoldSpec {
  const HostData *hist = nullptr;
  ocffm_fold fo{};
  double *delta = nullptr;
  uint32_t *nhist = nullptr;
};

struct ModelBase {
  virtual ~ModelBase() = default;
  virtual void set_items(const HostData &V) = 0;
  virtual void set_popularity(const double *pop, uint64_t npop) = 0;
  virtual void recommend(const HostData &X, uint64_t row0, uint64_t rows, uint32_t topn, uint32_t flags,
                         uint32_t *items, double *scores, const FoldSpec *fold) = 0;
  virtual void label_ranks(const HostData &X, const HostData *seen, uint32_t *ranks, double *scores,
                           uint32_t *ncand, const FoldSpec *fold) = 0;
  virtual void fold_in(const HostData &X, const FoldSpec &fold) = 0;
  virtual void score(const HostData &X, uint64_t npairs, const uint32_t *prow, const uint32_t *pitem, double *out) = 0;
  virtual void recommend_among(const HostData &X, uint64_t row0, uint64_t rows, const uint64_t *cptr,
                               const uint32_t *ccol, uint32_t topn, uint32_t flags, uint32_t *items,
                               double *scores) = 0;
  virtual void label_ranks_among(const HostData &X, const HostData *seen, const uint64_t *cptr, const uint32_t *ccol,
                                 uint32_t *ranks, double *scores, uint32_t *ncand) = 0;
  virtual void similar_items(uint64_t nq, const uint32_t *qitem, const uint64_t *xptr, const uint32_t *xcol,
                             uint32_t topn, uint32_t flags, uint32_t *items, double *scores) = 0;
  virtual void similar_to(const HostData &Vq, uint64_t row0, uint64_t rows, const uint64_t *xptr, const uint32_t *xcol,
                          uint32_t topn, uint32_t flags, uint32_t *items, double *scores) = 0;
  virtual void item_similarity(uint64_t npairs, const uint32_t *pa, const uint32_t *pb, uint32_t flags,
                               double *out) = 0;
  virtual void recommend_diverse(const HostData &X, uint64_t row0, uint64_t rows, const uint64_t *cptr,
                                 const uint32_t *ccol, uint32_t topn, uint32_t pool, double theta, uint32_t flags,
                                 uint32_t *items, double *scores, double *mmr, uint32_t *pos) = 0;
  virtual uint64_t get(char what, uint32_t b12, double *out, uint64_t cap) = 0;
  virtual void info(ocffm_model_info *out) const = 0;
  virtual const std::vector<uint64_t> &ds() const = 0;
  std::map<std::string, int64_t> counters;
};

template <typename real> class Model final : public ModelBase {
 public:
  Model(int device, uint32_t f, uint32_t fu, uint32_t fv, uint32_t k, const std::vector<uint64_t> &Ds,
        const std::vector<uint8_t> &used)
      : device_(device), f_(f), fu_(fu), fv_(fv), k_(k), kp_(model_pad_k(k)), C_(fu * fv), Ds_(Ds), used_(used) {
    HIPCHK(hipSetDevice(device_));
    HIPCHK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_));
    ncu_ = (unsigned)std::max(1, prop.multiProcessorCount);
    if (const char *e = std::getenv("OCFFM_REC_SLICES")) rec_slices_ = (unsigned)std::clamp(std::atoi(e), 1, 256);
    if (const char *e = std::getenv("OCFFM_REC_ROWS")) rec_rows_ = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    rec_seg_ = RankModel<real>::seg_from_env();
    // OCFFM_PROJECT_BLOCKS: the projection's grid (tests: a capped grid whose subgroups stride)
    if (const char *e = std::getenv("OCFFM_PROJECT_BLOCKS")) proj_blocks_ = (unsigned)std::clamp(std::atoi(e), 1, 1 << 20);
    W_.resize(used_.size());
    H_.resize(used_.size());
    for (uint32_t f1 = 0; f1 < f_; f1++)
      for (uint32_t f2 = f1; f2 < f_; f2++) {
        const uint32_t b12 = ModelFile::block_index(f1, f2, f_);
        if (!used_[b12]) continue;
        W_[b12].alloc(Ds_[f1] * kp_);
        H_[b12].alloc(Ds_[f2] * kp_);
      }
  }
  ~Model() override {
    if (stream_) (void)hipStreamDestroy(stream_);
  }

  // W / H from a file's host tables, cast and padded as ocffm_problem_load_binary does
  void adopt(const ModelFile &mf) {
    std::vector<real> pad;
    for (uint32_t f1 = 0; f1 < f_; f1++)
      for (uint32_t f2 = f1; f2 < f_; f2++) {
        const uint32_t b12 = ModelFile::block_index(f1, f2, f_);
        if (!used_[b12]) continue;
        for (int t = 0; t < 2; t++) {
          const std::vector<double> &w = t == 0 ? mf.W[b12] : mf.H[b12];
          const uint64_t D = Ds_[t == 0 ? f1 : f2];
          pad.assign(D * kp_, (real)0);
          for (uint64_t rr = 0; rr < D; rr++)
            for (uint32_t cc = 0; cc < k_; cc++) pad[rr * kp_ + cc] = (real)w[rr * k_ + cc];
          real *dst = t == 0 ? W_[b12].p : H_[b12].p;
          if (D) HIPCHK(hipMemcpy(dst, pad.data(), pad.size() * sizeof(real), hipMemcpyHostToDevice));
        }
      }
    build_tables();
  }
  // The problem's W / H, item side and popularity, device to device
  void adopt(const ModelSource &src) {
    for (size_t b = 0; b < used_.size(); b++) {
      if (!used_[b]) continue;
      if (W_[b].n) HIPCHK(hipMemcpy(W_[b].p, src.W[b], W_[b].bytes(), hipMemcpyDeviceToDevice));
      if (H_[b].n) HIPCHK(hipMemcpy(H_[b].p, src.H[b], H_[b].bytes(), hipMemcpyDeviceToDevice));
    }
    build_tables();
    alloc_items(src.n);
    if (src.n) {
      for (uint32_t c = 0; c < C_; c++)
        HIPCHK(hipMemcpy(qtab_.p + (size_t)c * src.n * kp_, src.Q[c], src.n * kp_ * sizeof(real), hipMemcpyDeviceToDevice));
      HIPCHK(hipMemcpy(b_.p, src.b, src.n * sizeof(real), hipMemcpyDeviceToDevice));
    }
    npop_ = src.npop;
    popular_.alloc(npop_, false);
    if (npop_) HIPCHK(hipMemcpy(popular_.p, src.popular, npop_ * sizeof(double), hipMemcpyDeviceToDevice));
    HIPCHK(hipDeviceSynchronize());
  }

  // ---------------------------------------------------------- catalogue
  void set_items(const HostData &V) override {
    use_device();
    if (V.f > fv_) throw Error(OCFFM_E_ARG, "V has more fields than the model's item side");
    check_nodes(V, 0, V.m, fv_, fu_);
    sync();
    // laid out and projected into fresh buffers: a failure leaves the old catalogue
    SideRows sr;
    layout(sr, V, 0, V.m, fv_);
    DevBuf<real> tab, bias;
    DevBuf<real *> tp;
    const auto t0 = std::chrono::steady_clock::now();
    project(1, sr, V.m, tab, tp, bias);
    sync();
    counters["project_us"] =
        (int64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    qtab_ = std::move(tab);
    qt_ = std::move(tp);
    b_ = std::move(bias);
    n_ = V.m;
    has_items_ = true;
    popular_.release();
    npop_ = 0;
    fold_ready_ = false;  // (the aggregates are the old catalogue's)
    sim_ready_ = false;   // (so are the inverse norms)
  }
  void set_popularity(const double *pop, uint64_t npop) override {
    use_device();
    if (npop && !pop) throw Error(OCFFM_E_ARG, "null popularity");
    need_items();
    sync();
    npop_ = std::min<uint64_t>(npop, n_);
    popular_.upload(pop, npop_);
  }

  // ------------------------------------------------------------ serving
  void recommend(const HostData &X, uint64_t row0, uint64_t rows, uint32_t topn, uint32_t flags, uint32_t *items,
                 double *scores, const FoldSpec *fold) override {
    use_device();
    need_items();
    check_topn(X, row0, rows, topn, items);
    if (fold) fold_check(X, *fold);
    check_rows(X, row0, rows);
    if (rows == 0) return;
    if (n_ == 0) return none_lists(rows, topn, items, scores);
    begin();
    const bool excl = (flags & OCFFM_REC_EXCLUDE_LABELS) && X.yptr.size() == X.m + 1 && !X.ycol.empty();
    Query L;
    query(L, X, row0, rows, excl ? &X : nullptr, fold);
    const RankModel<real> m = rank_model();
    Rank{*this, m}.recommend(L, rows, topn, excl, items, scores, "rec_setup_us");
    end();
  }
  void score(const HostData &X, uint64_t npairs, const uint32_t *prow, const uint32_t *pitem, double *out) override {
    use_device();
    need_items();
    if (npairs && (!prow || !pitem || !out)) throw Error(OCFFM_E_ARG, "null pair or output array");
    for (uint64_t e = 0; e < npairs; e++)
      if (prow[e] >= X.m) throw Error(OCFFM_E_ARG, "pair row outside X");
    check_rows(X, 0, X.m);
    if (npairs == 0) return;
    if (n_ == 0) {
      for (uint64_t e = 0; e < npairs; e++) out[e] = -std::numeric_limits<double>::infinity();
      return;
    }
    begin();
    Query L;
    query(L, X, 0, X.m, nullptr);
    const RankModel<real> m = rank_model();
    Rank{*this, m}.score(L, npairs, prow, pitem, out, "rec_setup_us");
    end();
  }
  void recommend_among(const HostData &X, uint64_t row0, uint64_t rows, const uint64_t *cptr, const uint32_t *ccol,
                       uint32_t topn, uint32_t flags, uint32_t *items, double *scores) override {
    use_device();
    need_items();
    check_topn(X, row0, rows, topn, items);
    check_lists(cptr, ccol, rows);
    check_rows(X, row0, rows);
    if (rows == 0) return;
    if (n_ == 0) return none_lists(rows, topn, items, scores);
    begin();
    const bool excl = (flags & OCFFM_REC_EXCLUDE_LABELS) && X.yptr.size() == X.m + 1 && !X.ycol.empty();
    Query L;
    query(L, X, row0, rows, excl ? &X : nullptr);
    const RankModel<real> m = rank_model();
    Rank{*this, m}.rerank(L, rows, cptr, ccol, topn, excl, items, scores, "rec_setup_us");
    end();
  }
  void label_ranks(const HostData &X, const HostData *seen, uint32_t *ranks, double *scores,
                   uint32_t *ncand, const FoldSpec *fold) override {
    use_device();
    need_items();
    label_check(X, seen, ranks);
    if (fold) fold_check(X, *fold);
    check_rows(X, 0, X.m);
    if (X.m == 0) return;
    if (n_ == 0) return none_ranks(X, ranks, scores, ncand);
    begin();
    Query L;
    query(L, X, 0, X.m, seen, fold);
    const RankModel<real> m = rank_model();
    Rank{*this, m}.label_ranks(L, X, seen != nullptr, ranks, scores, ncand, "eval_setup_us");
    end();
  }
  void label_ranks_among(const HostData &X, const HostData *seen, const uint64_t *cptr, const uint32_t *ccol,
                         uint32_t *ranks, double *scores, uint32_t *ncand) override {
    use_device();
    need_items();
    label_check(X, seen, ranks);
    check_lists(cptr, ccol, X.m);
    check_rows(X, 0, X.m);
    if (X.m == 0) return;
    if (n_ == 0) return none_ranks(X, ranks, scores, ncand);
    begin();
    Query L;
    query(L, X, 0, X.m, seen);
    const RankModel<real> m = rank_model();
    Rank{*this, m}.label_ranks_among(L, X, cptr, ccol, ranks, scores, ncand, "eval_setup_us");
    end();
  }

  // delta_i and |H_i| of every row of X (ocffm_model_fold_in)
  void fold_in(const HostData &X, const FoldSpec &fold) override {
    use_device();
    need_items();
    fold_check(X, fold);
    check_rows(X, 0, X.m);
    const uint64_t d = (uint64_t)fv_ * k_;
    std::fill(fold.delta, fold.delta + X.m * d, 0.0);
    if (fold.nhist) std::fill(fold.nhist, fold.nhist + X.m, 0u);
    counters["fold_us"] = 0;
    counters["fold_rows"] = 0;
    if (X.m == 0 || n_ == 0) return;
    begin();
    Query L;
    query(L, X, 0, X.m, nullptr, &fold);
    end();
  }

  // ------------------------------------------------------ similar items
  // Top-N catalogue items by similarity to the catalogue items qitem[0..nq)
  // (ocffm_similar.h): recommend's sweep in REC_SIM mode; a chunk's query rows
  // are gathered from the catalogue's own tables just before its sweep, so the
  // scratch is chunk x depth.
  void similar_items(uint64_t nq, const uint32_t *qitem, const uint64_t *xptr, const uint32_t *xcol, uint32_t topn,
                     uint32_t flags, uint32_t *items, double *scores) override {
    use_device();
    need_items();
    sim_check(nq, xptr, xcol, topn, flags, items);
    if (nq && !qitem) throw Error(OCFFM_E_ARG, "null qitem");
    for (uint64_t e = 0; e < nq; e++)
      if (qitem[e] >= n_) throw Error(OCFFM_E_ARG, "query item outside the catalogue");
    if (nq == 0) return;
    sim_norms();
    begin();
    const bool dot = (flags & OCFFM_SIM_DOT) != 0;
    RankRows<real> L;
    const bool excl = sim_exclusions(L, nq, (flags & OCFFM_SIM_KEEP_SELF) ? nullptr : qitem, xptr, xcol);
    DevBuf<uint32_t> dq;
    dq.upload(qitem, nq);
    RankModel<real> m = rank_model();
    m.sv = dot ? nullptr : siminv_.p;
    SimRank dr{*this, m};
    const uint64_t chunk = dr.chunk(nq);
    DevBuf<real> tab, qinv;
    DevBuf<real *> tp;
    tab.alloc((size_t)C_ * chunk * kp_, false);
    qinv.alloc(chunk, false);
    std::vector<real *> tl(C_);
    for (uint32_t c = 0; c < C_; c++) tl[c] = tab.p + (size_t)c * chunk * kp_;
    tp.upload(tl);
    L.P = tp.p;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> gev;
    dr.recommend(L, nq, topn, excl, items, scores, "sim_setup_us", "similar",
                 [&](RecArgs<real> &g, uint64_t c0, uint64_t cr) {
                   hipEvent_t ea, eb;
                   HIPCHK(hipEventCreate(&ea));
                   HIPCHK(hipEventCreate(&eb));
                   gev.push_back({ea, eb});
                   HIPCHK(hipEventRecord(ea, stream_));
                   with_kp(kp_, [&](auto K) {
                     constexpr int KP = decltype(K)::value;
                     // a memory-bound copy: at most 2048 blocks, the threads stride over the rest
                     const uint64_t vecs = cr * C_ * (KP * sizeof(real) / 16);
                     const unsigned grid = (unsigned)std::clamp<uint64_t>((vecs + BLOCK - 1) / BLOCK, 1, 2048);
                     launch(k_sim_gather<real, KP>, grid, BLOCK, 0, cr, (int)C_, dq.p + c0, (const real *const *)qt_.p,
                            (real *const *)tp.p, dot ? nullptr : siminv_.p, qinv.p);
                   });
                   HIPCHK(hipEventRecord(eb, stream_));
                   sim_args(g);
                   g.p0 = 0;  // (the chunk's own tables and norms)
                   g.su = dot ? nullptr : qinv.p;
                 });
    double gus = 0;  // (recommend has waited for the stream)
    for (auto &e : gev) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, e.first, e.second));
      gus += 1e3 * ms;
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
    counters["sim_gather_us"] = (int64_t)gus;
    end();
  }
  // The same for rows [row0, row0 + rows) of Vq, item rows in the model's item
  // field space: projected as the catalogue is, their norms by the catalogue's
  // kernel
  void similar_to(const HostData &Vq, uint64_t row0, uint64_t rows, const uint64_t *xptr, const uint32_t *xcol,
                  uint32_t topn, uint32_t flags, uint32_t *items, double *scores) override {
    use_device();
    need_items();
    if (row0 > Vq.m || rows > Vq.m - row0) throw Error(OCFFM_E_ARG, "row range outside Vq");
    sim_check(rows, xptr, xcol, topn, flags, items);
    if (Vq.f > fv_) throw Error(OCFFM_E_ARG, "Vq has more fields than the model's item side");
    check_nodes(Vq, row0, rows, fv_, fu_);
    if (rows == 0) return;
    if (n_ == 0) return none_lists(rows, topn, items, scores);
    sim_norms();
    begin();
    const bool dot = (flags & OCFFM_SIM_DOT) != 0;
    RankRows<real> L;
    const bool excl = sim_exclusions(L, rows, nullptr, xptr, xcol);
    SideRows sr;
    layout(sr, Vq, row0, rows, fv_);
    DevBuf<real> tab, bias, qinv;
    DevBuf<real *> tp;
    project(1, sr, rows, tab, tp, bias);
    qinv.alloc(rows, false);
    if (!dot) prof_launch("similar", 0, [&] { inv_norms((const real *const *)tp.p, rows, qinv.p); });
    RankModel<real> m = rank_model();
    m.sv = dot ? nullptr : siminv_.p;
    L.P = tp.p;
    L.su = dot ? nullptr : qinv.p;
    SimRank{*this, m}.recommend(L, rows, topn, excl, items, scores, "sim_setup_us", "similar",
                                [&](RecArgs<real> &g, uint64_t, uint64_t) { sim_args(g); });
    end();
  }
  // sim of the catalogue pairs (pa[e], pb[e]): k_eval_label_scores in REC_SIM
  // mode on the catalogue's tables from both sides, the sweep's bits
  void item_similarity(uint64_t npairs, const uint32_t *pa, const uint32_t *pb, uint32_t flags, double *out) override {
    use_device();
    need_items();
    if (flags & ~(OCFFM_SIM_DOT | OCFFM_SIM_KEEP_SELF)) throw Error(OCFFM_E_ARG, "unknown flag bits");
    if (npairs && (!pa || !pb || !out)) throw Error(OCFFM_E_ARG, "null pair or output array");
    if (npairs == 0) return;
    std::vector<uint32_t> krow, kitem;
    std::vector<uint64_t> where;
    for (uint64_t e = 0; e < npairs; e++) {
      out[e] = -std::numeric_limits<double>::infinity();
      if (pa[e] >= n_ || pb[e] >= n_) continue;
      krow.push_back(pa[e]);
      kitem.push_back(pb[e]);
      where.push_back(e);
    }
    if (kitem.empty()) return;
    sim_norms();
    begin();
    const bool dot = (flags & OCFFM_SIM_DOT) != 0;
    RankModel<real> m = rank_model();
    m.sv = dot ? nullptr : siminv_.p;
    RankRows<real> L;
    L.P = qt_.p;
    L.su = m.sv;
    sync();
    rank_setup_done("sim_setup_us");
    const std::vector<double> kv = SimRank{*this, m}.score_pairs(L, krow, kitem, "similar");
    flush_prof();
    for (size_t t = 0; t < kv.size(); t++) out[where[t]] = kv[t];
    end();
  }

  // -------------------------------------------------------- diversified
  // Greedy MMR re-ranking of each row's top-`pool` list (ocffm_diverse.h):
  // recommend's sweep (or recommend_among's list path when cptr is given) with
  // topn = pool, and k_mmr as the driver's post-chunk hook on the chunk's
  // device lists; only the rows x topn selection comes back.  Scratch is per
  // chunk: chunk x topn results, and pool x pool similarities in LDS.
  void recommend_diverse(const HostData &X, uint64_t row0, uint64_t rows, const uint64_t *cptr, const uint32_t *ccol,
                         uint32_t topn, uint32_t pool, double theta, uint32_t flags, uint32_t *items, double *scores,
                         double *mmr, uint32_t *pos) override {
    use_device();
    need_items();
    check_topn(X, row0, rows, topn, items);
    if (pool < topn || pool > OCFFM_DIV_MAX_POOL) throw Error(OCFFM_E_ARG, "pool must be in topn..OCFFM_DIV_MAX_POOL");
    if (!(theta >= 0.0 && theta <= 1.0)) throw Error(OCFFM_E_ARG, "theta must be in [0, 1]");
    if (flags & ~OCFFM_REC_EXCLUDE_LABELS) throw Error(OCFFM_E_ARG, "unknown flag bits");
    if (cptr) check_lists(cptr, ccol, rows);
    else if (ccol) throw Error(OCFFM_E_ARG, "ccol without cptr");
    check_rows(X, row0, rows);
    if (rows == 0) return;
    if (n_ == 0) {
      none_lists(rows, topn, items, scores);
      for (uint64_t e = 0; e < rows * topn; e++) {
        if (mmr) mmr[e] = -std::numeric_limits<double>::infinity();
        if (pos) pos[e] = OCFFM_REC_NONE;
      }
      return;
    }
    sim_norms();
    begin();
    const bool excl = (flags & OCFFM_REC_EXCLUDE_LABELS) && X.yptr.size() == X.m + 1 && !X.ycol.empty();
    Query L;
    query(L, X, row0, rows, excl ? &X : nullptr);
    const RankModel<real> m = rank_model();
    Rank dr{*this, m};
    const uint64_t chunk = dr.chunk(rows);
    DevBuf<uint32_t> dj, dp;
    DevBuf<double> dv, dm;
    dj.alloc(chunk * topn, false);
    dp.alloc(chunk * topn, false);
    dv.alloc(chunk * topn, false);
    dm.alloc(chunk * topn, false);
    MmrArgs<real> a{};
    a.C = (int)C_;
    a.pool = (int)pool;
    a.topn = (int)topn;
    a.ld = mmr_ld(pool);
    a.Q = (const real *const *)qt_.p;
    a.inv = siminv_.p;
    a.w = 1.0 - theta;
    a.theta = theta;
    a.items = dj.p;
    a.pos = dp.p;
    a.scores = dv.p;
    a.mmr = dm.p;
    // LDS from the pool: a small pool keeps several workgroups per CU; above 64 KiB the kernel opts in
    const size_t smem = mmr_lds_bytes<real>(pool);
    if (smem > (64u << 10))
      with_kp(kp_, [&](auto K) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mmr<real, decltype(K)::value>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
      });
    std::vector<std::pair<hipEvent_t, hipEvent_t>> dev;
    auto post = [&](uint64_t c0, uint64_t cr, const uint32_t *pj, const double *pv) {
      hipEvent_t ea, eb;
      HIPCHK(hipEventCreate(&ea));
      HIPCHK(hipEventCreate(&eb));
      dev.push_back({ea, eb});
      a.R = cr;
      a.pool_j = pj;
      a.pool_v = pv;
      HIPCHK(hipEventRecord(ea, stream_));
      with_kp(kp_, [&](auto K) { launch(k_mmr<real, decltype(K)::value>, (unsigned)cr, BLOCK, smem, a); });
      HIPCHK(hipEventRecord(eb, stream_));
      const size_t o = c0 * topn, ne = cr * topn;
      return std::vector<RankCopy>{{dj.p, items + o, ne * sizeof(uint32_t)},
                                   {dv.p, scores ? scores + o : nullptr, ne * sizeof(double)},
                                   {dm.p, mmr ? mmr + o : nullptr, ne * sizeof(double)},
                                   {dp.p, pos ? pos + o : nullptr, ne * sizeof(uint32_t)}};
    };
    if (cptr)
      dr.rerank(L, rows, cptr, ccol, pool, excl, nullptr, nullptr, "div_setup_us", "diverse", post);
    else
      dr.recommend(L, rows, pool, excl, nullptr, nullptr, "div_setup_us", "diverse",
                   [](RecArgs<real> &, uint64_t, uint64_t) {}, post);
    double dus = 0;  // (the driver has waited for the stream)
    for (auto &e : dev) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, e.first, e.second));
      dus += 1e3 * ms;
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
    counters["div_kernel_us"] = (int64_t)dus;
    end();
  }

  // ------------------------------------------------------------- access
  uint64_t get(char what, uint32_t b12, double *out, uint64_t cap) override {
    use_device();
    const real *src = nullptr;
    uint64_t rows = 0, cols = k_;
    if (what == 'W' || what == 'H' || what == 'Q') {
      if (b12 >= used_.size() || !used_[b12]) throw Error(OCFFM_E_ARG, "block not in the model");
      uint32_t f1 = 0, f2 = 0;
      block_fields(b12, f1, f2);
      if (what == 'W') { src = W_[b12].p; rows = Ds_[f1]; }
      if (what == 'H') { src = H_[b12].p; rows = Ds_[f2]; }
      if (what == 'Q') {
        if (!(f1 < fu_ && f2 >= fu_)) throw Error(OCFFM_E_ARG, "Q is kept for the cross blocks");
        need_items();
        src = qtab_.p + (size_t)(f1 * fv_ + (f2 - fu_)) * n_ * kp_;
        rows = n_;
      }
    } else if (what == 'b') {
      need_items();
      src = b_.p;
      rows = n_;
      cols = 1;
    } else {
      throw Error(OCFFM_E_ARG, "unknown state name");
    }
    const uint64_t count = rows * cols;
    if (out && cap) {
      const uint64_t stride = what == 'b' ? 1 : kp_;
      std::vector<real> tmp(rows * stride);
      sync();
      if (rows) HIPCHK(hipMemcpy(tmp.data(), src, tmp.size() * sizeof(real), hipMemcpyDeviceToHost));
      for (uint64_t rr = 0, o = 0; rr < rows; rr++)
        for (uint64_t cc = 0; cc < cols && o < cap; cc++, o++) out[o] = (double)tmp[rr * stride + cc];
    }
    return count;
  }
  void info(ocffm_model_info *o) const override {
    o->f = f_;
    o->fu = fu_;
    o->fv = fv_;
    o->k = k_;
    o->kp = kp_;
    o->nblocks = (uint32_t)used_.size();
    o->nused = 0;
    for (uint8_t u : used_) o->nused += u;
    o->self_side = nside_[0] + nside_[1] > 0 ? 1 : 0;
    o->precision = std::is_same<real, double>::value ? OCFFM_FP64 : OCFFM_FP32;
    o->device = device_;
    o->has_items = has_items_ ? 1 : 0;
    o->n = n_;
    o->npop = npop_;
    if (o->Ds)
      for (uint32_t i = 0; i < f_ && i < o->ds_cap; i++) o->Ds[i] = Ds_[i];
    if (o->used)
      for (uint32_t b = 0; b < used_.size() && b < o->used_cap; b++) o->used[b] = used_[b];
  }
  const std::vector<uint64_t> &ds() const override { return Ds_; }

 private:
  void use_device() { HIPCHK(hipSetDevice(device_)); }
  void sync() { HIPCHK(hipStreamSynchronize(stream_)); }
  void need_items() const {
    if (!has_items_) throw Error(OCFFM_E_STATE, "call ocffm_model_set_items first");
  }
  void block_fields(uint32_t b12, uint32_t &o1, uint32_t &o2) const {
    for (uint32_t f1 = 0; f1 < f_; f1++)
      for (uint32_t f2 = f1; f2 < f_; f2++)
        if (ModelFile::block_index(f1, f2, f_) == b12) {
          o1 = f1;
          o2 = f2;
          return;
        }
  }

  // The projection's view of the model, per side (0: user rows, 1: item rows)
  void build_tables() {
    for (int s = 0; s < 2; s++) {
      const uint32_t lo = s ? fu_ : 0, hi = s ? f_ : fu_;
      std::vector<uint32_t> cfld;
      std::vector<const real *> ctab;
      for (uint32_t f1 = 0; f1 < fu_; f1++)
        for (uint32_t f2 = fu_; f2 < f_; f2++) {
          const uint32_t b12 = ModelFile::block_index(f1, f2, f_);
          cfld.push_back(s ? f2 - fu_ : f1);
          ctab.push_back(s ? H_[b12].p : W_[b12].p);
        }
      std::vector<uint32_t> sf1, sf2;
      std::vector<const real *> sW, sH;
      for (uint32_t f1 = lo; f1 < hi; f1++)
        for (uint32_t f2 = f1; f2 < hi; f2++) {
          const uint32_t b12 = ModelFile::block_index(f1, f2, f_);
          if (!used_[b12]) continue;
          sf1.push_back(f1 - lo);
          sf2.push_back(f2 - lo);
          sW.push_back(W_[b12].p);
          sH.push_back(H_[b12].p);
        }
      nside_[s] = (uint32_t)sf1.size();
      if (sf1.empty()) {  // (a pointer for a model without side blocks)
        sf1.push_back(0);
        sf2.push_back(0);
        sW.push_back(nullptr);
        sH.push_back(nullptr);
      }
      cfld_[s].upload(cfld);
      ctab_[s].upload(ctab);
      sf1_[s].upload(sf1);
      sf2_[s].upload(sf2);
      sW_[s].upload(sW);
      sH_[s].upload(sH);
    }
  }

  // ------------------------------------------------------ rows of a side
  struct SideRows {
    std::vector<DevBuf<int64_t>> xptr;
    std::vector<DevBuf<uint32_t>> xidx;
    std::vector<DevBuf<real>> xval;
    DevBuf<ProjField<real>> fld;
    uint64_t nnz = 0;
  };
  // Every node of rows [row0, row0 + rows) lies in the side's nf fields (the
  // model's fields f0 ..) and below their Ds
  void check_nodes(const HostData &X, uint64_t row0, uint64_t rows, uint32_t nf, uint32_t f0) const {
    for (uint64_t p = X.raw.xptr[row0]; p < X.raw.xptr[row0 + rows]; p++)
      if (X.raw.fid[p] >= nf || X.raw.idx[p] >= Ds_[f0 + X.raw.fid[p]])
        throw Error(OCFFM_E_DATA, "a node with idx >= Ds[fid] (read the rows with the model's Ds)");
  }
  // split_fields (ffm.cpp:185-257) of rows [row0, row0 + rows): per field, the
  // row pointers and the nodes in file order, values cast to real
  void layout(SideRows &sr, const HostData &X, uint64_t row0, uint64_t rows, uint32_t nf) {
    const Rows &r = X.raw;
    std::vector<std::vector<int64_t>> xptr(nf, std::vector<int64_t>(rows + 1, 0));
    std::vector<std::vector<uint32_t>> xidx(nf);
    std::vector<std::vector<real>> xval(nf);
    for (uint64_t i = 0; i < rows; i++) {
      for (uint64_t p = r.xptr[row0 + i]; p < r.xptr[row0 + i + 1]; p++) {
        xidx[r.fid[p]].push_back((uint32_t)r.idx[p]);
        xval[r.fid[p]].push_back((real)r.val[p]);
      }
      for (uint32_t fi = 0; fi < nf; fi++) xptr[fi][i + 1] = (int64_t)xidx[fi].size();
    }
    sr.xptr.resize(nf);
    sr.xidx.resize(nf);
    sr.xval.resize(nf);
    std::vector<ProjField<real>> fl(nf);
    for (uint32_t fi = 0; fi < nf; fi++) {
      sr.nnz += xidx[fi].size();
      sr.xptr[fi].upload(xptr[fi]);
      sr.xidx[fi].upload(xidx[fi]);
      sr.xval[fi].upload(xval[fi]);
      fl[fi] = ProjField<real>{sr.xptr[fi].p, sr.xidx[fi].p, sr.xval[fi].p};
    }
    sr.fld.upload(fl);
  }
  // k_project_side over R rows of side s: tab holds the C tables (each R x kp),
  // tp their pointers, bias the side terms
  void project(int s, const SideRows &sr, uint64_t R, DevBuf<real> &tab, DevBuf<real *> &tp, DevBuf<real> &bias) {
    tab.alloc(std::max<size_t>(1, (size_t)C_ * R * kp_), false);
    bias.alloc(std::max<uint64_t>(1, R), false);
    std::vector<real *> tl(C_);
    for (uint32_t c = 0; c < C_; c++) tl[c] = tab.p + (size_t)c * R * kp_;
    tp.upload(tl);
    if (R == 0) return;
    ProjSideArgs<real> a{};
    a.R = R;
    a.C = C_;
    a.nside = nside_[s];
    a.fld = sr.fld.p;
    a.cfld = cfld_[s].p;
    a.ctab = ctab_[s].p;
    a.out = tp.p;
    a.sf1 = sf1_[s].p;
    a.sf2 = sf2_[s].p;
    a.sW = sW_[s].p;
    a.sH = sH_[s].p;
    a.bias = bias.p;
    with_kp(kp_, [&](auto K) {
      constexpr int KP = decltype(K)::value;
      const uint64_t lpr = Geo<real, KP>::LPR;
      // memory-bound gathers: at most 2048 blocks, the subgroups stride over the rest
      const uint64_t want = (R * (C_ + 1) * lpr + BLOCK - 1) / BLOCK;
      const unsigned grid = (unsigned)std::min<uint64_t>(want, proj_blocks_ ? proj_blocks_ : 2048);
      launch(k_project_side<real, KP>, grid, BLOCK, 0, a);
    });
  }

  // The query rows of a call: their layout, projection, cold flags and exclusion lists
  struct Query : RankRows<real> {
    SideRows sr;
    DevBuf<real> tab, ax;
    DevBuf<real *> tp;
  };
  void query(Query &L, const HostData &X, uint64_t row0, uint64_t rows, const HostData *lab,
             const FoldSpec *fold = nullptr) {
    layout(L.sr, X, row0, rows, fu_);
    project(0, L.sr, rows, L.tab, L.tp, L.ax);
    L.cold.resize(rows);
    for (uint64_t i = 0; i < rows; i++) L.cold[i] = X.nnx[row0 + i] == 0;
    FoldRows fr;
    if (fold) fold_rows(fr, L, *fold, row0, rows);
    L.dcold.upload(L.cold);
    L.exclusions(lab, row0, rows, n_);
    L.P = L.tp.p;
    L.a = L.ax.p;
    if (fold) fold_apply(fr, L, *fold, row0, rows);
  }

  // ------------------------------------------------------------- fold-in
  // The folded rows of a call (those with a history item < n), compacted, and
  // their histories: sorted, distinct, < n
  struct FoldRows {
    std::vector<uint32_t> frow, hcol;
    std::vector<int64_t> hptr{0};
  };
  void fold_check(const HostData &X, const FoldSpec &fold) const {
    const ocffm_fold &fo = fold.fo;
    if (fo.field >= fu_) throw Error(OCFFM_E_ARG, "fold: field is not a user field of the model");
    if (!std::isfinite(fo.omega) || !std::isfinite(fo.lambda) || !std::isfinite(fo.r) || !(fo.lambda > 0) ||
        !(fo.omega >= 0))
      throw Error(OCFFM_E_ARG, "fold: lambda must be > 0, omega >= 0, and omega, lambda, r finite");
    const HostData &h = *fold.hist;
    if (h.m != X.m) throw Error(OCFFM_E_ARG, "fold: hist must have X's row count");
    if (h.m && (!h.has_label || h.yptr.size() != h.m + 1)) throw Error(OCFFM_E_ARG, "fold: hist has no labels");
    if ((uint64_t)fv_ * k_ > OCFFM_FOLD_MAX_D)
      throw Error(OCFFM_E_ARG, "fold: fv * k = " + std::to_string((uint64_t)fv_ * k_) +
                                   " exceeds OCFFM_FOLD_MAX_D = " + std::to_string(OCFFM_FOLD_MAX_D));
    if (X.m >= 0xffffffffull) throw Error(OCFFM_E_ARG, "too many rows");
  }
  // Host part, before the cold flags are uploaded: the histories of rows
  // [row0, row0 + rows); a folded row is not cold
  void fold_rows(FoldRows &fr, Query &L, const FoldSpec &fold, uint64_t row0, uint64_t rows) {
    const HostData &h = *fold.hist;
    for (uint64_t i = 0; i < rows; i++) {
      const size_t b = fr.hcol.size();
      for (uint64_t p = h.yptr[row0 + i]; p < h.yptr[row0 + i + 1]; p++)
        if (h.ycol[p] < n_) fr.hcol.push_back((uint32_t)h.ycol[p]);
      std::sort(fr.hcol.begin() + b, fr.hcol.end());
      fr.hcol.erase(std::unique(fr.hcol.begin() + b, fr.hcol.end()), fr.hcol.end());
      if (fold.nhist) fold.nhist[row0 + i] = (uint32_t)(fr.hcol.size() - b);
      if (fr.hcol.size() == b) continue;
      fr.frow.push_back((uint32_t)i);
      fr.hptr.push_back((int64_t)fr.hcol.size());
      L.cold[i] = 0;
    }
  }
  // The catalogue aggregates G, s, t in fp64 by the objective's kernels on qt_
  // / b_, once per catalogue.  The row ranges are a function of n alone and
  // their partials are summed in range order.
  void fold_stats() {
    if (fold_ready_) return;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t C = C_, ntp = C * (C + 1) / 2;
    const uint64_t D = (uint64_t)C * kp_, gsz = std::max<uint64_t>(1, (uint64_t)ntp * kp_ * kp_), nvec = 2 * D + 2;
    const uint32_t G = std::min(2u, std::max(C, 1u)), ng = (C + G - 1) / G, ngp = ng * (ng + 1) / 2;
    const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(1, (256ull << 20) / (gsz * 8)),
                                            std::max<uint64_t>(1, 1024 / std::max(ngp, 1u)));
    const uint64_t nbx = std::clamp<uint64_t>((n_ + 31) / 32, 1, cap), rpb = std::max<uint64_t>(1, (n_ + nbx - 1) / nbx);
    DevBuf<double> part;
    part.alloc(nbx * std::max(gsz, nvec), false);
    foldG_.alloc(gsz);
    foldvec_.alloc(nvec);
    const real *const *tabs = (const real *const *)qt_.p;
    with_kp(kp_, [&](auto K) {
      constexpr int KP = decltype(K)::value;
      if (C > 0) {
        const dim3 grid((unsigned)nbx, ngp);
        const unsigned threads = 64u * std::min<uint32_t>(BLOCK / 64, G * G);
        bool done = false;
        if constexpr (obj_mfma_kp<real, KP>()) {
          if (n_ * kp_ * sizeof(real) < 0xffffff00ull) {  // (the MFMA tiles' buffer views)
            launch(k_obj_gram<real, KP, true>, grid, threads, 0, (uint64_t)n_, C, tabs, part.p, rpb, G, ng);
            done = true;
          }
        }
        if (!done) launch(k_obj_gram<real, KP, false>, grid, threads, 0, (uint64_t)n_, C, tabs, part.p, rpb, G, ng);
        launch(k_reduce_parts<double, double>, (unsigned)((gsz + 15) / 16), BLOCK, 0, nbx, gsz, (uint64_t)0, gsz,
               (const double *)part.p, (uint64_t)0, (double *)nullptr, foldG_.p);
      }
      launch(k_obj_vecs<real, KP>, (unsigned)nbx, BLOCK, 0, (uint64_t)n_, (int)C, tabs, (const real *)b_.p, 0.0, part.p,
             rpb);
      launch(k_reduce_parts<double, double>, (unsigned)((nvec + 15) / 16), BLOCK, 0, nbx, nvec, (uint64_t)0, nvec,
             (const double *)part.p, (uint64_t)0, (double *)nullptr, foldvec_.p);
    });
    sync();
    fold_ready_ = true;
    counters["fold_stats_builds"]++;
    counters["fold_stats_us"] =
        (int64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  }
  // Device part, on the call's projected tables: build, solve, apply
  void fold_apply(const FoldRows &fr, Query &L, const FoldSpec &fold, uint64_t row0, uint64_t rows) {
    const uint32_t d = fv_ * k_;
    const uint64_t nf = fr.frow.size();
    counters["fold_rows"] = (int64_t)nf;
    counters["fold_us"] = 0;
    if (nf == 0) return;
    fold_stats();
    DevBuf<uint32_t> dfrow, dhcol;
    DevBuf<int64_t> dhptr;
    DevBuf<double> ddelta;
    DevBuf<int> dbad;
    dfrow.upload(fr.frow);
    dhcol.upload(fr.hcol);
    dhptr.upload(fr.hptr);
    ddelta.alloc(rows * d);
    dbad.alloc(1);
    FoldArgs<real> a{};
    a.C = C_;
    a.fv = fv_;
    a.k = k_;
    a.field = fold.fo.field;
    a.d = d;
    a.omega = fold.fo.omega;
    a.lambda = fold.fo.lambda;
    a.r = fold.fo.r;
    a.P = L.tp.p;
    a.a = L.ax.p;
    a.Q = (const real *const *)qt_.p;
    a.b = b_.p;
    a.G = foldG_.p;
    a.vec = foldvec_.p;
    a.frow = dfrow.p;
    a.hptr = dhptr.p;
    a.hcol = dhcol.p;
    a.delta = ddelta.p;
    a.bad = dbad.p;
    // LDS from d: small d keeps several workgroups per CU; above 64 KiB the kernel opts in
    const size_t smem = fold_lds_bytes(d);
    if (smem > (160u << 10)) throw Error(OCFFM_E_ARG, "fold: the LDS request exceeds 160 KiB");
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    try {
      HIPCHK(hipEventRecord(e0, stream_));
      with_kp(kp_, [&](auto K) {
        constexpr int KP = decltype(K)::value;
        if (smem > (64u << 10))
          HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fold_solve<real, KP>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        launch(k_fold_solve<real, KP>, (unsigned)nf, BLOCK, smem, a);
      });
      launch(k_fold_apply<real>, (unsigned)((nf * d + BLOCK - 1) / BLOCK), BLOCK, 0, nf, d, k_, kp_, fold.fo.field * fv_,
             (const uint32_t *)dfrow.p, (const double *)ddelta.p, (real *const *)L.tp.p, L.dcold.p);
      HIPCHK(hipEventRecord(e1, stream_));
      sync();
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, e0, e1));
      counters["fold_us"] = (int64_t)(1e3 * ms);
    } catch (...) {
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
      throw;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    int bad = 0;
    HIPCHK(hipMemcpy(&bad, dbad.p, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) throw Error(OCFFM_E_DATA, "fold: a pivot of the normal equations was not positive and finite");
    if (fold.delta)
      HIPCHK(hipMemcpy(fold.delta + row0 * d, ddelta.p, rows * d * sizeof(double), hipMemcpyDeviceToHost));
  }
  // --------------------------------------------------------- similarity
  static void sim_check(uint64_t nq, const uint64_t *xptr, const uint32_t *xcol, uint32_t topn, uint32_t flags,
                        const uint32_t *items) {
    if (topn == 0 || topn > OCFFM_REC_MAX_TOPN) throw Error(OCFFM_E_ARG, "topn must be in 1..OCFFM_REC_MAX_TOPN");
    if (!items) throw Error(OCFFM_E_ARG, "null items");
    if (flags & ~(OCFFM_SIM_DOT | OCFFM_SIM_KEEP_SELF)) throw Error(OCFFM_E_ARG, "unknown flag bits");
    if (nq >= 0xffffffffull) throw Error(OCFFM_E_ARG, "too many queries");
    if (xptr) check_lists(xptr, xcol, nq);
    else if (xcol) throw Error(OCFFM_E_ARG, "xcol without xptr");
  }
  // Each query's exclusion list as the sweep takes it (sorted, distinct, < n):
  // the caller's list united with the query's own index (self: null keeps it).
  // Returns whether any list has an entry.
  bool sim_exclusions(RankRows<real> &L, uint64_t nq, const uint32_t *self, const uint64_t *xptr,
                      const uint32_t *xcol) const {
    L.lptr.assign(nq + 1, 0);
    L.lcol.clear();
    for (uint64_t i = 0; i < nq; i++) {
      const size_t b = L.lcol.size();
      if (self) L.lcol.push_back(self[i]);
      if (xptr)
        for (uint64_t p = xptr[i]; p < xptr[i + 1]; p++)
          if (xcol[p] < n_) L.lcol.push_back(xcol[p]);
      std::sort(L.lcol.begin() + b, L.lcol.end());
      L.lcol.erase(std::unique(L.lcol.begin() + b, L.lcol.end()), L.lcol.end());
      L.lptr[i + 1] = (int64_t)L.lcol.size();
    }
    const bool any = !L.lcol.empty();
    if (!any) L.lcol.push_back(0);
    L.dlptr.upload(L.lptr);
    L.dlcol.upload(L.lcol);
    return any;
  }
  // A REC_SIM sweep reads the two inverse norms and nothing else of the side terms
  static void sim_args(RecArgs<real> &g) {
    g.a = nullptr;
    g.b = nullptr;
    g.cold = nullptr;
    g.popular = nullptr;
  }
  // k_sim_inv_norm over the R rows of the C tables T
  void inv_norms(const real *const *T, uint64_t R, real *inv) {
    if (R == 0) return;
    with_kp(kp_, [&](auto K) {
      constexpr int KP = decltype(K)::value;
      // a memory-bound stream: at most 2048 blocks, the subgroups stride over the rest
      const unsigned grid = (unsigned)std::min<uint64_t>((R * 16 + BLOCK - 1) / BLOCK, 2048);
      launch(k_sim_inv_norm<real, KP>, grid, BLOCK, 0, R, (int)C_, T, inv);
    });
  }
  // The catalogue's inverse norms, once per catalogue
  void sim_norms() {
    if (sim_ready_) return;
    sync();
    const auto t0 = std::chrono::steady_clock::now();
    siminv_.alloc(std::max<uint64_t>(1, n_), false);
    inv_norms((const real *const *)qt_.p, n_, siminv_.p);
    sync();
    sim_ready_ = true;
    counters["sim_norm_builds"]++;
    counters["sim_norm_us"] =
        (int64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  }
  void alloc_items(uint64_t n) {
    qtab_.alloc(std::max<size_t>(1, (size_t)C_ * n * kp_), false);
    b_.alloc(std::max<uint64_t>(1, n), false);
    std::vector<real *> tl(C_);
    for (uint32_t c = 0; c < C_; c++) tl[c] = qtab_.p + (size_t)c * n * kp_;
    qt_.upload(tl);
    n_ = n;
    has_items_ = true;
  }

  // ------------------------------------------------------------- checks
  void check_rows(const HostData &X, uint64_t row0, uint64_t rows) const {
    if (X.f > fu_) throw Error(OCFFM_E_ARG, "X has more fields than the model's user side");
    check_nodes(X, row0, rows, fu_, 0);
  }
  static void check_topn(const HostData &X, uint64_t row0, uint64_t rows, uint32_t topn, const uint32_t *items) {
    if (topn == 0 || topn > OCFFM_REC_MAX_TOPN) throw Error(OCFFM_E_ARG, "topn must be in 1..OCFFM_REC_MAX_TOPN");
    if (row0 > X.m || rows > X.m - row0) throw Error(OCFFM_E_ARG, "row range outside X");
    if (!items) throw Error(OCFFM_E_ARG, "null items");
  }
  static void label_check(const HostData &X, const HostData *seen, const uint32_t *ranks) {
    if (!ranks) throw Error(OCFFM_E_ARG, "null ranks");
    if (!X.has_label || X.yptr.size() != X.m + 1) throw Error(OCFFM_E_ARG, "X has no labels");
    if (seen && (seen->m != X.m || (seen->m && seen->yptr.size() != seen->m + 1)))
      throw Error(OCFFM_E_ARG, "seen must have X's row count (and labels)");
    if (X.m >= 0xffffffffull) throw Error(OCFFM_E_ARG, "too many rows");
  }
  // An empty catalogue: no row has a candidate
  static void none_lists(uint64_t rows, uint32_t topn, uint32_t *items, double *scores) {
    for (uint64_t e = 0; e < rows * topn; e++) {
      items[e] = OCFFM_REC_NONE;
      if (scores) scores[e] = -std::numeric_limits<double>::infinity();
    }
  }
  static void none_ranks(const HostData &X, uint32_t *ranks, double *scores, uint32_t *ncand) {
    for (uint64_t p = 0; p < X.yptr[X.m]; p++) {
      ranks[p] = OCFFM_RANK_NONE;
      if (scores) scores[p] = -std::numeric_limits<double>::infinity();
    }
    if (ncand)
      for (uint64_t i = 0; i < X.m; i++) ncand[i] = 0;
  }

  // ------------------------------------- the driver's host (rank_driver.hpp)
  using Rank = RankDriver<real, REC_PLAIN, Model>;
  using SimRank = RankDriver<real, REC_SIM, Model>;
  friend Rank;
  friend SimRank;
  RankModel<real> rank_model() const {
    RankModel<real> m;
    m.Q = qt_.p;
    m.b = b_.p;
    m.popular = popular_.p;
    m.n = n_;
    m.npop = npop_;
    m.C = C_;
    m.kp = kp_;
    m.slices = rec_slices_;
    m.chunk_rows = rec_rows_;
    m.rec_seg = rec_seg_;
    m.stream = stream_;
    return m;
  }
  // The call's clock starts
  void begin() {
    sync();
    rank_t0_ = std::chrono::steady_clock::now();
    kernel_us_ = 0;
  }
  void end() { counters["rank_kernel_us"] = (int64_t)kernel_us_; }
  template <typename... KArgs, typename... A>
  void launch(void (*k)(KArgs...), dim3 grid, dim3 block, size_t smem, A... a) {
    static_assert(sizeof...(KArgs) == sizeof...(A), "kernel argument count");
    hipLaunchKernelGGL(k, grid, block, (uint32_t)smem, stream_, static_cast<KArgs>(a)...);
    HIPCHK(hipGetLastError());
  }
  // The timing hook sums the launches' time between HIP events on the model's stream
  template <class L> void prof_launch(const char *, double, L &&body, double = 0) {
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    pending_.push_back({a, b});
    HIPCHK(hipEventRecord(a, stream_));
    body();
    HIPCHK(hipEventRecord(b, stream_));
  }
  void flush_prof() {
    sync();
    for (auto &e : pending_) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, e.first, e.second));
      kernel_us_ += 1e3 * ms;
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
    pending_.clear();
  }
  template <typename... KArgs> unsigned resident(void (*k)(KArgs...), size_t smem) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void *>(k), BLOCK, smem) !=
            hipSuccess || nb <= 0)
      nb = 1;
    return (unsigned)nb * ncu_;
  }
  void rank_setup_done(const char *counter) {
    counters[counter] =
        (int64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - rank_t0_).count();
  }

  int device_;
  uint32_t f_, fu_, fv_, k_, kp_, C_;
  std::vector<uint64_t> Ds_;
  std::vector<uint8_t> used_;
  hipStream_t stream_ = nullptr;
  unsigned ncu_ = 1;
  unsigned rec_slices_ = 0, proj_blocks_ = 0;
  uint64_t rec_rows_ = 0, rec_seg_ = 0;
  std::vector<DevBuf<real>> W_, H_;
  // the projection's tables per side (build_tables)
  uint32_t nside_[2] = {0, 0};
  DevBuf<uint32_t> cfld_[2], sf1_[2], sf2_[2];
  DevBuf<const real *> ctab_[2], sW_[2], sH_[2];
  // the catalogue
  bool has_items_ = false;
  uint64_t n_ = 0, npop_ = 0;
  DevBuf<real> qtab_, b_;
  DevBuf<real *> qt_;
  DevBuf<double> popular_;
  // the catalogue's fold aggregates (fold_stats): G's tiles; s, t
  bool fold_ready_ = false;
  DevBuf<double> foldG_, foldvec_;
  // the catalogue's inverse norms (sim_norms)
  bool sim_ready_ = false;
  DevBuf<real> siminv_;
  std::chrono::steady_clock::time_point rank_t0_;
  double kernel_us_ = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending_;
};

static std::unique_ptr<ModelBase> model_from_file(const ModelFile &mf, int precision, int device) {
  if (precision != OCFFM_FP64 && precision != OCFFM_FP32) throw Error(OCFFM_E_ARG, "precision must be OCFFM_FP64 or OCFFM_FP32");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(OCFFM_E_HIP, "no HIP device");
  if (device < 0 || device >= count) throw Error(OCFFM_E_ARG, "device ordinal out of range");
  if (precision == OCFFM_FP64) {
    auto m = std::make_unique<Model<double>>(device, mf.f, mf.fu, mf.fv, mf.k, mf.Ds, mf.used);
    m->adopt(mf);
    return m;
  }
  auto m = std::make_unique<Model<float>>(device, mf.f, mf.fu, mf.fv, mf.k, mf.Ds, mf.used);
  m->adopt(mf);
  return m;
}

}  // namespace ocffm

// ====================================================================== ABI
using namespace ocffm;

struct ocffm_model {
  std::unique_ptr<ModelBase> m;
};

extern "C" {

int ocffm_model_file_info(const char *path, int binary, ocffm_model_info *out) {
  std::string err;
  const int st = model_file_info(path, binary, out, err);
  if (st != OCFFM_OK) g_last_error = err;
  return st;
}

static int model_load(const char *path, int binary, int precision, int device, ocffm_model **out) {
  return guarded([&] {
    if (!path || !out) throw Error(OCFFM_E_ARG, "null path or output");
    *out = nullptr;
    ModelFile mf;
    try {
      mf = binary ? read_model_binary(path) : read_model_text(path);
    } catch (ModelFileError &e) {
      throw Error(e.code, e.what());
    }
    auto h = std::make_unique<ocffm_model>();
    h->m = model_from_file(mf, precision, device);
    *out = h.release();
  });
}
int ocffm_model_load_text(const char *path, int precision, int device, ocffm_model **out) {
  return model_load(path, 0, precision, device, out);
}
int ocffm_model_load_binary(const char *path, int precision, int device, ocffm_model **out) {
  return model_load(path, 1, precision, device, out);
}
int ocffm_model_from_problem(ocffm_problem *p, ocffm_model **out) {
  return guarded([&] {
    if (!out) throw Error(OCFFM_E_ARG, "null output");
    *out = nullptr;
    ModelSource src;
    problem_model_source(p, src);
    auto h = std::make_unique<ocffm_model>();
    if (src.precision == OCFFM_FP64) {
      auto m = std::make_unique<Model<double>>(src.device, src.f, src.fu, src.fv, src.k, src.Ds, src.used);
      m->adopt(src);
      h->m = std::move(m);
    } else {
      auto m = std::make_unique<Model<float>>(src.device, src.f, src.fu, src.fv, src.k, src.Ds, src.used);
      m->adopt(src);
      h->m = std::move(m);
    }
    *out = h.release();
  });
}

#define MODEL_CALL(body)                                             \
  return guarded([&] {                                               \
    if (!mod || !mod->m) throw Error(OCFFM_E_ARG, "null model");     \
    body;                                                            \
  })

int ocffm_model_set_items(ocffm_model *mod, const ocffm_data *V) {
  MODEL_CALL(if (!V) throw Error(OCFFM_E_ARG, "null V"); mod->m->set_items(V->d));
}
int ocffm_model_set_popularity(ocffm_model *mod, const double *pop, uint64_t npop) {
  MODEL_CALL(mod->m->set_popularity(pop, npop));
}
int ocffm_model_recommend(ocffm_model *mod, const ocffm_data *X, uint64_t row0, uint64_t rows, uint32_t topn,
                          uint32_t flags, uint32_t *items, double *scores) {
  MODEL_CALL(if (!X) throw Error(OCFFM_E_ARG, "null X");
             mod->m->recommend(X->d, row0, rows, topn, flags, items, scores, nullptr));
}
int ocffm_model_score(ocffm_model *mod, const ocffm_data *X, uint64_t npairs, const uint32_t *prow,
                      const uint32_t *pitem, double *out) {
  MODEL_CALL(if (!X) throw Error(OCFFM_E_ARG, "null X"); mod->m->score(X->d, npairs, prow, pitem, out));
}
int ocffm_model_recommend_among(ocffm_model *mod, const ocffm_data *X, uint64_t row0, uint64_t rows,
                                const uint64_t *cptr, const uint32_t *ccol, uint32_t topn, uint32_t flags,
                                uint32_t *items, double *scores) {
  MODEL_CALL(if (!X) throw Error(OCFFM_E_ARG, "null X");
             mod->m->recommend_among(X->d, row0, rows, cptr, ccol, topn, flags, items, scores));
}
int ocffm_model_label_ranks(ocffm_model *mod, const ocffm_data *X, const ocffm_data *seen, uint32_t *ranks,
                            double *scores, uint32_t *ncand) {
  MODEL_CALL(if (!X) throw Error(OCFFM_E_ARG, "null X");
             mod->m->label_ranks(X->d, seen ? &seen->d : nullptr, ranks, scores, ncand, nullptr));
}
int ocffm_model_label_ranks_among(ocffm_model *mod, const ocffm_data *X, const ocffm_data *seen, const uint64_t *cptr,
                                  const uint32_t *ccol, uint32_t *ranks, double *scores, uint32_t *ncand) {
  MODEL_CALL(if (!X) throw Error(OCFFM_E_ARG, "null X");
             mod->m->label_ranks_among(X->d, seen ? &seen->d : nullptr, cptr, ccol, ranks, scores, ncand));
}
// The fold arguments of an ABI call
static FoldSpec fold_spec(const ocffm_data *hist, const ocffm_fold *fo, double *delta = nullptr,
                          uint32_t *nhist = nullptr) {
  if (!hist || !fo) throw Error(OCFFM_E_ARG, "null hist or fold parameters");
  FoldSpec fs;
  fs.hist = &hist->d;
  fs.fo = *fo;
  fs.delta = delta;
  fs.nhist = nhist;
  return fs;
}
static int model_evaluate(ocffm_model *mod, const ocffm_data *X, const ocffm_data *hist, const ocffm_fold *fo,
                          bool fold, const ocffm_data *seen, const uint32_t *cuts, uint32_t ncut, ocffm_eval *out) {
  const ocffm_data *Xd = X;
  std::vector<uint32_t> ranks, ncand;
  std::vector<double> scores;
  const int st = guarded([&] {
    if (!mod || !mod->m) throw Error(OCFFM_E_ARG, "null model");
    if (!X) throw Error(OCFFM_E_ARG, "null X");
    if (!out) throw Error(OCFFM_E_ARG, "null output");
    model_check_cuts(cuts, ncut);
    const HostData &d = X->d;
    ranks.resize(d.ycol.size() + 1);
    ncand.resize(d.m + 1);
    scores.resize(d.ycol.size() + 1);
    const FoldSpec fs = fold ? fold_spec(hist, fo) : FoldSpec{};
    mod->m->label_ranks(d, seen ? &seen->d : nullptr, ranks.data(), scores.data(), ncand.data(), fold ? &fs : nullptr);
  });
  if (st != OCFFM_OK) return st;
  return ocffm_eval_from_ranks(Xd->d.m, Xd->d.yptr.data(), ranks.data(), scores.data(), ncand.data(), cuts, ncut, out);
}
int ocffm_model_evaluate(ocffm_model *mod, const ocffm_data *X, const ocffm_data *seen, const uint32_t *cuts,
                         uint32_t ncut, ocffm_eval *out) {
  return model_evaluate(mod, X, nullptr, nullptr, false, seen, cuts, ncut, out);
}
int ocffm_model_fold_in(ocffm_model *mod, const ocffm_data *X, const ocffm_data *hist, const ocffm_fold *fo,
                        double *delta, uint32_t *nhist) {
  MODEL_CALL(if (!X) throw Error(OCFFM_E_ARG, "null X"); if (!delta) throw Error(OCFFM_E_ARG, "null delta");
             const FoldSpec fs = fold_spec(hist, fo, delta, nhist); mod->m->fold_in(X->d, fs));
}
int ocffm_model_recommend_fold(ocffm_model *mod, const ocffm_data *X, const ocffm_data *hist, const ocffm_fold *fo,
                               uint64_t row0, uint64_t rows, uint32_t topn, uint32_t flags, uint32_t *items,
                               double *scores) {
  MODEL_CALL(if (!X) throw Error(OCFFM_E_ARG, "null X"); const FoldSpec fs = fold_spec(hist, fo);
             mod->m->recommend(X->d, row0, rows, topn, flags, items, scores, &fs));
}
int ocffm_model_label_ranks_fold(ocffm_model *mod, const ocffm_data *X, const ocffm_data *hist, const ocffm_fold *fo,
                                 const ocffm_data *seen, uint32_t *ranks, double *scores, uint32_t *ncand) {
  MODEL_CALL(if (!X) throw Error(OCFFM_E_ARG, "null X"); const FoldSpec fs = fold_spec(hist, fo);
             mod->m->label_ranks(X->d, seen ? &seen->d : nullptr, ranks, scores, ncand, &fs));
}
int ocffm_model_evaluate_fold(ocffm_model *mod, const ocffm_data *X, const ocffm_data *hist, const ocffm_fold *fo,
                              const ocffm_data *seen, const uint32_t *cuts, uint32_t ncut, ocffm_eval *out) {
  return model_evaluate(mod, X, hist, fo, true, seen, cuts, ncut, out);
}
int ocffm_model_evaluate_among(ocffm_model *mod, const ocffm_data *X, const ocffm_data *seen, const uint64_t *cptr,
                               const uint32_t *ccol, const uint32_t *cuts, uint32_t ncut, ocffm_eval *out) {
  const ocffm_data *Xd = X;
  std::vector<uint32_t> ranks, ncand;
  std::vector<double> scores;
  const int st = guarded([&] {
    if (!mod || !mod->m) throw Error(OCFFM_E_ARG, "null model");
    if (!X) throw Error(OCFFM_E_ARG, "null X");
    if (!out) throw Error(OCFFM_E_ARG, "null output");
    model_check_cuts(cuts, ncut);
    const HostData &d = X->d;
    ranks.resize(d.ycol.size() + 1);
    ncand.resize(d.m + 1);
    scores.resize(d.ycol.size() + 1);
    mod->m->label_ranks_among(d, seen ? &seen->d : nullptr, cptr, ccol, ranks.data(), scores.data(), ncand.data());
  });
  if (st != OCFFM_OK) return st;
  return ocffm_eval_from_ranks(Xd->d.m, Xd->d.yptr.data(), ranks.data(), scores.data(), ncand.data(), cuts, ncut, out);
}
int ocffm_model_similar_items(ocffm_model *mod, uint64_t nq, const uint32_t *qitem, const uint64_t *xptr,
                              const uint32_t *xcol, uint32_t topn, uint32_t flags, uint32_t *items, double *scores) {
  MODEL_CALL(mod->m->similar_items(nq, qitem, xptr, xcol, topn, flags, items, scores));
}
int ocffm_model_similar_to(ocffm_model *mod, const ocffm_data *Vq, uint64_t row0, uint64_t rows, const uint64_t *xptr,
                           const uint32_t *xcol, uint32_t topn, uint32_t flags, uint32_t *items, double *scores) {
  MODEL_CALL(if (!Vq) throw Error(OCFFM_E_ARG, "null Vq");
             mod->m->similar_to(Vq->d, row0, rows, xptr, xcol, topn, flags, items, scores));
}
int ocffm_model_item_similarity(ocffm_model *mod, uint64_t npairs, const uint32_t *pa, const uint32_t *pb,
                                uint32_t flags, double *out) {
  MODEL_CALL(mod->m->item_similarity(npairs, pa, pb, flags, out));
}
int ocffm_model_recommend_diverse(ocffm_model *mod, const ocffm_data *X, uint64_t row0, uint64_t rows,
                                  const uint64_t *cptr, const uint32_t *ccol, uint32_t topn, uint32_t pool,
                                  double theta, uint32_t flags, uint32_t *items, double *scores, double *mmr,
                                  uint32_t *pos) {
  MODEL_CALL(if (!X) throw Error(OCFFM_E_ARG, "null X");
             mod->m->recommend_diverse(X->d, row0, rows, cptr, ccol, topn, pool, theta, flags, items, scores, mmr, pos));
}
int ocffm_model_counter(ocffm_model *mod, const char *name, int64_t *value) {
  MODEL_CALL(if (!name || !value) throw Error(OCFFM_E_ARG, "null argument");
             const auto it = mod->m->counters.find(name); *value = it == mod->m->counters.end() ? 0 : it->second);
}
int ocffm_model_get_info(ocffm_model *mod, ocffm_model_info *out) {
  MODEL_CALL(if (!out) throw Error(OCFFM_E_ARG, "null output"); mod->m->info(out));
}
int ocffm_model_get_ds(ocffm_model *mod, uint64_t *out) {
  MODEL_CALL(if (!out) throw Error(OCFFM_E_ARG, "null output");
             const std::vector<uint64_t> &ds = mod->m->ds(); std::copy(ds.begin(), ds.end(), out));
}
int ocffm_model_get(ocffm_model *mod, char what, uint32_t b12, double *out, uint64_t cap, uint64_t *len) {
  MODEL_CALL(const uint64_t n = mod->m->get(what, b12, out, cap); if (len) *len = n);
}
void ocffm_model_destroy(ocffm_model *mod) { delete mod; }

}  // extern "C"
