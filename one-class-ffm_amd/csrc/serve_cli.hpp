// serve_cli.hpp — the serving options of the two CLI binaries (train.cpp after
// its solve, predict.cpp on a saved model): --recommend / --topn / --rec-out /
// --rec-unseen / --rec-candidates and --eval / --eval-cuts / --eval-seen /
// --eval-candidates: their parsing, their checks, the candidate-list files and
// the output writing.  Both binaries write the same bytes for the same model
// and rows.
#pragma once

#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ocffm.h"

// train.cpp:22-32: at least one digit somewhere in the token.
static bool is_numerical(const char *s) {
  for (; *s; s++)
    if (std::isdigit((unsigned char)*s)) return true;
  return false;
}

// --rec-candidates / --eval-candidates: one list per line of the file of
// option `rows_of`.  Throws std::invalid_argument (exit 1).
static void read_candidates(const std::string &path, const char *rows_of, std::uint64_t rows,
                            std::vector<std::uint64_t> &cptr, std::vector<std::uint32_t> &ccol) {
  std::ifstream in(path);
  if (!in) throw std::invalid_argument("cannot read " + path);
  cptr.assign(1, 0);
  std::string line;
  while (std::getline(in, line)) {
    const char *s = line.c_str();
    for (;;) {
      while (*s && std::isspace((unsigned char)*s)) s++;
      if (!*s) break;
      const char *b = s;
      std::uint64_t v = 0;
      for (; std::isdigit((unsigned char)*s); s++) {
        v = v * 10 + (std::uint64_t)(*s - '0');
        if (v > 0xffffffffull) v = 0xffffffffull;  // (no item: OCFFM_REC_NONE is never a candidate)
      }
      if (s == b || (*s && !std::isspace((unsigned char)*s)))
        throw std::invalid_argument(path + ": line " + std::to_string(cptr.size()) +
                                    ": an item index must be a non-negative integer");
      ccol.push_back((std::uint32_t)v);
    }
    cptr.push_back(ccol.size());
  }
  if (cptr.size() - 1 != rows)
    throw std::invalid_argument(path + ": " + std::to_string(cptr.size() - 1) + " lines for " + std::to_string(rows) +
                                " rows of the " + rows_of + " file");
}

struct Fail : std::runtime_error {
  int code;
  Fail(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

static void check(int st) {
  if (st != OCFFM_OK) throw Fail(st, ocffm_last_error());
}

// The usage lines of the serving options (`after`: "after training" or "")
static std::string serve_usage(const std::string &after) {
  return "--recommend <path>: " + after + "recommend items for every row of this file (read like -p)\n"
         "--topn <n>: items per row, 1..128 (default 10)\n"
         "--rec-out <path>: where the recommendations go (one line of item:score per row)\n"
         "--rec-unseen: leave out each row's own labels\n"
         "--rec-candidates <path>: rank every row among its own list only (line i: the item indices of row i of\n"
         "                         the --recommend file, whitespace-separated; a blank line is an empty list)\n"
         "--eval <path>: " + after + "print ranking metrics on the labelled rows of this file (read like -p)\n"
         "--eval-cuts <c1,c2,...>: up to 8 increasing cut-offs (default 5,10,20,40,80)\n"
         "--eval-seen <path>: rows whose labels are left out of the candidates (same row count as --eval)\n"
         "--eval-candidates <path>: rank every label among its row's own list and labels only (line i: the item\n"
         "                          indices of row i of the --eval file, in --rec-candidates' format)\n";
}

struct ServeOptions {
  std::string rec_path, rec_out, rec_cand, eval_path, eval_seen, eval_cand;
  std::vector<uint32_t> eval_cuts{5, 10, 20, 40, 80};
  long topn = 10;
  bool rec_unseen = false;

  // Takes option `a` if it is a serving option (value(numeric, msg): the
  // binary's own fetch of the next argument).
  template <class Value> bool take(const std::string &a, Value &&value) {
    if (a == "--recommend") rec_path = value(false, "need to specify path after --recommend");
    else if (a == "--rec-out") rec_out = value(false, "need to specify path after --rec-out");
    else if (a == "--topn") topn = std::atol(value(true, "need to specify the number of items after --topn"));
    else if (a == "--rec-unseen") rec_unseen = true;
    else if (a == "--rec-candidates") rec_cand = value(false, "need to specify path after --rec-candidates");
    else if (a == "--eval") eval_path = value(false, "need to specify path after --eval");
    else if (a == "--eval-seen") eval_seen = value(false, "need to specify path after --eval-seen");
    else if (a == "--eval-candidates") eval_cand = value(false, "need to specify path after --eval-candidates");
    else if (a == "--eval-cuts") {
      eval_cuts.clear();
      for (const char *s = value(true, "need to specify cut-offs after --eval-cuts"); *s;) {
        char *end = nullptr;
        const long c = std::strtol(s, &end, 10);
        if (end == s || c < 1 || (*end && *end != ',')) throw std::invalid_argument("--eval-cuts takes c1,c2,... with every c >= 1");
        eval_cuts.push_back((uint32_t)c);
        s = *end ? end + 1 : end;
      }
    }
    else return false;
    return true;
  }
  void validate() const {
    if (!rec_path.empty() && rec_out.empty()) throw std::invalid_argument("--recommend needs --rec-out <path>");
    if (!rec_cand.empty() && rec_path.empty()) throw std::invalid_argument("--rec-candidates needs --recommend <path>");
    if (topn < 1 || topn > OCFFM_REC_MAX_TOPN) throw std::invalid_argument("--topn must be in 1..128");
    if (!eval_seen.empty() && eval_path.empty()) throw std::invalid_argument("--eval-seen needs --eval <path>");
    if (!eval_cand.empty() && eval_path.empty()) throw std::invalid_argument("--eval-candidates needs --eval <path>");
    if (eval_cuts.empty() || eval_cuts.size() > OCFFM_EVAL_MAX_CUTS) throw std::invalid_argument("--eval-cuts takes 1..8 cut-offs");
    for (size_t s = 1; s < eval_cuts.size(); s++)
      if (eval_cuts[s] <= eval_cuts[s - 1]) throw std::invalid_argument("--eval-cuts must be strictly increasing");
  }
};

// The candidate lists and the rows they belong to, read and checked before any
// device work (ds: the user fields' Ds the rows are read with)
struct ServeLists {
  ocffm_data *Xrec = nullptr, *Xev = nullptr;
  std::vector<std::uint64_t> cptr, eptr;
  std::vector<std::uint32_t> ccol, ecol;

  void read(const ServeOptions &o, const std::uint64_t *ds, uint32_t nds) {
    if (!o.rec_cand.empty()) {
      ocffm_data_info xi;
      check(ocffm_data_read(o.rec_path.c_str(), 1, ds, nds, &Xrec));
      check(ocffm_data_get_info(Xrec, &xi));
      read_candidates(o.rec_cand, "--recommend", xi.m, cptr, ccol);
      ccol.push_back(0);  // (a pointer for an empty file)
    }
    if (!o.eval_cand.empty()) {
      ocffm_data_info xi;
      check(ocffm_data_read(o.eval_path.c_str(), 1, ds, nds, &Xev));
      check(ocffm_data_get_info(Xev, &xi));
      read_candidates(o.eval_cand, "--eval", xi.m, eptr, ecol);
      ecol.push_back(0);
    }
  }
};

// The serving calls of a problem or a model behind one face
struct ProblemServer {
  ocffm_problem *h;
  int recommend(const ocffm_data *X, std::uint64_t rows, uint32_t topn, uint32_t flags, uint32_t *items, double *scores) {
    return ocffm_problem_recommend(h, X, 0, rows, topn, flags, items, scores);
  }
  int recommend_among(const ocffm_data *X, std::uint64_t rows, const std::uint64_t *cptr, const uint32_t *ccol,
                      uint32_t topn, uint32_t flags, uint32_t *items, double *scores) {
    return ocffm_problem_recommend_among(h, X, 0, rows, cptr, ccol, topn, flags, items, scores);
  }
  int evaluate(const ocffm_data *X, const ocffm_data *seen, const uint32_t *cuts, uint32_t ncut, ocffm_eval *out) {
    return ocffm_problem_evaluate(h, X, seen, cuts, ncut, out);
  }
  int evaluate_among(const ocffm_data *X, const ocffm_data *seen, const std::uint64_t *cptr, const uint32_t *ccol,
                     const uint32_t *cuts, uint32_t ncut, ocffm_eval *out) {
    return ocffm_problem_evaluate_among(h, X, seen, cptr, ccol, cuts, ncut, out);
  }
};
struct ModelServer {
  ocffm_model *h;
  const ocffm_data *hist = nullptr;  // predict --fold-history: the rows are folded in first
  ocffm_fold fo{};
  double theta = -1;                 // predict --diversify: >= 0 re-ranks each row's top-`pool` list (ocffm_diverse.h)
  uint32_t pool = 0;
  int recommend(const ocffm_data *X, std::uint64_t rows, uint32_t topn, uint32_t flags, uint32_t *items, double *scores) {
    if (theta >= 0)
      return ocffm_model_recommend_diverse(h, X, 0, rows, nullptr, nullptr, topn, pool, theta, flags, items, scores,
                                           nullptr, nullptr);
    if (hist) return ocffm_model_recommend_fold(h, X, hist, &fo, 0, rows, topn, flags, items, scores);
    return ocffm_model_recommend(h, X, 0, rows, topn, flags, items, scores);
  }
  int recommend_among(const ocffm_data *X, std::uint64_t rows, const std::uint64_t *cptr, const uint32_t *ccol,
                      uint32_t topn, uint32_t flags, uint32_t *items, double *scores) {
    if (theta >= 0)
      return ocffm_model_recommend_diverse(h, X, 0, rows, cptr, ccol, topn, pool, theta, flags, items, scores, nullptr,
                                           nullptr);
    return ocffm_model_recommend_among(h, X, 0, rows, cptr, ccol, topn, flags, items, scores);
  }
  int evaluate(const ocffm_data *X, const ocffm_data *seen, const uint32_t *cuts, uint32_t ncut, ocffm_eval *out) {
    if (hist) return ocffm_model_evaluate_fold(h, X, hist, &fo, seen, cuts, ncut, out);
    return ocffm_model_evaluate(h, X, seen, cuts, ncut, out);
  }
  int evaluate_among(const ocffm_data *X, const ocffm_data *seen, const std::uint64_t *cptr, const uint32_t *ccol,
                     const uint32_t *cuts, uint32_t ncut, ocffm_eval *out) {
    return ocffm_model_evaluate_among(h, X, seen, cptr, ccol, cuts, ncut, out);
  }
};

// --recommend, then --eval: the calls and their output (the recommendation
// file: one line of item:score tokens per row; the `eval` table on stdout).
// phase(name): the binary's timing hook.
template <class Server, class Phase>
static void serve(Server srv, const ServeOptions &o, ServeLists &l, const std::uint64_t *ds, uint32_t nds, Phase &&phase) {
  const long topn = o.topn;
  if (!o.rec_path.empty()) {
    ocffm_data *X = l.Xrec;
    if (!X) check(ocffm_data_read(o.rec_path.c_str(), 1, ds, nds, &X));
    ocffm_data_info xi;
    check(ocffm_data_get_info(X, &xi));
    std::vector<uint32_t> items(xi.m * (size_t)topn + 1);
    std::vector<double> scores(xi.m * (size_t)topn + 1);
    const uint32_t flags = o.rec_unseen ? OCFFM_REC_EXCLUDE_LABELS : 0u;
    if (o.rec_cand.empty()) {
      check(srv.recommend(X, xi.m, (uint32_t)topn, flags, items.data(), scores.data()));
    } else {
      check(srv.recommend_among(X, xi.m, l.cptr.data(), l.ccol.data(), (uint32_t)topn, flags, items.data(),
                                scores.data()));
    }
    std::FILE *fp = std::fopen(o.rec_out.c_str(), "w");
    if (!fp) throw Fail(OCFFM_E_IO, "cannot write " + o.rec_out);
    for (std::uint64_t i = 0; i < xi.m; i++) {
      for (long t = 0; t < topn && items[i * topn + t] != OCFFM_REC_NONE; t++)
        std::fprintf(fp, t ? " %u:%.17g" : "%u:%.17g", items[i * topn + t], scores[i * topn + t]);
      std::fputc('\n', fp);
    }
    if (std::fclose(fp) != 0) throw Fail(OCFFM_E_IO, "write failed: " + o.rec_out);
    ocffm_data_free(X);
    l.Xrec = nullptr;
    phase("recommend");
  }
  if (!o.eval_path.empty()) {
    ocffm_data *X = l.Xev, *Sn = nullptr;
    if (!X) check(ocffm_data_read(o.eval_path.c_str(), 1, ds, nds, &X));
    if (!o.eval_seen.empty()) check(ocffm_data_read(o.eval_seen.c_str(), 1, ds, nds, &Sn));
    ocffm_eval ev;
    if (o.eval_cand.empty())
      check(srv.evaluate(X, Sn, o.eval_cuts.data(), (uint32_t)o.eval_cuts.size(), &ev));
    else
      check(srv.evaluate_among(X, Sn, l.eptr.data(), l.ecol.data(), o.eval_cuts.data(), (uint32_t)o.eval_cuts.size(),
                               &ev));
    std::printf("eval rows %llu rows_used %llu labels %llu labels_ranked %llu\n", (unsigned long long)ev.rows,
                (unsigned long long)ev.rows_used, (unsigned long long)ev.labels, (unsigned long long)ev.labels_ranked);
    std::printf("eval loss %.17g mrr %.17g auc %.17g\n", ev.loss, ev.mrr, ev.auc);
    std::printf("eval cut prec recall ndcg map hit\n");
    for (uint32_t s = 0; s < ev.ncut; s++)
      std::printf("eval %u %.17g %.17g %.17g %.17g %.17g\n", ev.cuts[s], ev.prec[s], ev.recall[s], ev.ndcg[s],
                  ev.map[s], ev.hit[s]);
    std::fflush(stdout);
    ocffm_data_free(X);
    l.Xev = nullptr;
    if (Sn) ocffm_data_free(Sn);
    phase("evaluate");
  }
}
