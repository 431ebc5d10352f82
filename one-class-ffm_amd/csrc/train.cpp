// train.cpp — drop-in replacement for the reference's `train` binary
// (train.cpp:1-208): same argv grammar, defaults, stdout table, model file
// and exit codes, running the epoch on the GPU through the C ABI.
//
//   train [options] item_file train_file
//   -l lambda  -t iters  -p test_file  -o model_file  -w omega  -r rating
//   -c threads  -k rank  --ns  --freq
// Build-only options (the reference would take them for the item file):
//   --fp32 / --fp64 (default fp64, the reference's arithmetic type),
//   --device N;
//   --recommend <file> --topn <n> --rec-out <path> [--rec-unseen]: after the
//   solve (and any model save) the top-n items of every row of <file> (read
//   like a -p file) go to <path>, one line of item:score tokens per row;
//   with --rec-candidates <file> (line i: the whitespace-separated item
//   indices row i is ranked among; a blank line is an empty list) the top-n
//   of every row's own list instead;
//   --eval <file> [--eval-cuts c1,c2,...] [--eval-seen <file>]: after that,
//   the ranking metrics of the model on the labelled rows of <file> (read
//   like a -p file) as one `eval` table on stdout; with
//   --eval-candidates <file> (--rec-candidates' format, one list per row of
//   the --eval file) every label is ranked among its row's list and labels.
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ocffm.h"

static std::string usage() {
  return "usage: train [options] item_feature_file train_file\n"
         "\n"
         "options:\n"
         "-l <lambda_2>: set regularization coefficient on r regularizer (default 1e-5)\n"
         "-t <iter>: set number of iterations (default 20)\n"
         "-p <path>: set path to test set\n"
         "-o <path>: set path to save model file\n"
         "-w <omega>: set cost weight for the negatives (default 0.1)\n"
         "-r <rating>: set rating for the negatives (default -1)\n"
         "-c <threads>: set number of cores\n"
         "-k <rank>: set number of rank (default 4)\n"
         "--ns: no self-side field pairs\n"
         "--freq: enable freq-aware lambda\n"
         "--fp32 | --fp64: device arithmetic (default fp64)\n"
         "--device <n>: HIP device ordinal\n"
         "--recommend <path>: after training, recommend items for every row of this file (read like -p)\n"
         "--topn <n>: items per row, 1..128 (default 10)\n"
         "--rec-out <path>: where the recommendations go (one line of item:score per row)\n"
         "--rec-unseen: leave out each row's own labels\n"
         "--rec-candidates <path>: rank every row among its own list only (line i: the item indices of row i of\n"
         "                         the --recommend file, whitespace-separated; a blank line is an empty list)\n"
         "--eval <path>: after training, print ranking metrics on the labelled rows of this file (read like -p)\n"
         "--eval-cuts <c1,c2,...>: up to 8 increasing cut-offs (default 5,10,20,40,80)\n"
         "--eval-seen <path>: rows whose labels are left out of the candidates (same row count as --eval)\n"
         "--eval-candidates <path>: rank every label among its row's own list and labels only (line i: the item\n"
         "                          indices of row i of the --eval file, in --rec-candidates' format)\n";
}

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

int main(int argc, char **argv) {
  ocffm_param prm;
  ocffm_param_default(&prm);
  std::string te_path, model_path, rec_path, rec_out, rec_cand, eval_path, eval_seen, eval_cand;
  std::vector<uint32_t> eval_cuts{5, 10, 20, 40, 80};
  long topn = 10;
  bool rec_unseen = false;
  try {
    if (argc == 1) throw std::invalid_argument(usage());
    int i = 1;
    for (; i < argc; i++) {
      const std::string a = argv[i];
      auto value = [&](bool numeric, const char *msg) -> const char * {
        if (i + 1 >= argc) throw std::invalid_argument(msg);
        i++;
        if (numeric && !is_numerical(argv[i])) throw std::invalid_argument(a + " should be followed by a number");
        return argv[i];
      };
      if (a == "-l") prm.lambda = std::atof(value(true, "need to specify l regularization coefficient after -l"));
      else if (a == "-k") prm.k = (uint32_t)std::atoi(value(true, "need to specify rank after -k"));
      else if (a == "-t") prm.nr_pass = (uint32_t)std::atoi(value(true, "need to specify max number of iterations after -t"));
      else if (a == "-w") prm.omega = std::atof(value(true, "need to specify omega after -w"));
      else if (a == "-r") prm.r = std::atof(value(true, "need to specify rating after -r"));
      else if (a == "-c") prm.nr_threads = (uint32_t)std::atof(value(true, "missing core numbers after -c"));
      else if (a == "-p") te_path = value(false, "need to specify path after -p");
      else if (a == "-o") model_path = value(false, "need to specify path after -o");
      else if (a == "--ns") prm.self_side = 0;
      else if (a == "--freq") prm.freq = 1;
      else if (a == "--fp32") prm.precision = OCFFM_FP32;
      else if (a == "--fp64") prm.precision = OCFFM_FP64;
      else if (a == "--device") prm.device = std::atoi(value(true, "need a device ordinal after --device"));
      else if (a == "--recommend") rec_path = value(false, "need to specify path after --recommend");
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
      else break;
    }
    if (!rec_path.empty() && rec_out.empty()) throw std::invalid_argument("--recommend needs --rec-out <path>");
    if (!rec_cand.empty() && rec_path.empty()) throw std::invalid_argument("--rec-candidates needs --recommend <path>");
    if (topn < 1 || topn > OCFFM_REC_MAX_TOPN) throw std::invalid_argument("--topn must be in 1..128");
    if (!eval_seen.empty() && eval_path.empty()) throw std::invalid_argument("--eval-seen needs --eval <path>");
    if (!eval_cand.empty() && eval_path.empty()) throw std::invalid_argument("--eval-candidates needs --eval <path>");
    if (eval_cuts.empty() || eval_cuts.size() > OCFFM_EVAL_MAX_CUTS) throw std::invalid_argument("--eval-cuts takes 1..8 cut-offs");
    for (size_t s = 1; s < eval_cuts.size(); s++)
      if (eval_cuts[s] <= eval_cuts[s - 1]) throw std::invalid_argument("--eval-cuts must be strictly increasing");
    if (i >= argc) throw std::invalid_argument("training data not specified");
    if (i + 1 >= argc) throw std::invalid_argument("training data not specified");
    const std::string item_path = argv[i], tr_path = argv[i + 1];

    // train.cpp:177-196.  OCFFM_TIMING=1: phase wall times on stderr.
    const bool timing = std::getenv("OCFFM_TIMING") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto phase = [&](const char *name) {
      const auto t = std::chrono::steady_clock::now();
      if (timing) std::fprintf(stderr, "[timing] %-8s %9.3f ms\n", name, std::chrono::duration<double, std::milli>(t - t_prev).count());
      t_prev = t;
    };
    ocffm_data *U = nullptr, *V = nullptr, *Ut = nullptr;
    check(ocffm_data_read(tr_path.c_str(), 1, nullptr, 0, &U));
    check(ocffm_data_read(item_path.c_str(), 0, nullptr, 0, &V));
    check(ocffm_data_trans_y(V, U));
    if (!te_path.empty()) {
      ocffm_data_info info;
      check(ocffm_data_get_info(U, &info));
      std::uint64_t *ds = new std::uint64_t[info.f ? info.f : 1];
      check(ocffm_data_get_ds(U, ds));
      check(ocffm_data_read(te_path.c_str(), 1, ds, (uint32_t)info.f, &Ut));
      delete[] ds;
    }
    // the candidate lists are read and checked before any device work
    ocffm_data *Xrec = nullptr;
    std::vector<std::uint64_t> cptr;
    std::vector<std::uint32_t> ccol;
    if (!rec_cand.empty()) {
      ocffm_data_info info, xi;
      check(ocffm_data_get_info(U, &info));
      std::vector<std::uint64_t> ds(info.f ? info.f : 1);
      check(ocffm_data_get_ds(U, ds.data()));
      check(ocffm_data_read(rec_path.c_str(), 1, ds.data(), (uint32_t)info.f, &Xrec));
      check(ocffm_data_get_info(Xrec, &xi));
      read_candidates(rec_cand, "--recommend", xi.m, cptr, ccol);
      ccol.push_back(0);  // (a pointer for an empty file)
    }
    ocffm_data *Xev = nullptr;
    std::vector<std::uint64_t> eptr;
    std::vector<std::uint32_t> ecol;
    if (!eval_cand.empty()) {
      ocffm_data_info info, xi;
      check(ocffm_data_get_info(U, &info));
      std::vector<std::uint64_t> ds(info.f ? info.f : 1);
      check(ocffm_data_get_ds(U, ds.data()));
      check(ocffm_data_read(eval_path.c_str(), 1, ds.data(), (uint32_t)info.f, &Xev));
      check(ocffm_data_get_info(Xev, &xi));
      read_candidates(eval_cand, "--eval", xi.m, eptr, ecol);
      ecol.push_back(0);
    }
    phase("read");
    ocffm_problem *prob = nullptr;
    check(ocffm_problem_create(U, Ut, V, &prm, &prob));
    phase("create");
    // The reference's init is the first consumer of the process rand()
    // stream (implicit seed 1, ffm.cpp:72); HIP/RCCL start-up above may have
    // drawn from it, so restore that state before the draws.
    std::srand(1);
    check(ocffm_problem_init(prob));
    check(ocffm_problem_sync(prob));
    phase("init");
    check(ocffm_problem_solve(prob));
    phase("solve");
    if (!model_path.empty()) check(ocffm_problem_save_model(prob, model_path.c_str()));
    phase("save");
    if (!rec_path.empty()) {
      ocffm_data_info info;
      check(ocffm_data_get_info(U, &info));
      std::vector<std::uint64_t> ds(info.f ? info.f : 1);
      check(ocffm_data_get_ds(U, ds.data()));
      ocffm_data *X = Xrec;
      if (!X) check(ocffm_data_read(rec_path.c_str(), 1, ds.data(), (uint32_t)info.f, &X));
      ocffm_data_info xi;
      check(ocffm_data_get_info(X, &xi));
      std::vector<uint32_t> items(xi.m * (size_t)topn + 1);
      std::vector<double> scores(xi.m * (size_t)topn + 1);
      const uint32_t flags = rec_unseen ? OCFFM_REC_EXCLUDE_LABELS : 0u;
      if (rec_cand.empty()) {
        check(ocffm_problem_recommend(prob, X, 0, xi.m, (uint32_t)topn, flags, items.data(), scores.data()));
      } else {
        check(ocffm_problem_recommend_among(prob, X, 0, xi.m, cptr.data(), ccol.data(), (uint32_t)topn, flags,
                                            items.data(), scores.data()));
      }
      std::FILE *fp = std::fopen(rec_out.c_str(), "w");
      if (!fp) throw Fail(OCFFM_E_IO, "cannot write " + rec_out);
      for (std::uint64_t i = 0; i < xi.m; i++) {
        for (long t = 0; t < topn && items[i * topn + t] != OCFFM_REC_NONE; t++)
          std::fprintf(fp, t ? " %u:%.17g" : "%u:%.17g", items[i * topn + t], scores[i * topn + t]);
        std::fputc('\n', fp);
      }
      if (std::fclose(fp) != 0) throw Fail(OCFFM_E_IO, "write failed: " + rec_out);
      ocffm_data_free(X);
      phase("recommend");
    }
    if (!eval_path.empty()) {
      ocffm_data_info info;
      check(ocffm_data_get_info(U, &info));
      std::vector<std::uint64_t> ds(info.f ? info.f : 1);
      check(ocffm_data_get_ds(U, ds.data()));
      ocffm_data *X = Xev, *Sn = nullptr;
      if (!X) check(ocffm_data_read(eval_path.c_str(), 1, ds.data(), (uint32_t)info.f, &X));
      if (!eval_seen.empty()) check(ocffm_data_read(eval_seen.c_str(), 1, ds.data(), (uint32_t)info.f, &Sn));
      ocffm_eval ev;
      if (eval_cand.empty())
        check(ocffm_problem_evaluate(prob, X, Sn, eval_cuts.data(), (uint32_t)eval_cuts.size(), &ev));
      else
        check(ocffm_problem_evaluate_among(prob, X, Sn, eptr.data(), ecol.data(), eval_cuts.data(),
                                           (uint32_t)eval_cuts.size(), &ev));
      std::printf("eval rows %llu rows_used %llu labels %llu labels_ranked %llu\n", (unsigned long long)ev.rows,
                  (unsigned long long)ev.rows_used, (unsigned long long)ev.labels, (unsigned long long)ev.labels_ranked);
      std::printf("eval loss %.17g mrr %.17g auc %.17g\n", ev.loss, ev.mrr, ev.auc);
      std::printf("eval cut prec recall ndcg map hit\n");
      for (uint32_t s = 0; s < ev.ncut; s++)
        std::printf("eval %u %.17g %.17g %.17g %.17g %.17g\n", ev.cuts[s], ev.prec[s], ev.recall[s], ev.ndcg[s],
                    ev.map[s], ev.hit[s]);
      std::fflush(stdout);
      ocffm_data_free(X);
      if (Sn) ocffm_data_free(Sn);
      phase("evaluate");
    }
    ocffm_problem_destroy(prob);
    ocffm_data_free(U);
    ocffm_data_free(V);
    if (Ut) ocffm_data_free(Ut);
  } catch (std::invalid_argument &e) {
    std::cerr << e.what() << std::endl;
    return 1;
  } catch (Fail &e) {
    std::cerr << "error: " << e.what() << std::endl;
    return e.code == OCFFM_E_ARG ? 1 : 2;
  }
  return 0;
}
