// predict.cpp — serve from a saved model (no reference counterpart: the
// reference writes its model files and reads none).
//
//   predict [options] model_file item_file
//   --fp32 / --fp64 (default fp64), --device N;
//   --binary: model_file is the snapshot of train --binary-out (default: the
//   text model of train -o, six digits per value);
//   --popularity <train_file>: the cold rows' scores, count / total of every
//   label of this labelled file (ffm.cpp:143,172-176); its labels are indices
//   into item_file, so this is for the training catalogue;
//   the serving options of train (serve_cli.hpp), with the same meaning and
//   the same output bytes: --recommend / --topn / --rec-out / --rec-unseen /
//   --rec-candidates, --eval / --eval-cuts / --eval-seen / --eval-candidates;
//   --fold-field <f> --fold-history <labelled file> [--fold-omega w]
//   [--fold-lambda l] [--fold-r r]: fold every row of the --recommend and
//   --eval files in from the labels of the same row of the history file
//   (ocffm_fold.h ocffm_model_fold_in) before it is served; w, l, r default to
//   train's -w, -l, -r defaults.  Not with the candidate-list options.
//   --similar <file | all> --sim-out <path> [--sim-metric cosine|dot]: the
//   --topn catalogue items most similar to each query item (ocffm_similar.h
//   ocffm_model_similar_items; the query itself left out), the queries being
//   the catalogue indices of the file, one per line, or every item for the
//   word `all`; the output has --rec-out's format, one line per query.
//   --diversify <theta> [--pool <n>]: --recommend's lists are re-ranked by
//   greedy MMR over each row's top-n pool (ocffm_diverse.h
//   ocffm_model_recommend_diverse; n defaults to min(128, 4 topn)); --rec-out
//   keeps its format, item:score with the model score, in the order the items
//   were taken.  With --rec-candidates and --rec-unseen; not with --fold-field.
// item_file is the catalogue: any item rows in the model's item field space
// (read with the model's item Ds, as a test file is with the train Ds).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ocffm.h"
#include "serve_cli.hpp"

static std::string usage() {
  return "usage: predict [options] model_file item_feature_file\n"
         "\n"
         "options:\n"
         "--fp32 | --fp64: device arithmetic (default fp64)\n"
         "--device <n>: HIP device ordinal\n"
         "--binary: model_file is a binary snapshot (train --binary-out); default: the text model (train -o)\n"
         "--popularity <path>: labelled train file whose label counts score the rows without features\n"
         "--fold-field <f>: fold the rows in as new values of user field f, from their histories\n"
         "--fold-history <path>: labelled file, one row per row of the --recommend / --eval file: the items the\n"
         "                       row's user has touched (only the labels are read)\n"
         "--fold-omega <w> | --fold-lambda <l> | --fold-r <r>: the fold's parameters (default: train's defaults)\n"
         "--similar <path | all>: the --topn items most similar to each catalogue item of this file (one index per\n"
         "                        line), or to every item for the word all\n"
         "--sim-out <path>: where the similar items go (--rec-out's format, one line per query item)\n"
         "--sim-metric cosine | dot: the similarity (default cosine)\n"
         "--diversify <theta>: re-rank --recommend's lists by greedy MMR, theta in [0, 1] the weight of the\n"
         "                     similarity to the items already taken (0: no change)\n"
         "--pool <n>: the MMR's pool, each row's top n, --topn..128 (default min(128, 4 topn))\n" +
         serve_usage("");
}

// The query items of --similar: one catalogue index per line (blank lines are
// skipped).  Throws std::invalid_argument (exit 1).
static std::vector<std::uint32_t> read_queries(const std::string &path) {
  std::ifstream in(path);
  if (!in) throw std::invalid_argument("cannot read " + path);
  std::vector<std::uint32_t> q;
  std::string line;
  for (std::uint64_t ln = 1; std::getline(in, line); ln++) {
    const char *s = line.c_str();
    while (*s && std::isspace((unsigned char)*s)) s++;
    if (!*s) continue;
    std::uint64_t v = 0;
    const char *b = s;
    for (; std::isdigit((unsigned char)*s); s++) {
      v = v * 10 + (std::uint64_t)(*s - '0');
      if (v > 0xffffffffull) v = 0xffffffffull;  // (outside any catalogue: the call reports it)
    }
    while (*s && std::isspace((unsigned char)*s)) s++;
    if (s == b || *s)
      throw std::invalid_argument(path + ": line " + std::to_string(ln) + ": a catalogue index must be a non-negative integer");
    q.push_back((std::uint32_t)v);
  }
  return q;
}

int main(int argc, char **argv) {
  int precision = OCFFM_FP64, device = 0;
  bool binary = false;
  std::string pop_path, fold_hist, sim_path, sim_out, sim_metric = "cosine";
  long fold_field = -1, pool = -1;
  double theta = -1;
  bool diversify = false;
  ocffm_param pd;
  ocffm_param_default(&pd);
  ocffm_fold fo{0, pd.omega, pd.lambda, pd.r};
  ServeOptions so;
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
      if (a == "--fp32") precision = OCFFM_FP32;
      else if (a == "--fp64") precision = OCFFM_FP64;
      else if (a == "--device") device = std::atoi(value(true, "need a device ordinal after --device"));
      else if (a == "--binary") binary = true;
      else if (a == "--popularity") pop_path = value(false, "need to specify path after --popularity");
      else if (a == "--fold-field") fold_field = std::atol(value(true, "need a user field after --fold-field"));
      else if (a == "--fold-history") fold_hist = value(false, "need to specify path after --fold-history");
      else if (a == "--fold-omega") fo.omega = std::atof(value(true, "need a number after --fold-omega"));
      else if (a == "--fold-lambda") fo.lambda = std::atof(value(true, "need a number after --fold-lambda"));
      else if (a == "--fold-r") fo.r = std::atof(value(true, "need a number after --fold-r"));
      else if (a == "--similar") sim_path = value(false, "need a path or the word all after --similar");
      else if (a == "--sim-out") sim_out = value(false, "need to specify path after --sim-out");
      else if (a == "--sim-metric") sim_metric = value(false, "need cosine or dot after --sim-metric");
      else if (a == "--diversify") {
        theta = std::atof(value(true, "need theta after --diversify"));
        diversify = true;
      }
      else if (a == "--pool") pool = std::atol(value(true, "need the pool size after --pool"));
      else if (so.take(a, value)) continue;
      else break;
    }
    so.validate();
    const bool fold = fold_field >= 0 || !fold_hist.empty();
    if (fold && (fold_field < 0 || fold_hist.empty()))
      throw std::invalid_argument("--fold-field and --fold-history go together");
    if (fold && so.rec_path.empty() && so.eval_path.empty())
      throw std::invalid_argument("--fold-field needs --recommend or --eval");
    if (fold && (!so.rec_cand.empty() || !so.eval_cand.empty()))
      throw std::invalid_argument("--fold-field cannot be combined with the candidate-list options");
    fo.field = fold ? (uint32_t)fold_field : 0u;
    if (!sim_path.empty() && sim_out.empty()) throw std::invalid_argument("--similar needs --sim-out <path>");
    if (sim_path.empty() && !sim_out.empty()) throw std::invalid_argument("--sim-out needs --similar <path | all>");
    if (sim_metric != "cosine" && sim_metric != "dot") throw std::invalid_argument("--sim-metric takes cosine or dot");
    if (pool >= 0 && !diversify) throw std::invalid_argument("--pool needs --diversify <theta>");
    if (diversify) {
      if (so.rec_path.empty()) throw std::invalid_argument("--diversify needs --recommend <path>");
      if (!(theta >= 0.0 && theta <= 1.0)) throw std::invalid_argument("--diversify takes theta in [0, 1]");
      if (fold)
        throw std::invalid_argument("--diversify cannot be combined with --fold-field: folded rows are not diversified");
      if (pool < 0) pool = so.topn * 4 < OCFFM_DIV_MAX_POOL ? so.topn * 4 : OCFFM_DIV_MAX_POOL;
      if (pool < so.topn || pool > OCFFM_DIV_MAX_POOL) throw std::invalid_argument("--pool must be in --topn..128");
    }
    if (i + 1 >= argc) throw std::invalid_argument("model file and item file not specified");
    if (i + 2 < argc) throw std::invalid_argument(std::string("unexpected argument: ") + argv[i + 2]);
    const std::string model_path = argv[i], item_path = argv[i + 1];

    const bool timing = std::getenv("OCFFM_TIMING") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto phase = [&](const char *name) {
      const auto t = std::chrono::steady_clock::now();
      if (timing) std::fprintf(stderr, "[timing] %-8s %9.3f ms\n", name, std::chrono::duration<double, std::milli>(t - t_prev).count());
      t_prev = t;
    };
    // the model file is read and checked on the host before any device work
    ocffm_model_info mi{};
    check(ocffm_model_file_info(model_path.c_str(), binary ? 1 : 0, &mi));
    std::vector<std::uint64_t> ds(mi.f);
    mi.Ds = ds.data();
    mi.ds_cap = mi.f;
    check(ocffm_model_file_info(model_path.c_str(), binary ? 1 : 0, &mi));
    ocffm_data *V = nullptr, *Up = nullptr;
    check(ocffm_data_read(item_path.c_str(), 0, ds.data() + mi.fu, mi.fv, &V));
    std::vector<double> pop;
    if (!pop_path.empty()) {
      check(ocffm_data_read(pop_path.c_str(), 1, nullptr, 0, &Up));
      ocffm_data_info ui;
      check(ocffm_data_get_info(Up, &ui));
      std::vector<std::uint64_t> yptr(ui.m + 1), ycol(ui.nnz_y + 1);
      check(ocffm_data_get_labels(Up, yptr.data(), ycol.data()));
      pop.assign(ui.n, 0.0);
      for (std::uint64_t p = 0; p < ui.nnz_y; p++) pop[ycol[p]] += 1;
      double s = 0;
      for (double v : pop) s += v;
      for (double &v : pop) v /= s;
      ocffm_data_free(Up);
    }
    ServeLists lists;
    lists.read(so, ds.data(), mi.fu);
    std::vector<std::uint32_t> simq;
    if (!sim_path.empty() && sim_path != "all") simq = read_queries(sim_path);
    ocffm_data *Hs = nullptr;
    if (fold) check(ocffm_data_read(fold_hist.c_str(), 1, ds.data(), mi.fu, &Hs));
    phase("read");
    ocffm_model *mod = nullptr;
    check(binary ? ocffm_model_load_binary(model_path.c_str(), precision, device, &mod)
                 : ocffm_model_load_text(model_path.c_str(), precision, device, &mod));
    phase("load");
    check(ocffm_model_set_items(mod, V));
    if (!pop.empty()) check(ocffm_model_set_popularity(mod, pop.data(), pop.size()));
    phase("items");
    serve(ModelServer{mod, Hs, fo, diversify ? theta : -1.0, (uint32_t)(diversify ? pool : 0)}, so, lists, ds.data(), mi.fu,
          phase);
    if (!sim_path.empty()) {
      if (sim_path == "all") {
        ocffm_data_info vi;
        check(ocffm_data_get_info(V, &vi));
        simq.resize(vi.m);
        for (std::uint64_t j = 0; j < vi.m; j++) simq[j] = (std::uint32_t)j;
      }
      const std::uint64_t nq = simq.size();
      const long topn = so.topn;
      std::vector<uint32_t> items(nq * (size_t)topn + 1);
      std::vector<double> scores(nq * (size_t)topn + 1);
      simq.push_back(0);  // (a pointer for an empty file)
      check(ocffm_model_similar_items(mod, nq, simq.data(), nullptr, nullptr, (uint32_t)topn,
                                      sim_metric == "dot" ? OCFFM_SIM_DOT : 0u, items.data(), scores.data()));
      std::FILE *fp = std::fopen(sim_out.c_str(), "w");
      if (!fp) throw Fail(OCFFM_E_IO, "cannot write " + sim_out);
      for (std::uint64_t i = 0; i < nq; i++) {
        for (long t = 0; t < topn && items[i * topn + t] != OCFFM_REC_NONE; t++)
          std::fprintf(fp, t ? " %u:%.17g" : "%u:%.17g", items[i * topn + t], scores[i * topn + t]);
        std::fputc('\n', fp);
      }
      if (std::fclose(fp) != 0) throw Fail(OCFFM_E_IO, "write failed: " + sim_out);
      phase("similar");
    }
    if (Hs) ocffm_data_free(Hs);
    ocffm_model_destroy(mod);
    ocffm_data_free(V);
  } catch (std::invalid_argument &e) {
    std::cerr << e.what() << std::endl;
    return 1;
  } catch (Fail &e) {
    std::cerr << "error: " << e.what() << std::endl;
    return e.code == OCFFM_E_ARG ? 1 : 2;
  }
  return 0;
}
