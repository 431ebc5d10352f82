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
//   --objective [every]: print the training objective before the first epoch
//   and after every `every`-th (default 1), one `objective` line each;
//   --tol <x>: stop after the epoch whose relative decrease of the objective
//   is at most x (implies --objective); without either flag the solve and
//   its output are the reference's;
//   --binary-out <path>: after the solve, the binary snapshot
//   (ocffm_problem_save_binary) that predict --binary serves from: the text
//   model of -o holds six digits per value;
//   the serving options (serve_cli.hpp, shared with predict.cpp):
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
#include "serve_cli.hpp"

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
         "--objective [every]: print the training objective at init and after every <every>-th iteration (default 1)\n"
         "--tol <x>: stop once an iteration lowers the objective by at most x relative to the previous evaluation\n"
         "--binary-out <path>: after training, write the binary snapshot (ocffm_problem_save_binary) predict reads\n" +
         serve_usage("after training, ");
}

int main(int argc, char **argv) {
  ocffm_param prm;
  ocffm_param_default(&prm);
  std::string te_path, model_path, binary_path;
  ServeOptions so;
  ocffm_solve_opts sopt = {0, 0.0, 0};
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
      else if (a == "--objective") {
        sopt.objective_every = 1;
        if (i + 1 < argc && is_numerical(argv[i + 1])) sopt.objective_every = (uint32_t)std::atoi(argv[++i]);
        if (sopt.objective_every == 0) throw std::invalid_argument("--objective takes a period of at least 1");
      } else if (a == "--tol") sopt.tol = std::atof(value(true, "need to specify the tolerance after --tol"));
      else if (a == "--binary-out") binary_path = value(false, "need to specify path after --binary-out");
      else if (so.take(a, value)) continue;
      else break;
    }
    so.validate();
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
    ocffm_data_info uinfo;
    check(ocffm_data_get_info(U, &uinfo));
    std::vector<std::uint64_t> uds(uinfo.f ? uinfo.f : 1);
    check(ocffm_data_get_ds(U, uds.data()));
    ServeLists lists;
    lists.read(so, uds.data(), (uint32_t)uinfo.f);
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
    if (sopt.objective_every || sopt.tol > 0) check(ocffm_problem_solve_ex(prob, &sopt, nullptr));
    else check(ocffm_problem_solve(prob));
    phase("solve");
    if (!model_path.empty()) check(ocffm_problem_save_model(prob, model_path.c_str()));
    if (!binary_path.empty()) check(ocffm_problem_save_binary(prob, binary_path.c_str()));
    phase("save");
    serve(ProblemServer{prob}, so, lists, uds.data(), (uint32_t)uinfo.f, phase);
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
