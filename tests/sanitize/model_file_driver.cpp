// Driver of the saved-model reader (one-class-ffm_amd/csrc/model_file.cpp)
// for the sanitizer build (tests/test_model_cpu.py): host code only.
//   model_file_driver (t|b) <path> [(t|b) <path> ...]
// One line per file: the status, and for a good file f fu fv k kp nused
// self_side, the Ds and the used flags.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "model_file.h"

int main(int argc, char **argv) {
  if (argc < 3 || argc % 2 != 1) {
    std::fprintf(stderr, "usage: model_file_driver (t|b) <path> ...\n");
    return 2;
  }
  for (int a = 1; a + 1 < argc; a += 2) {
    const int binary = std::strcmp(argv[a], "b") == 0;
    ocffm_model_info info{};
    std::string err;
    int st = ocffm::model_file_info(argv[a + 1], binary, &info, err);
    if (st != OCFFM_OK) {
      std::printf("%d\n", st);
      continue;
    }
    std::vector<uint64_t> ds(info.f);
    std::vector<uint8_t> used(info.nblocks);
    info.Ds = ds.data();
    info.used = used.data();
    info.ds_cap = info.f;
    info.used_cap = info.nblocks;
    st = ocffm::model_file_info(argv[a + 1], binary, &info, err);
    std::printf("%d %u %u %u %u %u %u %d |", st, info.f, info.fu, info.fv, info.k, info.kp, info.nused, info.self_side);
    for (uint64_t d : ds) std::printf(" %llu", (unsigned long long)d);
    std::printf(" |");
    for (uint8_t u : used) std::printf(" %d", (int)u);
    std::printf("\n");
  }
  return 0;
}
