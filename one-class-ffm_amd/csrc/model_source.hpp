// model_source.hpp — what a stand-alone model (model.hip) copies out of a
// problem (solver.hip): device pointers to the problem's current tables.  They
// are valid until the problem's next call; the copy is made right away.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/ocffm.h"

namespace ocffm {

struct ModelSource {
  int precision = 0, device = 0;
  uint32_t f = 0, fu = 0, fv = 0, k = 0, kp = 0;
  std::vector<uint64_t> Ds;     // f values, user fields first
  std::vector<uint8_t> used;    // per block b12
  std::vector<const void *> W, H;  // per block: D x kp of the problem's real (null: unused)
  std::vector<const void *> Q;  // per cross block c (f1 fv + f2 - fu): n x kp
  const void *b = nullptr;      // n
  uint64_t n = 0;
  const double *popular = nullptr;
  uint64_t npop = 0;
};

// Throws Error: OCFFM_E_STATE before init / load_binary, OCFFM_E_ARG for a
// sharded problem.  The owned tables are made whole and the stream is idle.
void problem_model_source(ocffm_problem *p, ModelSource &out);

}  // namespace ocffm
