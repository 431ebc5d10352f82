// model_file.h — host-only reader of the two saved-model formats: the
// reference's text model (save_model, ffm.cpp:1163-1237) and its binary
// snapshot (save_binary_model, ffm.cpp:1239-1267), as
// ocffm_problem_save_model / ocffm_problem_save_binary write them.  No HIP
// here: the file is read and checked whole into host tables, so a bad file
// never reaches a device and never leaves a half-built object.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ocffm.h"

namespace ocffm {

struct ModelFileError : std::runtime_error {
  int code;  // OCFFM_E_IO (not readable) or OCFFM_E_DATA (malformed)
  ModelFileError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

struct ModelFile {
  uint32_t f = 0, fu = 0, fv = 0, k = 0;
  std::vector<uint64_t> Ds;             // f values: the user fields, then the item fields
  std::vector<uint8_t> used;            // per block b12 = index_vec(f1, f2, f)
  std::vector<std::vector<double>> W, H;  // per used block: D1 x k and D2 x k, row-major

  static uint32_t block_index(uint32_t f1, uint32_t f2, uint32_t f) { return f2 + (f - 1) * f1 - f1 * (f1 - 1) / 2; }
  uint32_t nblocks() const { return f * (f + 1) / 2; }
  bool self_side() const;  // the side blocks are in the file
};

// Throw ModelFileError.  Cross blocks must be present; the side blocks are
// either all present or all absent (a model trained with --ns).
ModelFile read_model_text(const std::string &path);
ModelFile read_model_binary(const std::string &path);

// ocffm_model_file_info without the C ABI's error string: the status, and the
// message in err.
int model_file_info(const char *path, int binary, ocffm_model_info *out, std::string &err);
// f / fu / fv / k / kp, the block counts and (when the caller gave room) Ds and used
void fill_model_info(const ModelFile &mf, ocffm_model_info *out);

}  // namespace ocffm
