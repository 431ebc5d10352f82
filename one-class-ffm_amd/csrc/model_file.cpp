// model_file.cpp — host-only reader of saved models (model_file.h).
#include "model_file.h"

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>

namespace ocffm {

namespace {

constexpr uint32_t MAX_FIELDS = 1024;  // (a header read from garbage must not size the block lists)

[[noreturn]] void bad(const std::string &path, const std::string &what) {
  throw ModelFileError(OCFFM_E_DATA, "model file " + path + ": " + what);
}

void check_header(ModelFile &mf, const std::string &path) {
  if (mf.f == 0 || mf.f > MAX_FIELDS) bad(path, "field count out of range");
  if (mf.fu == 0 || mf.fv == 0 || (uint64_t)mf.fu + mf.fv != mf.f) bad(path, "fu + fv must equal f, both >= 1");
  if (mf.k == 0 || mf.k > 128) bad(path, "k must be in 1..128");
}

void check_sizes(const ModelFile &mf, const std::string &path) {
  for (uint64_t d : mf.Ds)
    if (d >= (1ull << 32) - 1 || d * mf.k > (1ull << 40)) bad(path, "field size out of range");
}

void size_blocks(ModelFile &mf) {
  mf.used.assign(mf.nblocks(), 0);
  mf.W.resize(mf.nblocks());
  mf.H.resize(mf.nblocks());
}

// Cross blocks present (the readers have checked that); side blocks all or none
void check_blocks(const ModelFile &mf, const std::string &path) {
  uint32_t side = 0, side_used = 0;
  for (uint32_t f1 = 0; f1 < mf.f; f1++)
    for (uint32_t f2 = f1; f2 < mf.f; f2++) {
      if ((f1 < mf.fu) != (f2 < mf.fu)) continue;
      side++;
      side_used += mf.used[ModelFile::block_index(f1, f2, mf.f)];
    }
  if (side_used != 0 && side_used != side) bad(path, "some side blocks are missing");
}

// An unsigned decimal that fills the whole of [s, e)
bool parse_u64(const char *s, const char *e, uint64_t &out) {
  if (s == e || e - s > 19) return false;
  uint64_t v = 0;
  for (const char *p = s; p < e; p++) {
    if (*p < '0' || *p > '9') return false;
    v = v * 10 + (uint64_t)(*p - '0');
  }
  out = v;
  return true;
}

struct TableLine {
  char t = 0;  // 'W' or 'H'
  uint64_t f1 = 0, f2 = 0, row = 0;
  const char *vals = nullptr;  // after the first blank
};

// "W,f1,f2,row v1 ... vk"
bool parse_prefix(const std::string &line, TableLine &o) {
  const char *s = line.c_str(), *e = s + line.size();
  if (e - s < 2 || (s[0] != 'W' && s[0] != 'H') || s[1] != ',') return false;
  o.t = s[0];
  const char *p = s + 2;
  uint64_t *dst[3] = {&o.f1, &o.f2, &o.row};
  for (int q = 0; q < 3; q++) {
    const char stop = q < 2 ? ',' : ' ';
    const char *z = p;
    while (z < e && *z != stop) z++;
    if (z == e && q < 2) return false;
    if (!parse_u64(p, z, *dst[q])) return false;
    p = z < e ? z + 1 : z;
  }
  o.vals = p;
  return true;
}

// Exactly k numbers separated by blanks, to the end of the line
bool parse_values(const char *p, uint32_t k, double *out) {
  for (uint32_t c = 0; c < k; c++) {
    while (*p == ' ' || *p == '\t') p++;
    if (*p == '\0') return false;
    char *end = nullptr;
    errno = 0;
    const double v = std::strtod(p, &end);
    if (end == p || (*end != '\0' && *end != ' ' && *end != '\t')) return false;
    out[c] = v;
    p = end;
  }
  while (*p == ' ' || *p == '\t') p++;
  return *p == '\0';
}

}  // namespace

bool ModelFile::self_side() const {
  for (uint32_t f1 = 0; f1 < f; f1++)
    for (uint32_t f2 = f1; f2 < f; f2++)
      if ((f1 < fu) == (f2 < fu)) return used[block_index(f1, f2, f)] != 0;
  return false;
}

ModelFile read_model_text(const std::string &path) {
  std::ifstream in(path, std::ios::binary);
  if (!in) throw ModelFileError(OCFFM_E_IO, "cannot read " + path);
  ModelFile mf;
  std::string line;
  bool have = false;  // `line` holds a line not yet consumed
  auto next = [&]() -> bool {
    if (have) return true;
    if (!std::getline(in, line)) return false;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    have = true;
    return true;
  };
  auto header = [&](const char *name) -> uint64_t {
    uint64_t v = 0;
    if (!next() || !parse_u64(line.c_str(), line.c_str() + line.size(), v))
      bad(path, std::string("header line '") + name + "' is missing or not a number");
    have = false;
    return v;
  };
  const uint64_t hf = header("f"), hfu = header("fu"), hfv = header("fv"), hk = header("k");
  if (hf > MAX_FIELDS || hfu > MAX_FIELDS || hfv > MAX_FIELDS || hk > 128) bad(path, "header value out of range");
  mf.f = (uint32_t)hf;
  mf.fu = (uint32_t)hfu;
  mf.fv = (uint32_t)hfv;
  mf.k = (uint32_t)hk;
  check_header(mf, path);
  for (uint32_t i = 0; i < mf.f; i++) mf.Ds.push_back(header("Ds"));
  check_sizes(mf, path);
  size_blocks(mf);
  TableLine tl;
  for (uint32_t f1 = 0; f1 < mf.f; f1++)
    for (uint32_t f2 = f1; f2 < mf.f; f2++) {
      const uint32_t b12 = ModelFile::block_index(f1, f2, mf.f);
      const bool cross = f1 < mf.fu && f2 >= mf.fu;
      bool here = false;
      if (next()) {
        if (!parse_prefix(line, tl)) bad(path, "not a table line: '" + line.substr(0, 40) + "'");
        here = tl.f1 == f1 && tl.f2 == f2;
      }
      if (!here) {
        if (cross) bad(path, "cross block " + std::to_string(f1) + "," + std::to_string(f2) + " is missing");
        continue;  // a side block that is wholly absent: unused
      }
      for (int t = 0; t < 2; t++) {
        const char want = t == 0 ? 'W' : 'H';
        const uint64_t D = mf.Ds[t == 0 ? f1 : f2];
        std::vector<double> &dst = t == 0 ? mf.W[b12] : mf.H[b12];
        dst.assign(D * mf.k, 0.0);
        for (uint64_t r = 0; r < D; r++) {
          if (!next()) bad(path, "ends inside a table");
          if (!parse_prefix(line, tl)) bad(path, "not a table line: '" + line.substr(0, 40) + "'");
          if (tl.t != want || tl.f1 != f1 || tl.f2 != f2 || tl.row != r)
            bad(path, std::string("expected row ") + want + "," + std::to_string(f1) + "," + std::to_string(f2) + "," +
                          std::to_string(r) + ", found '" + line.substr(0, 40) + "'");
          if (!parse_values(tl.vals, mf.k, dst.data() + r * mf.k))
            bad(path, "row '" + line.substr(0, 40) + "' does not hold k numbers");
          have = false;
        }
      }
      mf.used[b12] = 1;
    }
  if (next()) bad(path, "trailing text after the last table: '" + line.substr(0, 40) + "'");
  check_blocks(mf, path);
  return mf;
}

ModelFile read_model_binary(const std::string &path) {
  std::FILE *fp = std::fopen(path.c_str(), "rb");
  if (!fp) throw ModelFileError(OCFFM_E_IO, "cannot read " + path);
  std::unique_ptr<std::FILE, int (*)(std::FILE *)> guard(fp, &std::fclose);
  if (std::fseek(fp, 0, SEEK_END) != 0) throw ModelFileError(OCFFM_E_IO, "cannot seek in " + path);
  const long fsize = std::ftell(fp);
  if (fsize < 0) throw ModelFileError(OCFFM_E_IO, "cannot size " + path);
  std::rewind(fp);
  uint64_t left = (uint64_t)fsize;
  auto get = [&](void *v, uint64_t n) {
    if (n > left || std::fread(v, 1, n, fp) != n) bad(path, "truncated binary model");
    left -= n;
  };
  ModelFile mf;
  uint32_t hd[4];
  get(hd, sizeof(hd));
  mf.f = hd[0];
  mf.fu = hd[1];
  mf.fv = hd[2];
  mf.k = hd[3];
  check_header(mf, path);
  mf.Ds.resize(mf.f);
  get(mf.Ds.data(), (uint64_t)mf.f * sizeof(uint64_t));
  check_sizes(mf, path);
  size_blocks(mf);
  bool have = false;  // idx / nw / nh hold a block header not yet matched
  uint32_t idx = 0;
  uint64_t nw = 0, nh = 0;
  for (uint32_t f1 = 0; f1 < mf.f; f1++)
    for (uint32_t f2 = f1; f2 < mf.f; f2++) {
      const uint32_t b12 = ModelFile::block_index(f1, f2, mf.f);
      const bool cross = f1 < mf.fu && f2 >= mf.fu;
      if (!have && left > 0) {
        get(&idx, sizeof(idx));
        get(&nw, sizeof(nw));
        get(&nh, sizeof(nh));
        have = true;
      }
      if (!have || idx != b12) {
        if (cross) bad(path, have ? "block index out of order" : "truncated binary model: a cross block is missing");
        continue;  // a side block that is wholly absent: unused
      }
      if (nw != mf.Ds[f1] * mf.k || nh != mf.Ds[f2] * mf.k) bad(path, "block table size differs from Ds x k");
      if ((nw + nh) > left / sizeof(double)) bad(path, "truncated binary model");
      mf.W[b12].resize(nw);
      mf.H[b12].resize(nh);
      get(mf.W[b12].data(), nw * sizeof(double));
      get(mf.H[b12].data(), nh * sizeof(double));
      mf.used[b12] = 1;
      have = false;
    }
  if (have) bad(path, "block index out of order");
  if (left != 0) bad(path, "trailing bytes after the last block");
  check_blocks(mf, path);
  return mf;
}

void fill_model_info(const ModelFile &mf, ocffm_model_info *out) {
  out->f = mf.f;
  out->fu = mf.fu;
  out->fv = mf.fv;
  out->k = mf.k;
  out->kp = 4;
  while (out->kp < mf.k) out->kp <<= 1;
  out->nblocks = mf.nblocks();
  out->nused = 0;
  for (uint8_t u : mf.used) out->nused += u;
  out->self_side = mf.self_side() ? 1 : 0;
  if (out->Ds)
    for (uint32_t i = 0; i < mf.f && i < out->ds_cap; i++) out->Ds[i] = mf.Ds[i];
  if (out->used)
    for (uint32_t b = 0; b < mf.nblocks() && b < out->used_cap; b++) out->used[b] = mf.used[b];
}

int model_file_info(const char *path, int binary, ocffm_model_info *out, std::string &err) {
  try {
    if (!path || !out) throw ModelFileError(OCFFM_E_ARG, "null path or output");
    const ModelFile mf = binary ? read_model_binary(path) : read_model_text(path);
    fill_model_info(mf, out);
    out->precision = 0;
    out->device = -1;
    out->has_items = 0;
    out->n = out->npop = 0;
    return OCFFM_OK;
  } catch (ModelFileError &e) {
    err = e.what();
    return e.code;
  } catch (std::bad_alloc &) {
    err = "host out of memory";
    return OCFFM_E_DATA;
  }
}

}  // namespace ocffm
