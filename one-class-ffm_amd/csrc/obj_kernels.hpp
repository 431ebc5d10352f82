// obj_kernels.hpp — the training objective in closed form.
//
//   F = 1/2 [ pos + omega (all - on_pos) + reg ]
//   pos    = sum over the label entries (i,j) of (1 - yhat_ij)^2
//   on_pos = sum over the label entries of (r - yhat_ij)^2
//   all    = sum_{i<m} sum_{j<n} (r - yhat_ij)^2
//   reg    = sum over the used blocks' W and H rows d of lambda_d |row_d|^2
//
// This is the reference's func() (ffm.cpp:1321-1351) with its m x n loop
// replaced by the aggregates the solver's gradient already rests on.  Under
// --freq, lambda_d = lambda freq_d of the row's own field: func() ignores
// freq, but the gradient and CG use it (ffm.cpp:561-570), so the value
// returned under --freq is the function the solver actually descends, not
// func()'s.
//
// With D = C kp, p_i = [P_0[i] | ... | P_{C-1}[i]], q_j likewise, alpha_i =
// a_i - r:
//   all = <G_U, G_V>_F + 2 u_alpha^T v_1 + 2 u_1^T v_b
//         + n sum alpha^2 + m sum b^2 + 2 (sum alpha)(sum b)
//   G_U = sum_i p_i p_i^T, u_1 = sum_i p_i, u_alpha = sum_i alpha_i p_i
//   G_V = sum_j q_j q_j^T, v_1 = sum_j q_j, v_b     = sum_j b_j q_j
// G is held as its kp x kp tiles T[l][l'] = P_l^T P_l', l <= l' (G is
// symmetric: the Frobenius product weights the off-diagonal tile pairs by 2).
//
// Every sum across row ranges, blocks and tiles is fp64 in a fixed order; no
// floating-point atomics.  fp32 problems accumulate at most OBJ_FLUSH rows in
// fp32 (MFMA or VALU registers) before adding them to fp64 accumulators.
#pragma once

#include "kernels.hpp"

namespace ocffm {

constexpr int OBJ_FLUSH = 1024;  // rows an fp32 accumulator takes before it is added to its fp64 one

// Upper-triangle index of tile pair (la, lb), la <= lb < C.
__host__ __device__ __forceinline__ uint32_t obj_tile_index(uint32_t la, uint32_t lb, uint32_t C) {
  return la * C - la * (la - 1) / 2 + (lb - la);
}
// The y-th pair (ga, gb), ga <= gb < ng, in row-major order of the upper triangle.
__host__ __device__ __forceinline__ void obj_pair_of(uint32_t y, uint32_t ng, uint32_t &ga, uint32_t &gb) {
  ga = 0;
  while (y >= ng - ga) {
    y -= ng - ga;
    ga++;
  }
  gb = ga + y;
}

template <typename real, int KP> constexpr bool obj_mfma_kp() {
  return (sizeof(real) == 4 && (KP == 32 || KP == 64)) || (sizeof(real) == 8 && KP == 32);
}

// One kp x kp tile T[e][d] = sum_{j in [r0, r1)} A[j][e] B[j][d] by one wave,
// stored as doubles (row-major) at out.  Rows are loaded straight into the
// MFMA operands as k_gram_mfma64 / k_gram_mfma_f64 do (rows past the range
// read zero through the buffer range check).
template <int KP>
__device__ __forceinline__ void obj_tile_mfma(const float *A, const float *B, uint64_t R, uint64_t r0, uint64_t r1,
                                              double *__restrict__ out, int lane) {
  typedef float f16x __attribute__((ext_vector_type(16)));
  constexpr int NT = KP / 32, U = 4;
  constexpr uint32_t ROWB = KP * 4, OOB = 0xffffff00u;
  const int e = lane & 31, hf = lane >> 5;
  const BufView ab = buf_view(A, R * ROWB), bb = buf_view(B, R * ROWB);
  double dacc[NT * NT][16];
#pragma unroll
  for (int t = 0; t < NT * NT; t++)
#pragma unroll
    for (int r = 0; r < 16; r++) dacc[t][r] = 0.0;
  for (uint64_t jc = r0; jc < r1; jc += OBJ_FLUSH) {
    const uint64_t je = jc + OBJ_FLUSH < r1 ? jc + OBJ_FLUSH : r1;
    f16x acc[NT * NT];
#pragma unroll
    for (int t = 0; t < NT * NT; t++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[t][r] = 0.0f;
    float av[2][U][NT], bv[2][U][NT];
    auto load = [&](int sb, uint64_t j0) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t jj = j0 + 2 * u + hf;
        const uint32_t off = jj < je ? (uint32_t)(jj * ROWB + e * 4) : OOB;
#pragma unroll
        for (int h = 0; h < NT; h++) {
          av[sb][u][h] = bld1<float>(ab, off + h * 128);
          bv[sb][u][h] = bld1<float>(bb, off + h * 128);
        }
      }
    };
    auto step = [&](int sb) {
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int mt = 0; mt < NT; mt++)
#pragma unroll
          for (int nt = 0; nt < NT; nt++)
            acc[mt * NT + nt] =
                __builtin_amdgcn_mfma_f32_32x32x2f32(av[sb][u][mt], bv[sb][u][nt], acc[mt * NT + nt], 0, 0, 0);
    };
    for (uint64_t j0 = jc; j0 < je; j0 += 4 * U) {
      load(0, j0);
      load(1, j0 + 2 * U);
      step(0);
      step(1);
    }
#pragma unroll
    for (int t = 0; t < NT * NT; t++)
#pragma unroll
      for (int r = 0; r < 16; r++) dacc[t][r] += (double)acc[t][r];
  }
#pragma unroll
  for (int t = 0; t < NT * NT; t++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int m = (t / NT) * 32 + 8 * (r >> 2) + 4 * hf + (r & 3), n = (t % NT) * 32 + e;
      out[m * KP + n] = dacc[t][r];
    }
}

// fp64, KP = 32, on v_mfma_f64_16x16x4_f64 (the 2 x 2 tiles of 16 x 16; four rows are the K dimension).
__device__ __forceinline__ void obj_tile_mfma_f64(const double *A, const double *B, uint64_t R, uint64_t r0,
                                                  uint64_t r1, double *__restrict__ out, int lane) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  constexpr int U = 4;
  constexpr uint32_t OOB = 0xffffff00u;
  const int c16 = lane & 15, rq = lane >> 4;
  const BufView ab = buf_view(A, R * 256), bb = buf_view(B, R * 256);
  d4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  double av[2][U][2], bv[2][U][2];
  auto load = [&](int sb, uint64_t j0) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint64_t jj = j0 + 4 * u + rq;
      const uint32_t off = jj < r1 ? (uint32_t)(jj * 256 + c16 * 8) : OOB;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        av[sb][u][h] = bld1<double>(ab, off + h * 128);
        bv[sb][u][h] = bld1<double>(bb, off + h * 128);
      }
    }
  };
  auto step = [&](int sb) {
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++)
          acc[mt * 2 + nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[sb][u][mt], bv[sb][u][nt], acc[mt * 2 + nt], 0, 0, 0);
  };
  for (uint64_t j0 = r0; j0 < r1; j0 += 8 * U) {
    load(0, j0);
    load(1, j0 + 4 * U);
    step(0);
    step(1);
  }
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m = (t >> 1) * 16 + rq + 4 * r, n = (t & 1) * 16 + c16;
      out[m * 32 + n] = acc[t][r];
    }
}

// The VALU tile (every kp): the tile is cut into ST x ST sub-tiles (ST =
// min(kp, 64)); a lane of the LE x LE lane grid owns a PE x PE patch of the
// sub-tile and reads its PE elements of the A row and of the B row per row
// (the wave reads the same two rows: L1 hits).
template <typename real, int KP>
__device__ __forceinline__ void obj_tile_valu(const real *__restrict__ A, const real *__restrict__ B, uint64_t r0,
                                              uint64_t r1, double *__restrict__ out, int lane) {
  constexpr int ST = KP < 64 ? KP : 64, LE = ST < 8 ? ST : 8, PE = ST / LE;
  const bool active = lane < LE * LE;
  const int le = lane / LE, ld = lane % LE;
  if (!active) return;  // (no barrier and no cross-lane operation below)
  for (int se = 0; se < KP / ST; se++)
    for (int sd = 0; sd < KP / ST; sd++) {
      const real *pa = A + se * ST + le * PE, *pb = B + sd * ST + ld * PE;
      double dacc[PE * PE];
#pragma unroll
      for (int x = 0; x < PE * PE; x++) dacc[x] = 0.0;
      for (uint64_t jc = r0; jc < r1; jc += OBJ_FLUSH) {
        const uint64_t je = jc + OBJ_FLUSH < r1 ? jc + OBJ_FLUSH : r1;
        real acc[PE * PE];
#pragma unroll
        for (int x = 0; x < PE * PE; x++) acc[x] = 0;
        for (uint64_t j = jc; j < je; j++) {
          real av[PE], bv[PE];
#pragma unroll
          for (int x = 0; x < PE; x++) {
            av[x] = pa[j * KP + x];
            bv[x] = pb[j * KP + x];
          }
#pragma unroll
          for (int x = 0; x < PE; x++)
#pragma unroll
            for (int y = 0; y < PE; y++) acc[x * PE + y] += av[x] * bv[y];
        }
#pragma unroll
        for (int x = 0; x < PE * PE; x++) dacc[x] += (double)acc[x];
      }
#pragma unroll
      for (int x = 0; x < PE; x++)
#pragma unroll
        for (int y = 0; y < PE; y++)
          out[(se * ST + le * PE + x) * KP + sd * ST + ld * PE + y] = dacc[x * PE + y];
    }
}

// Pair-Gram pass of one side: block (x, y) takes row range x and group pair
// y = (ga, gb), ga <= gb, of the C tables cut into groups of G; its waves own
// the tile pairs (la in ga, lb in gb, la <= lb) and each walks the block's
// rows once per tile pair it owns.  part[x][tile][kp][kp] (doubles), tile =
// obj_tile_index(la, lb, C): every tile of every row range is written by
// exactly one wave (k_reduce_parts then sums the ranges in range order).
template <typename real, int KP, bool MFMA>
__global__ __launch_bounds__(BLOCK) void k_obj_gram(uint64_t R, uint32_t C, const real *const *__restrict__ tabs,
                                                    double *__restrict__ part, uint64_t rows_per_block, uint32_t G,
                                                    uint32_t ng) {
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint32_t ga, gb;
  obj_pair_of(blockIdx.y, ng, ga, gb);
  const uint32_t a0 = ga * G, a1 = min(C, a0 + G), b0 = gb * G, b1 = min(C, b0 + G);
  const uint32_t nb = b1 - b0, ntp = C * (C + 1) / 2;
  const uint64_t r0 = min(R, (uint64_t)blockIdx.x * rows_per_block);
  const uint64_t r1 = min(R, r0 + rows_per_block);
  for (uint32_t q = w; q < (a1 - a0) * nb; q += nw) {
    const uint32_t la = a0 + q / nb, lb = b0 + q % nb;
    if (la > lb) continue;  // (ga == gb: the lower triangle)
    double *out = part + ((size_t)blockIdx.x * ntp + obj_tile_index(la, lb, C)) * (KP * KP);
    const real *A = tabs[la], *B = tabs[lb];
    if constexpr (MFMA && sizeof(real) == 4 && (KP == 32 || KP == 64)) obj_tile_mfma<KP>(A, B, R, r0, r1, out, lane);
    else if constexpr (MFMA && sizeof(real) == 8 && KP == 32) obj_tile_mfma_f64(A, B, R, r0, r1, out, lane);
    else obj_tile_valu<real, KP>(A, B, r0, r1, out, lane);
  }
}

// The O(D) aggregates of one side over a block's rows, w_i = bias_i + shift:
// part[block] = [C kp: sum_i T_c[i][d] | C kp: sum_i w_i T_c[i][d] | sum w | sum w^2]
// (k_colsum_multi's row walk; row groups combined in fixed order through LDS).
template <typename real, int KP>
__global__ __launch_bounds__(BLOCK) void k_obj_vecs(uint64_t R, int C, const real *const *__restrict__ tabs,
                                                    const real *__restrict__ bias, double shift,
                                                    double *__restrict__ part, uint64_t rows_per_block) {
  using G = Geo<real, KP>;
  constexpr int RG = BLOCK / G::LPR;
  __shared__ double sh[2][RG][KP + 1];
  const int li = threadIdx.x % G::LPR, rg = threadIdx.x / G::LPR;
  const uint64_t r0 = min(R, (uint64_t)blockIdx.x * rows_per_block);
  const uint64_t r1 = min(R, r0 + rows_per_block);
  const uint64_t nout = 2 * (uint64_t)C * KP + 2;
  double *out = part + (uint64_t)blockIdx.x * nout;
  for (int c = 0; c < C; c++) {
    const real *T = tabs[c];
    double a[G::VE], aw[G::VE];
#pragma unroll
    for (int e = 0; e < G::VE; e++) a[e] = aw[e] = 0;
    for (uint64_t j = r0 + rg; j < r1; j += RG) {
      const vec_t<real> x = vld<real>(T + j * KP + li * G::VE);
      const double wj = (double)bias[j] + shift;
#pragma unroll
      for (int e = 0; e < G::VE; e++) {
        a[e] += (double)x[e];
        aw[e] += wj * (double)x[e];
      }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < G::VE; e++) {
      sh[0][rg][li * G::VE + e] = a[e];
      sh[1][rg][li * G::VE + e] = aw[e];
    }
    __syncthreads();
    if (threadIdx.x < 2 * KP) {
      const int h = threadIdx.x / KP, d = threadIdx.x % KP;
      double t = 0;
      for (int g = 0; g < RG; g++) t += sh[h][g][d];
      out[(uint64_t)h * C * KP + (uint64_t)c * KP + d] = t;
    }
  }
  double sw = 0, sww = 0;
  for (uint64_t j = r0 + threadIdx.x; j < r1; j += BLOCK) {
    const double wj = (double)bias[j] + shift;
    sw += wj;
    sww += wj * wj;
  }
  sw = block_sum(sw);
  sww = block_sum(sww);
  if (threadIdx.x == 0) {
    out[nout - 2] = sw;
    out[nout - 1] = sww;
  }
}

// The Frobenius reduction and the O(D) dot products, on the device in fp64:
//   out[0] = sum over tile pairs of wt <GU_tile, GV_tile>, wt = 1 (la == lb) or 2
//   out[1] = u_w^T v_1,  out[2] = u_1^T v_w
//   out[3..4] = the user side's sum w, sum w^2;  out[7..8] = the item side's
// vu, vv: the reduced k_obj_vecs outputs of the two sides (2 D + 2 doubles).
// Block b takes tile pairs b, b + grid, ...; block partials are combined in
// block order by the last block.
static __global__ __launch_bounds__(BLOCK) void k_obj_frob(uint32_t C, uint32_t kp, const double *__restrict__ GU,
                                                          const double *__restrict__ GV,
                                                          const double *__restrict__ vu,
                                                          const double *__restrict__ vv, double *part,
                                                          unsigned *tick, double *__restrict__ out) {
  const uint32_t ntp = C * (C + 1) / 2, ne = kp * kp;
  const uint64_t D = (uint64_t)C * kp;
  double s = 0, s1 = 0, s2 = 0;
  for (uint32_t tp = blockIdx.x; tp < ntp; tp += gridDim.x) {
    uint32_t la, lb;
    obj_pair_of(tp, C, la, lb);
    const double *a = GU + (size_t)tp * ne, *b = GV + (size_t)tp * ne;
    double t = 0;
    for (uint32_t x = threadIdx.x; x < ne; x += BLOCK) t += a[x] * b[x];
    s += la == lb ? t : 2.0 * t;
  }
  if (blockIdx.x == 0)
    for (uint64_t d = threadIdx.x; d < D; d += BLOCK) {
      s1 += vu[D + d] * vv[d];
      s2 += vu[d] * vv[D + d];
    }
  const double bv[3] = {block_sum(s), block_sum(s1), block_sum(s2)};
  double tot[3];
  if (last_block<3>(bv, part, tick, tot) && threadIdx.x == 0) {
    out[0] = tot[0];
    out[1] = tot[1];
    out[2] = tot[2];
    out[3] = vu[2 * D];
    out[4] = vu[2 * D + 1];
    out[7] = vv[2 * D];
    out[8] = vv[2 * D + 1];
  }
}

// Positives pass over the user-major positives: y~ = yt[p] + a_i + b_j (the
// factored residual, yhat - 1), out[0] = sum y~^2, out[1] = sum (y~ + shift)^2
// with shift = 1 - r.  A thread takes positions p, p + stride, ... and finds
// the row of each by bisection of yptr.
template <typename real>
__global__ __launch_bounds__(BLOCK) void k_obj_pos(uint64_t npos, uint64_t R, const int64_t *__restrict__ yptr,
                                                   const uint32_t *__restrict__ ycol, const real *__restrict__ yt,
                                                   const real *__restrict__ a, const real *__restrict__ b,
                                                   double shift, double *part, unsigned *tick,
                                                   double *__restrict__ out) {
  double s0 = 0, s1 = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; p < npos; p += (uint64_t)gridDim.x * BLOCK) {
    uint64_t lo = 0, hi = R;  // the row i with yptr[i] <= p < yptr[i + 1]
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if ((uint64_t)yptr[mid] <= p) lo = mid;
      else hi = mid;
    }
    const double y = (double)yt[p] + (double)a[lo] + (double)b[ycol[p]];
    s0 += y * y;
    s1 += (y + shift) * (y + shift);
  }
  const double bv[2] = {block_sum(s0), block_sum(s1)};
  double tot[2];
  if (last_block<2>(bv, part, tick, tot) && threadIdx.x == 0) {
    out[0] = tot[0];
    out[1] = tot[1];
  }
}

// Regulariser pass: out[0] = sum over the tables t and their elements of
// fw_t[row] x^2 (fw null: 1); lambda is applied by the host.
template <typename real> struct ObjTab {
  const real *T;
  const real *fw;
  uint64_t nelem;
};
template <typename real>
__global__ __launch_bounds__(BLOCK) void k_obj_reg(uint32_t ntab, const ObjTab<real> *__restrict__ tabs, uint32_t lgkp,
                                                   double *part, unsigned *tick, double *__restrict__ out) {
  double s = 0;
  for (uint32_t t = 0; t < ntab; t++) {
    const ObjTab<real> tb = tabs[t];
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < tb.nelem; e += (uint64_t)gridDim.x * BLOCK) {
      const double x = (double)tb.T[e];
      s += tb.fw ? (double)tb.fw[e >> lgkp] * (x * x) : x * x;
    }
  }
  const double bv[1] = {block_sum(s)};
  double tot[1];
  if (last_block<1>(bv, part, tick, tot) && threadIdx.x == 0) out[0] = tot[0];
}

}  // namespace ocffm
