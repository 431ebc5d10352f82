// fold_kernels.hpp — folding a new user in from an interaction history
// (ocffm_fold.h ocffm_model_fold_in).
//
// A query row i with the sorted distinct history H_i (items < n) gets a
// correction delta_i in R^d, d = fv k, to the rows of a new value-1 feature of
// user field f* towards the fv item fields: the minimiser of the training
// objective's per-row terms,
//   F_i = sum_{j in H} (1 - z_ij - <delta,q_j>)^2
//         + omega sum_{j<n, j not in H} (r - z_ij - <delta,q_j>)^2 + lambda |delta|^2
// with z_ij = a_i + b_j + <p_i, qfull_j> from the projected tables and q_j the
// first k entries of Q_{f* fv + g}[j], g < fv.  In closed form A delta = rhs,
//   A   = omega G_ff + lambda I + (1 - omega) sum_{j in H} q_j q_j^T
//   rhs = sum_{j in H} [(1 - z_ij) - omega (r - z_ij)] q_j
//         + omega [(r - a_i) s_f - t_f - G_f. p_i]
// G = sum_j qfull_j qfull_j^T (the objective's tiles, obj_kernels.hpp), s =
// sum_j qfull_j, t = sum_j b_j qfull_j (k_obj_vecs with shift 0); _f selects
// field f*'s d entries.
//
// All arithmetic is fp64 on the tables' values.  Every sum has a fixed order:
// the history in ascending item order, a thread's own entries of A only, and
// butterfly sums over 16 lanes.  No atomics, no inter-block communication.
#pragma once

#include "kernels.hpp"
#include "obj_kernels.hpp"

namespace ocffm {

constexpr int FOLD_TILE = 16;  // history items staged per step

// A is held as the lower triangle of 4 x 4 blocks, block (br, bc), bc <= br, at
// br (br + 1) / 2 + bc, 16 doubles row-major (the diagonal blocks whole).
__host__ __device__ __forceinline__ uint32_t fold_pad(uint32_t d) { return (d + 3) & ~3u; }
__host__ __device__ __forceinline__ uint32_t fold_blocks(uint32_t d) {
  const uint32_t nbr = fold_pad(d) >> 2;
  return nbr * (nbr + 1) / 2;
}
// The workgroup's LDS: A, the staged tile (FOLD_TILE x dp), the Cholesky
// diagonal, the solves' vector, the tile's rhs coefficients.
__host__ __device__ __forceinline__ size_t fold_lds_bytes(uint32_t d) {
  const uint32_t dp = fold_pad(d);
  return ((size_t)fold_blocks(d) * 16 + (size_t)FOLD_TILE * dp + 2 * (size_t)dp + FOLD_TILE) * sizeof(double);
}
// element (r, c), c <= r
__device__ __forceinline__ uint32_t fold_aidx(uint32_t r, uint32_t c) {
  const uint32_t br = r >> 2, bc = c >> 2;
  return ((br * (br + 1) / 2 + bc) << 4) + ((r & 3) << 2) + (c & 3);
}
__device__ __forceinline__ void fold_block_rc(uint32_t blk, uint32_t &br, uint32_t &bc) {
  br = (uint32_t)((sqrtf(8.0f * (float)blk + 1.0f) - 1.0f) * 0.5f);
  while (br * (br + 1) / 2 > blk) br--;
  while ((br + 1) * (br + 2) / 2 <= blk) br++;
  bc = blk - br * (br + 1) / 2;
}
// G[(ca, ta), (cb, tb)] from the upper-triangle tiles
template <int KP>
__device__ __forceinline__ double fold_g(const double *__restrict__ G, uint32_t C, uint32_t ca, uint32_t ta,
                                         uint32_t cb, uint32_t tb) {
  return ca <= cb ? G[(size_t)obj_tile_index(ca, cb, C) * (KP * KP) + ta * KP + tb]
                  : G[(size_t)obj_tile_index(cb, ca, C) * (KP * KP) + tb * KP + ta];
}

template <typename real> struct FoldArgs {
  uint32_t C, fv, k, field, d;
  double omega, lambda, r;
  real *const *P;             // the call's projected query tables (rows x KP)
  const real *a;              // a_i of the call's rows
  const real *const *Q;       // the catalogue's C tables (n x KP)
  const real *b;
  const double *G;            // C (C + 1) / 2 tiles of KP x KP
  const double *vec;          // [C KP: s | C KP: t | 2]
  const uint32_t *frow;       // folded row -> row of the call
  const int64_t *hptr;        // per folded row: its history in hcol
  const uint32_t *hcol;       // sorted distinct items < n
  double *delta;              // rows of the call x d
  int *bad;                   // set when a pivot was not positive and finite
};

// One workgroup per folded row: build A and rhs, Cholesky, two solves.
// Ownership is a fixed map of the thread index: block blk of A belongs to
// thread blk % BLOCK, entry e of rhs (and of the solves' vector) to thread e
// (d <= 128 <= BLOCK).
template <typename real, int KP>
__global__ __launch_bounds__(BLOCK) void k_fold_solve(FoldArgs<real> g) {
  extern __shared__ __attribute__((aligned(16))) char fold_smem[];
  const uint32_t tid = threadIdx.x;
  const uint32_t d = g.d, dp = fold_pad(d), nblk = fold_blocks(d), C = g.C, k = g.k;
  double *A = reinterpret_cast<double *>(fold_smem);
  double *tile = A + (size_t)nblk * 16;
  double *dg = tile + (size_t)FOLD_TILE * dp;
  double *xv = dg + dp;
  double *coef = xv + dp;
  const uint64_t row = g.frow[blockIdx.x];
  const uint32_t c0 = g.field * g.fv;
  const double omega = g.omega, ai = (double)g.a[row];

  // 1. A = omega G_ff + lambda I, rhs = omega [(r - a_i) s_f - t_f - G_f. p_i]
  for (uint32_t blk = tid; blk < nblk; blk += BLOCK) {
    uint32_t br, bc;
    fold_block_rc(blk, br, bc);
#pragma unroll
    for (uint32_t x = 0; x < 4; x++)
#pragma unroll
      for (uint32_t y = 0; y < 4; y++) {
        const uint32_t r = br * 4 + x, c = bc * 4 + y;
        double v = 0.0;
        if (r < d && c < d) {
          v = omega * fold_g<KP>(g.G, C, c0 + r / k, r % k, c0 + c / k, c % k);
          if (r == c) v += g.lambda;
        }
        A[blk * 16 + x * 4 + y] = v;
      }
  }
  double rhs = 0.0;
  if (tid < d) {
    const uint32_t ca = c0 + tid / k, ta = tid % k;
    double gp = 0.0;
    for (uint32_t c2 = 0; c2 < C; c2++) {
      const real *pp = g.P[c2] + row * KP;
      for (uint32_t t2 = 0; t2 < (uint32_t)KP; t2++) gp += fold_g<KP>(g.G, C, ca, ta, c2, t2) * (double)pp[t2];
    }
    const uint32_t D = C * KP;
    rhs = omega * (((g.r - ai) * g.vec[ca * KP + ta] - g.vec[D + ca * KP + ta]) - gp);
  }

  // 2. the history in tiles of FOLD_TILE items: 16 lanes gather an item's rows
  const int64_t h0 = g.hptr[blockIdx.x], h1 = g.hptr[blockIdx.x + 1];
  const double w1 = 1.0 - omega;
  const uint32_t s = tid >> 4, l = tid & 15;
  for (int64_t hb = h0; hb < h1; hb += FOLD_TILE) {
    const uint32_t cnt = (uint32_t)(h1 - hb < FOLD_TILE ? h1 - hb : FOLD_TILE);
    __syncthreads();  // A's initial values; the previous tile's readers
    if (s < cnt) {
      const uint64_t j = g.hcol[hb + s];
      double acc = 0.0;
      for (uint32_t c = 0; c < C; c++) {
        const real *pp = g.P[c] + row * KP, *qq = g.Q[c] + j * KP;
        for (uint32_t t = l; t < (uint32_t)KP; t += 16) acc += (double)pp[t] * (double)qq[t];
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 16);
      for (uint32_t e = l; e < dp; e += 16)
        tile[s * dp + e] = e < d ? (double)g.Q[c0 + e / k][j * KP + e % k] : 0.0;
      if (l == 0) {
        const double z = (ai + (double)g.b[j]) + acc;
        coef[s] = (1.0 - z) - omega * (g.r - z);
      }
    }
    __syncthreads();
    for (uint32_t blk = tid; blk < nblk; blk += BLOCK) {
      uint32_t br, bc;
      fold_block_rc(blk, br, bc);
      double av[16];
#pragma unroll
      for (int x = 0; x < 16; x++) av[x] = A[blk * 16 + x];
      for (uint32_t ss = 0; ss < cnt; ss++) {
        const double *q = tile + ss * dp;
        double qr[4], qc[4];
#pragma unroll
        for (int x = 0; x < 4; x++) {
          qr[x] = w1 * q[br * 4 + x];
          qc[x] = q[bc * 4 + x];
        }
#pragma unroll
        for (int x = 0; x < 4; x++)
#pragma unroll
          for (int y = 0; y < 4; y++) av[x * 4 + y] = fma(qr[x], qc[y], av[x * 4 + y]);
      }
#pragma unroll
      for (int x = 0; x < 16; x++) A[blk * 16 + x] = av[x];
    }
    if (tid < d)
      for (uint32_t ss = 0; ss < cnt; ss++) rhs = fma(coef[ss], tile[ss * dp + tid], rhs);
  }
  __syncthreads();

  // 3. in-place Cholesky without pivoting (L below the diagonal, the diagonal
  // in dg); every thread reads the same pivot, so a bad one ends all of them
  bool bad = false;
  for (uint32_t j = 0; j < d; j++) {
    const double pv = A[fold_aidx(j, j)];
    if (!(pv > 0.0) || !(pv < __builtin_huge_val())) {
      bad = true;
      break;
    }
    const double ljj = sqrt(pv);
    if (tid == 0) dg[j] = ljj;
    const uint32_t rr = j + 1 + tid;
    if (rr < d) A[fold_aidx(rr, j)] = A[fold_aidx(rr, j)] / ljj;
    __syncthreads();
    for (uint32_t blk = tid; blk < nblk; blk += BLOCK) {
      uint32_t br, bc;
      fold_block_rc(blk, br, bc);
      if (bc * 4 + 3 <= j) continue;  // (bc <= br: no entry right of column j)
      double lr[4], lc[4];
#pragma unroll
      for (uint32_t x = 0; x < 4; x++) {
        const uint32_t r = br * 4 + x, c = bc * 4 + x;
        lr[x] = (r > j && r < d) ? A[fold_aidx(r, j)] : 0.0;
        lc[x] = (c > j && c < d) ? A[fold_aidx(c, j)] : 0.0;
      }
#pragma unroll
      for (uint32_t x = 0; x < 4; x++)
#pragma unroll
        for (uint32_t y = 0; y < 4; y++) {
          const uint32_t r = br * 4 + x, c = bc * 4 + y;
          if (c <= r && c > j && r < d) A[blk * 16 + x * 4 + y] -= lr[x] * lc[y];
        }
    }
    __syncthreads();
  }
  if (bad) {
    if (tid < d) g.delta[row * d + tid] = __builtin_nan("");
    if (tid == 0) *g.bad = 1;
    return;
  }

  // L y = rhs, then L^T x = y
  double y = rhs;
  for (uint32_t j = 0; j < d; j++) {
    if (tid == j) {
      y = y / dg[j];
      xv[j] = y;
    }
    __syncthreads();
    if (tid > j && tid < d) y -= A[fold_aidx(tid, j)] * xv[j];
  }
  __syncthreads();
  for (uint32_t jj = d; jj > 0; jj--) {
    const uint32_t j = jj - 1;
    if (tid == j) {
      y = y / dg[j];
      xv[j] = y;
    }
    __syncthreads();
    if (tid < j) y -= A[fold_aidx(j, tid)] * xv[j];
  }
  if (tid < d) g.delta[row * d + tid] = y;
}

// P_c[i][t] <- (real)((double)P_c[i][t] + delta_i[g k + t]), c = f* fv + g, of
// the folded rows; a folded row is not cold.
template <typename real>
__global__ __launch_bounds__(BLOCK) void k_fold_apply(uint64_t nf, uint32_t d, uint32_t k, uint32_t kp, uint32_t c0,
                                                      const uint32_t *__restrict__ frow,
                                                      const double *__restrict__ delta, real *const *P,
                                                      uint8_t *cold) {
  const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (x >= nf * d) return;
  const uint64_t row = frow[x / d];
  const uint32_t e = (uint32_t)(x % d);
  real *p = P[c0 + e / k] + row * kp + e % k;
  *p = (real)((double)*p + delta[row * d + e]);
  if (e == 0) cold[row] = 0;
}

}  // namespace ocffm
