// sim_kernels.hpp — item-item similarity on a model's catalogue (DESIGN §14,
// ocffm_similar.h): the inverse norms of table rows and the gather of the
// query items' rows.  The scores themselves are the serving sweep's
// (rank_kernels.hpp: k_rec_topn and k_eval_label_scores in REC_SIM mode), so
// this file has no product of its own.  Included by model.hip.
#pragma once

#include "rank_kernels.hpp"

namespace ocffm {

// ------------------------------------------------------ inverse norms ---
// inv[r] = 1 / sqrt(<e_r, e_r>) of the R rows of C tables (R x KP each), e_r
// the concatenation of T_c[r] over c: the catalogue's items, or the projected
// query rows of similar_to, by the same text.
//
// One 16-lane subgroup per row.  Lane l takes the 4 consecutive depth elements
// from 64 t + 4 l for t = 0, 1, ... (one 16-byte load in fp32, 32 bytes in
// fp64; KP is a multiple of 4, so the four lie in one table: the subgroup's
// loads of one t are contiguous within a table row) and runs one fused chain
// over them in depth order, s = fma(x, x, s) in fp64 from s = 0, x the widened
// table value.  The 16 lane sums are then added by sg_sum's butterfly: lane
// pairs at distance 1, then 2, then the other quad, then the other half-row;
// every step adds a commuted pair, so all lanes end with the same bits.  The
// association is a function of the depth alone: it depends neither on the
// row's place nor on the grid (subgroups stride over the rows), and there is
// no atomic.  inv = 1 / sqrt(s), both correctly rounded in fp64, rounded once
// to real; 0 where s is not positive (a row of zeros).
// Algorithmic bytes: R C KP reals read once, R reals written.
template <typename real, int KP>
__global__ __launch_bounds__(BLOCK) void k_sim_inv_norm(uint64_t R, int C, const real *const *__restrict__ T,
                                                        real *__restrict__ inv) {
  using M = RecMma<real>;
  const int li = threadIdx.x & 15;
  const int depth = C * KP;
  const uint64_t nsg = (uint64_t)gridDim.x * (BLOCK / 16);
  for (uint64_t row = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) / 16; row < R; row += nsg) {
    double s = 0.0;
    for (int d = 4 * li; d < depth; d += 64) {
      const typename M::V v = M::ld(T[d / KP] + row * KP + d % KP);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const double x = (double)v[e];
        s = __builtin_fma(x, x, s);
      }
    }
    s = sg_sum<16>(s);
    if (li == 0) inv[row] = s > 0.0 ? (real)(1.0 / __builtin_sqrt(s)) : (real)0;
  }
}

// ------------------------------------------------------- query gather ---
// The sweep reads its query rows as a contiguous range of the P tables, so the
// rows qitem[0..R) of the C catalogue tables Q (and of inv, unless it is null:
// the inner product reads no norms) are copied into the chunk's R x KP query
// tables out (and qinv).  One 16-byte load and store per thread and step;
// threads stride over the R C KP sizeof(real) / 16 vectors of the chunk, a
// table row's vectors in consecutive lanes.
// Algorithmic bytes: R C KP reals read and written, R indices, R inverse norms.
template <typename real, int KP>
__global__ __launch_bounds__(BLOCK) void k_sim_gather(uint64_t R, int C, const uint32_t *__restrict__ qitem,
                                                      const real *const *__restrict__ Q, real *const *__restrict__ out,
                                                      const real *__restrict__ inv, real *__restrict__ qinv) {
  typedef uint32_t u4v __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(1))) u4v gsrc;
  typedef __attribute__((address_space(1))) u4v gdst;
  constexpr uint64_t VPR = (uint64_t)KP * sizeof(real) / 16;  // vectors per table row
  constexpr int EPV = 16 / sizeof(real);                      // elements per vector
  const uint64_t total = R * (uint64_t)C * VPR, nth = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; t < total; t += nth) {
    const uint64_t r = t / ((uint64_t)C * VPR), rem = t % ((uint64_t)C * VPR);
    const uint64_t c = rem / VPR, v = rem % VPR;
    const uint64_t j = qitem[r];
    *(gdst *)(out[c] + r * KP + v * EPV) = *(gsrc *)(Q[c] + j * KP + v * EPV);
    if (inv && rem == 0) qinv[r] = inv[j];
  }
}

}  // namespace ocffm
