// pg_tree.h — what the genome tree (pg_tree.hip) and its bootstrap
// (pg_boot.hip) share: the fixed point, the total order (Q, i, j) the minimum
// is taken under, and pg_tree.hip's per-join kernels, which the bootstrap
// launches over a replicate's matrix where no single workgroup can hold it.
#pragma once
#include "pg_prim.h"

namespace pg {

#define NJ_MAX_N 16384u
#define NJ_S 16                    // fractional bits
#define NJ_WAVES (RG_BLOCK / 64)
#define NJ_NONE_Q 0x7fffffffffffffffll
#define NJ_NONE_IJ (~0ull)

typedef long long ll;

struct NjKey {
  ll q;
  ull ij;                          // i << 32 | j
};

// (Q, i, j) < (Q2, i2, j2): the smallest Q, then the smallest i, then the smallest j
__device__ __forceinline__ bool nj_less(ll q, ull ij, ll q2, ull ij2) { return q < q2 || (q == q2 && ij < ij2); }
// the wave's minimum in every lane
__device__ __forceinline__ void nj_wave_min(ll& q, ull& ij) {
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const ll q2 = __shfl_xor(q, d);
    const ull ij2 = __shfl_xor(ij, d);
    if (nj_less(q2, ij2, q, ij)) {
      q = q2;
      ij = ij2;
    }
  }
}

// pg_tree.hip: the steps of one tree over M [n][n] (working D in the upper
// triangle), r, live and node; see there
__global__ void __launch_bounds__(RG_BLOCK) k_nj_init(ll* __restrict__ M, uint32_t n, ll* __restrict__ r,
                                                       uint8_t* __restrict__ live, uint32_t* __restrict__ node);
__global__ void __launch_bounds__(RG_BLOCK) k_nj_argmin(const ll* __restrict__ M, const ll* __restrict__ r,
                                                         const uint8_t* __restrict__ live, uint32_t n, ll m2,
                                                         NjKey* __restrict__ part);
__global__ void __launch_bounds__(RG_BLOCK) k_nj_pick(const NjKey* __restrict__ part, uint32_t n_part,
                                                       const ll* __restrict__ M, ll* __restrict__ r,
                                                       uint8_t* __restrict__ live, uint32_t* __restrict__ node,
                                                       uint32_t n, uint32_t m, uint32_t t, uint32_t* __restrict__ left,
                                                       uint32_t* __restrict__ right, ull* __restrict__ len_l,
                                                       ull* __restrict__ len_r, ull* __restrict__ sel);
__global__ void __launch_bounds__(RG_BLOCK) k_nj_update(ll* __restrict__ M, ll* __restrict__ r,
                                                         const uint8_t* __restrict__ live, uint32_t n,
                                                         const ull* __restrict__ sel);

}  // namespace pg
