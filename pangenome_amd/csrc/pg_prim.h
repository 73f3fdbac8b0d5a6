// pg_prim.h — what every pass after the build shares: the grid-stride loop,
// the launch on the context's stream and the no-return agent-scope atomics;
// rocPRIM calls on the context's stream and scratch.  (The texts are pg_text.h's;
// what only the passes over the region rows share is in pg_region.h.)
#pragma once
#include <rocprim/rocprim.hpp>

#include "pg_internal.h"

namespace pg {

typedef unsigned long long ull;

#define RG_BLOCK 256

#define RG_LOOP(i, n) \
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * blockDim.x)

#define RG_ADD(p, v) (void)__hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define RG_OR(p, v) (void)__hip_atomic_fetch_or((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define RG_MAX(p, v) (void)__hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define RG_MIN(p, v) (void)__hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// grid: a block count or a dim3; `c` is the caller's context
#define RG_LAUNCH(kern, grid, ...)                                                       \
  do {                                                                                   \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(RG_BLOCK), 0, c.stream, __VA_ARGS__);      \
    PG_HIP(hipGetLastError());                                                           \
  } while (0)

template <class F>
static void with_temp(Ctx& c, F&& f) {
  size_t bytes = 0;
  PG_HIP(f((void*)nullptr, bytes));
  c.scratch.reserve(bytes + 16);
  bytes = c.scratch.cap;
  PG_HIP(f(c.scratch.p, bytes));
}

template <class K, class V>
static void sort_pairs(Ctx& c, const K* kin, K* kout, const V* vin, V* vout, uint64_t n, int end_bit) {
  with_temp(c, [&](void* tmp, size_t& bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, (size_t)n, 0, end_bit, c.stream);
  });
}
// out: the items of in[0 .. n) (a pointer or any iterator) whose flag byte is set, in order; returns their number
template <class In, class T>
static uint64_t select_flagged(Ctx& c, In in, const uint8_t* flags, T* out, uint64_t n, DevBuf& cnt) {
  cnt.reserve(16);
  with_temp(c, [&](void* tmp, size_t& bytes) {
    return rocprim::select(tmp, bytes, in, flags, out, cnt.as<unsigned long long>(), (size_t)n, c.stream);
  });
  unsigned long long h = 0;
  PG_HIP(hipMemcpyAsync(&h, cnt.p, 8, hipMemcpyDeviceToHost, c.stream));
  c.sync();
  return h;
}
[[maybe_unused]] static uint64_t excl_scan_total(Ctx& c, const unsigned long long* len, unsigned long long* off,
                                                 uint64_t n) {
  // off[0..n]: exclusive prefix sums, off[n] = total (off may be len: the scan works in place)
  PG_HIP(hipMemsetAsync(const_cast<unsigned long long*>(len) + n, 0, 8, c.stream));
  with_temp(c, [&](void* tmp, size_t& bytes) {
    return rocprim::exclusive_scan(tmp, bytes, len, off, 0ull, (size_t)n + 1, rocprim::plus<unsigned long long>(),
                                   c.stream);
  });
  unsigned long long h = 0;
  PG_HIP(hipMemcpyAsync(&h, off + n, 8, hipMemcpyDeviceToHost, c.stream));
  c.sync();
  return h;
}
[[maybe_unused]] static int bits_for(uint64_t maxv) {
  int b = 1;
  while (b < 64 && (maxv >> b)) ++b;
  return b;
}

// pg_walk.hip: the node slots of an edge list (n0, v0, n1, v1) as sort keys
// with their positions, and dst[t] = src[pos[t]]
__global__ void k_nodes(const unsigned long long* __restrict__ tup, uint64_t nn, unsigned long long* __restrict__ key,
                        unsigned* __restrict__ val, unsigned long long* __restrict__ pos);
__global__ void k_gather_key(const unsigned long long* __restrict__ src, const unsigned long long* __restrict__ pos,
                             uint64_t n, unsigned long long* __restrict__ dst);

}  // namespace pg
