// pg_cluster.h — what the clusterers of the `.xyz` graph share (pg_cluster.hip defines it; pg_markov.hip
// uses it): the edge list of a call, the node ids, the union of two nodes in the lock-free union-find,
// and the steps from a hooked parent[] to the `.mcl` text and the label table.
#pragma once
#include <string>

#include "pg_prim.h"

namespace pg {

// one thread per item of n, up to 8192 blocks
#define CC_LAUNCH(kern, n, ...) RG_LAUNCH(kern, grid_for((n), RG_BLOCK, 8192), __VA_ARGS__)

// The edge list of a clustering call on the device: the host's tuples and counts uploaded (`up` owns them;
// -22 in `what`'s name, before any device work, for a node value above 2^32 - 1), or the last edge pass
// where it lies (h_tuples NULL).  vbits: the bits of the largest value.
struct CcEdges {
  DevBuf up;
  const unsigned long long* tup;
  const long long* cnt;
  uint64_t n;
  int vbits = 32;                              // (the edge pass holds values as 32-bit words)
};
CcEdges cc_edges(Ctx& c, const char* what, const uint64_t* h_tuples, const int64_t* h_counts, uint64_t n_edges);

// Step a of a clustering call, the node ids: the nn = 2 n_edges > 0 slots sorted by value, then stably by
// key, positions carried; ids (uint32 [nn]) = every slot's node, numbered by first appearance.  nodes
// non-null: uint64 [nu] keys, [nu] values of the nodes.  Returns their number nu (-34 in `what`'s name for
// 2^32 or more); the sort buffers are freed and the stream is idle when it returns.
uint64_t cc_node_ids(Ctx& c, const char* what, const CcEdges& e, DevBuf& ids, DevBuf* nodes);

// uint32 words per node that cc_finish needs behind parent[]
#define CC_UF_WORDS 11
// Steps d-g of a clustering call.  uf: uint32 [nu] x CC_UF_WORDS whose first nu words are the hooked
// parent[] (k_cc_init, then unions by cc_union); nkey, nval: the nodes.  Flattens the trees, orders the
// clusters and their members, writes the `.mcl` text and the label table into the context and marks the
// clustering ready.  nu == 0: the empty result.
void cc_finish(Ctx& c, uint64_t nu, DevBuf& uf, const unsigned long long* nkey, const unsigned long long* nval);

__global__ void k_cc_init(unsigned* __restrict__ parent, uint64_t nu);

__device__ __forceinline__ unsigned cc_load(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// root of x, with path halving; parent[y] < y for every non-root y, so the walk ends
__device__ __forceinline__ unsigned cc_find(unsigned* parent, unsigned x) {
  for (;;) {
    const unsigned p = cc_load(parent + x);
    if (p == x) return x;
    const unsigned g = cc_load(parent + p);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
  }
}
// join the trees of a and b; true if this call made the union
__device__ __forceinline__ bool cc_union(unsigned* parent, unsigned a, unsigned b) {
  a = cc_find(parent, a);
  b = cc_find(parent, b);
  while (a != b) {
    if (a < b) { const unsigned t = a; a = b; b = t; }        // the larger root goes under the smaller
    unsigned expect = a;
    if (__hip_atomic_compare_exchange_strong(parent + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return true;
    a = cc_find(parent, expect);                                // a got a parent meanwhile: go on from it
    b = cc_find(parent, b);
  }
  return false;
}

}  // namespace pg
