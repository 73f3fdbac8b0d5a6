// pg_steps.h — the kernels of pg_sites.hip that another row pass launches
// (pg_bubbles.hip): declared here, defined there, one definition each.
//   k_vs_steps     the used rows compacted to steps: label, length and genome
//                  per used row, and a flag byte whose bit 0 says the step has
//                  a step before it in its run (clear: the step heads a run)
//   k_vs_groupsum  per-genome sums over presence words
// Their arguments are described at the definitions.
#pragma once
#include "pg_region.h"

namespace pg {

#define ST_FOLLOWS 1u              // flag byte of a step (k_vs_steps' bit 0): it is no run head

__global__ void __launch_bounds__(RG_BLOCK) k_vs_steps(const long long* __restrict__ rows, uint64_t n,
                                                       const int* __restrict__ rec_group,
                                                       const uint8_t* __restrict__ rf, const ull* __restrict__ uoff,
                                                       long long* __restrict__ slab, ull* __restrict__ slen,
                                                       uint32_t* __restrict__ sgen, uint8_t* __restrict__ sf);
// (the kernel strides over its chunks of presence words by gridDim.y: any y is right)
__global__ void __launch_bounds__(RG_BLOCK) k_vs_groupsum(const ull* __restrict__ bits, uint64_t n, uint32_t W,
                                                          const uint32_t* __restrict__ only, uint32_t G, ull* out);

}  // namespace pg
