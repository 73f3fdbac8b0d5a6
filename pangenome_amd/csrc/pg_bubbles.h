// pg_bubbles.h — what pg_bubbles.hip shares with the pass that reads its
// result (pg_variants.hip): the layout of the sites and the alleles tables
// (c.bb_sites, c.bb_alleles) and the search over an ascending offset column.
#pragma once
#include "pg_region.h"

namespace pg {

// ------------------------------------------------------------ the tables
struct BbSites {
  long long *from, *to;
  ull *first, *count;
  uint32_t *nal, *ngen;
  static size_t bytes(uint64_t n) { return 40 * n + 64; }
  BbSites(const DevBuf& b, uint64_t n) {
    from = b.as<long long>();
    to = from + n;
    first = reinterpret_cast<ull*>(to + n);
    count = first + n;
    nal = reinterpret_cast<uint32_t*>(count + n);
    ngen = nal + n;
  }
};
// (n + 1 entries per 8-byte column: the scan of regions into ioff takes one more)
struct BbAlleles {
  ull *site, *regions, *frow, *count, *lo, *hi, *ioff;
  uint32_t* ngen;
  static size_t bytes(uint64_t n) { return 56 * (n + 1) + 4 * n + 64; }
  BbAlleles(const DevBuf& b, uint64_t n) {
    site = b.as<ull>();
    regions = site + n + 1;
    frow = regions + n + 1;
    count = frow + n + 1;
    lo = count + n + 1;
    hi = lo + n + 1;
    ioff = hi + n + 1;
    ngen = reinterpret_cast<uint32_t*>(ioff + n + 1);
  }
};
// the last j in [0, n) with off[j] + step * j <= i (off ascending from 0, off[n] + step * n > i)
__device__ __forceinline__ uint64_t bb_find(const ull* __restrict__ off, uint64_t n, ull step, ull i) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (off[mid] + step * mid <= i) lo = mid; else hi = mid;
  }
  return lo;
}
}  // namespace pg
