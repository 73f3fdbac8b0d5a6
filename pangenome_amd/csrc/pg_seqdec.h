// pg_seqdec.h — the sequence decoder of pg_regionseq.hip for the passes that
// decode spans of their own (pg_variants.hip): the table it reads and the two
// kernels, declared here, defined there, one definition each.
//   k_rs_decode  entry i of the table is bases [min(start, end), max(start,
//                end)) of record rec[i], as they stand if strand[i] == 1 and
//                reverse complemented otherwise; its letters start at byte
//                poff[i] of the blob (a multiple of 16), gc[i] and amb[i]
//                (zero before) are counted.  Reads rec, start, end, strand,
//                len and poff; n entries, nchunks = poff[n] / 16.
//   k_rs_copy    every entry's letters from the blob to dst + dst_off[entry]
// Their arguments are described at the definitions.  pg_variants.hip's placed
// table is laid out here as well, for the pass that reads it (pg_align.hip).
#pragma once
#include "pg_region.h"

namespace pg {

#define RS_DECODE_GRID 2048u       // blocks of k_rs_decode and k_rs_copy: past 8 MiB of letters a block loops
#define RS_NONE (~0ull)

// the table's columns, n + 1 entries each (off[n] and poff[n] are the totals)
struct RsTab {
  long long *label, *row, *rec, *start, *end, *strand;
  ull *len, *gc, *amb, *off, *poff;
  static size_t bytes(uint64_t n) { return 88 * (n + 1) + 64; }
  RsTab(const DevBuf& b, uint64_t n) {
    const uint64_t m = n + 1;
    label = b.as<long long>();
    row = label + m;
    rec = row + m;
    start = rec + m;
    end = start + m;
    strand = end + m;
    len = reinterpret_cast<ull*>(strand + m);
    gc = len + m;
    amb = gc + m;
    off = amb + m;
    poff = off + m;
  }
};

// pg_variants.hip's placed table (c.vr_place, n entries), which pg_align.hip reads too
struct VrPlaced {
  ull *site, *row, *len;
  long long *rec, *pos;
  uint32_t* refal;
  static size_t bytes(uint64_t n) { return 44 * n + 64; }
  VrPlaced(const DevBuf& b, uint64_t n) {
    site = b.as<ull>();
    row = site + n;
    len = row + n;
    rec = reinterpret_cast<long long*>(len + n);
    pos = rec + n;
    refal = reinterpret_cast<uint32_t*>(pos + n);
  }
};

__global__ void __launch_bounds__(RG_BLOCK) k_rs_decode(PackedCls pc, const long long* __restrict__ rec_start,
                                                        ull lastw, RsTab T, uint64_t n, uint64_t nchunks,
                                                        uint4* __restrict__ blob);
__global__ void __launch_bounds__(RG_BLOCK) k_rs_copy(const uint4* __restrict__ blob, RsTab T, uint64_t n,
                                                      uint64_t nchunks, const ull* __restrict__ dst_off,
                                                      char* __restrict__ dst);

}  // namespace pg
