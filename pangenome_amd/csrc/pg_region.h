// pg_region.h — the device side of what the passes over the region rows share
// (pg_freq.hip, the frequency table; pg_region.hip, the region graph;
// pg_regionseq.hip, the region sequences; pg_sites.hip, the variable sites):
// the row and the rule for a used one (RgRow, rs_used), the flag byte
// k_row_scan gives a row and the scan of one of its bits (scan_bit), a tile of
// rows through LDS with or without the row before it (rg_load_tile), the wave
// reductions, the lanes of a wave grouped by label (rg_by_label) and the node
// table of the graph.  The
// loop, launch and atomic macros are pg_prim.h's; the host side (row_input,
// row_scan, labels_seen, text_out, names_upload) is declared in pg_internal.h
// and lives at the top of pg_region.hip.
#pragma once
#include "pg_internal.h"
#include "pg_text.h"

namespace pg {

#define RG_AGG_MIN 4               // lanes of a wave sharing a label before one lane issues for them
#define RG_USED 1u                 // flag byte of a row (k_row_scan): it is used
#define RG_HEAD 2u                 //                                  it starts a run

// off[0 .. n]: the flag bytes with `bit` set before each position (f[n] must be 0); returns off[n]
struct RgBit {
  uint32_t bit;
  __host__ __device__ ull operator()(uint8_t f) const { return (f & bit) ? 1ull : 0ull; }
};
[[maybe_unused]] static uint64_t scan_bit(Ctx& c, const uint8_t* f, uint32_t bit, ull* off, uint64_t n) {
  with_temp(c, [&](void* tmp, size_t& bytes) {
    return rocprim::exclusive_scan(tmp, bytes, rocprim::make_transform_iterator(f, RgBit{bit}), off, 0ull,
                                   (size_t)n + 1, rocprim::plus<ull>(), c.stream);
  });
  ull h = 0;
  PG_HIP(hipMemcpyAsync(&h, off + n, 8, hipMemcpyDeviceToHost, c.stream));
  c.sync();
  return h;
}

struct RgRow {
  long long rec, start, end, strand, label;
};
// The one definition of "a row is used": it has a label and its record a genome.
__device__ __forceinline__ bool rs_used(const RgRow& r, const int* __restrict__ rec_group) {
  return r.label >= 0 && rec_group[r.rec] >= 0;
}
// One tile of RG_BLOCK rows (40 bytes each) through LDS, read as contiguous
// 8-byte loads (a wave: 512 contiguous bytes per load); every thread then
// takes its own row r.  HALO: the row before the tile (row tile * RG_BLOCK - 1,
// none for tile 0) comes with it, and every thread also takes the row before
// its own, p (has_prev: there is one).  Called by every thread of the block
// (two barriers); returns whether the thread has a row.
// lds: RG_TILE_WORDS(HALO) words.
#define RG_TILE_WORDS(HALO) (5 * (RG_BLOCK + ((HALO) ? 1 : 0)))
template <bool HALO>
__device__ __forceinline__ bool rg_load_tile(const long long* __restrict__ rows, uint64_t n, uint64_t tile,
                                             long long* lds, RgRow& r, RgRow& p, bool& has_prev) {
  const uint64_t base = tile * RG_BLOCK;                   // first row of the tile
  const uint32_t halo = HALO && base ? 1u : 0u;
  const uint32_t cnt = (uint32_t)(n - base < RG_BLOCK ? n - base : (uint64_t)RG_BLOCK);
  const uint32_t nw = 5 * (cnt + halo);
  const long long* src = rows + 5 * (base - halo);
  __syncthreads();                                         // (the previous tile's readers are done)
#pragma unroll
  for (uint32_t k = 0; k < (HALO ? 6u : 5u); ++k) {        // (the halo's five words are a sixth round)
    const uint32_t w = k * RG_BLOCK + threadIdx.x;
    if (w < nw) lds[w] = src[w];
  }
  __syncthreads();
  const bool have = threadIdx.x < cnt;
  has_prev = have && (threadIdx.x + halo) > 0;
  if (have) {
    const long long* q = lds + 5 * (threadIdx.x + halo);
    r.rec = q[0]; r.start = q[1]; r.end = q[2]; r.strand = q[3]; r.label = q[4];
    if (HALO && has_prev) { p.rec = q[-5]; p.start = q[-4]; p.end = q[-3]; p.strand = q[-2]; p.label = q[-1]; }
  }
  return have;
}
// the tile without a halo: the thread's own row alone
__device__ __forceinline__ bool rg_load_tile(const long long* __restrict__ rows, uint64_t n, uint64_t tile,
                                             long long* lds, RgRow& r) {
  RgRow p;
  bool has_prev;
  return rg_load_tile<false>(rows, n, tile, lds, r, p, has_prev);
}
__device__ __forceinline__ ull rg_len(const RgRow& r) {
  return r.end >= r.start ? (ull)r.end - (ull)r.start : (ull)r.start - (ull)r.end;
}
__device__ __forceinline__ ull rg_readlane64(ull v, int lane) {
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((ull)hi << 32) | lo;
}
__device__ __forceinline__ ull rg_wave_sum(ull v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ ull rg_wave_max(ull v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) { const ull w = __shfl_xor(v, o); v = w > v ? w : v; }
  return v;
}
__device__ __forceinline__ ull rg_wave_min(ull v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) { const ull w = __shfl_xor(v, o); v = w < v ? w : v; }
  return v;
}
// The lanes of a wave grouped by label (todo: the lane takes part).  A label
// held by RG_AGG_MIN lanes or more: agg(label, mine, leader) is called by
// every lane of the wave (it may reduce across the wave; `leader` is one of
// the lanes that hold the label).  Returns whether the lane is left to issue
// its own atomics.  Every lane of the wave must call it.
template <class Agg>
__device__ __forceinline__ bool rg_by_label(bool todo, ull lab, Agg&& agg) {
  const int lane = threadIdx.x & 63;
  bool own = false;
  for (;;) {
    const ull open = __ballot(todo);
    if (!open) break;
    const int lead = __ffsll(open) - 1;
    const ull lab0 = rg_readlane64(lab, lead);
    const bool mine = todo && lab == lab0;
    const ull m = __ballot(mine);
    todo = todo && !mine;
    if (__popcll(m) < RG_AGG_MIN) {
      own = own || mine;
      continue;
    }
    agg(lab0, mine, (ull)__popcll(m), lane == lead);
  }
  return own;
}

// the node table of the region graph (c.rg_nodes, nn entries)
struct RgNodes {
  long long* label;
  ull *rows, *maxlen;
  uint32_t *nout, *nin;
  static size_t bytes(uint64_t nn) { return 32 * nn + 64; }
  RgNodes(const DevBuf& b, uint64_t nn) {
    label = b.as<long long>();
    rows = reinterpret_cast<ull*>(label + nn);
    maxlen = rows + nn;
    nout = reinterpret_cast<uint32_t*>(maxlen + nn);
    nin = nout + nn;
  }
};

}  // namespace pg
