// pg_compare.hip — the genomes compared through the frequency table's presence
// bits: how many labels every pair of genomes shares (a matrix), and how the
// pan and the core genome change as genomes are added in given orders (the
// accumulation or "growth" curves).
//
// Input: bits [n][W] (label-major: genome g is bit g % 64 of word g / 64 of a
// label's row), on the device already (the last pg_freq's table) or uploaded.
// compare_bits runs the steps over any such device table: pg_freq_compare and
// pg_kmer_compare (pg_colors.hip, the "labels" being the dBG's keys) differ
// only in where the bits come from and where the result goes.
//
// Steps, each its own launch on c.stream (no hand-shake inside a kernel):
//   a. k_cmp_transpose  bits [n][W] -> T [G][NW], genome-major bit rows: bit
//                       l % 64 of T[g][l / 64] = bit g of label l.  NW =
//                       ceil(n / 64) rounded up to even, the padding zero.
//   b. k_cmp_shared     shared[g][h] = sum_w popc(T[g][w] & T[h][w]): a
//                       "popcount GEMM" in 64 x 64 tiles of (g, h) over chunks
//                       of w, the upper tile triangle only; k_cmp_mirror
//                       copies it below the diagonal
//   c. k_cmp_curves     per order and word column the running OR / AND of the
//                       rows taken in the order; their popcounts are the pan /
//                       core counts after 1 .. G genomes
//
// Every sum is an integer, every cross-block sum a no-return 64-bit add at
// agent scope: the result depends on the input alone, whatever the schedule.
#include <cstring>
#include <vector>

#include "pg_prim.h"

namespace pg {

#define CMP_MAX_GROUPS 32768u      // the matrix is dense: 8 GiB at this size
#define CMP_MAX_CHUNK (1u << 25)   // words per k_cmp_shared block: 64 x 2^25 = 2^31 bits, a 32-bit sum cannot wrap

// ------------------------------------------------------------ a. transpose
// A block takes TR_WORDS x 64 labels of one presence word w (64 genomes).
// Each wave loads 64 labels' word (lane = label) and turns it with 64 ballots:
// ballot((v >> b) & 1) is genome b's word for these 64 labels, kept by lane b.
// The words go through LDS so that the block stores, per genome row, one
// contiguous run of TR_WORDS words (128 bytes) instead of one word per lane
// to 64 different rows.  (LDS rows are TR_WORDS + 1 words apart: the 16 lanes
// of a store group then fall on 16 different bank pairs.)
#define TR_WORDS 16
#define TR_STRIDE (TR_WORDS + 1)
__global__ void __launch_bounds__(RG_BLOCK) k_cmp_transpose(const ull* __restrict__ bits, uint64_t n, uint32_t W,
                                                             uint32_t G, uint64_t NW, ull* __restrict__ T) {
  __shared__ ull lds[64 * TR_STRIDE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t ntile = (NW + TR_WORDS - 1) / TR_WORDS;
  for (uint64_t item = blockIdx.x; item < ntile * W; item += gridDim.x) {
    const uint64_t tile = item / W;
    const uint32_t w = (uint32_t)(item - tile * W);
    __syncthreads();                                       // (the previous item's readers are done)
    for (int k = wave; k < TR_WORDS; k += RG_BLOCK / 64) {
      const uint64_t l = (tile * TR_WORDS + k) * 64 + lane;
      const ull v = l < n ? bits[l * W + w] : 0ull;        // labels >= n: 0
      ull mine = 0;
#pragma unroll
      for (int b = 0; b < 64; ++b) {
        const ull m = __ballot((v >> b) & 1);
        if (lane == b) mine = m;
      }
      lds[lane * TR_STRIDE + k] = mine;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * TR_WORDS; i += RG_BLOCK) {
      const int r = i / TR_WORDS, k = i % TR_WORDS;
      const uint32_t g = w * 64 + (uint32_t)r;
      const uint64_t col = tile * TR_WORDS + (uint64_t)k;
      if (g < G && col < NW) T[(uint64_t)g * NW + col] = lds[r * TR_STRIDE + k];     // rows >= G are never written
    }
  }
}

// ------------------------------------------------------------ b. shared
// One block: a 64 x 64 tile (tr, tc >= tr) of (g, h) over the words
// [chunk * cw, (chunk + 1) * cw) of the label axis, SH_KT words at a time.
// Both row panels of a step lie in LDS with a stride of SH_KT + 1 words, so
// the 16 rows a half-wave reads at once fall on 16 different bank pairs
// (66 dwords apart: banks 0, 2, .. 30); the other operand is two addresses
// per half-wave, a broadcast.  Thread (ty, tx) holds the 4 x 4 micro-tile
// g = ty + 16 i, h = tx + 16 j in 32-bit sums.
#define SH_KT 32
#define SH_STRIDE (SH_KT + 1)
__device__ __forceinline__ void cmp_load_panel(const ull* __restrict__ T, uint64_t NW, uint32_t G, uint32_t row0,
                                               uint64_t w0, uint64_t w1, ull* lds) {
  for (int i = threadIdx.x; i < 64 * SH_KT; i += RG_BLOCK) {
    const uint32_t r = i / SH_KT, k = i % SH_KT;
    const uint32_t g = row0 + r;
    lds[r * SH_STRIDE + k] = (g < G && w0 + k < w1) ? T[(uint64_t)g * NW + w0 + k] : 0ull;
  }
}
__global__ void __launch_bounds__(RG_BLOCK) k_cmp_shared(const ull* __restrict__ T, uint64_t NW, uint32_t G,
                                                          uint32_t nT, uint32_t nU, uint64_t cw,
                                                          ull* __restrict__ shared) {
  __shared__ ull As[64 * SH_STRIDE];
  __shared__ ull Bs[64 * SH_STRIDE];
  uint32_t u = blockIdx.x % nU, tr = 0;
  const uint64_t chunk = blockIdx.x / nU;
  while (u >= nT - tr) { u -= nT - tr; ++tr; }             // the u-th tile of the upper triangle, row by row
  const uint32_t tc = tr + u;
  const uint64_t wb = chunk * cw, we = wb + cw < NW ? wb + cw : NW;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const ull* Bp = tr == tc ? As : Bs;
  uint32_t acc[4][4] = {};
  for (uint64_t w0 = wb; w0 < we; w0 += SH_KT) {
    __syncthreads();                                       // (the previous step's readers are done)
    cmp_load_panel(T, NW, G, tr * 64, w0, we, As);
    if (tr != tc) cmp_load_panel(T, NW, G, tc * 64, w0, we, Bs);
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < SH_KT; ++k) {
      ull a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[(ty + 16 * i) * SH_STRIDE + k];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Bp[(tx + 16 * j) * SH_STRIDE + k];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += __popcll(a[i] & b[j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t g = tr * 64 + ty + 16 * i, h = tc * 64 + tx + 16 * j;
      if (g < G && h < G && acc[i][j]) RG_ADD(shared + (uint64_t)g * G + h, (ull)acc[i][j]);
    }
}
// the tiles below the diagonal from their mirror images
__global__ void k_cmp_mirror(ull* __restrict__ shared, uint32_t G) {
  const uint64_t total = (uint64_t)G * G;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t g = (uint32_t)(i / G), h = (uint32_t)(i - (uint64_t)g * G);
    if (g / 64 > h / 64) shared[i] = shared[(uint64_t)h * G + g];
  }
}

// ------------------------------------------------------------ c. curves
// Grid: column chunks x orders.  A lane owns CV_COLS word columns (w = base +
// c * RG_BLOCK + thread: a wave's loads of one row are contiguous) and walks
// the order: x = T[order[n]][w], or |= x, and &= x.  `and` starts as the
// column's valid-label mask (all ones; the low n % 64 bits in the last word;
// 0 in the padding), so labels that do not exist are never in the core.  The
// two popcounts of a step are summed over the lane's columns and then over
// the wave in one 32-bit word, 16 bits each: 64 lanes x CV_COLS x 64 bits =
// 2^14 <= 2^15 while CV_COLS <= 8.  LDS form: the wave's sums go to per-block
// 32-bit LDS counters [G][2] (a block covers RG_BLOCK x CV_COLS x 64 = 2^16
// labels), flushed once with global 64-bit adds.  Above CMP_LDS_GROUPS genomes
// (16 KiB of counters) the wave's sums go straight to global atomics.
#define CV_COLS 4
#define CMP_LDS_GROUPS 2048u
template <bool LDS>
__global__ void __launch_bounds__(RG_BLOCK) k_cmp_curves(const ull* __restrict__ T, uint64_t NW, uint64_t n,
                                                          uint32_t G, const int* __restrict__ orders,
                                                          ull* __restrict__ pan, ull* __restrict__ core) {
  __shared__ uint32_t ctr[LDS ? 2 * CMP_LDS_GROUPS : 1];
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < 2 * G; i += RG_BLOCK) ctr[i] = 0;
    __syncthreads();
  }
  const uint32_t p = blockIdx.y;
  const int* ord = orders + (uint64_t)p * G;
  const uint64_t base = (uint64_t)blockIdx.x * (RG_BLOCK * CV_COLS) + threadIdx.x;
  const uint64_t full = n / 64;                            // words whose 64 labels all exist
  ull o[CV_COLS], a[CV_COLS], x[CV_COLS];
  bool in[CV_COLS];
#pragma unroll
  for (int c = 0; c < CV_COLS; ++c) {
    const uint64_t w = base + (uint64_t)c * RG_BLOCK;
    in[c] = w < NW;
    o[c] = 0;
    a[c] = w < full ? ~0ull : (w == full ? (1ull << (n & 63)) - 1ull : 0ull);
  }
  const ull* row = T + (uint64_t)ord[0] * NW;
#pragma unroll
  for (int c = 0; c < CV_COLS; ++c) x[c] = in[c] ? row[base + (uint64_t)c * RG_BLOCK] : 0ull;
  for (uint32_t s = 0; s < G; ++s) {
    uint32_t v = 0;
#pragma unroll
    for (int c = 0; c < CV_COLS; ++c) {
      o[c] |= x[c];
      a[c] &= x[c];
      v += (uint32_t)__popcll(o[c]) + ((uint32_t)__popcll(a[c]) << 16);
    }
    if (s + 1 < G) {                                       // the next row's loads fly during the reduction
      row = T + (uint64_t)ord[s + 1] * NW;
#pragma unroll
      for (int c = 0; c < CV_COLS; ++c) x[c] = in[c] ? row[base + (uint64_t)c * RG_BLOCK] : 0ull;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) {
      const uint32_t vp = v & 0xFFFFu, vc = v >> 16;
      if (LDS) {
        if (vp) atomicAdd(&ctr[2 * s], vp);
        if (vc) atomicAdd(&ctr[2 * s + 1], vc);
      } else {
        if (vp) RG_ADD(pan + (uint64_t)p * G + s, (ull)vp);
        if (vc) RG_ADD(core + (uint64_t)p * G + s, (ull)vc);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2 * G; i += RG_BLOCK)
      if (ctr[i]) RG_ADD(((i & 1) ? core : pan) + (uint64_t)p * G + (i >> 1), (ull)ctr[i]);
  }
}

// the arguments every comparison shares, checked before any device work
void compare_check(const char* what, uint64_t n, uint32_t G, const int32_t* orders, uint32_t P) {
  const std::string w(what);
  if (G == 0 && n) throw Error(-22, w + ": n_groups is 0 with labels");
  if (!orders && P) throw Error(-22, w + ": orders is NULL");
  if (G > CMP_MAX_GROUPS)
    throw Error(-34, w + ": " + std::to_string(G) + " genomes: the matrix is dense, at most " +
                         std::to_string(CMP_MAX_GROUPS));
  std::vector<uint8_t> seen(G);
  for (uint32_t p = 0; p < P; ++p) {
    std::fill(seen.begin(), seen.end(), 0);
    for (uint32_t i = 0; i < G; ++i) {
      const int32_t g = orders[(uint64_t)p * G + i];
      if (g < 0 || (uint32_t)g >= G || seen[g])
        throw Error(-22, w + ": order " + std::to_string(p) + " is not a permutation of 0.." + std::to_string(G) +
                             "-1 (entry " + std::to_string(i) + " = " + std::to_string(g) + ")");
      seen[g] = 1;
    }
  }
}

// Steps a to c over a device bit table [n][W]: shared [G][G] and curve [2][P][G] (reserved and zeroed here)
// hold the result when the stream has drained; the caller owns both and decides what they replace.
void compare_bits(Ctx& c, const char* what, const ull* bits, uint64_t n, uint32_t G, const int32_t* orders,
                  uint32_t P, DevBuf& shared, DevBuf& curve) {
  compare_check(what, n, G, orders, P);
  const uint32_t W = (uint32_t)(((uint64_t)G + 63) / 64);
  // ---- buffers (an allocation failure leaves the caller's previous result in place)
  const uint64_t NW = ((n + 63) / 64 + 1) & ~1ull;
  const size_t sh_bytes = 8 * (size_t)G * G, cv_bytes = 8 * (size_t)P * G;
  DevBuf tr, ord;
  shared.reserve(sh_bytes + 16);
  curve.reserve(2 * cv_bytes + 16);
  PG_HIP(hipMemsetAsync(shared.p, 0, sh_bytes + 16, c.stream));
  PG_HIP(hipMemsetAsync(curve.p, 0, 2 * cv_bytes + 16, c.stream));
  if (n && G) {
    tr.reserve(8 * (size_t)G * NW);
    ull* T = tr.as<ull>();
    const unsigned cus = (unsigned)std::max(1, c.n_cu);
    // ---- a. transpose
    const uint64_t items = (NW + TR_WORDS - 1) / TR_WORDS * W;
    RG_LAUNCH(k_cmp_transpose, dim3((unsigned)std::min<uint64_t>(items, 64u * cus)), bits, n, W, G, NW, T);
    // ---- b. shared.  Words per block: PG_TUNE_CMP_CHUNK, or by default what
    // gives about four blocks per compute unit over the upper tile triangle,
    // a multiple of SH_KT and at least 8 steps of it (a block's flush is up
    // to 4096 atomics: it should be small beside its 4096 x cw popcounts).
    const uint32_t nT = (G + 63) / 64, nU = nT * (nT + 1) / 2;
    uint64_t cw = c.cmp_chunk;
    if (!cw) {
      const uint64_t want = std::max<uint64_t>(1, (4ull * cus + nU - 1) / nU);
      cw = ((NW + want - 1) / want + SH_KT - 1) / SH_KT * SH_KT;
      cw = std::max<uint64_t>(cw, 8 * SH_KT);
    }
    cw = std::max<uint64_t>(cw, ((uint64_t)NW * nU + (1ull << 30) - 1) >> 30);      // (the grid stays below 2^31)
    cw = std::min<uint64_t>(cw, CMP_MAX_CHUNK);
    const uint64_t nchunk = (NW + cw - 1) / cw;
    RG_LAUNCH(k_cmp_shared, dim3((unsigned)(nchunk * nU)), T, NW, G, nT, nU, cw, shared.as<ull>());
    if (nT > 1) RG_LAUNCH(k_cmp_mirror, dim3(grid_for((uint64_t)G * G, RG_BLOCK, 8192)), shared.as<ull>(), G);
    // ---- c. curves
    if (P) {
      ord.reserve(4 * (size_t)P * G);
      PG_HIP(hipMemcpyAsync(ord.p, orders, 4 * (size_t)P * G, hipMemcpyHostToDevice, c.stream));
      ull* pan = curve.as<ull>();
      ull* core = pan + (size_t)P * G;
      const unsigned gx = (unsigned)((NW + RG_BLOCK * CV_COLS - 1) / (RG_BLOCK * CV_COLS));
      // (the grid's y is at most 65535: orders in slices)
      for (uint32_t p0 = 0; p0 < P; p0 += 65535u) {
        const unsigned gy = std::min<uint32_t>(65535u, P - p0);
        const int* o = ord.as<int>() + (size_t)p0 * G;
        if (c.cmp_form == 0 && G <= CMP_LDS_GROUPS)
          RG_LAUNCH(k_cmp_curves<true>, dim3(gx, gy), T, NW, n, G, o, pan + (size_t)p0 * G, core + (size_t)p0 * G);
        else
          RG_LAUNCH(k_cmp_curves<false>, dim3(gx, gy), T, NW, n, G, o, pan + (size_t)p0 * G, core + (size_t)p0 * G);
      }
    }
  }
  c.sync();                                  // (tr and ord are read until here)
}

void freq_compare(Ctx& c, const uint64_t* h_bits, uint64_t n, uint32_t G, const int32_t* orders, uint32_t P) {
  // ---- arguments: everything refused here leaves the previous result in place
  const uint32_t W = (uint32_t)(((uint64_t)G + 63) / 64);
  if (!h_bits) {
    if (!c.fr_ready) throw Error(-22, "pg_freq_compare: no frequency table (call pg_freq first, or pass bits)");
    if (G != c.fr_groups)
      throw Error(-22, "pg_freq_compare: " + std::to_string(G) + " genomes, the table has " +
                           std::to_string(c.fr_groups));
    n = c.fr_n;
  }
  compare_check("pg_freq_compare", n, G, orders, P);
  if (h_bits && (G & 63)) {
    const uint64_t above = ~0ull << (G & 63);
    for (uint64_t l = 0; l < n; ++l)
      if (h_bits[l * W + W - 1] & above)
        throw Error(-22, "pg_freq_compare: row " + std::to_string(l) + " has a bit at or above genome " +
                             std::to_string(G));
  }
  DevBuf up, shared, curve;
  const ull* bits = nullptr;
  if (n && G) {
    if (h_bits) {
      up.reserve(8 * (size_t)W * n);
      PG_HIP(hipMemcpyAsync(up.p, h_bits, 8 * (size_t)W * n, hipMemcpyHostToDevice, c.stream));
      bits = up.as<ull>();
    } else {
      // the presence words inside c.fr_tab: after label, rows, plus, bases, min, max (pg_freq.hip)
      bits = c.fr_tab.as<ull>() + 6 * n;
    }
  }
  compare_bits(c, "pg_freq_compare", bits, n, G, orders, P, shared, curve);
  // ---- the new result replaces the previous one
  c.cmp_shared.swap(shared);
  c.cmp_curve.swap(curve);
  c.cmp_groups = G;
  c.cmp_orders = P;
  c.cmp_ready = true;
}

void freq_shared(Ctx& c, uint64_t* shared, uint64_t cap) {
  need(c.cmp_ready, "pg_freq_shared", NEED_COMPARE);
  const uint64_t cells = (uint64_t)c.cmp_groups * c.cmp_groups;
  if (cap < cells) throw Error(-34, "pg_freq_shared: buffer too small");
  if (!cells || !shared) return;
  PG_HIP(hipMemcpyAsync(shared, c.cmp_shared.p, 8 * cells, hipMemcpyDeviceToHost, c.stream));
  c.sync();
}

void freq_curve(Ctx& c, uint64_t* pan, uint64_t* core, uint64_t cap) {
  need(c.cmp_ready, "pg_freq_curve", NEED_COMPARE);
  const uint64_t cells = (uint64_t)c.cmp_orders * c.cmp_groups;
  if (cap < cells) throw Error(-34, "pg_freq_curve: buffer too small");
  if (!cells) return;
  if (pan) PG_HIP(hipMemcpyAsync(pan, c.cmp_curve.p, 8 * cells, hipMemcpyDeviceToHost, c.stream));
  if (core) PG_HIP(hipMemcpyAsync(core, c.cmp_curve.as<ull>() + cells, 8 * cells, hipMemcpyDeviceToHost, c.stream));
  c.sync();
}

}  // namespace pg
