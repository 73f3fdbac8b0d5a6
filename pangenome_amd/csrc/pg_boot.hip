// pg_boot.hip — bootstrap support for the genome tree (include/pangenome.h,
// "tree support", has the definition the kernels equal bit for bit;
// host.tree_bootstrap is the same in Python).
//
// The workload is R replicates of a small problem (G genomes: 8 to a few
// hundred), so every step takes the replicate as a grid dimension and a batch
// of replicates runs in four launches:
//   1. k_boot_gather   draw + gather + transpose in one pass: pg_compare.hip's
//                      ballot transpose with the label index replaced by
//                      idx(b, t), computed in the lane -> T_b [G][NW],
//                      genome-major bit rows of the drawn characters; the
//                      gathered label-major table is never made
//   2. k_boot_hamming  d_b(g, h) = sum_w popc(T_b[g][w] ^ T_b[h][w]): the
//                      64 x 64 popcount GEMM tile with a replicate index in
//                      the grid; the padding is zero on both sides
//   3. k_boot_nj       a replicate's whole neighbour joining by one workgroup,
//                      from the first join to the last: __syncthreads between
//                      the arg-min, the pick and the update where pg_tree_nj
//                      has launch boundaries, and no cross-block hand-shake.
//                      Form 1: the matrix in LDS (n <= 128: 8 n (n + 1) bytes,
//                      rows an odd number of words apart).  Form 2: the same
//                      code over the matrix where step 2 left it (by default
//                      up to 256 leaves from 4 replicates on and up to 512
//                      from 16 on, where it measured faster than form 3).
//                      Form 3 (the rest): pg_tree.hip's per-join kernels, one
//                      replicate after another.
//   4. k_boot_support  a block per replicate: clade words along the joins
//                      (thread w owns word w of every clade: children precede
//                      parents, so no barrier), then a thread per join
//                      canonicalises, hashes, finds the hash among the rated
//                      tree's (sorted on the host), compares all W words and
//                      adds one to that join's count
// Before the first batch steps 1 and 2 run once with idx = the identity and
// k_boot_differs compares the matrix with the rated tree's: the guard.
//
// Every value is an integer and a draw is a pure function of (seed, b, t): the
// result is the same whatever the batch size or the form.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pg_tree.h"

namespace pg {

#define BOOT_MAX_REPS 4096u
#define BOOT_LDS_N 128u            // form 1: 8 x 128 x 129 bytes of matrix + O(n), of the CU's 160 KiB
#define BOOT_WG_N 1024u            // form 2 when asked for: one workgroup's n^3 / 256 steps take seconds above it
#define BOOT_SCRATCH (256ull << 20)
#define BOOT_MAX_CHUNK (1u << 25)  // words per k_boot_hamming block: 64 x 2^25 = 2^31 bits, a 32-bit sum cannot wrap
#define BT_WORDS 16                // (k_cmp_transpose's tile)
#define BT_STRIDE (BT_WORDS + 1)
#define BH_KT 32                   // (k_cmp_shared's step)
#define BH_STRIDE (BH_KT + 1)

#define SM_GAMMA 0x9E3779B97F4A7C15ull
#define SM_STREAM 0xD1B54A32D192ED03ull

__host__ __device__ __forceinline__ ull boot_mix(ull z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the valid-genome mask of clade word w
__host__ __device__ __forceinline__ ull boot_word_mask(uint32_t w, uint32_t n) {
  return w < (n >> 6) ? ~0ull : (w == (n >> 6) ? (1ull << (n & 63)) - 1ull : 0ull);
}
// one word's share of a split's hash (the shares are summed: any order)
__host__ __device__ __forceinline__ ull boot_word_hash(ull c, uint32_t w) {
  return boot_mix(c + SM_GAMMA * (ull)(w + 1));
}

// ------------------------------------------------------------ 1. draw, gather, transpose
// Grid: x over the items (BT_WORDS x 64 draws of one presence word), y the
// replicate of the batch.  Lane = draw t: its row is bits[idx(b, t)] (ident:
// bits[t]); 64 ballots turn the 64 rows' word into 64 genomes' words, which go
// through LDS so that a genome row gets BT_WORDS contiguous words.  Every word
// of T_b [G][NW] is written, the draws >= L as zeros.
__global__ void __launch_bounds__(RG_BLOCK) k_boot_gather(const ull* __restrict__ bits, uint64_t L, uint32_t W,
                                                           uint32_t G, uint64_t NW, ull seed, uint32_t b0, int ident,
                                                           ull* __restrict__ T) {
  __shared__ ull lds[64 * BT_STRIDE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const ull state = seed ^ ((ull)(b0 + blockIdx.y + 1) * SM_STREAM);
  ull* Tb = T + (uint64_t)blockIdx.y * G * NW;
  const uint64_t ntile = (NW + BT_WORDS - 1) / BT_WORDS;
  for (uint64_t item = blockIdx.x; item < ntile * W; item += gridDim.x) {
    const uint64_t tile = item / W;
    const uint32_t w = (uint32_t)(item - tile * W);
    __syncthreads();                                       // (the previous item's readers are done)
    for (int k = wave; k < BT_WORDS; k += RG_BLOCK / 64) {
      const uint64_t t = (tile * BT_WORDS + k) * 64 + lane;
      ull v = 0;
      if (t < L) {
        const ull x = boot_mix(state + (t + 1) * SM_GAMMA);
        const uint64_t src = ident ? t : (((x >> 32) * L) >> 32);     // < L: (x >> 32) < 2^32
        v = bits[src * W + w];
      }
      ull mine = 0;
#pragma unroll
      for (int b = 0; b < 64; ++b) {
        const ull m = __ballot((v >> b) & 1);
        if (lane == b) mine = m;
      }
      lds[lane * BT_STRIDE + k] = mine;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * BT_WORDS; i += RG_BLOCK) {
      const int r = i / BT_WORDS, k = i % BT_WORDS;
      const uint32_t g = w * 64 + (uint32_t)r;
      const uint64_t col = tile * BT_WORDS + (uint64_t)k;
      if (g < G && col < NW) Tb[(uint64_t)g * NW + col] = lds[r * BT_STRIDE + k];
    }
  }
}

// ------------------------------------------------------------ 2. Hamming GEMM
// k_cmp_shared's tile (thread (ty, tx): the 4 x 4 micro-tile g = ty + 16 i,
// h = tx + 16 j, panels BH_KT + 1 words apart in LDS) with popc(a ^ b), the
// replicate in grid y.  A block adds its chunk's sums to d_b (zeroed before),
// a tile above the diagonal to both (g, h) and (h, g): no mirror pass.
__device__ __forceinline__ void boot_load_panel(const ull* __restrict__ T, uint64_t NW, uint32_t G, uint32_t row0,
                                                uint64_t w0, uint64_t w1, ull* lds) {
  for (int i = threadIdx.x; i < 64 * BH_KT; i += RG_BLOCK) {
    const uint32_t r = i / BH_KT, k = i % BH_KT;
    const uint32_t g = row0 + r;
    lds[r * BH_STRIDE + k] = (g < G && w0 + k < w1) ? T[(uint64_t)g * NW + w0 + k] : 0ull;
  }
}
__global__ void __launch_bounds__(RG_BLOCK) k_boot_hamming(const ull* __restrict__ T, uint64_t NW, uint32_t G,
                                                            uint32_t nT, uint32_t nU, uint64_t cw,
                                                            ull* __restrict__ D) {
  __shared__ ull As[64 * BH_STRIDE];
  __shared__ ull Bs[64 * BH_STRIDE];
  const ull* Tb = T + (uint64_t)blockIdx.y * G * NW;
  ull* Db = D + (uint64_t)blockIdx.y * G * G;
  uint32_t u = blockIdx.x % nU, tr = 0;
  const uint64_t chunk = blockIdx.x / nU;
  while (u >= nT - tr) { u -= nT - tr; ++tr; }             // the u-th tile of the upper triangle, row by row
  const uint32_t tc = tr + u;
  const uint64_t wb = chunk * cw, we = wb + cw < NW ? wb + cw : NW;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const ull* Bp = tr == tc ? As : Bs;
  uint32_t acc[4][4] = {};
  for (uint64_t w0 = wb; w0 < we; w0 += BH_KT) {
    __syncthreads();                                       // (the previous step's readers are done)
    boot_load_panel(Tb, NW, G, tr * 64, w0, we, As);
    if (tr != tc) boot_load_panel(Tb, NW, G, tc * 64, w0, we, Bs);
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < BH_KT; ++k) {
      ull a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[(ty + 16 * i) * BH_STRIDE + k];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Bp[(tx + 16 * j) * BH_STRIDE + k];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += __popcll(a[i] ^ b[j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t g = tr * 64 + ty + 16 * i, h = tc * 64 + tx + 16 * j;
      if (g < G && h < G && acc[i][j]) {
        RG_ADD(Db + (uint64_t)g * G + h, (ull)acc[i][j]);
        if (tr != tc) RG_ADD(Db + (uint64_t)h * G + g, (ull)acc[i][j]);
      }
    }
}

// the guard: bit 0 of *flag if the two matrices differ anywhere
__global__ void __launch_bounds__(RG_BLOCK) k_boot_differs(const ull* __restrict__ a, const ull* __restrict__ b,
                                                            uint64_t cells, unsigned* __restrict__ flag) {
  unsigned bad = 0;
  RG_LOOP(i, cells) if (a[i] != b[i]) bad = 1u;
  if (bad) RG_OR(flag, 1u);
}

// ------------------------------------------------------------ 3. a whole tree by one workgroup
// M: the full symmetric matrix, rows ld words apart, holding d on entry; r,
// live, node: [n]; sq, sij, ssum: [NJ_WAVES], in LDS.  The joins of
// include/pangenome.h, "genome tree": as pg_tree.hip, a wave takes the live
// rows i = wave, wave + 4, .. and its lanes the live j > i, each lane meeting
// its pairs in ascending (i, j) so that a strict `<` on Q keeps the smallest
// pair; across lanes and waves (Q, i, j) is compared.  Every thread reads the
// four partials and so knows the pair; thread k updates D(i, k) = D(k, i) and
// r_k for its live k; thread 0 closes the join.  Only (left, right) are kept.
__device__ __forceinline__ void boot_nj_run(ll* M, const uint32_t ld, ll* r, uint8_t* live, uint32_t* node, ll* sq,
                                            ull* sij, ll* ssum, const uint32_t n, uint32_t* left, uint32_t* right) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t i = wave; i < n; i += NJ_WAVES) {
    ll* row = M + (size_t)i * ld;
    ll s = 0;
    for (uint32_t k = lane; k < n; k += 64) {
      const ll v = row[k] << NJ_S;
      row[k] = v;
      s += v;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) {
      r[i] = s;
      live[i] = 1;
      node[i] = i;
    }
  }
  __syncthreads();
  const uint32_t J = n > 3 ? n - 3 : 0;
  for (uint32_t t = 0; t < J; ++t) {
    const ll m2 = (ll)(n - t) - 2;
    ll bq = NJ_NONE_Q;
    ull bij = NJ_NONE_IJ;
    for (uint32_t i = wave; i + 1 < n; i += NJ_WAVES) {
      if (!live[i]) continue;
      const ll* row = M + (size_t)i * ld;
      const ll ri = r[i];
      for (uint32_t j = i + 1 + lane; j < n; j += 64) {
        if (!live[j]) continue;
        const ll q = m2 * row[j] - ri - r[j];
        if (q < bq) {
          bq = q;
          bij = (ull)i << 32 | j;
        }
      }
    }
    nj_wave_min(bq, bij);
    if (lane == 0) {
      sq[wave] = bq;
      sij[wave] = bij;
    }
    __syncthreads();
    bq = sq[0];
    bij = sij[0];
#pragma unroll
    for (int w = 1; w < NJ_WAVES; ++w)
      if (nj_less(sq[w], sij[w], bq, bij)) {
        bq = sq[w];
        bij = sij[w];
      }
    const bool found = bij != NJ_NONE_IJ;                  // (always, with more than three live slots)
    const uint32_t i = found ? (uint32_t)(bij >> 32) : 0u, j = found ? (uint32_t)bij : 0u;
    ll sum = 0;
    if (found) {
      ll* ri = M + (size_t)i * ld;
      const ll* rj = M + (size_t)j * ld;
      const ll dij = ri[j];                                // (no thread writes D(i, j))
      for (uint32_t k = tid; k < n; k += RG_BLOCK) {
        if (!live[k] || k == i || k == j) continue;
        const ll dik = ri[k], djk = rj[k];
        ll nd = (dik + djk - dij) >> 1;
        if (nd < 0) nd = 0;
        ri[k] = nd;
        M[(size_t)k * ld + i] = nd;
        r[k] += nd - dik - djk;
        sum += nd;
      }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane == 0) ssum[wave] = sum;
    __syncthreads();
    if (tid == 0 && found) {
      for (int w = 1; w < NJ_WAVES; ++w) sum += ssum[w];
      left[t] = node[i];
      right[t] = node[j];
      node[i] = n + t;
      live[j] = 0;
      r[i] = sum;
    }
    __syncthreads();
  }
}

// Form 1.  One LDS array holds everything: M [n][n | 1] (a half-wave's 32
// consecutive words of a row are one 256-byte bank row; down a column the odd
// stride puts 32 rows on 32 different bank pairs), r, the partials, node, live.
template <int MAXN>
__global__ void __launch_bounds__(RG_BLOCK) k_boot_nj_lds(const ull* __restrict__ D, uint32_t n, uint32_t J,
                                                           uint32_t* __restrict__ jl, uint32_t* __restrict__ jr) {
  __shared__ ll sm[MAXN * (MAXN + 1) + MAXN + 3 * NJ_WAVES + MAXN / 2 + MAXN / 8];
  if (n > (uint32_t)MAXN) return;                          // (the host never launches it so)
  ll* M = sm;
  ll* r = M + MAXN * (MAXN + 1);
  ll* sq = r + MAXN;
  ull* sij = reinterpret_cast<ull*>(sq + NJ_WAVES);
  ll* ssum = sq + 2 * NJ_WAVES;
  uint32_t* node = reinterpret_cast<uint32_t*>(ssum + NJ_WAVES);
  uint8_t* live = reinterpret_cast<uint8_t*>(node + MAXN);
  const uint32_t ld = n | 1u;
  const ull* Db = D + (uint64_t)blockIdx.x * n * n;
  for (uint32_t e = threadIdx.x; e < n * n; e += RG_BLOCK) {
    const uint32_t i = e / n, k = e - i * n;
    M[i * ld + k] = (ll)Db[e];
  }
  __syncthreads();
  boot_nj_run(M, ld, r, live, node, sq, sij, ssum, n, jl + (uint64_t)blockIdx.x * J, jr + (uint64_t)blockIdx.x * J);
}
// Form 2: in place over the replicate's matrix; r, node and live in global scratch.
__global__ void __launch_bounds__(RG_BLOCK) k_boot_nj_glob(ull* D, uint32_t n, uint32_t J, ll* rbuf, uint32_t* nodebuf,
                                                            uint8_t* livebuf, uint32_t* __restrict__ jl,
                                                            uint32_t* __restrict__ jr) {
  __shared__ ll sp[3 * NJ_WAVES];
  const uint64_t b = blockIdx.x;
  boot_nj_run(reinterpret_cast<ll*>(D) + b * n * n, n, rbuf + b * n, livebuf + b * n, nodebuf + b * n, sp,
              reinterpret_cast<ull*>(sp + NJ_WAVES), sp + 2 * NJ_WAVES, n, jl + b * J, jr + b * J);
}

// ------------------------------------------------------------ 4. clades and matching
// A block per replicate.  clade: [J][W] scratch; rh: the rated splits' hashes
// ascending, ri: their joins, rw: their words [J][W] (by join).
__global__ void __launch_bounds__(RG_BLOCK) k_boot_support(const uint32_t* __restrict__ jl,
                                                            const uint32_t* __restrict__ jr, uint32_t n, uint32_t J,
                                                            uint32_t W, ull* clade_all, const ull* __restrict__ rh,
                                                            const uint32_t* __restrict__ ri,
                                                            const ull* __restrict__ rw,
                                                            uint32_t* __restrict__ support) {
  const uint32_t* left = jl + (uint64_t)blockIdx.x * J;
  const uint32_t* right = jr + (uint64_t)blockIdx.x * J;
  ull* clade = clade_all + (uint64_t)blockIdx.x * J * W;
  for (uint32_t w = threadIdx.x; w < W; w += RG_BLOCK)
    for (uint32_t t = 0; t < J; ++t) {
      ull c = 0;
      for (int s = 0; s < 2; ++s) {
        const uint32_t x = s ? right[t] : left[t];
        if (x < n)
          c |= (x >> 6) == w ? 1ull << (x & 63) : 0ull;
        else if (x - n < t)                                // (children precede parents)
          c |= clade[(uint64_t)(x - n) * W + w];
      }
      clade[(uint64_t)t * W + w] = c;
    }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < J; t += RG_BLOCK) {
    const ull* c = clade + (uint64_t)t * W;
    const bool flip = c[0] & 1ull;                         // leaf 0 is in it: the complement
    ull h = 0;
    for (uint32_t w = 0; w < W; ++w) h += boot_word_hash(flip ? ~c[w] & boot_word_mask(w, n) : c[w], w);
    uint32_t lo = 0, hi = J;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (rh[mid] < h) lo = mid + 1; else hi = mid;
    }
    for (; lo < J && rh[lo] == h; ++lo) {
      const ull* q = rw + (uint64_t)ri[lo] * W;
      bool same = true;
      for (uint32_t w = 0; w < W && same; ++w) same = q[w] == (flip ? ~c[w] & boot_word_mask(w, n) : c[w]);
      if (same) {
        atomicAdd(support + ri[lo], 1u);                   // (a replicate's splits are distinct: one per (b, join))
        break;
      }
    }
  }
}

// ------------------------------------------------------------ host
void tree_bootstrap(Ctx& c, const uint64_t* h_bits, uint64_t L, uint32_t G, uint32_t R, uint64_t seed,
                    uint64_t* rep_dist, uint64_t rep_dist_cap) {
  // ---- arguments: everything refused here or below leaves the previous result in place
  if (!c.nj_ready) throw Error(-22, "pg_tree_bootstrap: no tree (call pg_tree_nj first)");
  if (G != c.nj_n)
    throw Error(-22, "pg_tree_bootstrap: " + std::to_string(G) + " genomes, the tree has " + std::to_string(c.nj_n) +
                         " leaves");
  const uint32_t W = (uint32_t)(((uint64_t)G + 63) / 64);
  if (!h_bits) {
    if (!c.fr_ready) throw Error(-22, "pg_tree_bootstrap: no frequency table (call pg_freq first, or pass bits)");
    if (G != c.fr_groups)
      throw Error(-22, "pg_tree_bootstrap: " + std::to_string(G) + " genomes, the table has " +
                           std::to_string(c.fr_groups));
    L = c.fr_n;
  }
  if (R < 1 || R > BOOT_MAX_REPS)
    throw Error(-22, "pg_tree_bootstrap: " + std::to_string(R) + " replicates: 1 to " + std::to_string(BOOT_MAX_REPS));
  if (G == 0 && L) throw Error(-22, "pg_tree_bootstrap: n_groups is 0 with labels");
  if (L > (1ull << 31)) throw Error(-34, "pg_tree_bootstrap: " + std::to_string(L) + " labels: at most 2^31");
  if (h_bits && (G & 63)) {
    const uint64_t above = ~0ull << (G & 63);
    for (uint64_t l = 0; l < L; ++l)
      if (h_bits[l * W + W - 1] & above)
        throw Error(-22, "pg_tree_bootstrap: row " + std::to_string(l) + " has a bit at or above genome " +
                             std::to_string(G));
  }
  const uint32_t n = G, J = n > 3 ? n - 3 : 0;
  const uint64_t cells = (uint64_t)n * n;
  if (rep_dist && rep_dist_cap < (uint64_t)R * cells) throw Error(-34, "pg_tree_bootstrap: rep_dist buffer too small");

  // ---- the rated tree's splits: canonical words by join, and the joins in hash order
  std::vector<ull> rw((size_t)J * W + 1, 0ull), rh(J + 1, 0ull);
  std::vector<uint32_t> ri(J + 1, 0u);
  {
    std::vector<ull> raw((size_t)J * W + 1, 0ull);
    std::vector<std::pair<ull, uint32_t>> order(J);
    for (uint32_t t = 0; t < J; ++t) {
      ull* cw = raw.data() + (size_t)t * W;
      for (int s = 0; s < 2; ++s) {
        const uint32_t x = c.nj_join[s ? (size_t)J + t : t];
        if (x < n)
          cw[x >> 6] |= 1ull << (x & 63);
        else
          for (uint32_t w = 0; w < W; ++w) cw[w] |= raw[(size_t)(x - n) * W + w];
      }
      const bool flip = cw[0] & 1ull;
      ull h = 0;
      for (uint32_t w = 0; w < W; ++w) {
        const ull v = flip ? ~cw[w] & boot_word_mask(w, n) : cw[w];
        rw[(size_t)t * W + w] = v;
        h += boot_word_hash(v, w);
      }
      order[t] = {h, t};
    }
    std::sort(order.begin(), order.end());
    for (uint32_t t = 0; t < J; ++t) {
      rh[t] = order[t].first;
      ri[t] = order[t].second;
    }
  }

  // ---- the form and the batches
  uint32_t form = (uint32_t)c.bt_form_tune;
  if (form == 1 && n > BOOT_LDS_N) form = 0;
  if (form == 2 && n > BOOT_WG_N) form = 3;
  // by size: where each form measured faster than form 3 (profiles/tree_bootstrap_time.json) - the LDS
  // form wherever it is legal; the global form while enough replicates run side by side to pay for a
  // workgroup's long serial run (at 1024 leaves it lost even with 100)
  if (form == 0) form = n <= BOOT_LDS_N ? 1 : ((n <= 256 && R >= 4) || (n <= 512 && R >= 16) ? 2 : 3);
  const uint64_t NW = ((L + 63) / 64 + 1) & ~1ull;
  const uint64_t per_rep =
      8 * (uint64_t)G * NW + 8 * cells + 8 * (uint64_t)J * W + 8 * (uint64_t)J + 13 * (uint64_t)n + 64;
  const uint64_t budget = c.bt_scratch ? c.bt_scratch : BOOT_SCRATCH;
  const uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(R, budget / per_rep));
  const unsigned cus = (unsigned)std::max(1, c.n_cu);

  // ---- buffers (an allocation failure leaves the previous result in place)
  DevBuf up, tr, dist, gdist, clade, jn, work, rated, sup, flagb, part, sel, lens;
  tr.reserve(8 * (size_t)G * NW * batch + 16);
  dist.reserve(8 * (size_t)cells * batch + 16);
  gdist.reserve(8 * (size_t)cells + 16);
  clade.reserve(8 * (size_t)J * W * batch + 16);
  jn.reserve(8 * (size_t)J * batch + 16);                  // uint32 left [batch][J], right [batch][J]
  work.reserve(13 * (size_t)n * batch + 64);               // [batch][n] each: int64 r, uint32 node, uint8 live
  rated.reserve(8 * ((size_t)J * W + 1) + 12 * ((size_t)J + 1) + 16);   // words, hashes, joins
  sup.reserve(4 * (size_t)J + 16);
  flagb.reserve(16);
  const unsigned B3 =
      c.nj_blocks ? (unsigned)c.nj_blocks : std::max(1u, std::min((n + NJ_WAVES - 1) / NJ_WAVES, 4 * cus));
  if (form == 3) {
    part.reserve(sizeof(NjKey) * (size_t)B3);
    sel.reserve(64);
    lens.reserve(16 * (size_t)J + 16);
  }
  std::vector<uint32_t> h_sup(J, 0u), h_jn(2 * (size_t)R * J, 0u);
  ull* T = tr.as<ull>();
  ull* D = dist.as<ull>();
  uint32_t* jl = jn.as<uint32_t>();
  uint32_t* jr = jl + (size_t)batch * J;
  ll* wr = work.as<ll>();
  uint32_t* wnode = reinterpret_cast<uint32_t*>(wr + (size_t)batch * n);
  uint8_t* wlive = reinterpret_cast<uint8_t*>(wnode + (size_t)batch * n);
  ull* d_rw = rated.as<ull>();
  ull* d_rh = d_rw + (size_t)J * W + 1;
  uint32_t* d_ri = reinterpret_cast<uint32_t*>(d_rh + J + 1);

  double ms[3] = {0, 0, 0};
  uint32_t n_batches = 0;
  if (cells) {
    const ull* bits = nullptr;
    if (L) {
      if (h_bits) {
        up.reserve(8 * (size_t)W * L);
        PG_HIP(hipMemcpyAsync(up.p, h_bits, 8 * (size_t)W * L, hipMemcpyHostToDevice, c.stream));
        bits = up.as<ull>();
      } else {
        bits = c.fr_tab.as<ull>() + 6 * L;                 // the presence words inside c.fr_tab (pg_freq.hip)
      }
    }
    // the two distance launches over nb replicates from b0 on (ident: the table itself), into Dst
    const uint64_t items = (NW + BT_WORDS - 1) / BT_WORDS * W;
    const uint32_t nT = (G + 63) / 64, nU = nT * (nT + 1) / 2;
    auto distances = [&](uint32_t b0, uint32_t nb, int ident, ull* Dst) {
      PG_HIP(hipMemsetAsync(Dst, 0, 8 * (size_t)cells * nb, c.stream));
      if (!L) return;
      const unsigned gx = (unsigned)std::min<uint64_t>(items, std::max<uint64_t>(1, 64ull * cus / nb));
      RG_LAUNCH(k_boot_gather, dim3(gx, nb), bits, L, W, G, NW, (ull)seed, b0, ident, T);
      // words per block: about four blocks per compute unit over the batch's tiles, a multiple of
      // BH_KT and at least 8 steps of it (pg_compare.hip's rule)
      const uint64_t want = std::max<uint64_t>(1, (4ull * cus + (uint64_t)nU * nb - 1) / ((uint64_t)nU * nb));
      uint64_t cw = ((NW + want - 1) / want + BH_KT - 1) / BH_KT * BH_KT;
      cw = std::max<uint64_t>(cw, 8 * BH_KT);
      cw = std::max<uint64_t>(cw, ((uint64_t)NW * nU + (1ull << 30) - 1) >> 30);    // (the grid stays below 2^31)
      cw = std::min<uint64_t>(cw, BOOT_MAX_CHUNK);
      const uint64_t nchunk = (NW + cw - 1) / cw;
      RG_LAUNCH(k_boot_hamming, dim3((unsigned)(nchunk * nU), nb), T, NW, G, nT, nU, cw, Dst);
    };

    // ---- the guard
    unsigned* flag = flagb.as<unsigned>();
    PG_HIP(hipMemsetAsync(flag, 0, 4, c.stream));
    distances(0, 1, 1, gdist.as<ull>());
    RG_LAUNCH(k_boot_differs, grid_for(cells, RG_BLOCK, 8192), gdist.as<ull>(), c.nj_dist.as<ull>(), cells, flag);
    unsigned h_flag = 0;
    PG_HIP(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    if (h_flag) throw Error(-22, "pg_tree_bootstrap: the tree was not built from this table");

    // ---- the replicates
    PG_HIP(hipMemcpyAsync(d_rw, rw.data(), 8 * ((size_t)J * W + 1), hipMemcpyHostToDevice, c.stream));
    PG_HIP(hipMemcpyAsync(d_rh, rh.data(), 8 * ((size_t)J + 1), hipMemcpyHostToDevice, c.stream));
    PG_HIP(hipMemcpyAsync(d_ri, ri.data(), 4 * ((size_t)J + 1), hipMemcpyHostToDevice, c.stream));
    PG_HIP(hipMemsetAsync(sup.p, 0, 4 * (size_t)J + 16, c.stream));
    for (auto& t : c.t_bt) t.init();
    for (uint32_t b0 = 0; b0 < R; b0 += batch, ++n_batches) {
      const uint32_t nb = std::min(batch, R - b0);
      c.t_bt[0].start(c.stream);
      distances(b0, nb, 0, D);
      c.t_bt[0].stop(c.stream);
      if (rep_dist)
        PG_HIP(hipMemcpyAsync(rep_dist + (size_t)b0 * cells, D, 8 * (size_t)cells * nb, hipMemcpyDeviceToHost,
                              c.stream));
      c.t_bt[1].start(c.stream);
      if (J) {
        if (form == 1) {
          if (n <= 64)
            RG_LAUNCH(k_boot_nj_lds<64>, nb, D, n, J, jl, jr);
          else
            RG_LAUNCH(k_boot_nj_lds<(int)BOOT_LDS_N>, nb, D, n, J, jl, jr);
        } else if (form == 2) {
          RG_LAUNCH(k_boot_nj_glob, nb, D, n, J, wr, wnode, wlive, jl, jr);
        } else {
          // pg_tree_nj's launches over each matrix in turn (its D lives in the upper triangle)
          for (uint32_t b = 0; b < nb; ++b) {
            ll* M = reinterpret_cast<ll*>(D) + (size_t)b * cells;
            RG_LAUNCH(k_nj_init, std::min((n + NJ_WAVES - 1) / NJ_WAVES, 8 * cus), M, n, wr, wlive, wnode);
            for (uint32_t t = 0; t < J; ++t) {
              RG_LAUNCH(k_nj_argmin, B3, M, wr, wlive, n, (ll)(n - t) - 2, part.as<NjKey>());
              RG_LAUNCH(k_nj_pick, 1, part.as<NjKey>(), B3, M, wr, wlive, wnode, n, n - t, t, jl + (size_t)b * J,
                        jr + (size_t)b * J, lens.as<ull>(), lens.as<ull>() + J, sel.as<ull>());
              RG_LAUNCH(k_nj_update, grid_for(n, RG_BLOCK, 64), M, wr, wlive, n, sel.as<ull>());
            }
          }
        }
      }
      c.t_bt[1].stop(c.stream);
      c.t_bt[2].start(c.stream);
      if (J) {
        RG_LAUNCH(k_boot_support, nb, jl, jr, n, J, W, clade.as<ull>(), d_rh, d_ri, d_rw, sup.as<uint32_t>());
        PG_HIP(hipMemcpyAsync(h_jn.data() + (size_t)b0 * J, jl, 4 * (size_t)nb * J, hipMemcpyDeviceToHost, c.stream));
        PG_HIP(hipMemcpyAsync(h_jn.data() + ((size_t)R + b0) * J, jr, 4 * (size_t)nb * J, hipMemcpyDeviceToHost,
                              c.stream));
      }
      c.t_bt[2].stop(c.stream);
      for (int k = 0; k < 3; ++k) ms[k] += c.t_bt[k].ms();
    }
    if (J) PG_HIP(hipMemcpyAsync(h_sup.data(), sup.p, 4 * (size_t)J, hipMemcpyDeviceToHost, c.stream));
  } else {
    n_batches = 0;
  }
  c.sync();
  // ---- the new result replaces the previous one
  uint64_t work_cells = 0;
  for (uint32_t t = 0; t < J; ++t) work_cells += (uint64_t)(n - t) * (n - t);
  c.bt_support.swap(h_sup);
  c.bt_join.swap(h_jn);
  c.bt_reps = R;
  c.bt_form = J ? form : 0;
  c.bt_batches = n_batches;
  for (int k = 0; k < 3; ++k) c.ms_bt[k] = ms[k];
  c.bt_cells = work_cells * R;
  c.bt_ready = true;
}

#define NEED_BOOT "no support (call pg_tree_bootstrap after pg_tree_nj)"

void tree_support(Ctx& c, uint32_t* support, uint64_t cap, uint32_t* n_reps) {
  need(c.bt_ready, "pg_tree_support", NEED_BOOT);
  if (cap < c.bt_support.size()) throw Error(-34, "pg_tree_support: buffer too small");
  if (support) std::copy(c.bt_support.begin(), c.bt_support.end(), support);
  if (n_reps) *n_reps = c.bt_reps;
}

void tree_bootstrap_joins(Ctx& c, uint32_t* left, uint32_t* right, uint64_t cap) {
  need(c.bt_ready, "pg_tree_bootstrap_joins", NEED_BOOT);
  const size_t RJ = c.bt_join.size() / 2;
  if (cap < RJ) throw Error(-34, "pg_tree_bootstrap_joins: buffer too small");
  if (left) std::copy_n(c.bt_join.begin(), RJ, left);
  if (right) std::copy_n(c.bt_join.begin() + RJ, RJ, right);
}

void tree_bootstrap_time(Ctx& c, double* ms_dist, double* ms_nj, double* ms_support, uint64_t* cells) {
  need(c.bt_ready, "pg_tree_bootstrap_time", NEED_BOOT);
  if (ms_dist) *ms_dist = c.ms_bt[0];
  if (ms_nj) *ms_nj = c.ms_bt[1];
  if (ms_support) *ms_support = c.ms_bt[2];
  if (cells) *cells = c.bt_cells;
}

void tree_bootstrap_form(Ctx& c, uint32_t* form, uint32_t* n_batches) {
  need(c.bt_ready, "pg_tree_bootstrap_form", NEED_BOOT);
  if (form) *form = c.bt_form;
  if (n_batches) *n_batches = c.bt_batches;
}

}  // namespace pg
