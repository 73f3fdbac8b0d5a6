// pg_markov.hip — Markov clustering of the rdBG (pg_cluster_markov; include/pangenome.h has the
// definition, pangenome_amd/host.py cluster_markov the specification this file equals bit for bit).
//
// Everything is unsigned fixed point, 1.0 = 2^31, and every sum is a sum of integers, so no schedule can
// change a bit.  A matrix is three arrays with a fixed stride of `select` entries per column: uint32
// col_len [U], rows [U x select], vals [U x select], a column's entries by row ascending.
//
// Node ids are pg_cluster.hip's (cc_node_ids).  The weights: every kept edge as a (min id, max id) key,
// radix-sorted and summed per key, then scattered both ways into per-column lists; mk_prune makes the
// initial columns from them, the same function that ends every iteration.
//
// An iteration works column by column.  k_mk_classes bounds the candidates of every column j (the summed
// lengths of the columns j stores) and lists j in one of three classes: up to MK_WAVE_CAND candidates, a
// block of one wave with a 256-slot LDS table, many per CU; up to MK_MID_CAND, four waves with 2048 slots;
// more (at most select^2 = 4096), four waves with an 8192-slot table (96 KB).  k_mk_iter then runs each
// list: column k is one 64-lane load, M[k, j] is uniform in the wave, and each lane adds its product into
// the LDS hash keyed by row (the key claimed by CAS, the value added with a 64-bit LDS atomic).  The
// table's values are then scaled and inflated, and the survivors compacted (into the storage of the keys,
// which are done with) for mk_prune: the distinct rows are often far fewer than the bound, and the sort
// is sized by them.
//
// mk_prune sorts (value descending, row ascending) with a bitonic network over the whole array, so the
// order in which candidates arrived (hash slots, atomic scatter) cannot matter; the first wave then
// renormalises the kept entries, orders them by row, stores them and reduces the column's chaos.
//
// No kernel waits for another thread and nothing is handed over inside a launch: the lists, the bounds
// and the matrices pass between launches on c.stream.  The host reads one word per iteration, the chaos.
// The components are one cc_union per stored entry (the agent-scope atomic rule of pg_cluster.hip), then
// cc_finish.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pg_cluster.h"
#include "pg_internal.h"
#include "pg_region.h"

namespace pg {
namespace {

constexpr ull MK_ONE = 1ull << 31;
constexpr ull MK_CUT = MK_ONE / 10000;
constexpr ull MK_STOP = MK_ONE / 1000;
constexpr unsigned MK_EMPTY = 0xFFFFFFFFu;
constexpr unsigned MK_WAVE_CAND = 128;         // the wave class: bounds up to this
constexpr unsigned MK_WAVE_SLOTS = 256;
constexpr unsigned MK_MID_CAND = 1024;         // the middle class: bounds up to this
constexpr unsigned MK_MID_SLOTS = 2048;
constexpr unsigned MK_BLOCK_SLOTS = 8192;      // select^2 = 4096 candidates at half load
constexpr int MK_CLASSES = 3;
constexpr unsigned MK_BLOCK_THREADS = 256;

struct MkMat {
  unsigned *col_len, *rows, *vals;
};

#define MK_LAUNCH(kern, grid, block, lds, ...)                                            \
  do {                                                                                    \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), (lds), c.stream, __VA_ARGS__);      \
    PG_HIP(hipGetLastError());                                                            \
  } while (0)

// ------------------------------------------------------------ block-wide helpers (T threads, all call)
template <int T>
__device__ __forceinline__ ull mk_sum(ull v, ull* red) {
  v = rg_wave_sum(v);
  if constexpr (T > 64) {
    __syncthreads();                           // (red[] is free of its last use)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0;
    for (int w = 0; w < T / 64; ++w) v += red[w];
  }
  return v;
}
template <int T>
__device__ __forceinline__ ull mk_max(ull v, ull* red) {
  v = rg_wave_max(v);
  if constexpr (T > 64) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0;
    for (int w = 0; w < T / 64; ++w) v = red[w] > v ? red[w] : v;
  }
  return v;
}

// a[0 .. P) descending, P a power of two: the bitonic network, a barrier between its stages
template <int T>
__device__ __forceinline__ void mk_sort_desc(ull* a, unsigned P) {
  for (unsigned k = 2; k <= P; k <<= 1)
    for (unsigned j = k >> 1; j; j >>= 1) {
      __syncthreads();
      for (unsigned t = threadIdx.x; t < P; t += T) {
        const unsigned p = t ^ j;
        if (p > t) {
          const ull x = a[t], y = a[p];
          if ((t & k) == 0 ? x < y : x > y) {
            a[t] = y;
            a[p] = x;
          }
        }
      }
    }
  __syncthreads();
}

// floor(sqrt(x)), exact whatever the double root's last bit
__device__ __forceinline__ ull mk_isqrt(ull x) {
  ull s = (ull)sqrt((double)x);
  while (s * s > x) --s;
  while ((s + 1) * (s + 1) <= x) ++s;
  return s;
}
// x^(inflation2 / 2) in fixed point
__device__ __forceinline__ ull mk_inflate(ull x, unsigned inflation2) {
  ull y = MK_ONE;
  for (unsigned h = inflation2 >> 1; h; --h) y = (y * x) >> 31;
  if (inflation2 & 1) y = (y * mk_isqrt(x << 31)) >> 31;
  return y;
}

// prune(f, select) of column j.  a[0 .. P), P a power of two, LDS or device memory of this block: a
// candidate is (f << 32) | row with 0 < f < 2^32, every other word 0, in any order, at least one candidate.
// Stores the column into `out` and raises *chaos to the column's.  a[] is spent on return.
template <int T>
__device__ __forceinline__ void mk_prune(ull* a, unsigned P, unsigned j, unsigned select, const MkMat& out,
                                         ull* chaos, ull* red) {
  ull s = 0;
  for (unsigned t = threadIdx.x; t < P; t += T) s += a[t] >> 32;
  const ull total = mk_sum<T>(s, red);
  ull ge = 0;
  for (unsigned t = threadIdx.x; t < P; t += T) {
    const ull v = a[t];
    if (!v) continue;
    const ull n = ((v >> 32) << 31) / total;
    ge += n >= MK_CUT;
    a[t] = (n << 32) | (ull)(0xFFFFFFFFu - (unsigned)v);       // (a row is below 2^32 - 1: the word is not 0)
  }
  const ull n_ge = mk_sum<T>(ge, red);
  mk_sort_desc<T>(a, P);
  if (threadIdx.x < 64) {                      // the kept entries, at most 64: the first wave
    const unsigned lane = threadIdx.x;
    const unsigned K = (unsigned)(n_ge < 1 ? 1 : (n_ge > select ? select : n_ge));
    const ull key = lane < K ? a[lane] : 0ull;
    const ull n = key >> 32;
    const unsigned row = 0xFFFFFFFFu - (unsigned)key;
    const ull kept = rg_wave_sum(n);
    const ull v = lane < K ? (n << 31) / kept : 0ull;
    unsigned pos = 0;                          // by row ascending (rows are distinct)
    for (unsigned o = 0; o < K; ++o) pos += (unsigned)__shfl(row, (int)o) < row;
    if (lane < K) {
      out.rows[(size_t)j * select + pos] = row;
      out.vals[(size_t)j * select + pos] = (unsigned)v;
    }
    const ull mx = rg_wave_max(v), sq = rg_wave_sum(v * v);
    if (lane == 0) {
      out.col_len[j] = K;
      const ull ch = mx - (sq >> 31);
      if (ch) RG_MAX(chaos, ch);
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------ the weights
// edge e as a key (min id << 32 | max id) with its count, at most 2^32; a light edge or a self-loop: the
// key above every pair, nu << 32, with 0
__global__ void k_mk_pairs(const unsigned* __restrict__ id, const long long* __restrict__ cnt, uint64_t ne,
                           long long min_weight, ull nu, ull* __restrict__ key, ull* __restrict__ w) {
  RG_LOOP(e, ne) {
    const unsigned a = id[2 * e], b = id[2 * e + 1];
    const long long n = cnt[e];
    const bool keep = n >= min_weight && a != b;
    key[e] = keep ? ((ull)(a < b ? a : b) << 32) | (ull)(a < b ? b : a) : nu << 32;
    w[e] = keep ? ((ull)n > (1ull << 32) ? (1ull << 32) : (ull)n) : 0ull;
  }
}
// a sum that stays at 2^33 once there: no wrap whatever the number of terms (each at most 2^32)
struct MkSatAdd {
  __host__ __device__ ull operator()(ull a, ull b) const {
    const ull s = a + b;
    return s > (1ull << 33) ? (1ull << 33) : s;
  }
};
// the pairs' degrees, and *bad set by a summed weight of 2^32 or more
__global__ void k_mk_degree(const ull* __restrict__ key, const ull* __restrict__ w, uint64_t nq, ull* deg,
                            unsigned* bad) {
  RG_LOOP(q, nq) {
    if (w[q] >= (1ull << 32)) RG_OR(bad, 1u);
    RG_ADD(deg + (key[q] >> 32), 1ull);
    RG_ADD(deg + (key[q] & 0xFFFFFFFFull), 1ull);
  }
}
// the words a column's prune takes: its edges and its loop, rounded up to a power of two
__global__ void k_mk_words(const ull* __restrict__ deg, uint64_t nu, ull* __restrict__ words) {
  RG_LOOP(j, nu) {
    ull p = 1;
    while (p < deg[j] + 1) p <<= 1;
    words[j] = p;
  }
}
// both directions of every pair into the columns' lists (in any order: mk_prune orders)
__global__ void k_mk_scatter(const ull* __restrict__ key, const ull* __restrict__ w, uint64_t nq,
                             const ull* __restrict__ off, ull* cur, ull* __restrict__ ent) {
  RG_LOOP(q, nq) {
    const ull a = key[q] >> 32, b = key[q] & 0xFFFFFFFFull;
    const ull pa = __hip_atomic_fetch_add(cur + a, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ent[off[a] + pa] = (w[q] << 32) | b;
    const ull pb = __hip_atomic_fetch_add(cur + b, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ent[off[b] + pb] = (w[q] << 32) | a;
  }
}
// the initial matrix: column j = prune of its weights and its loop (the largest of them, 1 without any),
// in the column's own words of `work`
__global__ void __launch_bounds__(MK_BLOCK_THREADS) k_mk_first(const ull* __restrict__ ent, const ull* __restrict__ off,
                                                               const ull* __restrict__ woff, ull* work, uint64_t nu,
                                                               unsigned select, MkMat out, ull* chaos) {
  __shared__ ull red[MK_BLOCK_THREADS / 64];
  for (uint64_t j = blockIdx.x; j < nu; j += gridDim.x) {
    const ull* e = ent + off[j];
    const ull d = off[j + 1] - off[j];
    ull* a = work + woff[j];
    const unsigned P = (unsigned)(woff[j + 1] - woff[j]);
    ull mx = 1;
    for (ull t = threadIdx.x; t < d; t += MK_BLOCK_THREADS) mx = (e[t] >> 32) > mx ? (e[t] >> 32) : mx;
    mx = mk_max<MK_BLOCK_THREADS>(mx, red);
    for (unsigned t = threadIdx.x; t < P; t += MK_BLOCK_THREADS)
      a[t] = t < d ? e[t] : (t == d ? (mx << 32) | (ull)j : 0ull);
    __syncthreads();
    mk_prune<MK_BLOCK_THREADS>(a, P, (unsigned)j, select, out, chaos, red);
  }
}

// ------------------------------------------------------------ one iteration
// Column j's bound = the summed lengths of the columns it stores; j goes to the list of its class (bound
// at most MK_WAVE_CAND, at most MK_MID_CAND, more), one add per wave and list.  list: uint32 [MK_CLASSES][nu];
// cnt[cls]: the lists' lengths.
__global__ void __launch_bounds__(RG_BLOCK) k_mk_classes(MkMat m, uint64_t nu, unsigned select,
                                                         unsigned* __restrict__ list, unsigned* cnt) {
  const unsigned lane = threadIdx.x & 63;
  for (uint64_t base = blockIdx.x * (uint64_t)RG_BLOCK; base < nu; base += (uint64_t)gridDim.x * RG_BLOCK) {
    const uint64_t j = base + threadIdx.x;
    const bool todo = j < nu;
    unsigned bound = 0;
    if (todo)
      for (unsigned t = 0, n = m.col_len[j]; t < n; ++t) bound += m.col_len[m.rows[j * select + t]];
    const int my_cls = bound <= MK_WAVE_CAND ? 0 : (bound <= MK_MID_CAND ? 1 : 2);
    for (int cls = 0; cls < MK_CLASSES; ++cls) {
      const bool mine = todo && my_cls == cls;
      const ull mask = __ballot(mine);
      if (!mask) continue;
      const int lead = __ffsll(mask) - 1;
      unsigned at = 0;
      if ((int)lane == lead)
        at = __hip_atomic_fetch_add(cnt + cls, (unsigned)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      at = __shfl(at, lead);
      if (mine) list[cls * nu + at + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned)j;
    }
  }
}

// The columns of one list, a block each: expansion into the LDS table, scaling, inflation, prune.
template <int T, unsigned SLOTS, int SLOT_BITS>
__global__ void __launch_bounds__(T) k_mk_iter(MkMat in, MkMat out, const unsigned* __restrict__ list,
                                               const unsigned* __restrict__ n_list, unsigned select,
                                               unsigned inflation2, ull* chaos) {
  // ull [SLOTS] sums, uint32 [SLOTS] rows (later ull [SLOTS / 2] candidates), ull [T / 64] reductions, a counter
  extern __shared__ ull mk_lds[];
  ull* tval = mk_lds;
  unsigned* tkey = reinterpret_cast<unsigned*>(tval + SLOTS);
  ull* cand = reinterpret_cast<ull*>(tkey);
  ull* red = reinterpret_cast<ull*>(tkey + SLOTS);
  unsigned* n_cand = reinterpret_cast<unsigned*>(red + T / 64);
  const unsigned n = *n_list, lane = threadIdx.x & 63;
  for (unsigned c = blockIdx.x; c < n; c += gridDim.x) {
    const unsigned j = list[c];
    for (unsigned s = threadIdx.x; s < SLOTS; s += T) {
      tkey[s] = MK_EMPTY;
      tval[s] = 0ull;
    }
    if (threadIdx.x == 0) *n_cand = 0u;
    __syncthreads();
    // ---- expansion: acc[i] += M[i, k] * M[k, j], a wave per stored k
    const unsigned len = in.col_len[j];
    for (unsigned t = threadIdx.x >> 6; t < len; t += T / 64) {
      const unsigned k = in.rows[(size_t)j * select + t];
      const ull m = in.vals[(size_t)j * select + t];
      if (lane < in.col_len[k]) {
        const unsigned i = in.rows[(size_t)k * select + lane];
        const ull p = m * (ull)in.vals[(size_t)k * select + lane];
        unsigned s = (i * 2654435761u) >> (32 - SLOT_BITS);
        for (unsigned probe = 0; probe < SLOTS; ++probe) {     // (the bound keeps the table at most half full)
          const unsigned old = atomicCAS(tkey + s, MK_EMPTY, i);
          if (old == MK_EMPTY || old == i) {
            atomicAdd(tval + s, p);
            break;
          }
          s = (s + 1) & (SLOTS - 1);
        }
      }
    }
    __syncthreads();
    // ---- e = acc >> 31, scaled to the column's largest, inflated; a slot becomes a candidate word or 0
    ull mx = 0;
    for (unsigned s = threadIdx.x; s < SLOTS; s += T) mx = (tval[s] >> 31) > mx ? (tval[s] >> 31) : mx;
    mx = mk_max<T>(mx, red);
    for (unsigned s = threadIdx.x; s < SLOTS; s += T) {
      const unsigned i = tkey[s];
      if (i == MK_EMPTY) continue;
      const ull y = mk_inflate(((tval[s] >> 31) << 31) / mx, inflation2);
      tval[s] = y ? (y << 32) | (ull)i : 0ull;
    }
    __syncthreads();
    // ---- the candidates side by side (at most SLOTS / 2 rows: the bound), padded to a power of two
    for (unsigned s = threadIdx.x; s < SLOTS; s += T) {
      const ull v = tval[s];
      if (v) cand[atomicAdd(n_cand, 1u)] = v;
    }
    __syncthreads();
    const unsigned nc = *n_cand;
    unsigned P = 1;
    while (P < nc) P <<= 1;
    for (unsigned t = nc + threadIdx.x; t < P; t += T) cand[t] = 0ull;
    __syncthreads();
    mk_prune<T>(cand, P, j, select, out, chaos, red);
  }
}

// ------------------------------------------------------------ components
__global__ void k_mk_hook(MkMat m, uint64_t nu, unsigned select, unsigned* parent) {
  RG_LOOP(t, nu * select) {
    const uint64_t j = t / select;
    if (t - j * select >= m.col_len[j]) continue;
    const unsigned i = m.rows[t];
    if (i != (unsigned)j) cc_union(parent, i, (unsigned)j);
  }
}

MkMat mk_view(const DevBuf& b, uint64_t nu, unsigned select) {
  unsigned* p = b.as<unsigned>();
  return MkMat{p, p + nu, p + nu + nu * select};
}

}  // namespace

void markov_drop(Ctx& c) {
  c.mk_mat.release();
  c.mk_ready = false;
  c.mk_nodes = c.mk_cols_wave = c.mk_cols_mid = c.mk_cols_block = 0;
}

void cluster_markov(Ctx& c, const uint64_t* h_tuples, const int64_t* h_counts, uint64_t n_edges, int64_t min_weight,
                    uint32_t inflation2, uint32_t select, uint32_t max_iter, uint32_t* n_iter, uint64_t* chaos) {
  const char* what = "pg_cluster_markov";
  const CcEdges e = cc_edges(c, what, h_tuples, h_counts, n_edges);
  n_edges = e.n;
  uint64_t nu = 0, cols_wave = 0, cols_mid = 0, cols_block = 0;
  uint32_t it = 0;
  ull h_chaos = 0;
  DevBuf nodes, uf, mat[2];
  if (n_edges) {
    DevBuf ids;                                // uint32 [2 n_edges]
    nu = cc_node_ids(c, what, e, ids, &nodes);
    // ---- the weights: pairs sorted and summed
    DevBuf pr, st;
    pr.reserve(8 * 4 * n_edges + 64);
    auto* pkey = pr.as<ull>();
    auto* pw = pkey + n_edges;
    auto* ukey = pw + n_edges;                 // (sorted here, then the unique pairs over pkey, pw)
    auto* usum = ukey + n_edges;
    // ull [max_iter + 1] chaos per matrix, then uint32 [max_iter][4] list lengths, a flag, the pair count
    const size_t st_words = (size_t)max_iter + 1;
    st.reserve(8 * st_words + 16 * (size_t)max_iter + 8 + 16);
    auto* d_chaos = st.as<ull>();
    auto* d_cnt = reinterpret_cast<unsigned*>(d_chaos + st_words);
    auto* d_bad = d_cnt + 4 * (size_t)max_iter;
    auto* d_nq = reinterpret_cast<ull*>(d_bad + 2);
    PG_HIP(hipMemsetAsync(st.p, 0, 8 * st_words + 16 * (size_t)max_iter + 8 + 16, c.stream));
    CC_LAUNCH(k_mk_pairs, n_edges, ids.as<unsigned>(), e.cnt, n_edges, (long long)min_weight, (ull)nu, pkey, pw);
    sort_pairs(c, pkey, ukey, pw, usum, n_edges, 32 + bits_for(nu));
    with_temp(c, [&](void* tmp, size_t& bytes) {
      return rocprim::reduce_by_key(tmp, bytes, ukey, usum, (size_t)n_edges, pkey, pw, d_nq, MkSatAdd(),
                                    rocprim::equal_to<ull>(), c.stream);
    });
    ull h_nq = 0, h_last = 0;
    PG_HIP(hipMemcpyAsync(&h_nq, d_nq, 8, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    PG_HIP(hipMemcpyAsync(&h_last, pkey + (h_nq - 1), 8, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    const uint64_t nq = h_nq - ((h_last >> 32) == nu);         // (the dropped edges' key is the last group)
    // ---- degrees, the columns' lists, the words of their prunes
    DevBuf dg, ent, work;
    dg.reserve(8 * 5 * (nu + 1) + 64);
    auto* deg = dg.as<ull>();                  // [nu + 1] each: degrees, list offsets, cursors, words, word offsets
    auto* off = deg + (nu + 1);
    auto* cur = off + (nu + 1);
    auto* words = cur + (nu + 1);
    auto* woff = words + (nu + 1);
    PG_HIP(hipMemsetAsync(dg.p, 0, 8 * 5 * (nu + 1), c.stream));
    if (nq) CC_LAUNCH(k_mk_degree, nq, pkey, pw, nq, deg, d_bad);
    unsigned h_bad = 0;
    PG_HIP(hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, c.stream));
    CC_LAUNCH(k_mk_words, nu, deg, nu, words);
    PG_HIP(hipMemcpyAsync(off, deg, 8 * nu, hipMemcpyDeviceToDevice, c.stream));
    const uint64_t n_ent = excl_scan_total(c, off, off, nu);
    if (h_bad) throw Error(-34, std::string(what) + ": a summed weight of 2^32 or more");
    const uint64_t n_words = excl_scan_total(c, words, woff, nu);
    ent.reserve(8 * n_ent + 16);
    work.reserve(8 * n_words + 16);
    mat[0].reserve((4 + 8 * (size_t)select) * nu + 16);
    mat[1].reserve((4 + 8 * (size_t)select) * nu + 16);
    uf.reserve(4 * CC_UF_WORDS * nu + 16);
    if (nq) CC_LAUNCH(k_mk_scatter, nq, pkey, pw, nq, off, cur, ent.as<ull>());
    // ---- the initial matrix
    MkMat M = mk_view(mat[0], nu, select), N = mk_view(mat[1], nu, select);
    MK_LAUNCH(k_mk_first, grid_for(nu, 1, 8192), MK_BLOCK_THREADS, 0, ent.as<ull>(), off, woff, work.as<ull>(), nu,
              select, M, d_chaos);
    PG_HIP(hipMemcpyAsync(&h_chaos, d_chaos, 8, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    pr.release();
    ent.release();
    work.release();
    // ---- the iterations
    DevBuf lists;                              // uint32 [MK_CLASSES][nu] the classes' columns
    lists.reserve(4 * MK_CLASSES * nu + 16);
    auto* list = lists.as<unsigned>();
    const auto wave_kern = k_mk_iter<64, MK_WAVE_SLOTS, 8>;
    const auto mid_kern = k_mk_iter<MK_BLOCK_THREADS, MK_MID_SLOTS, 11>;
    const auto block_kern = k_mk_iter<MK_BLOCK_THREADS, MK_BLOCK_SLOTS, 13>;
    const size_t wave_lds = 12 * MK_WAVE_SLOTS + 16, mid_lds = 12 * MK_MID_SLOTS + 8 * (MK_BLOCK_THREADS / 64) + 8,
                 block_lds = 12 * MK_BLOCK_SLOTS + 8 * (MK_BLOCK_THREADS / 64) + 8;
    PG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(block_kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)block_lds));
    const unsigned cus = (unsigned)std::max(1, c.n_cu);
    const unsigned wave_grid = grid_for(nu, 1, 64 * cus), mid_grid = grid_for(nu, 1, 12 * cus),
                   block_grid = grid_for(nu, 1, 2 * cus);
    while (it < max_iter) {
      unsigned* cnt = d_cnt + 4 * (size_t)it;
      RG_LAUNCH(k_mk_classes, grid_for(nu, RG_BLOCK, 8192), M, nu, select, list, cnt);
      MK_LAUNCH(wave_kern, wave_grid, 64, wave_lds, M, N, list, cnt, select, inflation2, d_chaos + it + 1);
      MK_LAUNCH(mid_kern, mid_grid, MK_BLOCK_THREADS, mid_lds, M, N, list + nu, cnt + 1, select, inflation2,
                d_chaos + it + 1);
      MK_LAUNCH(block_kern, block_grid, MK_BLOCK_THREADS, block_lds, M, N, list + 2 * nu, cnt + 2, select, inflation2,
                d_chaos + it + 1);
      PG_HIP(hipMemcpyAsync(&h_chaos, d_chaos + it + 1, 8, hipMemcpyDeviceToHost, c.stream));
      c.sync();                                // the iteration's one round trip
      std::swap(M, N);
      mat[0].swap(mat[1]);
      ++it;
      if (h_chaos <= MK_STOP) break;
    }
    if (it) {
      std::vector<unsigned> h_cnt(4 * (size_t)it);
      PG_HIP(hipMemcpyAsync(h_cnt.data(), d_cnt, 16 * (size_t)it, hipMemcpyDeviceToHost, c.stream));
      c.sync();
      for (uint32_t i = 0; i < it; ++i) {
        cols_wave += h_cnt[4 * i];
        cols_mid += h_cnt[4 * i + 1];
        cols_block += h_cnt[4 * i + 2];
      }
    }
    mat[1].release();
    lists.release();
    // ---- the components of the stored entries
    CC_LAUNCH(k_cc_init, nu, uf.as<unsigned>(), nu);
    CC_LAUNCH(k_mk_hook, nu * select, M, nu, select, uf.as<unsigned>());
  }
  cc_finish(c, nu, uf, nodes.as<unsigned long long>(), nodes.as<unsigned long long>() + nu);
  c.mk_mat.swap(mat[0]);                       // (the matrix of the call before goes with mat[0])
  c.mk_nodes = nu;
  c.mk_select = select;
  c.mk_cols_wave = cols_wave;
  c.mk_cols_mid = cols_mid;
  c.mk_cols_block = cols_block;
  c.mk_ready = true;
  if (n_iter) *n_iter = it;
  if (chaos) *chaos = h_chaos;
}

// the kept matrix on the host; the words behind a column's length are 0
void markov_matrix(Ctx& c, uint32_t* col_len, uint32_t* rows, uint32_t* vals) {
  const uint64_t nu = c.mk_nodes, S = c.mk_select;
  if (!nu) return;
  const MkMat M = mk_view(c.mk_mat, nu, (unsigned)S);
  PG_HIP(hipMemcpyAsync(col_len, M.col_len, 4 * nu, hipMemcpyDeviceToHost, c.stream));
  PG_HIP(hipMemcpyAsync(rows, M.rows, 4 * nu * S, hipMemcpyDeviceToHost, c.stream));
  PG_HIP(hipMemcpyAsync(vals, M.vals, 4 * nu * S, hipMemcpyDeviceToHost, c.stream));
  c.sync();
  for (uint64_t j = 0; j < nu; ++j)
    for (uint64_t t = col_len[j]; t < S; ++t) rows[j * S + t] = vals[j * S + t] = 0;
}

}  // namespace pg
