// pg_tree.hip — a tree of the genomes by neighbour joining, in integers
// (include/pangenome.h, "genome tree", has the definition the kernels equal
// bit for bit; host.tree_nj is the same in Python).
//
// Input: a distance matrix d, uint64 [n][n], uploaded (and checked by a device
// reduction) or formed from the last pg_freq_compare's `shared` where it lies.
//
// One matrix holds both forms, so the call takes 8 n^2 + O(n) device bytes:
// the working D = d << 16 lives in the upper triangle, D(a, b) at
// [min(a, b)][max(a, b)], and the lower triangle keeps the d that came in.
// The arg-min only ever needs the pairs i < j, a row's upper part, which a
// wave reads coalesced; the row update reads what lies left of the diagonal
// down a column (n strided words per join beside the arg-min's rows).  After
// the last join k_nj_mirror copies the lower triangle back over the upper one
// and the matrix is pg_tree_dist's result.
//
// Steps, each its own launch on c.stream (no hand-shake inside a kernel):
//   k_nj_from_shared  d(g, h) = shared[g][g] + shared[h][h] - 2 shared[g][h]
//   k_nj_check        a host matrix: symmetric, zero diagonal, no entry > 2^31
//   k_nj_init         per row: r_i = (sum of d[i][.]) << 16, the upper part
//                     shifted in place, slot i = leaf i and live
//   per join, m live slots:
//   k_nj_argmin       a wave per live row i: Q(i, j) over the live j > i, every
//                     lane its best (Q, i, j); wave, then block, one partial
//                     per block
//   k_nj_pick         one block: the partials' minimum, the join record and
//                     its two lengths; slot j dies, r_i restarts at 0
//   k_nj_update       D[i][k] for every other live k, r_k in place, r_i summed
//   k_nj_root         the last three (two, one) live slots
//   k_nj_mirror       the d back over the upper triangle
//
// Every value is a signed 64-bit integer and the minimum is taken under the
// total order (Q, i, j): the result depends on the input alone, whatever the
// number of blocks (PG_TUNE_NJ_BLOCKS) or the order they finish in.
//
// Dead slots are not compacted: a dead row costs its wave one byte, and a live
// row reads the n - i words right of its diagonal, m n / 2 words a join on
// average against the m^2 of a full matrix kept dense.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pg_tree.h"

namespace pg {

#define NJ_UNROLL 4                // row words in flight per lane
#define NJ_TILE 64

// the block's minimum in thread 0
__device__ __forceinline__ void nj_block_min(ll& q, ull& ij) {
  __shared__ ll sq[NJ_WAVES];
  __shared__ ull sij[NJ_WAVES];
  nj_wave_min(q, ij);
  if ((threadIdx.x & 63) == 0) {
    sq[threadIdx.x >> 6] = q;
    sij[threadIdx.x >> 6] = ij;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < NJ_WAVES; ++w)
      if (nj_less(sq[w], sij[w], q, ij)) {
        q = sq[w];
        ij = sij[w];
      }
}
// floor(a / b), b > 0
__device__ __forceinline__ ll nj_floordiv(ll a, ll b) {
  ll q = a / b;
  if (a % b != 0 && a < 0) --q;
  return q;
}

// ------------------------------------------------------------ the matrix
__global__ void __launch_bounds__(RG_BLOCK) k_nj_from_shared(const ull* __restrict__ shared, uint32_t n,
                                                              ull* __restrict__ M) {
  RG_LOOP(idx, (uint64_t)n * n) {
    const uint32_t g = (uint32_t)(idx / n), h = (uint32_t)(idx - (uint64_t)g * n);
    M[idx] = shared[(uint64_t)g * n + g] + shared[(uint64_t)h * n + h] - 2 * shared[idx];
  }
}
// bad: bit 0 an entry above 2^31, bit 1 a non-zero diagonal, bit 2 not symmetric
__global__ void __launch_bounds__(RG_BLOCK) k_nj_check(const ull* __restrict__ M, uint32_t n, unsigned* __restrict__ bad) {
  unsigned b = 0;
  RG_LOOP(idx, (uint64_t)n * n) {
    const uint32_t g = (uint32_t)(idx / n), h = (uint32_t)(idx - (uint64_t)g * n);
    const ull v = M[idx];
    if (v > (1ull << 31)) b |= 1u;
    if (g == h && v) b |= 2u;
    if (g > h && v != M[(uint64_t)h * n + g]) b |= 4u;
  }
  if (b) RG_OR(bad, b);
}
// a wave per row: the row's sum, and its upper part shifted in place
__global__ void __launch_bounds__(RG_BLOCK) k_nj_init(ll* __restrict__ M, uint32_t n, ll* __restrict__ r,
                                                       uint8_t* __restrict__ live, uint32_t* __restrict__ node) {
  const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * NJ_WAVES;
  for (uint32_t i = blockIdx.x * NJ_WAVES + (threadIdx.x >> 6); i < n; i += nw) {
    ll* row = M + (uint64_t)i * n;
    ll s = 0;
    for (uint32_t k = lane; k < n; k += 64) {
      const ll v = row[k];
      s += v;
      if (k > i) row[k] = v << NJ_S;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) {
      r[i] = s << NJ_S;
      live[i] = 1;
      node[i] = i;
    }
  }
}
// the upper triangle from the lower one, tile by tile through LDS: block
// (x, y), x >= y, writes tile (row y, column x) from tile (row x, column y)
__global__ void __launch_bounds__(RG_BLOCK) k_nj_mirror(ull* __restrict__ M, uint32_t n) {
  __shared__ ull tile[NJ_TILE][NJ_TILE + 1];
  const uint32_t tc = blockIdx.x, tr = blockIdx.y;
  if (tc < tr) return;
  for (int e = threadIdx.x; e < NJ_TILE * NJ_TILE; e += RG_BLOCK) {
    const uint32_t y = e / NJ_TILE, x = e % NJ_TILE;
    const uint32_t g = tc * NJ_TILE + y, h = tr * NJ_TILE + x;     // (g, h) below the diagonal
    tile[y][x] = (g < n && h < n) ? M[(uint64_t)g * n + h] : 0ull;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < NJ_TILE * NJ_TILE; e += RG_BLOCK) {
    const uint32_t y = e / NJ_TILE, x = e % NJ_TILE;
    const uint32_t g = tr * NJ_TILE + y, h = tc * NJ_TILE + x;     // (g, h) above it
    if (g < h && h < n) M[(uint64_t)g * n + h] = tile[x][y];
  }
}

// ------------------------------------------------------------ one join
// A wave takes the live rows i = w, w + waves, ..; lane l the columns of the
// 64-aligned run around i + 1, then every 64th: the wave's loads are whole
// 512-byte lines.  A lane meets its pairs in ascending (i, j), so a strict
// `<` on Q keeps the smallest pair among equal Q; across lanes, waves and
// blocks the three keys are compared.
__global__ void __launch_bounds__(RG_BLOCK) k_nj_argmin(const ll* __restrict__ M, const ll* __restrict__ r,
                                                         const uint8_t* __restrict__ live, uint32_t n, ll m2,
                                                         NjKey* __restrict__ part) {
  const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * NJ_WAVES;
  ll bq = NJ_NONE_Q;
  ull bij = NJ_NONE_IJ;
  for (uint32_t i = blockIdx.x * NJ_WAVES + (threadIdx.x >> 6); i + 1 < n; i += nw) {
    if (!live[i]) continue;
    const ll* row = M + (uint64_t)i * n;
    const ll ri = r[i];
    for (uint32_t j0 = ((i + 1) & ~63u) + lane; j0 < n; j0 += 64 * NJ_UNROLL) {
      ll dv[NJ_UNROLL], rj[NJ_UNROLL];
      bool ok[NJ_UNROLL];
#pragma unroll
      for (int u = 0; u < NJ_UNROLL; ++u) {
        const uint32_t j = j0 + 64 * u;
        ok[u] = j > i && j < n && live[j];
        dv[u] = ok[u] ? row[j] : 0;
        rj[u] = ok[u] ? r[j] : 0;
      }
#pragma unroll
      for (int u = 0; u < NJ_UNROLL; ++u) {
        const ll q = m2 * dv[u] - ri - rj[u];
        if (ok[u] && q < bq) {
          bq = q;
          bij = (ull)i << 32 | (j0 + 64 * u);
        }
      }
    }
  }
  nj_block_min(bq, bij);
  if (threadIdx.x == 0) {
    part[blockIdx.x].q = bq;
    part[blockIdx.x].ij = bij;
  }
}

// sel: i, j, D[i][j] of the join (i = ~0: no pair was found, the update does nothing)
__global__ void __launch_bounds__(RG_BLOCK) k_nj_pick(const NjKey* __restrict__ part, uint32_t n_part,
                                                       const ll* __restrict__ M, ll* __restrict__ r,
                                                       uint8_t* __restrict__ live, uint32_t* __restrict__ node,
                                                       uint32_t n, uint32_t m, uint32_t t, uint32_t* __restrict__ left,
                                                       uint32_t* __restrict__ right, ull* __restrict__ len_l,
                                                       ull* __restrict__ len_r, ull* __restrict__ sel) {
  ll q = NJ_NONE_Q;
  ull ij = NJ_NONE_IJ;
  for (uint32_t p = threadIdx.x; p < n_part; p += RG_BLOCK)
    if (nj_less(part[p].q, part[p].ij, q, ij)) {
      q = part[p].q;
      ij = part[p].ij;
    }
  nj_block_min(q, ij);
  if (threadIdx.x) return;
  if (ij == NJ_NONE_IJ) {
    sel[0] = ~0ull;
    return;
  }
  const uint32_t i = (uint32_t)(ij >> 32), j = (uint32_t)ij;
  const ll dij = M[(uint64_t)i * n + j];
  ll li = (dij + nj_floordiv(r[i] - r[j], (ll)m - 2)) >> 1;
  li = li < 0 ? 0 : (li > dij ? dij : li);
  left[t] = node[i];
  right[t] = node[j];
  len_l[t] = (ull)li;
  len_r[t] = (ull)(dij - li);
  node[i] = n + t;
  live[j] = 0;
  r[i] = 0;                                                // (the update sums the new row into it)
  sel[0] = i;
  sel[1] = j;
  sel[2] = (ull)dij;
}

// D(a, b) lies at [min][max]
__device__ __forceinline__ uint64_t nj_at(uint32_t a, uint32_t b, uint32_t n) {
  return a < b ? (uint64_t)a * n + b : (uint64_t)b * n + a;
}
// Every live k but i (j is dead by now) is one thread's: it alone reads and
// writes D(i, k) and r_k, and D(j, k) is not written again.
__global__ void __launch_bounds__(RG_BLOCK) k_nj_update(ll* __restrict__ M, ll* __restrict__ r,
                                                         const uint8_t* __restrict__ live, uint32_t n,
                                                         const ull* __restrict__ sel) {
  __shared__ ll ssum[NJ_WAVES];
  if (sel[0] == ~0ull) return;
  const uint32_t i = (uint32_t)sel[0], j = (uint32_t)sel[1];
  const ll dij = (ll)sel[2];
  ll sum = 0;
  RG_LOOP(k64, n) {
    const uint32_t k = (uint32_t)k64;
    if (!live[k] || k == i) continue;
    const uint64_t pik = nj_at(i, k, n);
    const ll dik = M[pik], djk = M[nj_at(j, k, n)];
    ll nd = (dik + djk - dij) >> 1;
    if (nd < 0) nd = 0;
    M[pik] = nd;
    r[k] += nd - dik - djk;
    sum += nd;
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
  if ((threadIdx.x & 63) == 0) ssum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < NJ_WAVES; ++w) sum += ssum[w];
    if (sum) RG_ADD(r + i, sum);
  }
}

// root: uint32 n_children, child[3]; rlen: [3]
__global__ void __launch_bounds__(RG_BLOCK) k_nj_root(const ll* __restrict__ M, const uint8_t* __restrict__ live,
                                                       const uint32_t* __restrict__ node, uint32_t n,
                                                       uint32_t* __restrict__ root, ull* __restrict__ rlen) {
  __shared__ uint32_t cnt, lo, hi, sum;
  if (threadIdx.x == 0) {
    cnt = sum = hi = 0;
    lo = ~0u;
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < n; k += RG_BLOCK)
    if (live[k]) {
      atomicAdd(&cnt, 1u);
      atomicAdd(&sum, k);
      atomicMin(&lo, k);
      atomicMax(&hi, k);
    }
  __syncthreads();
  if (threadIdx.x) return;
  root[0] = cnt > 3 ? 0 : cnt;                             // (more than 3: never; nothing is read then)
  for (int s = 1; s < 4; ++s) root[s] = 0;
  rlen[0] = rlen[1] = rlen[2] = 0;
  if (cnt == 1) {
    root[1] = node[lo];
  } else if (cnt == 2) {
    const ll d = M[nj_at(lo, hi, n)];
    root[1] = node[lo];
    root[2] = node[hi];
    rlen[0] = (ull)(d >> 1);
    rlen[1] = (ull)(d - (d >> 1));
  } else if (cnt == 3) {
    const uint32_t a = lo, b = sum - lo - hi, c = hi;
    const ll ab = M[nj_at(a, b, n)], ac = M[nj_at(a, c, n)], bc = M[nj_at(b, c, n)];
    const ll xa = (ab + ac - bc) >> 1, xb = (ab + bc - ac) >> 1, xc = (ac + bc - ab) >> 1;
    root[1] = node[a];
    root[2] = node[b];
    root[3] = node[c];
    rlen[0] = (ull)(xa < 0 ? 0 : xa);
    rlen[1] = (ull)(xb < 0 ? 0 : xb);
    rlen[2] = (ull)(xc < 0 ? 0 : xc);
  }
}

// ------------------------------------------------------------ host
void tree_nj(Ctx& c, const uint64_t* h_dist, uint32_t n, uint64_t* n_joins) {
  // ---- arguments: everything refused here or below leaves the previous tree in place
  if (n > NJ_MAX_N)
    throw Error(-34, "pg_tree_nj: " + std::to_string(n) + " leaves: the matrix is dense, at most " +
                         std::to_string(NJ_MAX_N));
  if (!h_dist) {
    if (!c.cmp_ready) throw Error(-22, "pg_tree_nj: no comparison (call pg_freq_compare first, or pass dist)");
    if (n != c.cmp_groups)
      throw Error(-22, "pg_tree_nj: " + std::to_string(n) + " leaves, the comparison has " +
                           std::to_string(c.cmp_groups) + " genomes");
  }
  const uint64_t cells = (uint64_t)n * n;
  const uint32_t J = n > 3 ? n - 3 : 0;
  const unsigned cus = (unsigned)std::max(1, c.n_cu);
  // blocks of the arg-min: PG_TUNE_NJ_BLOCKS, or a wave per row up to four blocks per compute unit
  const unsigned B = c.nj_blocks ? (unsigned)c.nj_blocks : std::max(1u, std::min((n + NJ_WAVES - 1) / NJ_WAVES, 4 * cus));

  // ---- buffers (an allocation failure leaves the previous tree in place)
  DevBuf mat, rsum, flags, nodes, part, sel, jn, jl, rt;
  mat.reserve(8 * (size_t)cells + 16);
  rsum.reserve(8 * (size_t)n + 16);
  flags.reserve((size_t)n + 16);
  nodes.reserve(4 * (size_t)n + 16);
  part.reserve(sizeof(NjKey) * (size_t)B);
  sel.reserve(64);                                         // sel [3], the check's word at [4]
  jn.reserve(8 * (size_t)J + 16);                          // uint32 left [J], right [J]
  jl.reserve(16 * (size_t)J + 16);                         // uint64 left_len [J], right_len [J]
  rt.reserve(64);                                          // uint64 len [3]; uint32 n_children, child [3] at byte 32
  ll* M = mat.as<ll>();
  ll* r = rsum.as<ll>();
  uint8_t* live = flags.as<uint8_t>();
  uint32_t* node = nodes.as<uint32_t>();
  uint32_t* left = jn.as<uint32_t>();
  uint32_t* right = left + J;
  ull* len_l = jl.as<ull>();
  ull* len_r = len_l + J;
  ull* rlen = rt.as<ull>();
  uint32_t* root = rt.as<uint32_t>() + 8;

  // ---- the matrix
  if (n) {
    const unsigned gcells = grid_for(cells, RG_BLOCK, 8192);
    if (h_dist) {
      unsigned* bad = sel.as<unsigned>() + 8;
      PG_HIP(hipMemsetAsync(bad, 0, 4, c.stream));
      PG_HIP(hipMemcpyAsync(M, h_dist, 8 * (size_t)cells, hipMemcpyHostToDevice, c.stream));
      RG_LAUNCH(k_nj_check, gcells, mat.as<ull>(), n, bad);
      unsigned h_bad = 0;
      PG_HIP(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, c.stream));
      c.sync();
      if (h_bad)
        throw Error(-22, std::string("pg_tree_nj: the matrix") + ((h_bad & 1) ? " has an entry above 2^31;" : "") +
                             ((h_bad & 2) ? " has a non-zero diagonal;" : "") +
                             ((h_bad & 4) ? " is not symmetric;" : ""));
    } else {
      RG_LAUNCH(k_nj_from_shared, gcells, c.cmp_shared.as<ull>(), n, mat.as<ull>());
    }
    RG_LAUNCH(k_nj_init, std::min((n + NJ_WAVES - 1) / NJ_WAVES, 8 * cus), M, n, r, live, node);
  }

  // ---- the joins
  uint64_t work = 0;
  c.t_nj.init();
  c.t_nj.start(c.stream);
  for (uint32_t t = 0; t < J; ++t) {
    const uint32_t m = n - t;
    work += (uint64_t)m * m;
    RG_LAUNCH(k_nj_argmin, B, M, r, live, n, (ll)m - 2, part.as<NjKey>());
    RG_LAUNCH(k_nj_pick, 1, part.as<NjKey>(), B, M, r, live, node, n, m, t, left, right, len_l, len_r, sel.as<ull>());
    RG_LAUNCH(k_nj_update, grid_for(n, RG_BLOCK, 64), M, r, live, n, sel.as<ull>());
  }
  c.t_nj.stop(c.stream);
  std::vector<uint32_t> h_jn(2 * (size_t)J), h_root(4, 0);
  std::vector<uint64_t> h_jl(2 * (size_t)J), h_rlen(3, 0);
  if (n) {
    RG_LAUNCH(k_nj_root, 1, M, live, node, n, root, rlen);
    const unsigned nT = (n + NJ_TILE - 1) / NJ_TILE;
    RG_LAUNCH(k_nj_mirror, dim3(nT, nT), mat.as<ull>(), n);
    if (J) {
      PG_HIP(hipMemcpyAsync(h_jn.data(), left, 8 * (size_t)J, hipMemcpyDeviceToHost, c.stream));
      PG_HIP(hipMemcpyAsync(h_jl.data(), len_l, 16 * (size_t)J, hipMemcpyDeviceToHost, c.stream));
    }
    PG_HIP(hipMemcpyAsync(h_root.data(), root, 16, hipMemcpyDeviceToHost, c.stream));
    PG_HIP(hipMemcpyAsync(h_rlen.data(), rlen, 24, hipMemcpyDeviceToHost, c.stream));
  }
  c.sync();
  // ---- the new tree replaces the previous one
  c.ms_nj = c.t_nj.ms();
  c.nj_cells = work;
  c.nj_dist.swap(mat);
  c.nj_join.swap(h_jn);
  c.nj_len.swap(h_jl);
  c.nj_root.swap(h_root);
  c.nj_rlen.swap(h_rlen);
  c.nj_n = n;
  c.nj_ready = true;
  c.bt_ready = false;                                      // (the support described the old tree)
  if (n_joins) *n_joins = J;
}

#define NEED_TREE "no tree (call pg_tree_nj first)"

void tree_dist(Ctx& c, uint64_t* dist, uint64_t cap) {
  need(c.nj_ready, "pg_tree_dist", NEED_TREE);
  const uint64_t cells = (uint64_t)c.nj_n * c.nj_n;
  if (cap < cells) throw Error(-34, "pg_tree_dist: buffer too small");
  if (!cells || !dist) return;
  PG_HIP(hipMemcpyAsync(dist, c.nj_dist.p, 8 * cells, hipMemcpyDeviceToHost, c.stream));
  c.sync();
}

void tree_joins(Ctx& c, uint32_t* left, uint32_t* right, uint64_t* left_len, uint64_t* right_len, uint64_t cap) {
  need(c.nj_ready, "pg_tree_joins", NEED_TREE);
  const size_t J = c.nj_join.size() / 2;
  if (cap < J) throw Error(-34, "pg_tree_joins: buffer too small");
  if (left) std::copy_n(c.nj_join.begin(), J, left);
  if (right) std::copy_n(c.nj_join.begin() + J, J, right);
  if (left_len) std::copy_n(c.nj_len.begin(), J, left_len);
  if (right_len) std::copy_n(c.nj_len.begin() + J, J, right_len);
}

void tree_root(Ctx& c, uint32_t* n_children, uint32_t* child, uint64_t* len) {
  need(c.nj_ready, "pg_tree_root", NEED_TREE);
  if (n_children) *n_children = c.nj_root[0];
  if (child) std::copy_n(c.nj_root.begin() + 1, 3, child);
  if (len) std::copy_n(c.nj_rlen.begin(), 3, len);
}

void tree_time(Ctx& c, double* ms, uint64_t* cells) {
  need(c.nj_ready, "pg_tree_time", NEED_TREE);
  if (ms) *ms = c.ms_nj;
  if (cells) *cells = c.nj_cells;
}

}  // namespace pg
