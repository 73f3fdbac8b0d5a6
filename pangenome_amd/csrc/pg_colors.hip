// pg_colors.hip — the coloured dBG: which genomes hold every key of the dBG
// table (include/pangenome.h, "k-mer colours").
//
// Steps, each its own launch on c.stream (no hand-shake inside a kernel):
//   a. index   k_col_count + a device scan: every table entry's position in
//              the unsorted key list (pg_dbg_export's sweep order: the entry's
//              canonical key if present, then its reverse complement if
//              present); k_col_keys writes that list; a radix sort gives the
//              keys in pg_dbg_export's order and the permutation that made it
//   b. colour  k_col_paint: one thread per run of WW windows (pg_windows.h's
//              enumerator, the walks' own); every window is looked up with one
//              tab_get-style probe, its entry's position read, and genome g's
//              bit ORed into row [position][g / 64] - the word is read first
//              and the atomic issued only if the bit is not yet there (a stale
//              read costs a redundant atomic, never a wrong bit).  The rows
//              are in the unsorted order, so a window costs no rank lookup
//   c. tables  k_col_gather brings the rows into key order (n x W words once,
//              instead of one more dependent load per window); k_col_stat
//              takes the popcount of every row: the spectrum and the
//              per-genome counters through LDS, flushed once per block
//   d. pg_kmer_compare: pg_compare.hip's compare_bits over the rows
//
// Everything is an integer and OR is commutative: the result depends on the
// input alone, whatever the schedule.
#include <cstring>
#include <vector>

#include "pg_prim.h"
#include "pg_windows.h"

namespace pg {

#define KC_MAX_GROUPS 32768u       // as the comparison's
#define KC_LDS_GROUPS 2048u        // per-block LDS counters up to this many genomes (24 KiB), global atomics above

// tab_get's search returning the entry index too (entry index space as
// pg_dbg_export's sweep: [0, nw) primary words, then the overflow slots)
__device__ __forceinline__ uint32_t col_find(const TableView& T, uint64_t nw, uint64_t c, uint64_t& idx) {
  const uint64_t h = T.perm(c);
  const uint64_t b = h >> T.qbits, q = h & ((1ull << T.qbits) - 1ull);
  const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(T.prim + 2 * b);
  if (v.x == 0ull) return 0u;
  if ((v.x >> MW_BITS) == q) { idx = 2 * b; return (uint32_t)(v.x & MW_MASK); }
  if (v.y == 0ull) return 0u;
  if ((v.y >> MW_BITS) == q) { idx = 2 * b + 1; return (uint32_t)(v.y & MW_MASK); }
  const unsigned long long key1 = c + 1ull;
  uint64_t slot = fmix64(c) & T.omask;
  for (uint64_t probe = 0; probe <= T.omask; ++probe) {
    const Slot s = T.ovf[slot];
    if (s.key1 == key1) { idx = nw + slot; return s.mask; }
    if (s.key1 == 0ull) return 0u;
    slot = (slot + 1) & T.omask;
  }
  return 0u;
}

// ------------------------------------------------------------ a. index
__global__ void __launch_bounds__(RG_BLOCK) k_col_count(TableView T, uint64_t nw, uint64_t ntot,
                                                        uint32_t* __restrict__ cnt) {
  RG_LOOP(i, ntot + 1) {
    const uint32_t m = i < ntot ? entry_mask(T, nw, i) : 0u;
    cnt[i] = ((m & PRES_A) ? 1u : 0u) + ((m & PRES_B) ? 1u : 0u);
  }
}
__global__ void __launch_bounds__(RG_BLOCK) k_col_keys(TableView T, uint64_t nw, uint64_t ntot,
                                                       const uint32_t* __restrict__ ebase, ull* __restrict__ keys,
                                                       uint32_t* __restrict__ idx) {
  RG_LOOP(i, ntot) {
    uint32_t o = ebase[i];
    if (ebase[i + 1] == o) continue;
    const uint32_t m = entry_mask(T, nw, i);
    const uint64_t c = entry_key(T, nw, i);
    if (m & PRES_A) { keys[o] = c; idx[o] = o; ++o; }
    if (m & PRES_B) { keys[o] = T.rc(c); idx[o] = o; }
  }
}

// ------------------------------------------------------------ b. colour
struct ColArgs : WalkRuns {
  int rc;
  TableView T;
  uint64_t nw;
  const uint32_t* ebase;       // per table entry: its first position in the unsorted key list
  const int* group;            // per record: its genome (walked records: >= 0)
  ull* ubits;                  // [n][W], rows in the unsorted order
  uint32_t W;
  ull* counters;               // [0] windows looked up, [1] those whose key the table does not hold
};

__global__ void __launch_bounds__(WBLOCK) k_col_paint(ColArgs a, uint64_t nruns) {
  __shared__ ull s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  uint32_t nwin = 0, nmiss = 0;
  for (uint64_t u = blockIdx.x * (uint64_t)WBLOCK + threadIdx.x; u < nruns; u += (uint64_t)gridDim.x * WBLOCK) {
    uint64_t wr; int r; long long rs, n, q0, q1;
    run_locate(a, u, wr, r, rs, n, q0, q1);
    const uint32_t g = (uint32_t)a.group[r];
    const uint32_t word = g >> 6;
    const ull bit = 1ull << (g & 63);
    auto paint = [&](uint64_t x, uint64_t xrc) {
      if (x == SENTINEL) return;                            // (n < k: the table never holds it)
      ++nwin;
      const uint64_t c = x < xrc ? x : xrc;
      uint64_t e = 0;
      const uint32_t m = col_find(a.T, a.nw, c, e);
      const bool isb = x != c;
      if (!(m & (isb ? PRES_B : PRES_A))) { ++nmiss; return; }
      ull* p = a.ubits + ((uint64_t)a.ebase[e] + ((isb && (m & PRES_A)) ? 1u : 0u)) * a.W + word;
      if (!(*p & bit)) RG_OR(p, bit);
    };
    for_windows(a.cls, rs, n, a.k, a.shift, q0, q1, [&](long long, const Win& w) {
      paint(w.xf, w.xf_rc);
      if (a.rc) paint(w.xr, w.xr_rc);
    });
  }
  if (nwin) atomicAdd(&s_cnt[0], (ull)nwin);
  if (nmiss) atomicAdd(&s_cnt[1], (ull)nmiss);
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) RG_ADD(a.counters + threadIdx.x, s_cnt[threadIdx.x]);
}

// ------------------------------------------------------------ c. tables
__global__ void __launch_bounds__(RG_BLOCK) k_col_gather(const ull* __restrict__ ubits,
                                                         const uint32_t* __restrict__ perm, uint64_t n, uint32_t W,
                                                         ull* __restrict__ bits) {
  RG_LOOP(t, n * W) {
    const uint64_t j = t / W;
    const uint32_t w = (uint32_t)(t - j * W);
    bits[t] = ubits[(uint64_t)perm[j] * W + w];
  }
}

// stat: [G + 1] keys by number of genomes, then [G] the keys of genome g found
// in fewer than G genomes, then [G] those found in g alone.  A key in all G
// genomes adds one to by_g[G] and nothing else (every genome's core count is
// that one number), so the pass costs one counter per key of the core and one
// per set bit only outside it.
template <bool LDS>
__global__ void __launch_bounds__(RG_BLOCK) k_col_stat(const ull* __restrict__ bits, uint64_t n, uint32_t W,
                                                       uint32_t G, ull* __restrict__ stat) {
  __shared__ uint32_t ctr[LDS ? 3 * KC_LDS_GROUPS + 1 : 1];
  __shared__ ull s_all;
  const uint32_t nctr = 3 * G + 1;
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < nctr; i += RG_BLOCK) ctr[i] = 0;
  }
  if (threadIdx.x == 0) s_all = 0;
  __syncthreads();
  uint32_t all = 0;
  RG_LOOP(j, n) {
    const ull* row = bits + j * W;
    uint32_t cnt = 0;
    for (uint32_t w = 0; w < W; ++w) cnt += (uint32_t)__popcll(row[w]);
    if (cnt == G) { ++all; continue; }
    if (LDS) atomicAdd(&ctr[cnt], 1u); else RG_ADD(stat + cnt, 1ull);
    for (uint32_t w = 0; w < W; ++w) {
      ull v = row[w];
      while (v) {
        const uint32_t g = w * 64 + (uint32_t)__builtin_ctzll(v);
        v &= v - 1;
        if (LDS) {
          atomicAdd(&ctr[G + 1 + g], 1u);
          if (cnt == 1) atomicAdd(&ctr[2 * G + 1 + g], 1u);
        } else {
          RG_ADD(stat + G + 1 + g, 1ull);
          if (cnt == 1) RG_ADD(stat + 2 * G + 1 + g, 1ull);
        }
      }
    }
  }
  if (all) atomicAdd(&s_all, (ull)all);
  __syncthreads();
  if (threadIdx.x == 0 && s_all) RG_ADD(stat + G, s_all);
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < nctr; i += RG_BLOCK)
      if (ctr[i]) RG_ADD(stat + i, (ull)ctr[i]);
  }
}

// ------------------------------------------------------------------ host
static bool colors_valid(Ctx& c) {
  if (c.kc_ready && !(c.parsed && c.built && c.kc_gen == c.build_gen)) kmer_colors_drop(c);   // the table was replaced
  return c.kc_ready;
}
#define NEED_COLORS "no k-mer colours (call pg_kmer_colors first, after the last build or load)"
#define NEED_KCOMPARE "no k-mer comparison (call pg_kmer_compare first, after the last pg_kmer_colors)"

void kmer_colors_drop(Ctx& c) {
  c.kc_keys.release(); c.kc_bits.release(); c.kc_stat.release();
  c.kc_shared.release(); c.kc_curve.release();
  c.kc_ready = c.kc_cmp_ready = false;
  c.kc_n = 0;
}

void kmer_colors(Ctx& c, const int32_t* rec_group, const uint8_t* rec_flags, uint64_t n_records, uint32_t G,
                 int rc0, uint64_t* n_keys, uint64_t* n_windows, uint64_t* n_missing, uint64_t* n_uncoloured) {
  // ---- arguments: everything refused here leaves the previous result in place
  if (!c.parsed) throw Error(-22, "pg_kmer_colors: no parsed FASTA");
  if (!c.built) throw Error(-22, "pg_kmer_colors: no dBG table (call pg_build_dbg or pg_dbg_load first)");
  if (!rec_group) throw Error(-22, "pg_kmer_colors: rec_group is NULL");
  const uint64_t R = c.n_records;
  if (n_records != R)
    throw Error(-22, "pg_kmer_colors: " + std::to_string(n_records) + " records, the parse has " + std::to_string(R));
  if (G == 0 && R) throw Error(-22, "pg_kmer_colors: n_groups is 0 with records");
  if (G > KC_MAX_GROUPS)
    throw Error(-34, "pg_kmer_colors: " + std::to_string(G) + " genomes, at most " + std::to_string(KC_MAX_GROUPS));
  for (uint64_t r = 0; r < R; ++r)
    if (rec_group[r] < -1 || (int64_t)rec_group[r] >= (int64_t)G)
      throw Error(-22, "pg_kmer_colors: rec_group[" + std::to_string(r) + "] = " + std::to_string(rec_group[r]) +
                           " is outside [-1, " + std::to_string(G) + ")");
  if (2 * c.n_canon >= (1ull << 32)) throw Error(-34, "pg_kmer_colors: 2^32 keys or more");
  const uint32_t W = (uint32_t)(((uint64_t)G + 63) / 64);
  std::vector<uint8_t> walk(R + 1);
  for (uint64_t r = 0; r < R; ++r) walk[r] = (!rec_flags || rec_flags[r] != 0) && rec_group[r] >= 0;

  for (auto& t : c.t_kc) t.init();
  // ---- a. index
  const uint64_t nw = 2 * c.cap, ntot = nw + c.ovf_cap;
  DevBuf cnt, ebase, ukeys, uidx, keys, perm, ubits, bits, stat, grp, ctr;
  cnt.reserve(4 * (ntot + 2));
  ebase.reserve(4 * (ntot + 2));
  c.t_kc[0].start(c.stream);
  RG_LAUNCH(k_col_count, grid_for(ntot + 1, RG_BLOCK, 16384), c.tv, nw, ntot, cnt.as<uint32_t>());
  with_temp(c, [&](void* tmp, size_t& bytes) {
    return rocprim::exclusive_scan(tmp, bytes, cnt.as<uint32_t>(), ebase.as<uint32_t>(), 0u, (size_t)ntot + 1,
                                   rocprim::plus<uint32_t>(), c.stream);
  });
  uint32_t n32 = 0;
  PG_HIP(hipMemcpyAsync(&n32, ebase.as<uint32_t>() + ntot, 4, hipMemcpyDeviceToHost, c.stream));
  c.sync();
  cnt.release();
  const uint64_t n = n32;
  ukeys.reserve(8 * n);
  uidx.reserve(4 * n);
  keys.reserve(8 * n);
  perm.reserve(4 * n);
  if (n) {
    RG_LAUNCH(k_col_keys, grid_for(ntot, RG_BLOCK, 16384), c.tv, nw, ntot, ebase.as<uint32_t>(), ukeys.as<ull>(),
              uidx.as<uint32_t>());
    sort_pairs(c, ukeys.as<ull>(), keys.as<ull>(), uidx.as<uint32_t>(), perm.as<uint32_t>(), n, c.kb);
  }
  c.t_kc[0].stop(c.stream);
  // ---- b. colour
  ubits.reserve(8 * (size_t)W * n);
  bits.reserve(8 * (size_t)W * n);
  stat.reserve(8 * (3 * (size_t)G + 2));
  ctr.reserve(16);
  grp.reserve(4 * (R + 1));
  WalkPlan P;
  plan_walk(c, walk.data(), P);
  ColArgs a;
  fill_runs(c, P, a);
  a.rc = rc0 ? 1 : 0;
  a.T = c.tv;
  a.nw = nw;
  a.ebase = ebase.as<uint32_t>();
  a.group = grp.as<int>();
  a.ubits = ubits.as<ull>();
  a.W = W;
  a.counters = ctr.as<ull>();
  if (R) PG_HIP(hipMemcpyAsync(grp.p, rec_group, 4 * R, hipMemcpyHostToDevice, c.stream));
  PG_HIP(hipMemsetAsync(ctr.p, 0, 16, c.stream));
  PG_HIP(hipMemsetAsync(stat.p, 0, 8 * (3 * (size_t)G + 2), c.stream));
  if (n && W) PG_HIP(hipMemsetAsync(ubits.p, 0, 8 * (size_t)W * n, c.stream));
  c.t_kc[1].start(c.stream);
  if (P.nruns && W) RG_LAUNCH(k_col_paint, grid_for(P.nruns, WBLOCK, 8192), a, P.nruns);
  c.t_kc[1].stop(c.stream);
  // ---- c. tables
  c.t_kc[2].start(c.stream);
  if (n && W) {
    RG_LAUNCH(k_col_gather, grid_for(n * W, RG_BLOCK, 16384), ubits.as<ull>(), perm.as<uint32_t>(), n, W,
              bits.as<ull>());
    const unsigned gs = grid_for(n, RG_BLOCK, 4u * (unsigned)std::max(1, c.n_cu));
    if (G <= KC_LDS_GROUPS) RG_LAUNCH(k_col_stat<true>, gs, bits.as<ull>(), n, W, G, stat.as<ull>());
    else RG_LAUNCH(k_col_stat<false>, gs, bits.as<ull>(), n, W, G, stat.as<ull>());
  }
  c.t_kc[2].stop(c.stream);
  ull h_ctr[2] = {0, 0}, h_unc = 0;
  PG_HIP(hipMemcpyAsync(h_ctr, ctr.p, 16, hipMemcpyDeviceToHost, c.stream));
  PG_HIP(hipMemcpyAsync(&h_unc, stat.p, 8, hipMemcpyDeviceToHost, c.stream));
  c.sync();
  if (G == 0) h_unc = n;                      // (no genome: every key is in none; stat[0] is by_g[0] = by_g[G])
  // ---- the new result replaces the previous one
  c.kc_keys.swap(keys);
  c.kc_bits.swap(bits);
  c.kc_stat.swap(stat);
  c.kc_shared.release();
  c.kc_curve.release();
  c.kc_cmp_ready = false;
  c.kc_n = n;
  c.kc_gen = c.build_gen;
  c.kc_groups = G;
  c.kc_words = W;
  c.kc_windows = h_ctr[0];
  c.kc_missing = h_ctr[1];
  c.kc_ready = true;
  c.ms_kc_index = c.t_kc[0].ms() + c.t_kc[2].ms();
  c.ms_kc_colour = c.t_kc[1].ms();
  c.ms_kc_compare = 0;
  if (n_keys) *n_keys = n;
  if (n_windows) *n_windows = h_ctr[0];
  if (n_missing) *n_missing = h_ctr[1];
  if (n_uncoloured) *n_uncoloured = h_unc;
}

void kmer_colors_export(Ctx& c, uint64_t* keys, uint64_t* bits, uint64_t cap, uint64_t* n) {
  need(colors_valid(c), "pg_kmer_colors_export", NEED_COLORS);
  if (n) *n = c.kc_n;
  if (!keys && !bits) return;
  if (cap < c.kc_n) throw Error(-34, "pg_kmer_colors_export: buffer too small");
  get(c, keys, c.kc_keys.p, 8 * c.kc_n);
  get(c, bits, c.kc_bits.p, 8 * (size_t)c.kc_words * c.kc_n);
  c.sync();
}

void kmer_colors_spectrum(Ctx& c, uint64_t* kmers_by_g, uint64_t* g_kmers, uint64_t* g_core, uint64_t* g_shell,
                          uint64_t* g_unique) {
  need(colors_valid(c), "pg_kmer_colors_spectrum", NEED_COLORS);
  const uint32_t G = c.kc_groups;
  std::vector<uint64_t> h(3 * (size_t)G + 2, 0);
  PG_HIP(hipMemcpyAsync(h.data(), c.kc_stat.p, 8 * (3 * (size_t)G + 1), hipMemcpyDeviceToHost, c.stream));
  c.sync();
  if (G == 0) h[0] = c.kc_n;
  const uint64_t all = G ? h[G] : 0;           // the keys in every genome
  if (kmers_by_g) std::memcpy(kmers_by_g, h.data(), 8 * ((size_t)G + 1));
  for (uint32_t g = 0; g < G; ++g) {
    const uint64_t part = h[G + 1 + g], uniq = G > 1 ? h[2 * (size_t)G + 1 + g] : 0;
    if (g_kmers) g_kmers[g] = part + all;
    if (g_core) g_core[g] = all;
    if (g_unique) g_unique[g] = uniq;
    if (g_shell) g_shell[g] = part - uniq;
  }
}

void kmer_compare(Ctx& c, const int32_t* orders, uint32_t P) {
  need(colors_valid(c), "pg_kmer_compare", NEED_COLORS);
  DevBuf shared, curve;
  c.t_kc[3].init();
  c.t_kc[3].start(c.stream);
  compare_bits(c, "pg_kmer_compare", c.kc_bits.as<ull>(), c.kc_n, c.kc_groups, orders, P, shared, curve);
  c.t_kc[3].stop(c.stream);
  c.ms_kc_compare = c.t_kc[3].ms();
  c.kc_shared.swap(shared);
  c.kc_curve.swap(curve);
  c.kc_cmp_orders = P;
  c.kc_cmp_ready = true;
}

void kmer_compare_export(Ctx& c, uint64_t* shared, uint64_t shared_cap, uint64_t* pan, uint64_t* core,
                         uint64_t curve_cap) {
  need(colors_valid(c) && c.kc_cmp_ready, "pg_kmer_compare_export", NEED_KCOMPARE);
  const uint64_t sc = (uint64_t)c.kc_groups * c.kc_groups, cc = (uint64_t)c.kc_cmp_orders * c.kc_groups;
  if ((shared && shared_cap < sc) || ((pan || core) && curve_cap < cc))
    throw Error(-34, "pg_kmer_compare_export: buffer too small");
  get(c, shared, c.kc_shared.p, 8 * sc);
  get(c, pan, c.kc_curve.p, 8 * cc);
  get(c, core, c.kc_curve.as<ull>() + cc, 8 * cc);
  c.sync();
}

void kmer_colors_time(Ctx& c, double* ms_index, double* ms_colour, double* ms_compare, uint64_t* n_windows) {
  need(colors_valid(c), "pg_kmer_colors_time", NEED_COLORS);
  if (ms_index) *ms_index = c.ms_kc_index;
  if (ms_colour) *ms_colour = c.ms_kc_colour;
  if (ms_compare) *ms_compare = c.ms_kc_compare;
  if (n_windows) *n_windows = c.kc_windows;
}

}  // namespace pg
