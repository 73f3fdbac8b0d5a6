// pg_sites.hip — the variable sites of the region rows: where the genomes
// differ.  A site is a flank pair (a, c) of labels that two or more alleles
// join: the direct join (a directly followed by c) or one region x between
// them (a x c).  Only bubbles with at most one region inside are found.
//
// Rows, rec_group, the rule for a used row and the run are pg_region_graph's
// (pg_region.hip).  Two consecutive rows of a run give a direct record
// (a, c, via = -1, length 0), three a via record (a, c, via = x, length
// |end - start| of the middle row); the genome of a record is its record's.
// Nothing here is dense in the label: device memory follows the records.
//
// Steps, each its own launch on c.stream (no hand-shake inside a kernel):
//   a. k_row_scan   the shared front end: a flag byte per row; one scan of the
//                   used bit gives every used row its step index
//   b. k_vs_steps   the used rows compacted to steps (label, length, genome)
//                   with two flag bits: the step ends a direct record, the
//                   step ends a via record.  A run is a stretch of consecutive
//                   rows, so the rows before a step's are its run's: no triple
//                   is cut by a tile edge because none is read from a tile.
//      two scans of the flag bits number the direct and the via records
//      k_vs_emit    per step its records by those numbers (no atomics): the
//                   key words k2 = a << lb | c and k1 = (via + 1) << gb | genome,
//                   the length and the record's index
//   c. two stable radix sorts of (key word, index) pairs: by k1 over vb + gb
//      bits, then by k2, gathered through the first order, over 2 lb bits
//      (lb = bits of the largest label, vb = bits of 1 + that, gb = bits of
//      G - 1: up to 62 + 64 bits, so no single 64-bit key holds them); k1 and
//      the length are gathered through the final order.  The records are then
//      in (a, c, via, genome) order.
//   d. k_vs_flags   per record: a new pair, a new allele, a new (allele,
//                   genome); three scans number them.  k_vs_heads notes where
//                   every pair and allele starts; a pair with two alleles or
//                   more is a site (k_vs_keep), and two scans of the keep
//                   flags number the sites and their alleles.
//      k_vs_alleles / k_vs_sites fill the tables from the heads: a count is
//                   the distance between two heads, n_genomes the (allele,
//                   genome) changes between them
//      k_vs_reduce  min / max length and the presence bits of every allele:
//                   a segmented scan inside the wave (the records of an allele
//                   are adjacent lanes), then one atomic per segment and wave
//      k_vs_siteor  the OR of a site's alleles the same way, k_vs_sitegen its
//                   popcount
//   e. k_vs_groupsum  the per-genome sums from the bits: counters in LDS,
//                   2,048 genomes per pass, one global add per genome and block
//   f. AlleleLine   the text, one line per allele, kept on the device
//
// No thread walks a site, an allele or a run: a site with more alleles than a
// block has threads, or an allele with more records, is many lanes' work.
// Every sum is an integer and every atomic commutes: the result depends on
// the input alone, whatever the schedule.
#include "pg_region.h"

namespace pg {

#define VS_DIRECT 1u               // flag byte of a step: it ends a direct record (its run has a row before it)
#define VS_VIA 2u                  //                      it ends a via record (and one before that)
#define VS_PAIR 1u                 // flag byte of a sorted record: its (a, c) differs from the record before
#define VS_ALLELE 2u               //                               its (a, c, via) differs
#define VS_AG 4u                   //                               its (a, c, via, genome) differs
#define VS_CHUNK_WORDS 32          // presence words (64 genomes each) per pass of k_vs_groupsum

// ------------------------------------------------------------ the tables
struct VsSites {
  long long *from, *to;
  ull *first, *count;
  uint32_t *nal, *ngen;
  static size_t bytes(uint64_t n) { return 40 * n + 64; }
  VsSites(const DevBuf& b, uint64_t n) {
    from = b.as<long long>();
    to = from + n;
    first = reinterpret_cast<ull*>(to + n);
    count = first + n;
    nal = reinterpret_cast<uint32_t*>(count + n);
    ngen = nal + n;
  }
};
struct VsAlleles {
  ull* site;
  long long* via;
  ull *count, *lo, *hi;
  uint32_t* ngen;
  static size_t bytes(uint64_t n) { return 44 * n + 64; }
  VsAlleles(const DevBuf& b, uint64_t n) {
    site = b.as<ull>();
    via = reinterpret_cast<long long*>(site + n);
    count = reinterpret_cast<ull*>(via + n);
    lo = count + n;
    hi = lo + n;
    ngen = reinterpret_cast<uint32_t*>(hi + n);
  }
};

// ------------------------------------------------------------ b. steps and records
// uoff[i]: the used rows before row i.  sf[s]: VS_DIRECT | VS_VIA of step s
__global__ void __launch_bounds__(RG_BLOCK) k_vs_steps(const long long* __restrict__ rows, uint64_t n,
                                                       const int* __restrict__ rec_group,
                                                       const uint8_t* __restrict__ rf, const ull* __restrict__ uoff,
                                                       long long* __restrict__ slab, ull* __restrict__ slen,
                                                       uint32_t* __restrict__ sgen, uint8_t* __restrict__ sf) {
  __shared__ long long lds[RG_TILE_WORDS(false)];
  const uint64_t ntiles = (n + RG_BLOCK - 1) / RG_BLOCK;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    RgRow r;
    if (!rg_load_tile(rows, n, t, lds, r)) continue;
    const uint64_t i = t * RG_BLOCK + threadIdx.x;
    const uint32_t f = rf[i];
    if (!(f & RG_USED)) continue;
    // a used row that is no head has the used row before it in its run (so i >= 1), and that one is
    // the step before this one
    const bool direct = !(f & RG_HEAD);
    const bool via = direct && !(rf[i - 1] & RG_HEAD);
    const ull s = uoff[i];
    slab[s] = r.label;
    slen[s] = rg_len(r);
    sgen[s] = (uint32_t)rec_group[r.rec];
    sf[s] = (uint8_t)((direct ? VS_DIRECT : 0u) | (via ? VS_VIA : 0u));
  }
}
// doff[s] / voff[s]: the direct / via records before step s; the direct records come first, nd of them
__global__ void k_vs_emit(const long long* __restrict__ slab, const ull* __restrict__ slen,
                          const uint32_t* __restrict__ sgen, const uint8_t* __restrict__ sf,
                          const ull* __restrict__ doff, const ull* __restrict__ voff, uint64_t nu, ull nd, int lb,
                          int gb, ull* __restrict__ k1, ull* __restrict__ k2, ull* __restrict__ len,
                          ull* __restrict__ idx) {
  RG_LOOP(s, nu) {
    const uint32_t f = sf[s];
    if (!(f & VS_DIRECT)) continue;                        // (VS_VIA comes with VS_DIRECT; then s >= 1)
    const ull c = (ull)slab[s], g = (ull)sgen[s];
    const ull j = doff[s];
    k1[j] = g;                                             // via + 1 = 0
    k2[j] = ((ull)slab[s - 1] << lb) | c;
    len[j] = 0;
    idx[j] = j;
    if (f & VS_VIA) {                                      // (s >= 2)
      const ull v = nd + voff[s];
      k1[v] = (((ull)slab[s - 1] + 1ull) << gb) | g;
      k2[v] = ((ull)slab[s - 2] << lb) | c;
      len[v] = slen[s - 1];
      idx[v] = v;
    }
  }
}
__global__ void k_vs_gather2(const ull* __restrict__ a, const ull* __restrict__ b, const ull* __restrict__ pos,
                             uint64_t n, ull* __restrict__ da, ull* __restrict__ db) {
  RG_LOOP(j, n) {
    const ull p = pos[j];
    da[j] = a[p];
    if (b) db[j] = b[p];
  }
}

// ------------------------------------------------------------ d. pairs, alleles, sites
// K2 / K1: the records in (a, c, via, genome) order; fl[n] = 0
__global__ void k_vs_flags(const ull* __restrict__ K2, const ull* __restrict__ K1, uint64_t n, int gb,
                           uint8_t* __restrict__ fl) {
  RG_LOOP(j, n) {
    const bool pair = j == 0 || K2[j] != K2[j - 1];
    const bool allele = pair || (K1[j] >> gb) != (K1[j - 1] >> gb);
    const bool ag = allele || K1[j] != K1[j - 1];
    fl[j] = (uint8_t)((pair ? VS_PAIR : 0u) | (allele ? VS_ALLELE : 0u) | (ag ? VS_AG : 0u));
  }
}
// pnum / anum / gnum [n + 1]: the pairs / alleles / (allele, genome) heads before each record.
// ppos / pfa [np0 + 1]: a pair's first record and first allele; apos / agp [na0 + 1]: an allele's first
// record and the (allele, genome) heads before it; apair [na0]: its pair
__global__ void k_vs_heads(const uint8_t* __restrict__ fl, const ull* __restrict__ pnum,
                           const ull* __restrict__ anum, const ull* __restrict__ gnum, uint64_t n, ull np0, ull na0,
                           ull ng, ull* __restrict__ ppos, ull* __restrict__ pfa, ull* __restrict__ apos,
                           ull* __restrict__ agp, ull* __restrict__ apair) {
  RG_LOOP(j, n) {
    const uint32_t f = fl[j];
    if (f & VS_PAIR) {
      ppos[pnum[j]] = j;
      pfa[pnum[j]] = anum[j];
    }
    if (f & VS_ALLELE) {
      const ull q = anum[j];
      apos[q] = j;
      agp[q] = gnum[j];
      apair[q] = pnum[j + 1] - 1ull;
    }
    if (j == 0) {
      ppos[np0] = n;
      pfa[np0] = na0;
      apos[na0] = n;
      agp[na0] = ng;
    }
  }
}
// keep[p] / keepa[q]: the pair has two alleles or more - it is a site (keep[np0] = keepa[na0] = 0)
__global__ void k_vs_keep(const ull* __restrict__ pfa, const ull* __restrict__ apair, uint64_t np0, uint64_t na0,
                          uint8_t* __restrict__ keep, uint8_t* __restrict__ keepa) {
  RG_LOOP(i, na0) {
    const ull p = apair[i];
    keepa[i] = pfa[p + 1] - pfa[p] >= 2ull;
    if (i < np0) keep[i] = pfa[i + 1] - pfa[i] >= 2ull;   // (np0 <= na0)
  }
}
// fs[p] / fa[q]: the sites / site alleles before pair p / allele q
__global__ void k_vs_alleles(const ull* __restrict__ K1, const uint8_t* __restrict__ keepa,
                             const ull* __restrict__ fa, const ull* __restrict__ fs, const ull* __restrict__ apos,
                             const ull* __restrict__ agp, const ull* __restrict__ apair, uint64_t na0, int gb,
                             VsAlleles A) {
  RG_LOOP(q, na0) {
    if (!keepa[q]) continue;
    const ull al = fa[q], j = apos[q];
    A.site[al] = fs[apair[q]];
    A.via[al] = (long long)(K1[j] >> gb) - 1;
    A.count[al] = apos[q + 1] - j;
    A.ngen[al] = (uint32_t)(agp[q + 1] - agp[q]);
    A.lo[al] = ~0ull;
    A.hi[al] = 0ull;
  }
}
__global__ void k_vs_sites(const ull* __restrict__ K2, const uint8_t* __restrict__ keep, const ull* __restrict__ fs,
                           const ull* __restrict__ fa, const ull* __restrict__ ppos, const ull* __restrict__ pfa,
                           uint64_t np0, int lb, VsSites S) {
  RG_LOOP(p, np0) {
    if (!keep[p]) continue;
    const ull s = fs[p], j = ppos[p];
    S.from[s] = (long long)(K2[j] >> lb);
    S.to[s] = (long long)(K2[j] & ((1ull << lb) - 1ull));
    S.first[s] = fa[pfa[p]];
    S.count[s] = ppos[p + 1] - j;
    S.nal[s] = (uint32_t)(pfa[p + 1] - pfa[p]);
  }
}
// The inclusive scan of v over the lanes of a wave that share id (equal ids are adjacent lanes): the
// last lane of a segment holds op over the whole of it.  Every lane of the wave must call it.
template <class Op>
__device__ __forceinline__ ull vs_seg_scan(ull id, ull v, Op op) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const ull idn = __shfl_up(id, o), vn = __shfl_up(v, o);
    if (lane >= o && idn == id) v = op(v, vn);
  }
  return v;
}
// the lane is the last of its segment in the wave
__device__ __forceinline__ bool vs_seg_tail(ull id) {
  const ull idn = __shfl_down(id, 1);
  return (threadIdx.x & 63) == 63 || idn != id;
}
struct VsMin { __device__ ull operator()(ull a, ull b) const { return a < b ? a : b; } };
struct VsMax { __device__ ull operator()(ull a, ull b) const { return a > b ? a : b; } };
struct VsOr { __device__ ull operator()(ull a, ull b) const { return a | b; } };
#define VS_NONE (~0ull)            // the segment id of a lane that takes no part

// per record of a site: its allele's min / max length and its genome's presence bit
__global__ void __launch_bounds__(RG_BLOCK) k_vs_reduce(const ull* __restrict__ K1, const ull* __restrict__ LEN,
                                                        const ull* __restrict__ anum,
                                                        const uint8_t* __restrict__ keepa,
                                                        const ull* __restrict__ fa, uint64_t n, int gb, uint32_t W,
                                                        VsAlleles A, ull* bits) {
  // (whole blocks step together: every lane of a wave runs the scans)
  for (uint64_t base = blockIdx.x * (uint64_t)RG_BLOCK; base < n; base += (uint64_t)gridDim.x * RG_BLOCK) {
    const uint64_t j = base + threadIdx.x;
    ull al = VS_NONE, word = VS_NONE, len = 0, bit = 0;
    if (j < n) {
      const ull q = anum[j + 1] - 1ull;                    // the allele of record j
      if (keepa[q]) {
        const ull g = K1[j] & ((1ull << gb) - 1ull);
        al = fa[q];
        word = al * W + (g >> 6);                          // (genomes ascend inside an allele: a word's records are adjacent)
        bit = 1ull << (g & 63);
        len = LEN[j];
      }
    }
    const ull lo = vs_seg_scan(al, len, VsMin()), hi = vs_seg_scan(al, len, VsMax());
    const ull bb = vs_seg_scan(word, bit, VsOr());
    const bool tail_al = vs_seg_tail(al), tail_w = vs_seg_tail(word);
    if (al != VS_NONE && tail_al) {
      RG_MIN(A.lo + al, lo);
      RG_MAX(A.hi + al, hi);
    }
    if (word != VS_NONE && tail_w) RG_OR(bits + word, bb);
  }
}
// sbits[site][W] |= bits[allele][W] over the site's alleles
__global__ void __launch_bounds__(RG_BLOCK) k_vs_siteor(VsAlleles A, uint64_t na, uint32_t W,
                                                        const ull* __restrict__ bits, ull* sbits) {
  for (uint64_t base = blockIdx.x * (uint64_t)RG_BLOCK; base < na; base += (uint64_t)gridDim.x * RG_BLOCK) {
    const uint64_t al = base + threadIdx.x;
    const ull site = al < na ? A.site[al] : VS_NONE;
    const bool tail = vs_seg_tail(site);
    for (uint32_t w = 0; w < W; ++w) {
      const ull v = vs_seg_scan(site, al < na ? bits[al * W + w] : 0ull, VsOr());
      if (site != VS_NONE && tail && v) RG_OR(sbits + site * W + w, v);
    }
  }
}
__global__ void k_vs_sitegen(VsSites S, uint64_t ns, uint32_t W, const ull* __restrict__ sbits) {
  RG_LOOP(s, ns) {
    uint32_t g = 0;
    for (uint32_t w = 0; w < W; ++w) g += (uint32_t)__popcll(sbits[s * W + w]);
    S.ngen[s] = g;
  }
}

// ------------------------------------------------------------ e. per genome
// out[g] += the entries of bits [n][W] with bit g set (only: those with only[e] == 1).  A block counts
// VS_CHUNK_WORDS words' genomes in LDS at a time (blockIdx.y and on: the chunks) and adds what it found.
__global__ void __launch_bounds__(RG_BLOCK) k_vs_groupsum(const ull* __restrict__ bits, uint64_t n, uint32_t W,
                                                          const uint32_t* __restrict__ only, uint32_t G, ull* out) {
  __shared__ uint32_t h[64 * VS_CHUNK_WORDS];
  const uint32_t nchunks = (W + VS_CHUNK_WORDS - 1) / VS_CHUNK_WORDS;
  for (uint32_t ch = blockIdx.y; ch < nchunks; ch += gridDim.y) {
    const uint32_t w0 = ch * VS_CHUNK_WORDS, w1 = W - w0 < VS_CHUNK_WORDS ? W : w0 + VS_CHUNK_WORDS;
    __syncthreads();                                       // (the previous chunk's readers are done)
    for (uint32_t i = threadIdx.x; i < 64 * VS_CHUNK_WORDS; i += RG_BLOCK) h[i] = 0;
    __syncthreads();
    RG_LOOP(e, n) {
      if (only && only[e] != 1u) continue;
      for (uint32_t w = w0; w < w1; ++w) {
        ull v = bits[e * W + w];
        while (v) {
          const uint32_t b = (uint32_t)__ffsll((long long)v) - 1u;
          v &= v - 1ull;
          atomicAdd(&h[(w - w0) * 64 + b], 1u);
        }
      }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 64 * VS_CHUNK_WORDS; i += RG_BLOCK) {
      const uint64_t g = (uint64_t)w0 * 64 + i;
      if (h[i] && g < G) RG_ADD(out + g, (ull)h[i]);
    }
  }
}

// ------------------------------------------------------------ f. text
#define VS_HEADER "#from\tto\tvia\tcount\tgenomes\tmin\tmax\n"

// <from> <to> <via or *> <count> <genomes> <min> <max>, tab separated
struct AlleleLine {
  VsSites S;
  VsAlleles A;
  template <class T>
  __device__ __forceinline__ void operator()(T& s, uint64_t i) const {
    const ull site = A.site[i];
    s.dec((ull)S.from[site]); s.ch('\t');
    s.dec((ull)S.to[site]); s.ch('\t');
    if (A.via[i] < 0) s.ch('*'); else s.dec((ull)A.via[i]);
    s.ch('\t');
    s.dec(A.count[i]); s.ch('\t');
    s.dec(A.ngen[i]); s.ch('\t');
    s.dec(A.lo[i]); s.ch('\t');
    s.dec(A.hi[i]); s.ch('\n');
  }
};

void region_sites(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                  uint32_t G, uint64_t* n_sites, uint64_t* n_alleles, uint64_t* n_records_emitted,
                  uint64_t* n_skipped) {
  // ---- arguments: everything refused here leaves the previous result in place
  const RowInput in = row_input(c, "pg_region_sites", h_rows5, n_rows, rec_group, n_records, G, false);
  const uint64_t n = in.n;

  // ---- a. the flags and the largest label, found before anything is allocated or replaced
  DevBuf rf;
  rf.reserve(n + 16);
  const RowScan sc = row_scan(c, "pg_region_sites", in, rf.as<uint8_t>(), nullptr);
  const uint64_t L = sc.L, nu = sc.used;
  const int lb = bits_for(L ? L - 1 : 0);                  // a label; a pair key a << lb | c has at most 62 bits
  const int vb = bits_for(L);                              // via + 1
  const int gb = bits_for(G ? G - 1 : 0);                  // a genome: k1 = (via + 1) << gb | genome, at most 64 bits
  const uint32_t W = (G + 63) / 64;

  DevBuf sites, alleles, bits, grp, toff, text;
  uint64_t nd = 0, nv = 0, nrec = 0, ns = 0, na = 0;
  // the records in (a, c, via, genome) order and what the tables are filled from; they live to the end of
  // the call, the buffers of the steps and of the sorts only inside their blocks
  DevBuf K1, K2, LEN, fl, pnum, anum, gnum, ppos, apos, apair, keep, keepa, fs, fa;
  if (nu) {
    // ---- b. the steps and their records
    DevBuf uoff, steps, sf, doff, voff, k1, k2, len, idx, idx1;
    uoff.reserve(8 * (n + 1));
    if (scan_bit(c, rf.as<uint8_t>(), RG_USED, uoff.as<ull>(), n) != nu)
      throw Error(-5, "pg_region_sites: the scan disagrees with the row pass");
    steps.reserve(20 * nu + 64);
    long long* slab = steps.as<long long>();
    ull* slen = reinterpret_cast<ull*>(slab + nu);
    uint32_t* sgen = reinterpret_cast<uint32_t*>(slen + nu);
    sf.reserve(nu + 16);
    PG_HIP(hipMemsetAsync(sf.as<uint8_t>() + nu, 0, 1, c.stream));
    RG_LAUNCH(k_vs_steps, in.grid_rows, in.rows, n, in.group, rf.as<uint8_t>(), uoff.as<ull>(), slab, slen, sgen,
              sf.as<uint8_t>());
    doff.reserve(8 * (nu + 1));
    voff.reserve(8 * (nu + 1));
    nd = scan_bit(c, sf.as<uint8_t>(), VS_DIRECT, doff.as<ull>(), nu);
    nv = scan_bit(c, sf.as<uint8_t>(), VS_VIA, voff.as<ull>(), nu);
    if (nd >= nu || nv > nd) throw Error(-5, "pg_region_sites: the scans disagree with the row pass");
    nrec = nd + nv;
    if (nrec) {
      k1.reserve(8 * nrec);
      k2.reserve(8 * nrec);
      len.reserve(8 * nrec);
      idx.reserve(8 * nrec);
      RG_LAUNCH(k_vs_emit, grid_for(nu, RG_BLOCK, 8192), slab, slen, sgen, sf.as<uint8_t>(), doff.as<ull>(),
                voff.as<ull>(), nu, (ull)nd, lb, gb, k1.as<ull>(), k2.as<ull>(), len.as<ull>(), idx.as<ull>());
      // ---- c. (a, c, via, genome) order: stable sorts by k1, then by k2
      K1.reserve(8 * nrec);                                // (first the sorted k1 that nobody reads, then k2 gathered)
      K2.reserve(8 * nrec);
      LEN.reserve(8 * nrec);
      idx1.reserve(8 * nrec);
      const unsigned grid = grid_for(nrec, RG_BLOCK, 8192);
      sort_pairs(c, k1.as<ull>(), K1.as<ull>(), idx.as<ull>(), idx1.as<ull>(), nrec, vb + gb);
      RG_LAUNCH(k_vs_gather2, grid, k2.as<ull>(), (const ull*)nullptr, idx1.as<ull>(), nrec, K1.as<ull>(),
                (ull*)nullptr);
      sort_pairs(c, K1.as<ull>(), K2.as<ull>(), idx1.as<ull>(), idx.as<ull>(), nrec, 2 * lb);
      RG_LAUNCH(k_vs_gather2, grid, k1.as<ull>(), len.as<ull>(), idx.as<ull>(), nrec, K1.as<ull>(), LEN.as<ull>());
    }
  }
  uint64_t np0 = 0, na0 = 0, ng = 0;
  if (nrec) {
    // ---- d. pairs, alleles and (allele, genome) heads; the pairs with two alleles or more
    const unsigned grid = grid_for(nrec, RG_BLOCK, 8192);
    fl.reserve(nrec + 16);
    pnum.reserve(8 * (nrec + 1));
    anum.reserve(8 * (nrec + 1));
    gnum.reserve(8 * (nrec + 1));
    PG_HIP(hipMemsetAsync(fl.as<uint8_t>() + nrec, 0, 1, c.stream));
    RG_LAUNCH(k_vs_flags, grid, K2.as<ull>(), K1.as<ull>(), nrec, gb, fl.as<uint8_t>());
    np0 = scan_bit(c, fl.as<uint8_t>(), VS_PAIR, pnum.as<ull>(), nrec);
    na0 = scan_bit(c, fl.as<uint8_t>(), VS_ALLELE, anum.as<ull>(), nrec);
    ng = scan_bit(c, fl.as<uint8_t>(), VS_AG, gnum.as<ull>(), nrec);
    if (!np0 || np0 > na0 || na0 > ng || ng > nrec)
      throw Error(-5, "pg_region_sites: the scans disagree with the sorted records");
    ppos.reserve(16 * (np0 + 1));
    apos.reserve(16 * (na0 + 1));
    apair.reserve(8 * (na0 + 1));
    ull *d_ppos = ppos.as<ull>(), *d_pfa = d_ppos + np0 + 1, *d_apos = apos.as<ull>(), *d_agp = d_apos + na0 + 1;
    RG_LAUNCH(k_vs_heads, grid, fl.as<uint8_t>(), pnum.as<ull>(), anum.as<ull>(), gnum.as<ull>(), nrec, (ull)np0,
              (ull)na0, (ull)ng, d_ppos, d_pfa, d_apos, d_agp, apair.as<ull>());
    keep.reserve(np0 + 16);
    keepa.reserve(na0 + 16);
    fs.reserve(8 * (np0 + 1));
    fa.reserve(8 * (na0 + 1));
    PG_HIP(hipMemsetAsync(keep.as<uint8_t>() + np0, 0, 1, c.stream));
    PG_HIP(hipMemsetAsync(keepa.as<uint8_t>() + na0, 0, 1, c.stream));
    RG_LAUNCH(k_vs_keep, grid_for(na0, RG_BLOCK, 8192), d_pfa, apair.as<ull>(), np0, na0, keep.as<uint8_t>(),
              keepa.as<uint8_t>());
    ns = scan_bit(c, keep.as<uint8_t>(), 1u, fs.as<ull>(), np0);
    na = scan_bit(c, keepa.as<uint8_t>(), 1u, fa.as<ull>(), na0);
    if (na < 2 * ns) throw Error(-5, "pg_region_sites: a site with fewer than two alleles");
  }
  // ---- the tables
  sites.reserve(VsSites::bytes(ns));
  alleles.reserve(VsAlleles::bytes(na));
  bits.reserve(8 * ((size_t)na + (size_t)ns) * W + 64);    // the alleles' words, then (scratch) the sites'
  grp.reserve(24 * (size_t)G + 64);
  VsSites S(sites, ns);
  VsAlleles A(alleles, na);
  ull *d_bits = bits.as<ull>(), *d_sbits = d_bits + (size_t)na * W, *d_grp = grp.as<ull>();
  PG_HIP(hipMemsetAsync(grp.p, 0, 24 * (size_t)G + 64, c.stream));
  if (ns) {
    PG_HIP(hipMemsetAsync(bits.p, 0, 8 * ((size_t)na + (size_t)ns) * W, c.stream));
    const ull *d_ppos = ppos.as<ull>(), *d_pfa = d_ppos + np0 + 1, *d_apos = apos.as<ull>(),
              *d_agp = d_apos + na0 + 1;
    RG_LAUNCH(k_vs_alleles, grid_for(na0, RG_BLOCK, 8192), K1.as<ull>(), keepa.as<uint8_t>(), fa.as<ull>(),
              fs.as<ull>(), d_apos, d_agp, apair.as<ull>(), na0, gb, A);
    RG_LAUNCH(k_vs_sites, grid_for(np0, RG_BLOCK, 8192), K2.as<ull>(), keep.as<uint8_t>(), fs.as<ull>(),
              fa.as<ull>(), d_ppos, d_pfa, np0, lb, S);
    RG_LAUNCH(k_vs_reduce, grid_for(nrec, RG_BLOCK, 8192), K1.as<ull>(), LEN.as<ull>(), anum.as<ull>(),
              keepa.as<uint8_t>(), fa.as<ull>(), nrec, gb, W, A, d_bits);
    RG_LAUNCH(k_vs_siteor, grid_for(na, RG_BLOCK, 8192), A, na, W, d_bits, d_sbits);
    RG_LAUNCH(k_vs_sitegen, grid_for(ns, RG_BLOCK, 8192), S, ns, W, d_sbits);
    // ---- e. per genome: the sites it is in, its alleles, the alleles that are its alone
    const unsigned chunks = std::min(1024u, (W + VS_CHUNK_WORDS - 1) / VS_CHUNK_WORDS);
    RG_LAUNCH(k_vs_groupsum, dim3(grid_for(ns, RG_BLOCK, 1024), chunks), d_sbits, ns, W, (const uint32_t*)nullptr, G,
              d_grp);
    RG_LAUNCH(k_vs_groupsum, dim3(grid_for(na, RG_BLOCK, 1024), chunks), d_bits, na, W, (const uint32_t*)nullptr, G,
              d_grp + G);
    RG_LAUNCH(k_vs_groupsum, dim3(grid_for(na, RG_BLOCK, 1024), chunks), d_bits, na, W, A.ngen, G, d_grp + 2 * (size_t)G);
  }
  // ---- f. the text: the header, then one line per allele
  const size_t hdr = sizeof(VS_HEADER) - 1;
  const AlleleLine line{S, A};
  const uint64_t body = text_measure(c, line, na, toff);
  text.reserve(hdr + body + 16);
  PG_HIP(hipMemcpyAsync(text.p, VS_HEADER, hdr, hipMemcpyHostToDevice, c.stream));
  text_write(c, line, na, toff, text.as<char>() + hdr);
  c.sync();
  // ---- the new result replaces the previous one
  c.vs_sites.swap(sites);
  c.vs_alleles.swap(alleles);
  c.vs_bits.swap(bits);
  c.vs_grp.swap(grp);
  c.vs_text.swap(text);
  c.vs_ns = ns;
  c.vs_na = na;
  c.vs_total = hdr + body;
  c.vs_groups = G;
  c.vs_words = W;
  c.vs_ready = true;
  if (n_sites) *n_sites = ns;
  if (n_alleles) *n_alleles = na;
  if (n_records_emitted) *n_records_emitted = nrec;
  if (n_skipped) *n_skipped = sc.skipped;
}

void region_sites_table(Ctx& c, int64_t* from, int64_t* to, uint32_t* n_alleles, uint64_t* first, uint64_t* count,
                        uint32_t* n_genomes, uint64_t cap) {
  need(c.vs_ready, "pg_region_sites_table", NEED_SITES);
  const uint64_t ns = c.vs_ns;
  if (cap < ns) throw Error(-34, "pg_region_sites_table: buffer too small");
  if (!ns) return;
  VsSites S(c.vs_sites, ns);
  get(c, from, S.from, 8 * ns);
  get(c, to, S.to, 8 * ns);
  get(c, n_alleles, S.nal, 4 * ns);
  get(c, first, S.first, 8 * ns);
  get(c, count, S.count, 8 * ns);
  get(c, n_genomes, S.ngen, 4 * ns);
  c.sync();
}

void region_sites_alleles(Ctx& c, uint64_t* site, int64_t* via, uint64_t* count, uint32_t* n_genomes,
                          uint64_t* min_len, uint64_t* max_len, uint64_t* bits, uint64_t cap) {
  need(c.vs_ready, "pg_region_sites_alleles", NEED_SITES);
  const uint64_t na = c.vs_na;
  if (cap < na) throw Error(-34, "pg_region_sites_alleles: buffer too small");
  if (!na) return;
  VsAlleles A(c.vs_alleles, na);
  get(c, site, A.site, 8 * na);
  get(c, via, A.via, 8 * na);
  get(c, count, A.count, 8 * na);
  get(c, n_genomes, A.ngen, 4 * na);
  get(c, min_len, A.lo, 8 * na);
  get(c, max_len, A.hi, 8 * na);
  get(c, bits, c.vs_bits.p, 8 * na * c.vs_words);
  c.sync();
}

void region_sites_groups(Ctx& c, uint64_t* sites, uint64_t* alleles, uint64_t* private_, uint64_t cap) {
  need(c.vs_ready, "pg_region_sites_groups", NEED_SITES);
  const uint64_t G = c.vs_groups;
  if (cap < G) throw Error(-34, "pg_region_sites_groups: buffer too small");
  if (!G) return;
  const ull* g = c.vs_grp.as<ull>();
  get(c, sites, g, 8 * G);
  get(c, alleles, g + G, 8 * G);
  get(c, private_, g + 2 * G, 8 * G);
  c.sync();
}

// the alleles' text of the last region_sites: its size (out null, fd < 0), copied into out, or written to fd
uint64_t format_region_sites(Ctx& c, char* out, uint64_t cap, int fd) {
  need(c.vs_ready, fd >= 0 ? "pg_region_sites_format_fd" : "pg_region_sites_format", NEED_SITES);
  return text_out(c, c.vs_text.p, c.vs_total, out, cap, fd, "pg_region_sites_format", "pg_region_sites_format_fd");
}

}  // namespace pg
