// pg_bubbles.hip — the variable sites between anchor regions: where the
// genomes differ, however many regions the difference spans.  An anchor is a
// label carried by min_genomes genomes or more; inside a run two anchor steps
// with no anchor step between them bound a segment with flanks (a, c) and an
// inner path, the labels between them (possibly none).  An allele of a flank
// pair is a distinct inner path, a site a flank pair with two alleles or more.
//
// Rows, rec_group, the rule for a used row and the run are pg_region_graph's
// (pg_region.hip); the steps are pg_region_sites' (k_vs_steps, pg_steps.h).
// Nothing here is dense in the label: device memory follows the rows, the
// segments and the alleles.
//
// Steps, each its own launch on c.stream (no hand-shake inside a kernel):
//   a. k_row_scan   the shared front end: a flag byte per row; one scan of the
//                   used bit gives every used row its step index
//      k_vs_steps   the used rows compacted to steps (label, length, genome,
//                   run head); a select of the used rows' indices gives every
//                   step its row
//   b. anchors      the keys label << gb | genome of the steps in a stable
//                   radix sort with the steps' indices; k_bb_lgflags marks where
//                   the label and where (label, genome) change, two scans number
//                   the labels and count the changes: a label's genomes are the
//                   changes between two label heads.  k_bb_anchor gives every
//                   step its anchor bit through the sorted index.
//   c. segments     two max scans: the last anchor step and the last run head
//                   at or before every step.  An anchor step that is no head and
//                   whose previous anchor step is not before its run's head
//                   closes a segment (k_bb_close); a scan of the closing bit
//                   numbers the segments.  bp comes from a prefix sum of the
//                   lengths.
//   d. the hash     a step is the map h -> h * B + (label + 1) mod 2^61 - 1,
//                   an anchor step or a run head the map h -> 0; one scan
//                   composes the maps (two bases at once), so the step before a
//                   closing one holds the hash of the inner path.  The hash is a
//                   fixed function of the labels.  No thread walks a segment.
//   e. the order    stable radix sorts of (key word, index), last word first:
//                   the two hash words, regions, (a, c).  A stable sort keeps
//                   segments with equal words in closing order, which is row
//                   order: the first segment of a group is its earliest.
//   f. k_bb_flags   per sorted segment: a new pair, a new group (regions or a
//                   hash word differs); k_bb_verify compares every inner label
//                   of every segment with its group's first segment, one thread
//                   per inner step - a mismatch ends the call with -5.  A pair
//                   with two groups or more is a site.  The groups are sorted
//                   by (pair, first row) and the kept ones numbered: the alleles.
//   g. k_bb_alleles / k_bb_sites fill the tables from the heads;
//      k_bb_reduce  count is the distance between two heads; min / max bp and
//                   the presence bits by a segmented scan inside the wave and
//                   one atomic per segment of lanes; k_bb_siteor the OR of a
//                   site's alleles the same way; k_vs_groupsum the per-genome
//                   sums
//   h. k_bb_inner   the inner array, one thread per inner label
//   i. BubbleLine   the text, one thread per token: an allele's line is its
//                   head (from, to), one item per inner label and its tail
//
// Device bytes while the call runs, beside the tables: 9 per row; per used row
// 29 for the steps and their rows, 33 more while the anchors are found, then
// 65 for the scans and the maps; per segment 168 while they are sorted, then
// 89, and at most 99 more per group of any pair.  The tables: 40 + 8 W per
// site, 60 + 8 W per allele (and 8 of scratch), 8 per inner label, 12 per
// label for the anchors; the text's offsets 8 per inner label and 16 per
// allele.
//
// Every sum is an integer and every atomic commutes: the result depends on
// the input alone, whatever the schedule.
#include "pg_bubbles.h"
#include "pg_steps.h"

namespace pg {

#define BB_ANCHOR 1u               // flag byte of a step: its label is an anchor
#define BB_CLOSE 2u                //                      it closes a segment
#define BB_LAB 1u                  // flag byte of a sorted (label, genome) key: its label differs from the key before
#define BB_LG 2u                   //                                            its (label, genome) differs
#define BB_PAIR 1u                 // flag byte of a sorted segment: its (a, c) differs from the segment before
#define BB_GROUP 2u                //                                its (a, c), regions or hash differs
#define BB_P61 ((1ull << 61) - 1ull)
#define BB_BASE1 0x0123456789ABCDEFull   // (both below 2^61 - 1)
#define BB_BASE2 0x0FEDCBA987654321ull
#define BB_GS_WORDS 32             // presence words a k_vs_groupsum block takes per chunk
#define BB_NONE (~0ull)            // the segment id of a lane that takes no part

// the segments' columns (n + 1 entries each), in closing order or sorted
struct BbSegs {
  ull *ac, *reg, *h1, *h2, *gen, *bp, *frow, *ist;
  static size_t bytes(uint64_t n) { return 64 * (n + 1) + 64; }
  BbSegs(const DevBuf& b, uint64_t n) {
    ac = b.as<ull>();
    reg = ac + n + 1;
    h1 = reg + n + 1;
    h2 = h1 + n + 1;
    gen = h2 + n + 1;
    bp = gen + n + 1;
    frow = bp + n + 1;
    ist = frow + n + 1;
  }
};

// ------------------------------------------------------------ b. anchors
__global__ void k_bb_lgkeys(const long long* __restrict__ slab, const uint32_t* __restrict__ sgen, uint64_t nu, int gb,
                            ull* __restrict__ key, ull* __restrict__ idx) {
  RG_LOOP(s, nu) {
    key[s] = ((ull)slab[s] << gb) | (ull)sgen[s];
    idx[s] = s;
  }
}
__global__ void k_bb_lgflags(const ull* __restrict__ K, uint64_t nu, int gb, uint8_t* __restrict__ fl) {
  RG_LOOP(j, nu) {
    const bool lab = j == 0 || (K[j] >> gb) != (K[j - 1] >> gb);
    const bool lg = lab || K[j] != K[j - 1];
    fl[j] = (uint8_t)((lab ? BB_LAB : 0u) | (lg ? BB_LG : 0u));
  }
}
// lnum / gnum [nu + 1]: the label / (label, genome) heads before each key.  lpos / lgp [nlab + 1]: a
// label's first key and the (label, genome) heads before it
__global__ void k_bb_labheads(const uint8_t* __restrict__ fl, const ull* __restrict__ lnum,
                              const ull* __restrict__ gnum, uint64_t nu, ull nlab, ull nlg, ull* __restrict__ lpos,
                              ull* __restrict__ lgp) {
  RG_LOOP(j, nu) {
    if (fl[j] & BB_LAB) {
      lpos[lnum[j]] = j;
      lgp[lnum[j]] = gnum[j];
    }
    if (j == 0) {
      lpos[nlab] = nu;
      lgp[nlab] = nlg;
    }
  }
}
// per label: its genomes, and whether min_genomes of them make it an anchor (keep[nlab] = 0)
__global__ void k_bb_labels(const ull* __restrict__ K, const ull* __restrict__ lpos, const ull* __restrict__ lgp,
                            uint64_t nlab, int gb, uint32_t min_genomes, long long* __restrict__ label,
                            uint32_t* __restrict__ ngen, uint8_t* __restrict__ keep) {
  RG_LOOP(l, nlab) {
    const uint32_t g = (uint32_t)(lgp[l + 1] - lgp[l]);
    label[l] = (long long)(K[lpos[l]] >> gb);
    ngen[l] = g;
    keep[l] = g >= min_genomes;
  }
}
// I[j]: the step of sorted key j.  sfl[s] = BB_ANCHOR or 0
__global__ void k_bb_anchor(const ull* __restrict__ I, const ull* __restrict__ lnum, const uint8_t* __restrict__ keep,
                            uint64_t nu, uint8_t* __restrict__ sfl) {
  RG_LOOP(j, nu) sfl[I[j]] = keep[lnum[j + 1] - 1ull] ? (uint8_t)BB_ANCHOR : (uint8_t)0;
}

// ------------------------------------------------------------ c. segments, d. the hash
// One step as a map of the hash of the labels since the last anchor step or run head, for two bases:
// h -> h * m + a (mod 2^61 - 1).  An anchor step and a run head are h -> 0.
struct BbMap {
  ull m1, a1, m2, a2;
};
__host__ __device__ __forceinline__ ull bb_mul(ull a, ull b) {
  const unsigned __int128 p = (unsigned __int128)a * b;
  const ull r = (ull)(p & BB_P61) + (ull)(p >> 61);
  return r >= BB_P61 ? r - BB_P61 : r;
}
__host__ __device__ __forceinline__ ull bb_add(ull a, ull b) {
  const ull r = a + b;
  return r >= BB_P61 ? r - BB_P61 : r;
}
// f, then g
struct BbCompose {
  __host__ __device__ __forceinline__ BbMap operator()(const BbMap& f, const BbMap& g) const {
    return BbMap{bb_mul(f.m1, g.m1), bb_add(bb_mul(f.a1, g.m1), g.a1), bb_mul(f.m2, g.m2),
                 bb_add(bb_mul(f.a2, g.m2), g.a2)};
  }
};
// pa[s] / rh[s]: s + 1 if the step is an anchor / a run head, else 0; map[s]: the step's map
__global__ void k_bb_marks(const long long* __restrict__ slab, const uint8_t* __restrict__ sf,
                           const uint8_t* __restrict__ sfl, uint64_t nu, ull* __restrict__ pa, ull* __restrict__ rh,
                           BbMap* __restrict__ map) {
  RG_LOOP(s, nu) {
    const bool anchor = sfl[s] & BB_ANCHOR, head = !(sf[s] & ST_FOLLOWS);
    pa[s] = anchor ? s + 1 : 0;
    rh[s] = head ? s + 1 : 0;
    const ull x = (ull)slab[s] + 1ull;
    map[s] = anchor || head ? BbMap{0, 0, 0, 0} : BbMap{BB_BASE1, x, BB_BASE2, x};
  }
}
// pa / rh scanned: 1 + the last anchor step / run head at or before each step (0: none).  The anchor
// step s that is no head has the step s - 1 in its run; the anchor before it is in its run iff it is not
// before the run's head.
__global__ void k_bb_close(const uint8_t* __restrict__ sf, const ull* __restrict__ pa, const ull* __restrict__ rh,
                           uint64_t nu, uint8_t* __restrict__ sfl) {
  RG_LOOP(s, nu) {
    const uint32_t f = sfl[s];
    if ((f & BB_ANCHOR) && (sf[s] & ST_FOLLOWS) && pa[s - 1] >= rh[s]) sfl[s] = (uint8_t)(f | BB_CLOSE);
  }
}
// cnum[s]: the closing steps before s; lp[s]: the lengths of the steps before s; srow[s]: the step's row
__global__ void k_bb_segs(const long long* __restrict__ slab, const uint32_t* __restrict__ sgen,
                          const ull* __restrict__ srow, const uint8_t* __restrict__ sfl, const ull* __restrict__ cnum,
                          const ull* __restrict__ pa, const ull* __restrict__ lp, const BbMap* __restrict__ map,
                          uint64_t nu, int lb, ull mask1, ull mask2, BbSegs U, ull* __restrict__ idx) {
  RG_LOOP(s, nu) {
    if (!(sfl[s] & BB_CLOSE)) continue;                    // (then s >= 1 and pa[s - 1] >= 1)
    const ull t = cnum[s], p = pa[s - 1] - 1ull;
    U.ac[t] = ((ull)slab[p] << lb) | (ull)slab[s];
    U.reg[t] = s - p - 1ull;
    U.h1[t] = map[s - 1].a1 & mask1;                       // (no inner step: s - 1 is the anchor, whose map is 0)
    U.h2[t] = map[s - 1].a2 & mask2;
    U.gen[t] = sgen[s];
    U.bp[t] = lp[s] - lp[p + 1];
    U.frow[t] = srow[p];
    U.ist[t] = p + 1ull;
    idx[t] = t;
  }
}
__global__ void k_bb_gather(BbSegs U, const ull* __restrict__ ord, uint64_t n, BbSegs S) {
  RG_LOOP(j, n) {
    const ull t = ord[j];
    S.ac[j] = U.ac[t]; S.reg[j] = U.reg[t]; S.h1[j] = U.h1[t]; S.h2[j] = U.h2[t];
    S.gen[j] = U.gen[t]; S.bp[j] = U.bp[t]; S.frow[j] = U.frow[t]; S.ist[j] = U.ist[t];
  }
}

// ------------------------------------------------------------ f. pairs, groups, alleles
__global__ void k_bb_flags(BbSegs S, uint64_t n, uint8_t* __restrict__ fl) {
  RG_LOOP(j, n) {
    const bool pair = j == 0 || S.ac[j] != S.ac[j - 1];
    const bool group = pair || S.reg[j] != S.reg[j - 1] || S.h1[j] != S.h1[j - 1] || S.h2[j] != S.h2[j - 1];
    fl[j] = (uint8_t)((pair ? BB_PAIR : 0u) | (group ? BB_GROUP : 0u));
  }
}
// pnum / anum [n + 1]: the pair / group heads before each segment.  ppos / pfa [np0 + 1]: a pair's first
// segment and first group; apos [na0 + 1]: a group's first segment; apair [na0]: its pair
__global__ void k_bb_heads(const uint8_t* __restrict__ fl, const ull* __restrict__ pnum, const ull* __restrict__ anum,
                           uint64_t n, ull np0, ull na0, ull* __restrict__ ppos, ull* __restrict__ pfa,
                           ull* __restrict__ apos, ull* __restrict__ apair) {
  RG_LOOP(j, n) {
    const uint32_t f = fl[j];
    if (f & BB_PAIR) {
      ppos[pnum[j]] = j;
      pfa[pnum[j]] = anum[j];
    }
    if (f & BB_GROUP) {
      apos[anum[j]] = j;
      apair[anum[j]] = pnum[j + 1] - 1ull;
    }
    if (j == 0) {
      ppos[np0] = n;
      pfa[np0] = na0;
      apos[na0] = n;
    }
  }
}
// ioff[j]: the inner steps of the segments before j.  Inner step i of all: its segment's label against
// the same position of its group's first segment (equal regions: the position exists there)
__global__ void k_bb_verify(BbSegs S, const ull* __restrict__ ioff, const ull* __restrict__ anum,
                            const ull* __restrict__ apos, const long long* __restrict__ slab, uint64_t n, uint64_t total,
                            ull* bad) {
  RG_LOOP(i, total) {
    const uint64_t j = bb_find(ioff, n, 0, i);
    const ull h = apos[anum[j + 1] - 1ull], k = i - ioff[j];
    if (h != j && slab[S.ist[j] + k] != slab[S.ist[h] + k]) RG_OR(bad, 1ull);
  }
}
// keep[p] / keepa[q]: the pair has two groups or more - it is a site (keep[np0] = 0); gkey[q]: the
// group's first row, gidx[q] = q
__global__ void k_bb_keep(BbSegs S, const ull* __restrict__ pfa, const ull* __restrict__ apos,
                          const ull* __restrict__ apair, uint64_t np0, uint64_t na0, uint8_t* __restrict__ keep,
                          uint8_t* __restrict__ keepa, ull* __restrict__ gkey, ull* __restrict__ gidx) {
  RG_LOOP(i, na0) {
    const ull p = apair[i];
    keepa[i] = pfa[p + 1] - pfa[p] >= 2ull;
    gkey[i] = S.frow[apos[i]];
    gidx[i] = i;
    if (i < np0) keep[i] = pfa[i + 1] - pfa[i] >= 2ull;   // (np0 <= na0)
  }
}
// gord[r]: the groups in (pair, first row) order; keepr[r]: group gord[r] is kept (keepr[na0] = 0)
__global__ void k_bb_keepr(const ull* __restrict__ gord, const uint8_t* __restrict__ keepa, uint64_t na0,
                           uint8_t* __restrict__ keepr) {
  RG_LOOP(r, na0) keepr[r] = keepa[gord[r]];
}
// fs[p]: the sites before pair p; fa[r]: the alleles before position r of gord.  fin[q]: the allele of
// a kept group; aist[al]: the first inner step of the allele's first segment
__global__ void k_bb_alleles(BbSegs S, const ull* __restrict__ gord, const uint8_t* __restrict__ keepr,
                             const ull* __restrict__ fa, const ull* __restrict__ fs, const ull* __restrict__ apos,
                             const ull* __restrict__ apair, uint64_t na0, BbAlleles A, ull* __restrict__ fin,
                             ull* __restrict__ aist) {
  RG_LOOP(r, na0) {
    if (!keepr[r]) continue;
    const ull q = gord[r], al = fa[r], j = apos[q];
    A.site[al] = fs[apair[q]];
    A.regions[al] = S.reg[j];
    A.frow[al] = S.frow[j];
    A.count[al] = apos[q + 1] - j;
    A.lo[al] = ~0ull;
    A.hi[al] = 0ull;
    aist[al] = S.ist[j];
    fin[q] = al;
  }
}
// (the groups of a pair take the same positions in gord as in hash order: pfa[p] is its first there too)
__global__ void k_bb_sites(BbSegs S, const uint8_t* __restrict__ keep, const ull* __restrict__ fs,
                           const ull* __restrict__ fa, const ull* __restrict__ ppos, const ull* __restrict__ pfa,
                           uint64_t np0, int lb, BbSites T) {
  RG_LOOP(p, np0) {
    if (!keep[p]) continue;
    const ull s = fs[p], j = ppos[p];
    T.from[s] = (long long)(S.ac[j] >> lb);
    T.to[s] = (long long)(S.ac[j] & ((1ull << lb) - 1ull));
    T.first[s] = fa[pfa[p]];
    T.count[s] = ppos[p + 1] - j;
    T.nal[s] = (uint32_t)(pfa[p + 1] - pfa[p]);
  }
}

// ------------------------------------------------------------ g. reductions
// The inclusive scan of v over the lanes of a wave that share id (equal ids on adjacent lanes): the
// last lane of such a stretch holds op over the whole of it.  Every lane of the wave must call it.
template <class Op>
__device__ __forceinline__ ull bb_seg_scan(ull id, ull v, Op op) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const ull idn = __shfl_up(id, o), vn = __shfl_up(v, o);
    if (lane >= o && idn == id) v = op(v, vn);
  }
  return v;
}
__device__ __forceinline__ bool bb_seg_tail(ull id) {
  const ull idn = __shfl_down(id, 1);
  return (threadIdx.x & 63) == 63 || idn != id;
}
struct BbMin { __device__ ull operator()(ull a, ull b) const { return a < b ? a : b; } };
struct BbMax { __device__ ull operator()(ull a, ull b) const { return a > b ? a : b; } };
struct BbOr { __device__ ull operator()(ull a, ull b) const { return a | b; } };

// per sorted segment of a site: its allele's min / max bp and its genome's presence bit.  The segments
// of an allele are adjacent lanes; its genomes come in row order, so a presence word may take more
// than one atomic per wave
__global__ void __launch_bounds__(RG_BLOCK) k_bb_reduce(BbSegs S, const ull* __restrict__ anum,
                                                        const uint8_t* __restrict__ keepa,
                                                        const ull* __restrict__ fin, uint64_t n, uint32_t W,
                                                        BbAlleles A, ull* bits) {
  // (whole blocks step together: every lane of a wave runs the scans)
  for (uint64_t base = blockIdx.x * (uint64_t)RG_BLOCK; base < n; base += (uint64_t)gridDim.x * RG_BLOCK) {
    const uint64_t j = base + threadIdx.x;
    ull al = BB_NONE, word = BB_NONE, bp = 0, bit = 0;
    if (j < n) {
      const ull q = anum[j + 1] - 1ull;                    // the group of segment j
      if (keepa[q]) {
        const ull g = S.gen[j];
        al = fin[q];
        word = al * W + (g >> 6);
        bit = 1ull << (g & 63);
        bp = S.bp[j];
      }
    }
    const ull lo = bb_seg_scan(al, bp, BbMin()), hi = bb_seg_scan(al, bp, BbMax());
    const ull bb = bb_seg_scan(word, bit, BbOr());
    const bool tail_al = bb_seg_tail(al), tail_w = bb_seg_tail(word);
    if (al != BB_NONE && tail_al) {
      RG_MIN(A.lo + al, lo);
      RG_MAX(A.hi + al, hi);
    }
    if (word != BB_NONE && tail_w) RG_OR(bits + word, bb);
  }
}
// sbits[site][W] |= bits[allele][W] over the site's alleles (adjacent lanes); ngen of the allele
__global__ void __launch_bounds__(RG_BLOCK) k_bb_siteor(BbAlleles A, uint64_t na, uint32_t W,
                                                        const ull* __restrict__ bits, ull* sbits) {
  for (uint64_t base = blockIdx.x * (uint64_t)RG_BLOCK; base < na; base += (uint64_t)gridDim.x * RG_BLOCK) {
    const uint64_t al = base + threadIdx.x;
    const ull site = al < na ? A.site[al] : BB_NONE;
    const bool tail = bb_seg_tail(site);
    uint32_t g = 0;
    for (uint32_t w = 0; w < W; ++w) {
      const ull mine = al < na ? bits[al * W + w] : 0ull;
      g += (uint32_t)__popcll(mine);
      const ull v = bb_seg_scan(site, mine, BbOr());
      if (site != BB_NONE && tail && v) RG_OR(sbits + site * W + w, v);
    }
    if (al < na) A.ngen[al] = g;
  }
}
__global__ void k_bb_sitegen(BbSites T, uint64_t ns, uint32_t W, const ull* __restrict__ sbits) {
  RG_LOOP(s, ns) {
    uint32_t g = 0;
    for (uint32_t w = 0; w < W; ++w) g += (uint32_t)__popcll(sbits[s * W + w]);
    T.ngen[s] = g;
  }
}

// ------------------------------------------------------------ h. the inner array
__global__ void k_bb_inner(BbAlleles A, uint64_t na, const ull* __restrict__ aist, const long long* __restrict__ slab,
                           uint64_t total, long long* __restrict__ inner) {
  RG_LOOP(i, total) {
    const uint64_t al = bb_find(A.ioff, na, 0, i);
    inner[i] = slab[aist[al] + (i - A.ioff[al])];
  }
}

// ------------------------------------------------------------ i. text
#define BB_HEADER "#from\tto\tinner\tregions\tcount\tgenomes\tmin\tmax\n"

// <from> <to> <inner labels joined by , or *> <regions> <count> <genomes> <min> <max>, tab separated.
// Allele al takes the items ioff[al] + 2 al and on: its head (from, to, and `*` for no inner label), one
// item per inner label, its tail (the five counts).  No thread writes an inner path.
struct BubbleLine {
  BbSites T;
  BbAlleles A;
  const long long* inner;
  uint64_t na;
  template <class Sink>
  __device__ __forceinline__ void operator()(Sink& s, uint64_t i) const {
    const uint64_t al = bb_find(A.ioff, na, 2, i);
    const ull k = i - (A.ioff[al] + 2ull * al), r = A.regions[al];
    if (k == 0) {
      const ull site = A.site[al];
      s.dec((ull)T.from[site]); s.ch('\t');
      s.dec((ull)T.to[site]); s.ch('\t');
      if (!r) s.ch('*');
    } else if (k <= r) {
      s.dec((ull)inner[A.ioff[al] + k - 1ull]);
      if (k < r) s.ch(',');
    } else {
      s.ch('\t'); s.dec(r); s.ch('\t');
      s.dec(A.count[al]); s.ch('\t');
      s.dec(A.ngen[al]); s.ch('\t');
      s.dec(A.lo[al]); s.ch('\t');
      s.dec(A.hi[al]); s.ch('\n');
    }
  }
};

// in place: v[i] = max(v[0 .. i])
static void scan_max(Ctx& c, ull* v, uint64_t n) {
  with_temp(c, [&](void* tmp, size_t& bytes) {
    return rocprim::inclusive_scan(tmp, bytes, v, v, (size_t)n, rocprim::maximum<ull>(), c.stream);
  });
}
// One pass of the order, last word first: ord (null: the identity, idx) stably sorted by word[ord[.]]
// over `bits` bits into ord2; returns with ord the new order
static void sort_by(Ctx& c, const ull* word, uint64_t n, int bits, const ull* idx, DevBuf& ord, DevBuf& ord2,
                    DevBuf& kin, DevBuf& kout, bool& first) {
  if (first) {
    sort_pairs(c, word, kout.as<ull>(), idx, ord2.as<ull>(), n, bits);
  } else {
    hipLaunchKernelGGL(k_gather_key, dim3(grid_for(n, RG_BLOCK, 8192)), dim3(RG_BLOCK), 0, c.stream, word,
                       ord.as<ull>(), n, kin.as<ull>());
    PG_HIP(hipGetLastError());
    sort_pairs(c, kin.as<ull>(), kout.as<ull>(), ord.as<ull>(), ord2.as<ull>(), n, bits);
  }
  ord.swap(ord2);
  first = false;
}

void region_bubbles(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                    uint32_t G, uint32_t min_genomes, uint64_t* n_anchors, uint64_t* n_segments, uint64_t* n_sites,
                    uint64_t* n_alleles, uint64_t* n_skipped) {
  // ---- arguments: everything refused here leaves the previous result in place
  if (min_genomes < 1 || (G && min_genomes > G))
    throw Error(-22, "pg_region_bubbles: min_genomes = " + std::to_string(min_genomes) + " is outside [1, " +
                         std::to_string(G) + "]");
  const RowInput in = row_input(c, "pg_region_bubbles", h_rows5, n_rows, rec_group, n_records, G, false);
  const uint64_t n = in.n;

  // ---- a. the flags and the largest label, found before anything is allocated or replaced
  DevBuf rf;
  rf.reserve(n + 16);
  const RowScan sc = row_scan(c, "pg_region_bubbles", in, rf.as<uint8_t>(), nullptr);
  const uint64_t L = sc.L, nu = sc.used;
  const int lb = bits_for(L ? L - 1 : 0);                  // a label: at most 31 bits
  const int gb = bits_for(G ? G - 1 : 0);                  // a genome: label << gb | genome has at most 63 bits
  const uint32_t W = (G + 63) / 64;
  const ull mask1 = c.bb_hash_bits ? (1ull << c.bb_hash_bits) - 1ull : ~0ull, mask2 = c.bb_hash_bits ? 0ull : ~0ull;

  DevBuf sites, alleles, bits, inner, grp, anchors, toff, text;
  uint64_t nanc = 0, nseg = 0, ns = 0, na = 0, nin = 0;
  // what the tables are filled from lives to the end of the call, the rest inside its block
  DevBuf steps, sf, sorted, fl, pnum, anum, ppos, apos, apair, keep, keepa, keepr, gord, fs, fa, fin, aist;
  uint64_t np0 = 0, na0 = 0;
  long long* slab = nullptr;
  if (nu) {
    // ---- a. the steps and their rows
    DevBuf uoff, cnt, sfl, key, idx, K, I, lgf, lnum, gnum, lpos, lab, labkeep;
    uoff.reserve(8 * (n + 1));
    if (scan_bit(c, rf.as<uint8_t>(), RG_USED, uoff.as<ull>(), n) != nu)
      throw Error(-5, "pg_region_bubbles: the scan disagrees with the row pass");
    steps.reserve(28 * nu + 64);
    slab = steps.as<long long>();
    ull *slen = reinterpret_cast<ull*>(slab + nu), *srow = slen + nu;
    uint32_t* sgen = reinterpret_cast<uint32_t*>(srow + nu);
    sf.reserve(nu + 16);
    RG_LAUNCH(k_vs_steps, in.grid_rows, in.rows, n, in.group, rf.as<uint8_t>(), uoff.as<ull>(), slab, slen, sgen,
              sf.as<uint8_t>());
    // (a used row's flag byte is not 0: the used rows' indices, in order)
    if (select_flagged(c, rocprim::counting_iterator<ull>(0), rf.as<uint8_t>(), srow, n, cnt) != nu)
      throw Error(-5, "pg_region_bubbles: the select disagrees with the row pass");
    uoff.release();
    // ---- b. the anchors: (label, genome) order, a label's genomes, every step's anchor bit
    const unsigned gu = grid_for(nu, RG_BLOCK, 8192);
    key.reserve(8 * nu);
    idx.reserve(8 * nu);
    K.reserve(8 * nu);
    I.reserve(8 * nu);
    RG_LAUNCH(k_bb_lgkeys, gu, slab, sgen, nu, gb, key.as<ull>(), idx.as<ull>());
    sort_pairs(c, key.as<ull>(), K.as<ull>(), idx.as<ull>(), I.as<ull>(), nu, lb + gb);
    key.release();
    idx.release();
    lgf.reserve(nu + 16);
    lnum.reserve(8 * (nu + 1));
    gnum.reserve(8 * (nu + 1));
    PG_HIP(hipMemsetAsync(lgf.as<uint8_t>() + nu, 0, 1, c.stream));
    RG_LAUNCH(k_bb_lgflags, gu, K.as<ull>(), nu, gb, lgf.as<uint8_t>());
    const uint64_t nlab = scan_bit(c, lgf.as<uint8_t>(), BB_LAB, lnum.as<ull>(), nu);
    const uint64_t nlg = scan_bit(c, lgf.as<uint8_t>(), BB_LG, gnum.as<ull>(), nu);
    if (!nlab || nlab > nlg || nlg > nu) throw Error(-5, "pg_region_bubbles: the scans disagree with the sorted keys");
    lpos.reserve(16 * (nlab + 1));
    lab.reserve(12 * nlab + 64);
    labkeep.reserve(nlab + 16);
    ull *d_lpos = lpos.as<ull>(), *d_lgp = d_lpos + nlab + 1;
    long long* d_lab = lab.as<long long>();
    uint32_t* d_labg = reinterpret_cast<uint32_t*>(d_lab + nlab);
    RG_LAUNCH(k_bb_labheads, gu, lgf.as<uint8_t>(), lnum.as<ull>(), gnum.as<ull>(), nu, (ull)nlab, (ull)nlg, d_lpos,
              d_lgp);
    PG_HIP(hipMemsetAsync(labkeep.as<uint8_t>() + nlab, 0, 1, c.stream));
    RG_LAUNCH(k_bb_labels, grid_for(nlab, RG_BLOCK, 8192), K.as<ull>(), d_lpos, d_lgp, nlab, gb, min_genomes, d_lab,
              d_labg, labkeep.as<uint8_t>());
    anchors.reserve(12 * nlab + 64);                       // (sized by the labels: the anchors are not yet counted)
    nanc = select_flagged(c, d_lab, labkeep.as<uint8_t>(), anchors.as<long long>(), nlab, cnt);
    if (nanc) {
      // (the columns of the table lie at the anchors' count: the genomes after the labels)
      if (select_flagged(c, d_labg, labkeep.as<uint8_t>(), reinterpret_cast<uint32_t*>(anchors.as<long long>() + nanc),
                         nlab, cnt) != nanc)
        throw Error(-5, "pg_region_bubbles: the selects disagree");
    }
    sfl.reserve(nu + 16);
    PG_HIP(hipMemsetAsync(sfl.as<uint8_t>() + nu, 0, 1, c.stream));
    RG_LAUNCH(k_bb_anchor, gu, I.as<ull>(), lnum.as<ull>(), labkeep.as<uint8_t>(), nu, sfl.as<uint8_t>());
    K.release(); I.release(); lgf.release(); lnum.release(); gnum.release(); lpos.release(); lab.release();
    if (nanc) {
      // ---- c. the segments, d. the hash of their inner paths
      DevBuf pa, rh, lp, map, cnum;
      pa.reserve(8 * nu);
      rh.reserve(8 * nu);
      lp.reserve(8 * nu);
      map.reserve(sizeof(BbMap) * nu);
      cnum.reserve(8 * (nu + 1));
      RG_LAUNCH(k_bb_marks, gu, slab, sf.as<uint8_t>(), sfl.as<uint8_t>(), nu, pa.as<ull>(), rh.as<ull>(),
                map.as<BbMap>());
      scan_max(c, pa.as<ull>(), nu);
      scan_max(c, rh.as<ull>(), nu);
      RG_LAUNCH(k_bb_close, gu, sf.as<uint8_t>(), pa.as<ull>(), rh.as<ull>(), nu, sfl.as<uint8_t>());
      nseg = scan_bit(c, sfl.as<uint8_t>(), BB_CLOSE, cnum.as<ull>(), nu);
      if (nseg >= nu) throw Error(-5, "pg_region_bubbles: more segments than steps");
      if (nseg) {
        with_temp(c, [&](void* tmp, size_t& bytes) {
          return rocprim::exclusive_scan(tmp, bytes, slen, lp.as<ull>(), 0ull, (size_t)nu, rocprim::plus<ull>(),
                                         c.stream);
        });
        with_temp(c, [&](void* tmp, size_t& bytes) {
          return rocprim::inclusive_scan(tmp, bytes, map.as<BbMap>(), map.as<BbMap>(), (size_t)nu, BbCompose(),
                                         c.stream);
        });
        DevBuf unsorted, ord, ord2, kin, kout;
        unsorted.reserve(BbSegs::bytes(nseg));
        idx.reserve(8 * nseg);
        BbSegs U(unsorted, nseg);
        RG_LAUNCH(k_bb_segs, gu, slab, sgen, srow, sfl.as<uint8_t>(), cnum.as<ull>(), pa.as<ull>(), lp.as<ull>(),
                  map.as<BbMap>(), nu, lb, mask1, mask2, U, idx.as<ull>());
        pa.release(); rh.release(); lp.release(); map.release(); cnum.release();
        // ---- e. (a, c, regions, hash) order: stable sorts, the last word first
        ord.reserve(8 * nseg);
        ord2.reserve(8 * nseg);
        kin.reserve(8 * nseg);
        kout.reserve(8 * nseg);
        bool first = true;
        if (mask2) sort_by(c, U.h2, nseg, 61, idx.as<ull>(), ord, ord2, kin, kout, first);
        sort_by(c, U.h1, nseg, c.bb_hash_bits ? c.bb_hash_bits : 61, idx.as<ull>(), ord, ord2, kin, kout, first);
        sort_by(c, U.reg, nseg, bits_for(nu), idx.as<ull>(), ord, ord2, kin, kout, first);
        sort_by(c, U.ac, nseg, 2 * lb, idx.as<ull>(), ord, ord2, kin, kout, first);
        sorted.reserve(BbSegs::bytes(nseg));
        RG_LAUNCH(k_bb_gather, grid_for(nseg, RG_BLOCK, 8192), U, ord.as<ull>(), nseg, BbSegs(sorted, nseg));
      }
    }
  }
  if (nseg) {
    // ---- f. pairs and groups; every segment verified against its group's first; the pairs with two groups
    const BbSegs S(sorted, nseg);
    const unsigned grid = grid_for(nseg, RG_BLOCK, 8192);
    DevBuf ioff, bad, gkey, gidx, gk2, gi2;
    fl.reserve(nseg + 16);
    pnum.reserve(8 * (nseg + 1));
    anum.reserve(8 * (nseg + 1));
    PG_HIP(hipMemsetAsync(fl.as<uint8_t>() + nseg, 0, 1, c.stream));
    RG_LAUNCH(k_bb_flags, grid, S, nseg, fl.as<uint8_t>());
    np0 = scan_bit(c, fl.as<uint8_t>(), BB_PAIR, pnum.as<ull>(), nseg);
    na0 = scan_bit(c, fl.as<uint8_t>(), BB_GROUP, anum.as<ull>(), nseg);
    if (!np0 || np0 > na0 || na0 > nseg) throw Error(-5, "pg_region_bubbles: the scans disagree with the sorted segments");
    ppos.reserve(16 * (np0 + 1));
    apos.reserve(8 * (na0 + 1));
    apair.reserve(8 * (na0 + 1));
    ull *d_ppos = ppos.as<ull>(), *d_pfa = d_ppos + np0 + 1;
    RG_LAUNCH(k_bb_heads, grid, fl.as<uint8_t>(), pnum.as<ull>(), anum.as<ull>(), nseg, (ull)np0, (ull)na0, d_ppos,
              d_pfa, apos.as<ull>(), apair.as<ull>());
    ioff.reserve(8 * (nseg + 1));
    const uint64_t inner_steps = excl_scan_total(c, S.reg, ioff.as<ull>(), nseg);
    if (inner_steps > nu) throw Error(-5, "pg_region_bubbles: more inner steps than steps");
    if (inner_steps) {
      bad.reserve(16);
      PG_HIP(hipMemsetAsync(bad.p, 0, 8, c.stream));
      RG_LAUNCH(k_bb_verify, grid_for(inner_steps, RG_BLOCK, 8192), S, ioff.as<ull>(), anum.as<ull>(), apos.as<ull>(),
                slab, nseg, inner_steps, bad.as<ull>());
      ull h = 0;
      PG_HIP(hipMemcpyAsync(&h, bad.p, 8, hipMemcpyDeviceToHost, c.stream));
      c.sync();
      if (h)
        throw Error(-5, "pg_region_bubbles: two inner paths of one flank pair share their length and their hash (" +
                            std::string(c.bb_hash_bits ? "PG_TUNE_BUBBLE_HASH_BITS keeps " +
                                                             std::to_string(c.bb_hash_bits) + " bits"
                                                       : "the full hash") +
                            ")");
    }
    ioff.release();
    keep.reserve(np0 + 16);
    keepa.reserve(na0 + 16);
    keepr.reserve(na0 + 16);
    gkey.reserve(8 * na0);
    gidx.reserve(8 * na0);
    gk2.reserve(8 * na0);
    gi2.reserve(8 * na0);
    gord.reserve(8 * na0);
    fs.reserve(8 * (np0 + 1));
    fa.reserve(8 * (na0 + 1));
    PG_HIP(hipMemsetAsync(keep.as<uint8_t>() + np0, 0, 1, c.stream));
    PG_HIP(hipMemsetAsync(keepr.as<uint8_t>() + na0, 0, 1, c.stream));
    RG_LAUNCH(k_bb_keep, grid_for(na0, RG_BLOCK, 8192), S, d_pfa, apos.as<ull>(), apair.as<ull>(), np0, na0,
              keep.as<uint8_t>(), keepa.as<uint8_t>(), gkey.as<ull>(), gidx.as<ull>());
    // the groups by (pair, first row): by first row, then stably by pair
    sort_pairs(c, gkey.as<ull>(), gk2.as<ull>(), gidx.as<ull>(), gi2.as<ull>(), na0, bits_for(n ? n - 1 : 0));
    hipLaunchKernelGGL(k_gather_key, dim3(grid_for(na0, RG_BLOCK, 8192)), dim3(RG_BLOCK), 0, c.stream,
                       apair.as<ull>(), gi2.as<ull>(), na0, gkey.as<ull>());
    PG_HIP(hipGetLastError());
    sort_pairs(c, gkey.as<ull>(), gk2.as<ull>(), gi2.as<ull>(), gord.as<ull>(), na0, bits_for(np0 - 1));
    RG_LAUNCH(k_bb_keepr, grid_for(na0, RG_BLOCK, 8192), gord.as<ull>(), keepa.as<uint8_t>(), na0,
              keepr.as<uint8_t>());
    ns = scan_bit(c, keep.as<uint8_t>(), 1u, fs.as<ull>(), np0);
    na = scan_bit(c, keepr.as<uint8_t>(), 1u, fa.as<ull>(), na0);
    if (na < 2 * ns) throw Error(-5, "pg_region_bubbles: a site with fewer than two alleles");
  }
  // ---- the tables
  sites.reserve(BbSites::bytes(ns));
  alleles.reserve(BbAlleles::bytes(na));
  bits.reserve(8 * ((size_t)na + (size_t)ns) * W + 64);    // the alleles' words, then (scratch) the sites'
  grp.reserve(24 * (size_t)G + 64);
  anchors.reserve(64);
  BbSites T(sites, ns);
  BbAlleles A(alleles, na);
  ull *d_bits = bits.as<ull>(), *d_sbits = d_bits + (size_t)na * W, *d_grp = grp.as<ull>();
  PG_HIP(hipMemsetAsync(grp.p, 0, 24 * (size_t)G + 64, c.stream));
  if (ns) {
    // ---- g. the tables from the heads, the reductions, the per-genome sums
    const BbSegs S(sorted, nseg);
    const ull *d_ppos = ppos.as<ull>(), *d_pfa = d_ppos + np0 + 1;
    fin.reserve(8 * na0);
    aist.reserve(8 * na);
    PG_HIP(hipMemsetAsync(bits.p, 0, 8 * ((size_t)na + (size_t)ns) * W, c.stream));
    RG_LAUNCH(k_bb_alleles, grid_for(na0, RG_BLOCK, 8192), S, gord.as<ull>(), keepr.as<uint8_t>(), fa.as<ull>(),
              fs.as<ull>(), apos.as<ull>(), apair.as<ull>(), na0, A, fin.as<ull>(), aist.as<ull>());
    RG_LAUNCH(k_bb_sites, grid_for(np0, RG_BLOCK, 8192), S, keep.as<uint8_t>(), fs.as<ull>(), fa.as<ull>(), d_ppos,
              d_pfa, np0, lb, T);
    RG_LAUNCH(k_bb_reduce, grid_for(nseg, RG_BLOCK, 8192), S, anum.as<ull>(), keepa.as<uint8_t>(), fin.as<ull>(), nseg,
              W, A, d_bits);
    RG_LAUNCH(k_bb_siteor, grid_for(na, RG_BLOCK, 8192), A, na, W, d_bits, d_sbits);
    RG_LAUNCH(k_bb_sitegen, grid_for(ns, RG_BLOCK, 8192), T, ns, W, d_sbits);
    const unsigned chunks = std::min(1024u, (W + BB_GS_WORDS - 1) / BB_GS_WORDS);
    RG_LAUNCH(k_vs_groupsum, dim3(grid_for(ns, RG_BLOCK, 1024), chunks), d_sbits, ns, W, (const uint32_t*)nullptr, G,
              d_grp);
    RG_LAUNCH(k_vs_groupsum, dim3(grid_for(na, RG_BLOCK, 1024), chunks), d_bits, na, W, (const uint32_t*)nullptr, G,
              d_grp + G);
    RG_LAUNCH(k_vs_groupsum, dim3(grid_for(na, RG_BLOCK, 1024), chunks), d_bits, na, W, A.ngen, G,
              d_grp + 2 * (size_t)G);
    // ---- h. the inner array
    nin = excl_scan_total(c, A.regions, A.ioff, na);
    inner.reserve(8 * nin + 64);
    if (nin)
      RG_LAUNCH(k_bb_inner, grid_for(nin, RG_BLOCK, 8192), A, na, aist.as<ull>(), slab, nin, inner.as<long long>());
  } else {
    inner.reserve(64);
  }
  // ---- i. the text: the header, then per allele its head, its inner labels and its tail
  const size_t hdr = sizeof(BB_HEADER) - 1;
  const BubbleLine line{T, A, inner.as<long long>(), na};
  const uint64_t body = text_measure(c, line, nin + 2 * na, toff);
  text.reserve(hdr + body + 16);
  PG_HIP(hipMemcpyAsync(text.p, BB_HEADER, hdr, hipMemcpyHostToDevice, c.stream));
  text_write(c, line, nin + 2 * na, toff, text.as<char>() + hdr);
  c.sync();
  // ---- the new result replaces the previous one
  c.bb_sites.swap(sites);
  c.bb_alleles.swap(alleles);
  c.bb_bits.swap(bits);
  c.bb_inner.swap(inner);
  c.bb_grp.swap(grp);
  c.bb_anchors.swap(anchors);
  c.bb_text.swap(text);
  c.bb_ns = ns;
  c.bb_na = na;
  c.bb_nin = nin;
  c.bb_nanc = nanc;
  c.bb_total = hdr + body;
  c.bb_groups = G;
  c.bb_words = W;
  c.bb_ready = true;
  c.vr_ready = false;                                      // (the variants described the old tables)
  c.al_ready = false;                                      // (and so did their alignments)
  if (n_anchors) *n_anchors = nanc;
  if (n_segments) *n_segments = nseg;
  if (n_sites) *n_sites = ns;
  if (n_alleles) *n_alleles = na;
  if (n_skipped) *n_skipped = sc.skipped;
}

void region_bubbles_table(Ctx& c, int64_t* from, int64_t* to, uint32_t* n_alleles, uint64_t* first, uint64_t* count,
                          uint32_t* n_genomes, uint64_t cap) {
  need(c.bb_ready, "pg_region_bubbles_table", NEED_BUBBLES);
  const uint64_t ns = c.bb_ns;
  if (cap < ns) throw Error(-34, "pg_region_bubbles_table: buffer too small");
  if (!ns) return;
  BbSites T(c.bb_sites, ns);
  get(c, from, T.from, 8 * ns);
  get(c, to, T.to, 8 * ns);
  get(c, n_alleles, T.nal, 4 * ns);
  get(c, first, T.first, 8 * ns);
  get(c, count, T.count, 8 * ns);
  get(c, n_genomes, T.ngen, 4 * ns);
  c.sync();
}

void region_bubbles_alleles(Ctx& c, uint64_t* site, uint64_t* regions, uint64_t* first_row, uint64_t* count,
                            uint32_t* n_genomes, uint64_t* min_bp, uint64_t* max_bp, uint64_t* inner_off,
                            uint64_t* bits, uint64_t cap) {
  need(c.bb_ready, "pg_region_bubbles_alleles", NEED_BUBBLES);
  const uint64_t na = c.bb_na;
  if (cap < na) throw Error(-34, "pg_region_bubbles_alleles: buffer too small");
  if (!na) return;
  BbAlleles A(c.bb_alleles, na);
  get(c, site, A.site, 8 * na);
  get(c, regions, A.regions, 8 * na);
  get(c, first_row, A.frow, 8 * na);
  get(c, count, A.count, 8 * na);
  get(c, n_genomes, A.ngen, 4 * na);
  get(c, min_bp, A.lo, 8 * na);
  get(c, max_bp, A.hi, 8 * na);
  get(c, inner_off, A.ioff, 8 * na);
  get(c, bits, c.bb_bits.p, 8 * na * c.bb_words);
  c.sync();
}

uint64_t region_bubbles_inner(Ctx& c, int64_t* inner, uint64_t cap) {
  need(c.bb_ready, "pg_region_bubbles_inner", NEED_BUBBLES);
  const uint64_t nin = c.bb_nin;
  if (!inner) return nin;
  if (cap < nin) throw Error(-34, "pg_region_bubbles_inner: buffer too small");
  get(c, inner, c.bb_inner.p, 8 * nin);
  c.sync();
  return nin;
}

void region_bubbles_groups(Ctx& c, uint64_t* sites, uint64_t* alleles, uint64_t* private_, uint64_t cap) {
  need(c.bb_ready, "pg_region_bubbles_groups", NEED_BUBBLES);
  const uint64_t G = c.bb_groups;
  if (cap < G) throw Error(-34, "pg_region_bubbles_groups: buffer too small");
  if (!G) return;
  const ull* g = c.bb_grp.as<ull>();
  get(c, sites, g, 8 * G);
  get(c, alleles, g + G, 8 * G);
  get(c, private_, g + 2 * G, 8 * G);
  c.sync();
}

void region_bubbles_anchors(Ctx& c, int64_t* label, uint32_t* n_genomes, uint64_t cap) {
  need(c.bb_ready, "pg_region_bubbles_anchors", NEED_BUBBLES);
  const uint64_t nanc = c.bb_nanc;
  if (cap < nanc) throw Error(-34, "pg_region_bubbles_anchors: buffer too small");
  if (!nanc) return;
  const long long* l = c.bb_anchors.as<long long>();
  get(c, label, l, 8 * nanc);
  get(c, n_genomes, l + nanc, 4 * nanc);
  c.sync();
}

// the alleles' text of the last region_bubbles: its size (out null, fd < 0), copied into out, or written to fd
uint64_t format_region_bubbles(Ctx& c, char* out, uint64_t cap, int fd) {
  need(c.bb_ready, fd >= 0 ? "pg_region_bubbles_format_fd" : "pg_region_bubbles_format", NEED_BUBBLES);
  return text_out(c, c.bb_text.p, c.bb_total, out, cap, fd, "pg_region_bubbles_format",
                  "pg_region_bubbles_format_fd");
}

}  // namespace pg
