// pg_align.hip — every allele of the bubbles aligned against its site's
// reference: unit-cost global alignment with a fixed tie rule, the CIGARs, the
// primitive differences and, for the placed sites, the primitives merged into
// the lines of a VCF.  pg_region_variants says what the alleles read; this
// pass says where two of them differ.  include/pangenome.h has the definition.
//
// The letters are pg_region_variants' (c.vr_blob: every entry starts at a
// multiple of 16, a placed site's REF one byte later, behind its padding
// base); the sites, the alleles and their presence bits are the bubbles'.
//
// Steps, each its own launch on c.stream (no hand-shake inside a kernel):
//   a. k_al_pairs   one thread per allele: its pair, or none for the skipped one
//   b. k_al_trim    one wave per pair: the common suffix, then the prefix, 64
//                   letters a round and a ballot; the core's sizes, the status,
//                   the words a fill needs and the bound of its runs
//   c. the host orders the pairs with a core by cells, largest first, and cuts
//      the list into batches whose direction bits fit the scratch budget
//   d. k_al_fill    one wave per pair, the hot path: 64-row strips, lane l owns
//                   row 64 strip + l + 1 and at step s computes column s - l +
//                   1.  Left is its own last value, up lane l - 1's last value
//                   (one cross-lane move), the diagonal the up of the step
//                   before.  The query letter travels down the lanes the same
//                   way.  Lane 0 takes its up values and letters, and lane 63
//                   leaves its row, through registers that the wave loads and
//                   stores 64 columns at a time (the row buffer, b + 1 int32;
//                   strip 0 reads D[0][j] = j from nowhere); the stores run 62
//                   columns behind the loads, so one buffer serves in place.
//                   Each lane packs 16 two-bit choices into a word and stores
//                   it into the row-major bit matrix (ceil(b / 16) words a row)
//   e. k_al_trace   one lane per pair follows the bits from (a, b) and writes
//                   its runs backwards into the pair's bound; the sums come
//                   from the same walk, and D[a][b] of the fill must equal them
//   d'. PG_TUNE_ALIGN_BAND: the pairs above the cap, in rounds at the thresholds t0,
//      2 t0, 4 t0, ...: k_al_fill_band is k_al_fill over the cells with |j - i|
//      <= t alone, a strip's column window instead of its whole rows, and the
//      walk back (k_al_trace<true>) takes a pair whose D[a][b] is within t -
//      exactly what the whole matrix gives - and leaves the others to 2 t
//   f. k_al_count, two scans, k_al_emit: the exact run and primitive arrays
//   g. lines: the placed sites' primitives selected, their letters hashed,
//      stable radix sorts by (site, tpos, type, tlen, qlen, hash), boundary
//      flags, every member's letters against its group head's (PG_EDEVICE if
//      they differ), the groups sorted into the VCF's order, carrier words
//   h. the texts through pg_text.h: one thread per pair; one per line's head
//      and one per GT cell
//
// Every sum is an integer and no result depends on an atomic's order: the
// result depends on the input alone, whatever the schedule or the batching.
#include "pg_bubbles.h"
#include "pg_seqdec.h"
#include "pg_text.h"

#include <numeric>

namespace pg {

#define AL_NONE (~0ull)
#define AL_WAVES (RG_BLOCK / 64)   // pairs per block of the wave-per-pair kernels
#define AL_BAD_BOUND 1ull          // what a kernel found wrong: more runs than a pair's bound
#define AL_BAD_DIST 2ull           //   the walk's sums are not the fill's D[a][b]
#define AL_BAD_HASH 4ull           //   equal keys and hashes, unequal letters
#define AL_SNV 0u
#define AL_DEL 1u
#define AL_INS 2u
#define AL_REPL 3u
#define AL_INF (1 << 30)           // a cell outside the band: it never wins, and + 1 does not overflow
#define AL_BAND_MOST (1ull << 30)  // a + b of a band candidate stays below it: every value inside the band is below AL_INF

// the pair table's columns, n + 1 entries each (the scans take one more); the first 17 are exported
// (toff, qoff: where T and Q start in the blob)
struct AlPairs {
  ull *site, *allele, *placed, *tlen, *qlen, *prefix, *suffix, *status, *dist, *neq, *nsub, *nins, *ndel, *opoff,
      *nops, *primoff, *nprims, *toff, *qoff;
  static size_t bytes(uint64_t n) { return 19 * 8 * (n + 1) + 64; }
  AlPairs(const DevBuf& b, uint64_t n) {
    ull** col = &site;
    for (int k = 0; k < 19; ++k) col[k] = b.as<ull>() + (size_t)k * (n + 1);
  }
  const ull* column(int k) const { return (&site)[k]; }      // (the members are the columns in order)
};
static_assert(sizeof(AlPairs) == 19 * sizeof(ull*), "AlPairs: the columns one after another");
struct AlPrims {
  ull *pair, *tpos, *qpos, *tlen, *qlen;
  uint8_t* type;
  static size_t bytes(uint64_t n) { return 41 * (n + 1) + 64; }
  AlPrims(const DevBuf& b, uint64_t n) {
    pair = b.as<ull>();
    tpos = pair + n + 1;
    qpos = tpos + n + 1;
    tlen = qpos + n + 1;
    qlen = tlen + n + 1;
    type = reinterpret_cast<uint8_t*>(qlen + n + 1);
  }
};
struct AlLines {
  ull *site, *pos, *tpos, *tlen, *qlen, *first, *ac, *mstart, *rec, *place;
  uint32_t* ngen;
  uint8_t* type;
  static size_t bytes(uint64_t n) { return 85 * (n + 1) + 64; }
  AlLines(const DevBuf& b, uint64_t n) {
    site = b.as<ull>();
    pos = site + n + 1;
    tpos = pos + n + 1;
    tlen = tpos + n + 1;
    qlen = tlen + n + 1;
    first = qlen + n + 1;
    ac = first + n + 1;
    mstart = ac + n + 1;
    rec = mstart + n + 1;
    place = rec + n + 1;
    ngen = reinterpret_cast<uint32_t*>(place + n + 1);
    type = reinterpret_cast<uint8_t*>(ngen + n + 1);
  }
};

// ------------------------------------------------------------ a. the pairs
__global__ void k_al_site(VrPlaced P, uint64_t np, ull* __restrict__ pl) {
  RG_LOOP(p, np) pl[P.site[p]] = p;
}
// pl[s]: site s's entry of the placed table, all ones if it has none
__global__ void k_al_pairs(BbSites T, BbAlleles A, RsTab V, VrPlaced P, const ull* __restrict__ pl, uint64_t na,
                           AlPairs R) {
  RG_LOOP(al, na) {
    const ull s = A.site[al], first = T.first[s], k = al - first, p = pl[s];
    const bool placed = p != AL_NONE;
    const ull skip = placed ? (ull)P.refal[p] : 0ull;
    if (k == skip) continue;
    const ull j = al - s - (k > skip ? 1ull : 0ull);
    R.site[j] = s;
    R.allele[j] = k;
    R.placed[j] = placed;
    R.tlen[j] = placed ? P.len[p] : V.len[first];
    R.toff[j] = placed ? V.poff[na + p] + 1ull : V.poff[first];
    R.qlen[j] = V.len[al];
    R.qoff[j] = V.poff[al];
  }
}

// ------------------------------------------------------------ b. trimming
// need[j]: the 32-bit words pair j's fill takes (0: no fill - not aligned, or an empty core);
// bound[j]: the most runs its core can have; cells[j]: a x b if it is filled.  band: a pair above the cap with
// an empty core side is aligned as it stands, and one with two sides (a candidate of the band form) gets its bound
__global__ void __launch_bounds__(RG_BLOCK) k_al_trim(const char* __restrict__ blob, AlPairs R, uint64_t n, ull cap,
                                                      int band, ull* __restrict__ need, ull* __restrict__ bound,
                                                      ull* __restrict__ cells) {
  const unsigned l = threadIdx.x & 63u;
  for (uint64_t j = blockIdx.x * (uint64_t)AL_WAVES + (threadIdx.x >> 6); j < n; j += (uint64_t)gridDim.x * AL_WAVES) {
    const char *t = blob + R.toff[j], *u = blob + R.qoff[j];
    const ull nn = R.tlen[j], m = R.qlen[j];
    ull lim = nn < m ? nn : m, q = 0, p = 0;
    while (q < lim) {
      const ull k = q + l;
      const ull diff = __ballot(k >= lim || t[nn - 1ull - k] != u[m - 1ull - k]);
      if (diff) {
        q += (ull)(__ffsll((long long)diff) - 1);
        break;
      }
      q += 64ull;
    }
    lim -= q;
    while (p < lim) {
      const ull k = p + l;
      const ull diff = __ballot(k >= lim || t[k] != u[k]);
      if (diff) {
        p += (ull)(__ffsll((long long)diff) - 1);
        break;
      }
      p += 64ull;
    }
    if (l == 0) {
      const ull a = nn - p - q, b = m - p - q;
      const bool over = a + 1ull > cap / (b + 1ull);       // (a + 1)(b + 1) > cap, without the product
      const bool core = !over && a && b, cand = band && over && a && b && a + b < AL_BAND_MOST;
      R.prefix[j] = p;
      R.suffix[j] = q;
      R.status[j] = over && !(band && (!a || !b));
      need[j] = core ? a * ((b + 15ull) >> 4) + b + 1ull : 0ull;
      cells[j] = core ? a * b : 0ull;
      const ull mn = a < b ? a : b;
      bound[j] = core || cand ? (a + b < 2ull * mn + 1ull ? a + b : 2ull * mn + 1ull) : 0ull;
    }
  }
}

// ------------------------------------------------------------ d. the fill
// batch entry w: pair order[w], its bit matrix and row buffer at scratch + moff[w]; fdist[pair] = D[a][b]
__global__ void __launch_bounds__(RG_BLOCK) k_al_fill(const char* __restrict__ blob, AlPairs R,
                                                      const ull* __restrict__ order, const ull* __restrict__ moff,
                                                      uint64_t nb, uint32_t* __restrict__ scratch,
                                                      ull* __restrict__ fdist) {
  const int l = (int)(threadIdx.x & 63u);
  const uint64_t w = blockIdx.x * (uint64_t)AL_WAVES + (threadIdx.x >> 6);
  if (w >= nb) return;                                     // (a whole wave)
  const ull j = order[w], p = R.prefix[j];
  const int a = (int)(R.tlen[j] - p - R.suffix[j]), b = (int)(R.qlen[j] - p - R.suffix[j]);
  const unsigned char* t = reinterpret_cast<const unsigned char*>(blob) + R.toff[j] + p;
  const unsigned char* u = reinterpret_cast<const unsigned char*>(blob) + R.qoff[j] + p;
  const int stride = (b + 15) >> 4;
  uint32_t* M = scratch + moff[w];
  int* row = reinterpret_cast<int*>(M + (size_t)a * stride);
  const int steps = (b + 63 + 63) & ~63;                   // lane 63's last column, rounded up to whole loads
  for (int st = 0; st * 64 < a; ++st) {
    const int i = st * 64 + l + 1;
    const bool mine = i <= a, leave = st * 64 + 64 <= a;   // lane 63 has a row: the next strip reads it
    const int tc = mine ? (int)t[i - 1] : 0;
    uint32_t* Mi = M + (size_t)(mine ? i - 1 : 0) * stride;
    int cur = 0, diag = 0, qc = 0, rb = 0, uq = 0, wb = 0;
    uint32_t bits = 0;
    for (int s = 0; s < steps; ++s) {
      if ((s & 63) == 0) {                                 // lane 0's next 64 letters and up values
        const int c = s + l;
        uq = c < b ? (int)u[c] : 0;
        rb = c < b ? (st ? row[c + 1] : c + 1) : 0;
      }
      int up = __shfl_up(cur, 1), uc = __shfl_up(qc, 1);
      const int up0 = __builtin_amdgcn_readlane(rb, s & 63), uc0 = __builtin_amdgcn_readlane(uq, s & 63);
      if (l == 0) {
        up = up0;
        uc = uc0;
      }
      qc = uc;
      const int jj = s - l + 1;
      if (mine && jj >= 1 && jj <= b) {
        const int left = jj == 1 ? i : cur, dg = jj == 1 ? i - 1 : diag;
        const int ne = tc != uc;
        const int d0 = dg + ne, d1 = up + 1, d2 = left + 1;
        uint32_t code;
        int best;
        if (d0 <= d1 && d0 <= d2) {
          code = (uint32_t)ne;
          best = d0;
        } else if (d1 <= d2) {
          code = 2u;
          best = d1;
        } else {
          code = 3u;
          best = d2;
        }
        cur = best;
        diag = up;
        const int cb = (jj - 1) & 15;
        bits |= code << (2 * cb);
        if (cb == 15 || jj == b) {
          Mi[(jj - 1) >> 4] = bits;
          bits = 0;
        }
        if (i == a && jj == b) fdist[j] = (ull)best;
      }
      const int c63 = __builtin_amdgcn_readlane(cur, 63);  // lane 63 after step s: column s - 62
      if (l == (s & 63)) wb = c63;
      if ((s & 63) == 63 && leave) {
        const int col = s - 125 + l;
        if (col >= 1 && col <= b) row[col] = wb;
      }
    }
    __threadfence_block();                                 // the row is in memory before the next strip loads it
  }
}

// ------------------------------------------------------------ d'. the fill in a band
// The geometry of a band fill of an a x b core at threshold tt.  t: the threshold, no wider than the matrix.
// The choices of row i, strip st = (i - 1) / 64, lie in W words from bit column start(st) on: the strip's first
// column less one, max(0, 64 st - t), rounded down to a multiple of 16 - its last is below 64 st + 64 + t, so
// W = ceil(min(b, 2 t + 79) / 16) serves every strip.  A pair takes a W + b + 1 words.
struct AlBand {
  ull t, W;
  __host__ __device__ AlBand(ull a, ull b, ull tt) {
    const ull mx = a > b ? a : b;
    t = tt < mx ? tt : mx;
    const ull w = 2ull * t + 79ull;
    W = ((w < b ? w : b) + 15ull) >> 4;
  }
  __host__ __device__ ull start(ull st) const { return 64ull * st > t ? (64ull * st - t) & ~15ull : 0ull; }
  __host__ __device__ ull words(ull a, ull b) const { return a * W + b + 1ull; }
};

// k_al_fill over the cells with |j - i| <= t alone.  Strip st starts at column w0 = start(st): lane l computes
// column w0 + s - l at step s, if it lies in its row's part of the band, steps s0 .. s1.  Whatever lies outside
// the band is AL_INF made here, never read: a lane's value while it computes nothing (so the left of a row's
// first column and the up of its last one, one column right of the row above's), lane 0's up values from the
// row buffer outside row 64 st's part, and the border D[i][0] below row t.  Only the band's part of lane 63's
// row is written back.
__global__ void __launch_bounds__(RG_BLOCK) k_al_fill_band(const char* __restrict__ blob, AlPairs R,
                                                           const ull* __restrict__ order, const ull* __restrict__ moff,
                                                           uint64_t nb, ull tt, uint32_t* __restrict__ scratch,
                                                           ull* __restrict__ fdist) {
  const int l = (int)(threadIdx.x & 63u);
  const uint64_t w = blockIdx.x * (uint64_t)AL_WAVES + (threadIdx.x >> 6);
  if (w >= nb) return;                                     // (a whole wave)
  const ull j = order[w], p = R.prefix[j];
  const int a = (int)(R.tlen[j] - p - R.suffix[j]), b = (int)(R.qlen[j] - p - R.suffix[j]);
  const unsigned char* t = reinterpret_cast<const unsigned char*>(blob) + R.toff[j] + p;
  const unsigned char* u = reinterpret_cast<const unsigned char*>(blob) + R.qoff[j] + p;
  const AlBand B((ull)a, (ull)b, tt);
  const int th = (int)B.t;
  const size_t stride = (size_t)B.W;
  uint32_t* M = scratch + moff[w];
  int* row = reinterpret_cast<int*>(M + (size_t)a * stride);
  for (int st = 0; st * 64 < a; ++st) {
    const int r = st * 64, i = r + l + 1, w0 = (int)B.start((ull)st);
    const bool mine = i <= a, leave = r + 64 <= a;         // lane 63 has a row: the next strip reads it
    const int last = leave ? r + 64 : a;                   // the strip's last row and its last column
    const int chi = b - last <= th ? b : last + th;
    const int steps = (chi - w0 + last - r + 63) & ~63;    // that row's last step + 1, rounded up to whole loads
    const int jlo = i - th > 1 ? i - th : 1, jhi = b - i <= th ? b : i + th;
    const int s0 = mine ? jlo - w0 + l : 1, s1 = mine ? jhi - w0 + l : 0;
    const int tc = mine ? (int)t[i - 1] : 0;
    uint32_t* Mi = M + (size_t)(mine ? i - 1 : 0) * stride;
    int cur = AL_INF, diag = AL_INF, qc = 0, rb = AL_INF, uq = 0, wb = 0;
    uint32_t bits = 0;
    for (int s = 0; s < steps; ++s) {
      if ((s & 63) == 0) {                                 // lane 0's next 64 letters and up values
        const int c = w0 + s + l;
        const bool in = c >= 1 && c <= b;
        uq = in ? (int)u[c - 1] : 0;
        rb = in && c - r <= th && r - c <= th ? (st ? row[c] : c) : AL_INF;
      }
      int up = __shfl_up(cur, 1), uc = __shfl_up(qc, 1);
      const int up0 = __builtin_amdgcn_readlane(rb, s & 63), uc0 = __builtin_amdgcn_readlane(uq, s & 63);
      if (l == 0) {
        up = up0;
        uc = uc0;
      }
      qc = uc;
      int now = AL_INF;
      if (s >= s0 && s <= s1) {
        const int x = s - l - 1, jj = w0 + x + 1;          // bit column x of the strip's window
        const int left = jj == 1 ? (i <= th ? i : AL_INF) : cur, dg = jj == 1 ? i - 1 : diag;
        const int ne = tc != uc;
        const int d0 = dg + ne, d1 = up + 1, d2 = left + 1;
        uint32_t code;
        if (d0 <= d1 && d0 <= d2) {
          code = (uint32_t)ne;
          now = d0;
        } else if (d1 <= d2) {
          code = 2u;
          now = d1;
        } else {
          code = 3u;
          now = d2;
        }
        const int cb = x & 15;
        bits |= code << (2 * cb);
        if (cb == 15 || s == s1) {
          Mi[x >> 4] = bits;
          bits = 0;
        }
        if (i == a && jj == b) fdist[j] = (ull)now;
      }
      cur = now;
      diag = up;
      const int c63 = __builtin_amdgcn_readlane(cur, 63);  // lane 63 after step s: column w0 + s - 63
      if (l == (s & 63)) wb = c63;
      if ((s & 63) == 63 && leave) {
        const int col = w0 + s - 126 + l;
        if (col >= 1 && col <= b && col - last <= th && last - col <= th) row[col] = wb;
      }
    }
    __threadfence_block();                                 // the row is in memory before the next strip loads it
  }
}

// ------------------------------------------------------------ e. the traceback
// the runs of pair j's core, in target order, end at rop / rlen [roff[j] + bound[j]); nrun[j] of them.
// BAND: the bits lie as k_al_fill_band left them at threshold tt.  A pair whose D[a][b] is above it is left
// alone, done[w] = 0; any other is exact, and the walk stays inside the band: the pair gets status 0 and
// need[j] = 1 (steps f to h then read its runs), done[w] = 1
template <bool BAND>
__global__ void k_al_trace(AlPairs R, const ull* __restrict__ order, const ull* __restrict__ moff, uint64_t nb,
                           const uint32_t* __restrict__ scratch, const ull* __restrict__ roff,
                           const ull* __restrict__ bound, uint8_t* __restrict__ rop, uint32_t* __restrict__ rlen,
                           ull* __restrict__ nrun, const ull* __restrict__ fdist, ull* bad, ull tt,
                           ull* __restrict__ need, ull* __restrict__ done) {
  RG_LOOP(w, nb) {
    const ull j = order[w], p = R.prefix[j];
    const ull a = R.tlen[j] - p - R.suffix[j], b = R.qlen[j] - p - R.suffix[j];
    const AlBand B(a, b, tt);
    const ull stride = BAND ? B.W : (b + 15ull) >> 4;
    if (BAND) {
      done[w] = fdist[j] <= B.t;
      if (fdist[j] > B.t) continue;
    }
    const uint32_t* M = scratch + moff[w];
    const ull lo = roff[j];
    ull at = lo + bound[j], i = a, jj = b, runs = 0, eq = 0, sub = 0, del = 0, ins = 0, gaps = 0;
    uint32_t op = 4, len = 0;
    bool full = false, astray = false;
    while (i || jj) {
      const ull x = jj - 1ull, w0 = BAND ? B.start((i - 1ull) >> 6) : 0ull;
      if (BAND && i && jj && (x < w0 || (x - w0) >> 4 >= stride)) { astray = true; break; }
      const uint32_t code = i && jj ? (M[(i - 1ull) * stride + ((x - w0) >> 4)] >> (2u * (x & 15ull))) & 3u
                                    : (i ? 2u : 3u);
      if (code != op) {
        if (len) {
          if (at == lo) { full = true; break; }
          --at;
          rop[at] = (uint8_t)op;
          rlen[at] = len;
          ++runs;
        }
        op = code;
        len = 0;
        gaps += code >= 2u;
      }
      ++len;
      eq += code == 0u;
      sub += code == 1u;
      del += code == 2u;
      ins += code == 3u;
      i -= code != 3u;
      jj -= code != 2u;
    }
    if (len && !full) {
      if (at == lo) {
        full = true;
      } else {
        --at;
        rop[at] = (uint8_t)op;
        rlen[at] = len;
        ++runs;
      }
    }
    if (full) RG_OR(bad, AL_BAD_BOUND);
    if (astray || sub + del + ins != fdist[j]) RG_OR(bad, AL_BAD_DIST);
    if (BAND) {
      R.status[j] = 0;
      need[j] = 1;
    }
    nrun[j] = runs;
    R.neq[j] = eq;
    R.nsub[j] = sub;
    R.ndel[j] = del;
    R.nins[j] = ins;
    R.nprims[j] = sub + gaps;
  }
}

// ------------------------------------------------------------ f. the exact arrays
// every pair's sums with the trimmed ends, its runs and primitives counted (need[j] != 0: k_al_trace left
// the core's)
__global__ void k_al_count(AlPairs R, uint64_t n, const ull* __restrict__ need, const ull* __restrict__ nrun) {
  RG_LOOP(j, n) {
    const ull p = R.prefix[j], q = R.suffix[j], a = R.tlen[j] - p - q, b = R.qlen[j] - p - q;
    const ull ends = (p ? 1ull : 0ull) + (q ? 1ull : 0ull);
    if (need[j]) {
      R.neq[j] += p + q;
      R.dist[j] = R.nsub[j] + R.nins[j] + R.ndel[j];
      R.nops[j] = ends + nrun[j];
    } else {
      R.neq[j] = p + q;
      R.nsub[j] = 0;
      R.ndel[j] = a;
      R.nins[j] = b;
      R.dist[j] = R.status[j] ? AL_NONE : a + b;
      R.nops[j] = ends + (a ? 1ull : 0ull) + (b ? 1ull : 0ull);
      R.nprims[j] = R.status[j] ? 1ull : (a ? 1ull : 0ull) + (b ? 1ull : 0ull);
    }
  }
}
__global__ void k_al_emit(AlPairs R, uint64_t n, const ull* __restrict__ need, const ull* __restrict__ roff,
                          const ull* __restrict__ bound, const ull* __restrict__ nrun,
                          const uint8_t* __restrict__ rop, const uint32_t* __restrict__ rlen, uint8_t* __restrict__ op,
                          ull* __restrict__ len, AlPrims Q) {
  RG_LOOP(j, n) {
    const ull p = R.prefix[j], q = R.suffix[j], a = R.tlen[j] - p - q, b = R.qlen[j] - p - q;
    ull o = R.opoff[j], r = R.primoff[j], tp = p, qp = p;
    auto run = [&](char c, ull L) {
      op[o] = (uint8_t)c;
      len[o++] = L;
    };
    auto prim = [&](uint32_t type, ull tl, ull ql) {
      Q.pair[r] = j;
      Q.type[r] = (uint8_t)type;
      Q.tpos[r] = tp;
      Q.qpos[r] = qp;
      Q.tlen[r] = tl;
      Q.qlen[r++] = ql;
    };
    if (p) run('=', p);
    if (R.status[j]) {
      if (a) run('D', a);
      if (b) run('I', b);
      prim(AL_REPL, a, b);
    } else if (!need[j]) {
      if (a) {
        run('D', a);
        prim(AL_DEL, a, 0);
      }
      if (b) {
        run('I', b);
        prim(AL_INS, 0, b);
      }
    } else {
      const ull end = roff[j] + bound[j];
      for (ull k = end - nrun[j]; k < end; ++k) {
        const uint32_t c = rop[k];
        const ull L = rlen[k];
        run("=XDI"[c], L);
        if (c == 1u) {
          for (ull x = 0; x < L; ++x, ++tp, ++qp) prim(AL_SNV, 1, 1);
        } else if (c == 2u) {
          prim(AL_DEL, L, 0);
          tp += L;
        } else if (c == 3u) {
          prim(AL_INS, 0, L);
          qp += L;
        } else {
          tp += L;
          qp += L;
        }
      }
    }
    if (q) run('=', q);
  }
}

// ------------------------------------------------------------ g. the lines
__global__ void k_al_flagp(AlPairs R, AlPrims Q, uint64_t n, uint8_t* __restrict__ flag) {
  RG_LOOP(r, n) flag[r] = R.placed[Q.pair[r]] != 0;
}
// FNV-1a over a primitive's query letters, cut to `keep` low bits (64: all)
__global__ void k_al_hash(const char* __restrict__ blob, AlPairs R, AlPrims Q, uint64_t n, int keep,
                          ull* __restrict__ hash) {
  RG_LOOP(r, n) {
    const char* u = blob + R.qoff[Q.pair[r]] + Q.qpos[r];
    ull h = 0xCBF29CE484222325ull;
    for (ull x = 0; x < Q.qlen[r]; ++x) h = (h ^ (ull)(unsigned char)u[x]) * 0x100000001B3ull;
    hash[r] = keep >= 64 ? h : h & ((1ull << keep) - 1ull);
  }
}
// key[k] = field f of primitive ord[k]
__global__ void k_al_key(AlPairs R, AlPrims Q, const ull* __restrict__ hash, const ull* __restrict__ ord, uint64_t m,
                         int f, ull* __restrict__ key) {
  RG_LOOP(k, m) {
    const ull r = ord[k];
    key[k] = f == 0 ? hash[r] : f == 1 ? Q.qlen[r] : f == 2 ? Q.tlen[r] : f == 3 ? (ull)Q.type[r] : f == 4 ? Q.tpos[r]
                                                                                                         : R.site[Q.pair[r]];
  }
}
__global__ void k_al_heads(AlPairs R, AlPrims Q, const ull* __restrict__ hash, const ull* __restrict__ ord, uint64_t m,
                           uint8_t* __restrict__ head) {
  RG_LOOP(k, m) {
    bool h = k == 0;
    if (!h) {
      const ull x = ord[k - 1], y = ord[k];
      h = R.site[Q.pair[x]] != R.site[Q.pair[y]] || Q.tpos[x] != Q.tpos[y] || Q.type[x] != Q.type[y] ||
          Q.tlen[x] != Q.tlen[y] || Q.qlen[x] != Q.qlen[y] || hash[x] != hash[y];
    }
    head[k] = h;
  }
}
// the group of sorted position k: the last g with heads[g] <= k
__device__ __forceinline__ uint64_t al_group(const ull* __restrict__ heads, uint64_t ng, ull k) {
  uint64_t lo = 0, hi = ng;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (heads[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}
// every member's letters against its group head's; memb[k]: the allele that carries sorted position k
__global__ void k_al_verify(const char* __restrict__ blob, AlPairs R, AlPrims Q, BbSites T, const ull* __restrict__ ord,
                            uint64_t m, const ull* __restrict__ heads, uint64_t ng, ull* __restrict__ memb, ull* bad) {
  RG_LOOP(k, m) {
    const ull y = ord[k], x = ord[heads[al_group(heads, ng, k)]], jy = Q.pair[y], jx = Q.pair[x];
    const char *u = blob + R.qoff[jy] + Q.qpos[y], *v = blob + R.qoff[jx] + Q.qpos[x];
    bool same = true;
    for (ull i = 0; i < Q.qlen[y] && same; ++i) same = u[i] == v[i];
    if (!same) RG_OR(bad, AL_BAD_HASH);
    memb[k] = T.first[R.site[jy]] + R.allele[jy];
  }
}
// group g as a line, before the lines are ordered
__global__ void k_al_groups(AlPairs R, AlPrims Q, VrPlaced P, const ull* __restrict__ pl, const ull* __restrict__ ord,
                            uint64_t m, const ull* __restrict__ heads, uint64_t ng, AlLines L) {
  RG_LOOP(g, ng) {
    const ull k = heads[g], r = ord[k], s = R.site[Q.pair[r]], p = pl[s];
    L.site[g] = s;
    L.place[g] = p;
    L.rec[g] = (ull)P.rec[p];
    L.pos[g] = (ull)P.pos[p] + Q.tpos[r] + (Q.type[r] == AL_SNV ? 1ull : 0ull);
    L.type[g] = Q.type[r];
    L.tpos[g] = Q.tpos[r];
    L.tlen[g] = Q.tlen[r];
    L.qlen[g] = Q.qlen[r];
    L.first[g] = r;
    L.mstart[g] = k;
    L.ac[g] = (g + 1 < ng ? heads[g + 1] : (ull)m) - k;
  }
}
// key[k] = field f of group ord[k]
__global__ void k_al_lkey(AlLines L, const ull* __restrict__ ord, uint64_t n, int f, ull* __restrict__ key) {
  RG_LOOP(k, n) {
    const ull g = ord[k];
    key[k] = f == 0 ? L.first[g] : f == 1 ? L.qlen[g] : f == 2 ? L.tlen[g] : f == 3 ? (ull)L.type[g] : f == 4 ? L.site[g]
                                                                            : f == 5 ? L.pos[g] : L.rec[g];
  }
}
// line k = group ord[k], with its carrier words and their popcount
__global__ void k_al_lines(AlLines G, const ull* __restrict__ ord, uint64_t n, const ull* __restrict__ memb,
                           const ull* __restrict__ abits, uint32_t W, AlLines L, ull* __restrict__ bits) {
  RG_LOOP(k, n) {
    const ull g = ord[k];
    L.site[k] = G.site[g];
    L.place[k] = G.place[g];
    L.rec[k] = G.rec[g];
    L.pos[k] = G.pos[g];
    L.type[k] = G.type[g];
    L.tpos[k] = G.tpos[g];
    L.tlen[k] = G.tlen[g];
    L.qlen[k] = G.qlen[g];
    L.first[k] = G.first[g];
    L.mstart[k] = G.mstart[g];
    L.ac[k] = G.ac[g];
    uint32_t pop = 0;
    for (uint32_t w = 0; w < W; ++w) {
      ull acc = 0;
      for (ull x = 0; x < G.ac[g]; ++x) acc |= abits[memb[G.mstart[g] + x] * W + w];
      bits[k * W + w] = acc;
      pop += (uint32_t)__popcll(acc);
    }
    L.ngen[k] = pop;
  }
}

// ------------------------------------------------------------ h. texts
// line 0: the header; line j + 1: pair j
struct AlignLine {
  AlPairs R;
  BbSites T;
  const uint8_t* op;
  const ull* len;
  template <class S>
  __device__ __forceinline__ void operator()(S& s, uint64_t i) const {
    if (i == 0) {
      s.lit("#from\tto\tallele\ttarget\ttlen\tqlen\tprefix\tsuffix\tdist\teq\tsub\tins\tdel\tcigar\n");
      return;
    }
    const uint64_t j = i - 1;
    const ull site = R.site[j];
    s.dec((ull)T.from[site]); s.ch('\t'); s.dec((ull)T.to[site]); s.ch('\t'); s.dec(R.allele[j]); s.ch('\t');
    if (R.placed[j]) s.lit("ref"); else s.ch('0');
    s.ch('\t'); s.dec(R.tlen[j]); s.ch('\t'); s.dec(R.qlen[j]); s.ch('\t'); s.dec(R.prefix[j]);
    s.ch('\t'); s.dec(R.suffix[j]); s.ch('\t');
    if (R.status[j]) s.ch('.'); else s.dec(R.dist[j]);
    s.ch('\t'); s.dec(R.neq[j]); s.ch('\t'); s.dec(R.nsub[j]); s.ch('\t'); s.dec(R.nins[j]);
    s.ch('\t'); s.dec(R.ndel[j]); s.ch('\t');
    if (!R.nops[j]) s.ch('*');
    for (ull k = R.opoff[j]; k < R.opoff[j] + R.nops[j]; ++k) {
      s.dec(len[k]);
      s.ch((char)op[k]);
    }
    s.ch('\n');
  }
};
// item i: line i / (G + 1); its head (everything up to GT) or the cell of genome i % (G + 1) - 1
struct PrimVcfLine {
  AlLines L;
  AlPairs R;
  AlPrims Q;
  RsTab V;
  BbSites T;
  const ull* memb;
  const ull* abits;
  const char* blob;
  const char* names;
  const long long* name_off;
  uint64_t na;
  uint32_t G, W;
  template <class S>
  __device__ __forceinline__ void operator()(S& s, uint64_t i) const {
    const uint64_t k = i / (G + 1ull);
    const uint32_t c = (uint32_t)(i % (G + 1ull));
    const ull site = L.site[k];
    if (c == 0) {
      const ull r = L.rec[k], f = L.first[k], tpos = L.tpos[k];
      const char* t = blob + V.poff[na + L.place[k]] + 1ull;   // T[0]; the padding base lies before it
      const char* u = blob + R.qoff[Q.pair[f]] + Q.qpos[f];
      s.bytes(names + name_off[r], (ull)(name_off[r + 1] - name_off[r]));
      s.ch('\t'); s.dec(L.pos[k]); s.ch('\t');
      s.dec((ull)T.from[site]); s.ch('_'); s.dec((ull)T.to[site]); s.ch('\t');
      if (L.type[k] == AL_SNV) {
        s.bytes(t + tpos, 1); s.ch('\t'); s.bytes(u, 1);
      } else {
        s.bytes(t + tpos - 1, 1ull + L.tlen[k]); s.ch('\t');
        s.bytes(t + tpos - 1, 1); s.bytes(u, L.qlen[k]);
      }
      s.lit("\t.\t.\tNS="); s.dec(T.ngen[site]); s.lit(";AC="); s.dec(L.ac[k]); s.lit("\tGT");
      if (!G) s.ch('\n');
    } else {
      const uint32_t g = c - 1u;
      const ull bit = 1ull << (g & 63u);
      const size_t w = g >> 6;
      ull have = 0, carry = 0;                               // the site's alleles with bit g; those that carry the line
      for (ull a = T.first[site]; a < T.first[site] + T.nal[site]; ++a) have += (abits[a * W + w] & bit) != 0;
      for (ull x = 0; x < L.ac[k]; ++x) carry += (abits[memb[L.mstart[k] + x] * W + w] & bit) != 0;
      s.ch('\t');
      if (have > carry) s.ch('0');
      if (have > carry && carry) s.ch('/');
      if (carry) s.ch('1');
      if (!have) s.ch('.');
      if (g + 1u == G) s.ch('\n');
    }
  }
};

static ull read_flags(Ctx& c, const DevBuf& bad) {
  ull h = 0;
  PG_HIP(hipMemcpyAsync(&h, bad.p, 8, hipMemcpyDeviceToHost, c.stream));
  c.sync();
  return h;
}
// ord (in place) stably sorted by key[k] = kern(..., ord, f): one pass of a least-significant-first sort
template <class Launch>
static void sort_step(Ctx& c, DevBuf& ord, DevBuf& ord2, DevBuf& kin, DevBuf& kout, uint64_t n, int bits,
                      Launch&& launch) {
  launch(ord.as<ull>(), kin.as<ull>());
  sort_pairs(c, kin.as<ull>(), kout.as<ull>(), ord.as<ull>(), ord2.as<ull>(), n, bits);
  ord.swap(ord2);
}

void region_align(Ctx& c, uint64_t* n_pairs, uint64_t* n_aligned, uint64_t* n_ops, uint64_t* n_prims,
                  uint64_t* n_lines) {
  const char* what = "pg_region_align";
  const std::string w = std::string(what) + ": ";
  need(c.vr_ready && c.bb_ready, what, NEED_VARIANTS);
  const uint64_t ns = c.bb_ns, na = c.vr_na, np = c.vr_np, n = na - ns;
  const uint32_t W = c.bb_words;
  const ull cells_cap = c.al_cells_cap ? c.al_cells_cap : 1ull << 24;
  const uint64_t budget = (c.al_scratch ? c.al_scratch : 256ull << 20) / 4;   // in words
  const ull band_cap = c.al_band_cap ? c.al_band_cap : 1ull << 26, band_t0 = c.al_band_t0 ? c.al_band_t0 : 64ull;
  const BbSites T(c.bb_sites, ns);
  const BbAlleles A(c.bb_alleles, na);
  const RsTab V(c.vr_tab, na + np);
  const VrPlaced P(c.vr_place, np);
  const char* blob = c.vr_blob.as<char>();
  const ull* abits = c.bb_bits.as<ull>();

  // ---- everything is built aside; the context's result is replaced at the end
  DevBuf pairs, ops, prims, lines, lbits, memb, bad, pl, needw, bound, cellw, roff, nrun, fdist, rop, rlen, scratch, dord,
      dmoff, bdone;
  uint64_t aligned = 0, nops = 0, nprims = 0, nl = 0, cells = 0, nover = 0, nbanded = 0, nattempts = 0, bandcells = 0;
  double ms = 0, msband = 0;
  pairs.reserve(AlPairs::bytes(n));
  bad.reserve(16);
  PG_HIP(hipMemsetAsync(bad.p, 0, 8, c.stream));
  pl.reserve(8 * (ns + 1));
  if (ns) PG_HIP(hipMemsetAsync(pl.p, 0xFF, 8 * ns, c.stream));
  if (np) RG_LAUNCH(k_al_site, grid_for(np, RG_BLOCK, 8192), P, np, pl.as<ull>());
  AlPairs R(pairs, n);
  if (n) {
    // ---- a. b. the pairs, trimmed
    needw.reserve(8 * (n + 1));
    bound.reserve(8 * (n + 1));
    roff.reserve(8 * (n + 1));
    nrun.reserve(8 * (n + 1));
    fdist.reserve(8 * (n + 1));
    RG_LAUNCH(k_al_pairs, grid_for(na, RG_BLOCK, 8192), T, A, V, P, pl.as<ull>(), na, R);
    cellw.reserve(8 * (n + 1));
    RG_LAUNCH(k_al_trim, grid_for(n, AL_WAVES, 8192), blob, R, n, cells_cap, c.al_band, needw.as<ull>(), bound.as<ull>(),
              cellw.as<ull>());
    const uint64_t nbound = excl_scan_total(c, bound.as<ull>(), roff.as<ull>(), n);
    rop.reserve(nbound + 16);
    rlen.reserve(4 * nbound + 16);
    // ---- c. the batches: pairs with a core, largest first
    std::vector<ull> hneed(n), hstat(n), hcells(n);
    PG_HIP(hipMemcpyAsync(hneed.data(), needw.p, 8 * n, hipMemcpyDeviceToHost, c.stream));
    PG_HIP(hipMemcpyAsync(hstat.data(), R.status, 8 * n, hipMemcpyDeviceToHost, c.stream));
    PG_HIP(hipMemcpyAsync(hcells.data(), cellw.p, 8 * n, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    std::vector<ull> order;
    for (uint64_t j = 0; j < n; ++j) {
      aligned += !hstat[j];
      cells += hcells[j];
      if (hneed[j]) order.push_back(j);
    }
    std::stable_sort(order.begin(), order.end(), [&](ull x, ull y) { return hneed[x] > hneed[y]; });
    const uint64_t nf = order.size();
    std::vector<ull> moff;
    std::vector<uint64_t> cut;                             // batch b = order[cut[b] .. cut[b + 1])
    // words[k]: what the k-th pair of a list takes; its place in its batch's scratch, the cuts, the largest batch
    auto batches = [&](auto&& words, uint64_t count) {
      moff.assign(count, 0);
      cut.assign(1, 0);
      uint64_t most = 0, used = 0;
      for (uint64_t k = 0; k < count; ++k) {
        // (a batch is one grid of a fill: a wave per pair and no loop)
        if (used && (used + words(k) > budget || k - cut.back() >= 65536ull * AL_WAVES)) {
          cut.push_back(k);
          used = 0;
        }
        moff[k] = used;
        used += words(k);
        most = std::max(most, used);
      }
      cut.push_back(count);
      return most;
    };
    const uint64_t most = batches([&](uint64_t k) { return hneed[order[k]]; }, nf);
    if (nf) {
      scratch.reserve(4 * most + 16);
      dord.reserve(8 * nf);
      dmoff.reserve(8 * nf);
      PG_HIP(hipMemcpyAsync(dord.p, order.data(), 8 * nf, hipMemcpyHostToDevice, c.stream));
      PG_HIP(hipMemcpyAsync(dmoff.p, moff.data(), 8 * nf, hipMemcpyHostToDevice, c.stream));
      c.t_al.init();
    }
    // ---- d. e. batch by batch: the fill, then the walk back over its bits
    for (size_t bt = 0; bt + 1 < cut.size() && nf; ++bt) {
      const uint64_t k0 = cut[bt], nb = cut[bt + 1] - k0;
      c.t_al.start(c.stream);
      RG_LAUNCH(k_al_fill, grid_for(nb, AL_WAVES), blob, R, dord.as<ull>() + k0, dmoff.as<ull>() + k0, nb,
                scratch.as<uint32_t>(), fdist.as<ull>());
      c.t_al.stop(c.stream);
      RG_LAUNCH(k_al_trace<false>, grid_for(nb, RG_BLOCK, 8192), R, dord.as<ull>() + k0, dmoff.as<ull>() + k0, nb,
                scratch.as<uint32_t>(), roff.as<ull>(), bound.as<ull>(), rop.as<uint8_t>(), rlen.as<uint32_t>(),
                nrun.as<ull>(), fdist.as<ull>(), bad.as<ull>(), 0ull, nullptr, nullptr);
      c.sync();
      ms += c.t_al.ms();
    }
    // ---- d'. the band form: the pairs above the cap with two core sides, round k at the threshold t0 2^k.  A
    // pair joins at the first threshold that holds |a - b|, leaves aligned once D[a][b] is within the threshold,
    // and leaves as it is (status 1) when the next band would take more than band_cap cells
    if (c.al_band) {
      struct Cand { ull j, a, b; uint64_t k; };
      std::vector<Cand> alive, round;
      std::vector<ull> ht(n), hq(n), hp(n), hs(n), hdone;
      PG_HIP(hipMemcpyAsync(ht.data(), R.tlen, 8 * n, hipMemcpyDeviceToHost, c.stream));
      PG_HIP(hipMemcpyAsync(hq.data(), R.qlen, 8 * n, hipMemcpyDeviceToHost, c.stream));
      PG_HIP(hipMemcpyAsync(hp.data(), R.prefix, 8 * n, hipMemcpyDeviceToHost, c.stream));
      PG_HIP(hipMemcpyAsync(hs.data(), R.suffix, 8 * n, hipMemcpyDeviceToHost, c.stream));
      c.sync();
      auto bcells = [](const Cand& x, ull t) { return x.a * std::min(x.b, 2ull * t + 1ull); };
      for (uint64_t j = 0; j < n; ++j) {
        const ull a = ht[j] - hp[j] - hs[j], b = hq[j] - hp[j] - hs[j];
        if (a + 1ull <= cells_cap / (b + 1ull)) continue;
        ++nover;
        if (!a || !b) {                                    // (k_al_trim gave it status 0: counted as aligned above)
          ++nbanded;
          continue;
        }
        Cand x{j, a, b, 0};
        while (band_t0 << x.k < (a > b ? a - b : b - a)) ++x.k;
        if (a + b < AL_BAND_MOST && bcells(x, band_t0 << x.k) <= band_cap) alive.push_back(x);
      }
      if (!alive.empty()) c.t_al.init();
      for (uint64_t k = 0; !alive.empty(); ++k) {
        const ull t = band_t0 << k;
        round.clear();
        for (const Cand& x : alive)
          if (x.k <= k) round.push_back(x);
        const uint64_t nr = round.size();
        if (!nr) continue;
        auto words = [&](const Cand& x) { return AlBand(x.a, x.b, t).words(x.a, x.b); };
        std::stable_sort(round.begin(), round.end(), [&](const Cand& x, const Cand& y) { return words(x) > words(y); });
        const uint64_t top = batches([&](uint64_t i) { return words(round[i]); }, nr);
        std::vector<ull> ord(nr);
        for (uint64_t i = 0; i < nr; ++i) ord[i] = round[i].j;
        scratch.reserve(4 * top + 16);
        dord.reserve(8 * nr);
        dmoff.reserve(8 * nr);
        bdone.reserve(8 * nr);
        PG_HIP(hipMemcpyAsync(dord.p, ord.data(), 8 * nr, hipMemcpyHostToDevice, c.stream));
        PG_HIP(hipMemcpyAsync(dmoff.p, moff.data(), 8 * nr, hipMemcpyHostToDevice, c.stream));
        for (size_t bt = 0; bt + 1 < cut.size(); ++bt) {
          const uint64_t k0 = cut[bt], nb = cut[bt + 1] - k0;
          c.t_al.start(c.stream);
          RG_LAUNCH(k_al_fill_band, grid_for(nb, AL_WAVES), blob, R, dord.as<ull>() + k0, dmoff.as<ull>() + k0, nb, t,
                    scratch.as<uint32_t>(), fdist.as<ull>());
          c.t_al.stop(c.stream);
          RG_LAUNCH(k_al_trace<true>, grid_for(nb, RG_BLOCK, 8192), R, dord.as<ull>() + k0, dmoff.as<ull>() + k0, nb,
                    scratch.as<uint32_t>(), roff.as<ull>(), bound.as<ull>(), rop.as<uint8_t>(), rlen.as<uint32_t>(),
                    nrun.as<ull>(), fdist.as<ull>(), bad.as<ull>(), t, needw.as<ull>(), bdone.as<ull>() + k0);
          c.sync();
          msband += c.t_al.ms();
        }
        hdone.resize(nr);
        PG_HIP(hipMemcpyAsync(hdone.data(), bdone.p, 8 * nr, hipMemcpyDeviceToHost, c.stream));
        c.sync();
        std::vector<ull> left;                             // the pairs of this round that go on to 2 t
        for (uint64_t i = 0; i < nr; ++i) {
          ++nattempts;
          bandcells += bcells(round[i], t);
          if (hdone[i]) {
            ++nbanded;
            ++aligned;
          } else if (bcells(round[i], 2ull * t) <= band_cap) {
            left.push_back(round[i].j);
          }
        }
        std::sort(left.begin(), left.end());
        std::vector<Cand> next;
        for (const Cand& x : alive)
          if (x.k > k || std::binary_search(left.begin(), left.end(), x.j)) next.push_back(x);
        alive.swap(next);
      }
    }
    if (read_flags(c, bad))
      throw Error(-5, w + "the walk back over the direction bits does not agree with the fill");
    // ---- f. the exact arrays
    const unsigned gn = grid_for(n, RG_BLOCK, 8192);
    RG_LAUNCH(k_al_count, gn, R, n, needw.as<ull>(), nrun.as<ull>());
    nops = excl_scan_total(c, R.nops, R.opoff, n);
    nprims = excl_scan_total(c, R.nprims, R.primoff, n);
    ops.reserve(9 * nops + 64);
    prims.reserve(AlPrims::bytes(nprims));
    RG_LAUNCH(k_al_emit, gn, R, n, needw.as<ull>(), roff.as<ull>(), bound.as<ull>(), nrun.as<ull>(), rop.as<uint8_t>(),
              rlen.as<uint32_t>(), ops.as<uint8_t>() + 8 * nops, ops.as<ull>(), AlPrims(prims, nprims));
  } else {
    ops.reserve(64);
    prims.reserve(AlPrims::bytes(0));
  }
  // ---- g. the lines of the placed sites
  const AlPrims Q(prims, nprims);
  DevBuf flag, sel, ord2, kin, kout, hash, head, heads, cnt, groups, lord;
  uint64_t m = 0;
  if (nprims && np) {
    flag.reserve(nprims + 16);
    sel.reserve(8 * (nprims + 1));
    RG_LAUNCH(k_al_flagp, grid_for(nprims, RG_BLOCK, 8192), R, Q, nprims, flag.as<uint8_t>());
    m = select_flagged(c, rocprim::counting_iterator<ull>(0), flag.as<uint8_t>(), sel.as<ull>(), nprims, cnt);
  }
  memb.reserve(8 * (m + 1));
  if (m) {
    const unsigned gm = grid_for(m, RG_BLOCK, 8192);
    hash.reserve(8 * nprims);
    ord2.reserve(8 * (nprims + 1));
    kin.reserve(8 * m);
    kout.reserve(8 * m);
    head.reserve(m + 16);
    heads.reserve(8 * (m + 1));
    const int keep = c.al_hash_bits ? c.al_hash_bits : 64;
    RG_LAUNCH(k_al_hash, grid_for(nprims, RG_BLOCK, 8192), blob, R, Q, nprims, keep, hash.as<ull>());
    const int fbits[6] = {keep, 64, 64, 2, 64, bits_for(ns)};
    for (int f = 0; f < 6; ++f)
      sort_step(c, sel, ord2, kin, kout, m, fbits[f], [&](const ull* o, ull* key) {
        RG_LAUNCH(k_al_key, gm, R, Q, hash.as<ull>(), o, m, f, key);
      });
    RG_LAUNCH(k_al_heads, gm, R, Q, hash.as<ull>(), sel.as<ull>(), m, head.as<uint8_t>());
    const uint64_t ng = select_flagged(c, rocprim::counting_iterator<ull>(0), head.as<uint8_t>(), heads.as<ull>(), m, cnt);
    RG_LAUNCH(k_al_verify, gm, blob, R, Q, T, sel.as<ull>(), m, heads.as<ull>(), ng, memb.as<ull>(), bad.as<ull>());
    if (read_flags(c, bad))
      throw Error(-5, w + "two primitives of one site share their place, their lengths and their letters' hash (" +
                          std::string(c.al_hash_bits ? "PG_TUNE_ALIGN_HASH_BITS keeps " +
                                                           std::to_string(c.al_hash_bits) + " bits"
                                                     : "the full hash") +
                          ") and differ in their letters");
    nl = ng;
    groups.reserve(AlLines::bytes(nl));
    lord.reserve(8 * (nl + 1));
    kin.reserve(8 * nl);
    kout.reserve(8 * nl);
    ord2.reserve(8 * (nl + 1));
    const AlLines Gr(groups, nl);
    const unsigned gl = grid_for(nl, RG_BLOCK, 8192);
    RG_LAUNCH(k_al_groups, gl, R, Q, P, pl.as<ull>(), sel.as<ull>(), m, heads.as<ull>(), ng, Gr);
    std::vector<ull> iota(nl);
    std::iota(iota.begin(), iota.end(), 0ull);
    PG_HIP(hipMemcpyAsync(lord.p, iota.data(), 8 * nl, hipMemcpyHostToDevice, c.stream));
    c.sync();
    const int lbit[7] = {64, 64, 64, 2, bits_for(ns), 64, bits_for(c.n_records)};
    for (int f = 0; f < 7; ++f)
      sort_step(c, lord, ord2, kin, kout, nl, lbit[f], [&](const ull* o, ull* key) {
        RG_LAUNCH(k_al_lkey, gl, Gr, o, nl, f, key);
      });
    lines.reserve(AlLines::bytes(nl));
    lbits.reserve(8 * nl * (size_t)W + 16);
    RG_LAUNCH(k_al_lines, gl, Gr, lord.as<ull>(), nl, memb.as<ull>(), abits, W, AlLines(lines, nl), lbits.as<ull>());
  } else {
    lines.reserve(AlLines::bytes(0));
    lbits.reserve(16);
  }
  c.sync();
  // ---- the new result replaces the previous one
  c.al_pairs.swap(pairs);
  c.al_ops.swap(ops);
  c.al_prims.swap(prims);
  c.al_lines.swap(lines);
  c.al_bits.swap(lbits);
  c.al_memb.swap(memb);
  c.al_np = n;
  c.al_aligned = aligned;
  c.al_nops = nops;
  c.al_nprims = nprims;
  c.al_nl = nl;
  c.al_cells = cells;
  c.ms_al_fill = ms;
  c.al_nover = nover;
  c.al_nbanded = nbanded;
  c.al_nattempts = nattempts;
  c.al_bandcells = bandcells;
  c.ms_al_band = msband;
  c.al_ready = true;
  if (n_pairs) *n_pairs = n;
  if (n_aligned) *n_aligned = aligned;
  if (n_ops) *n_ops = nops;
  if (n_prims) *n_prims = nprims;
  if (n_lines) *n_lines = nl;
}

void region_align_pairs(Ctx& c, uint64_t* const cols[17], uint64_t cap) {
  need(c.al_ready, "pg_region_align_pairs", NEED_ALIGN);
  const uint64_t n = c.al_np;
  if (cap < n) throw Error(-34, "pg_region_align_pairs: buffer too small");
  if (!n) return;
  const AlPairs R(c.al_pairs, n);
  for (int k = 0; k < 17; ++k) get(c, cols[k], R.column(k), 8 * n);
  c.sync();
}

void region_align_ops(Ctx& c, uint8_t* op, uint64_t* len, uint64_t cap) {
  need(c.al_ready, "pg_region_align_ops", NEED_ALIGN);
  const uint64_t n = c.al_nops;
  if (cap < n) throw Error(-34, "pg_region_align_ops: buffer too small");
  if (!n) return;
  get(c, len, c.al_ops.p, 8 * n);
  get(c, op, c.al_ops.as<uint8_t>() + 8 * n, n);
  c.sync();
}

void region_align_prims(Ctx& c, uint64_t* pair, uint8_t* type, uint64_t* tpos, uint64_t* qpos, uint64_t* tlen,
                        uint64_t* qlen, uint64_t cap) {
  need(c.al_ready, "pg_region_align_prims", NEED_ALIGN);
  const uint64_t n = c.al_nprims;
  if (cap < n) throw Error(-34, "pg_region_align_prims: buffer too small");
  if (!n) return;
  const AlPrims Q(c.al_prims, n);
  get(c, pair, Q.pair, 8 * n);
  get(c, type, Q.type, n);
  get(c, tpos, Q.tpos, 8 * n);
  get(c, qpos, Q.qpos, 8 * n);
  get(c, tlen, Q.tlen, 8 * n);
  get(c, qlen, Q.qlen, 8 * n);
  c.sync();
}

void region_align_lines(Ctx& c, uint64_t* site, int64_t* pos, uint8_t* type, uint64_t* tpos, uint64_t* tlen,
                        uint64_t* qlen, uint64_t* first_prim, uint64_t* ac, uint32_t* n_genomes, uint64_t* bits,
                        uint64_t cap) {
  need(c.al_ready, "pg_region_align_lines", NEED_ALIGN);
  const uint64_t n = c.al_nl;
  if (cap < n) throw Error(-34, "pg_region_align_lines: buffer too small");
  if (!n) return;
  const AlLines L(c.al_lines, n);
  get(c, site, L.site, 8 * n);
  get(c, pos, L.pos, 8 * n);
  get(c, type, L.type, n);
  get(c, tpos, L.tpos, 8 * n);
  get(c, tlen, L.tlen, 8 * n);
  get(c, qlen, L.qlen, 8 * n);
  get(c, first_prim, L.first, 8 * n);
  get(c, ac, L.ac, 8 * n);
  get(c, n_genomes, L.ngen, 4 * n);
  get(c, bits, c.al_bits.p, 8 * n * (size_t)c.bb_words);
  c.sync();
}

// the pair table's text of the last region_align: its size (out null, fd < 0), copied into out, or written to fd
uint64_t format_region_align(Ctx& c, char* out, uint64_t cap, int fd) {
  const char* what = fd >= 0 ? "pg_region_align_format_fd" : "pg_region_align_format";
  need(c.al_ready && c.bb_ready, what, NEED_ALIGN);
  const uint64_t n = c.al_np;
  DevBuf toff, text;
  const AlignLine line{AlPairs(c.al_pairs, n), BbSites(c.bb_sites, c.bb_ns), c.al_ops.as<uint8_t>() + 8 * c.al_nops,
                       c.al_ops.as<ull>()};
  const uint64_t total = text_measure(c, line, n + 1, toff);
  if (!text_wanted(total, out, cap, fd, what)) return total;
  text.reserve(total + 16);
  text_write(c, line, n + 1, toff, text.as<char>());
  return text_out(c, text.p, total, out, cap, fd, what, what);
}

// the primitives' VCF body of the last region_align, the same three ways
uint64_t format_region_primitives_vcf(Ctx& c, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                                      uint64_t cap, int fd) {
  const char* what = fd >= 0 ? "pg_region_primitives_vcf_fd" : "pg_region_primitives_vcf";
  need(c.al_ready && c.vr_ready && c.bb_ready, what, NEED_ALIGN);
  const DevNames nm = names_upload(c, what, names, name_off, n_names, c.n_records, "lines");
  const uint64_t nl = c.al_nl, na = c.vr_na;
  if (!nl) return 0;
  DevBuf toff, text;
  const PrimVcfLine line{AlLines(c.al_lines, nl), AlPairs(c.al_pairs, c.al_np), AlPrims(c.al_prims, c.al_nprims),
                         RsTab(c.vr_tab, na + c.vr_np), BbSites(c.bb_sites, c.bb_ns), c.al_memb.as<ull>(),
                         c.bb_bits.as<ull>(), c.vr_blob.as<char>(), nm.bytes, nm.off, na, c.bb_groups, c.bb_words};
  const uint64_t ni = nl * (c.bb_groups + 1ull);
  const uint64_t total = text_measure(c, line, ni, toff);
  if (!text_wanted(total, out, cap, fd, what) || !total) return total;
  text.reserve(total + 16);
  text_write(c, line, ni, toff, text.as<char>());
  return text_out(c, text.p, total, out, cap, fd, what, what);
}

}  // namespace pg
