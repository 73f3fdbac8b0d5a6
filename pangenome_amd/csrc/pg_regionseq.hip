// pg_regionseq.hip — what a region is: one representative sequence per label
// of the region rows, decoded from the parse's packed class stream where it
// lies on the device; the table, the letters, a FASTA text and the sequences
// of the region graph's S lines (pg_region_gfa_seq).
//
// Rows are (record, start, end, strand, label); a row is used iff label >= 0
// and its record has a genome (pg_freq's rule).  The representative of a
// label is its used row with the largest |end - start|, the first in list
// order among equals.  Its sequence is bases [lo, hi) of the record's
// compacted sequence, one letter per base class (A C G T; N, '$' and "other"
// give N: K1's class stream has already folded case and the IUPAC codes), as
// it stands if strand == 1 and reverse complemented otherwise.
//
// Steps, each its own launch on c.stream (no hand-shake inside a kernel):
//   a. k_row_scan   the largest used label and record, the skipped rows and
//                   the used rows whose [lo, hi) leaves their record: all
//                   known before anything is allocated or replaced
//   b. k_rs_max     per label the largest length (64-bit atomic max), then
//      k_rs_first   the smallest row index among the rows that reach it
//                   (64-bit atomic min): no packed (length, index) word, so
//                   neither is capped.  Dense arrays, 16 x L bytes
//   c. select the labels seen, k_rs_gather their row, two scans: `offset`
//      (the letters before an entry) and the same with every length rounded
//      up to 16 (where the entry starts in the blob)
//   d. k_rs_decode  the hot path.  One thread per 16-letter chunk of the
//                   blob, never per region; a chunk belongs to one entry (a
//                   search over the padded offsets, narrowed per block to the
//                   entries its first and last chunk belong to) and is one
//                   aligned 128-bit store.  A block takes a contiguous range
//                   of chunks, a round of 256 at a time.  Forward: the two packed words
//                   that cover the 16 source bases, funnel-shifted to one.
//                   Reverse: the same for the 16 bases read downward, then
//                   the sixteen 2-bit groups reversed (bit reverse and a swap
//                   inside the pairs) and complemented (A0 <-> T3, C1 <-> G2:
//                   all bits flipped).  2 bits -> ASCII four at a time: the
//                   class bytes of unpack4 select from the constant "ACGT".
//                   A chunk whose source touches an exception (e16) goes base
//                   by base through PackedCls (K1 wrote the class bytes of
//                   exactly those chunks).  gc and amb come from the same
//                   word; a thread keeps them while its chunks stay in one
//                   entry, and they reach the table through atomics
//                   aggregated in the wave (rg_by_label) when it leaves it.
//   e. FastaLine (pg_text.h)     the FASTA text, one thread per header;
//      k_rs_copy    the letters, one thread per 16-byte piece of the blob
//                   (the FASTA and GFA texts and the export without padding)
//
// The table (RsTab) and the declarations of k_rs_decode and k_rs_copy are in
// pg_seqdec.h: pg_variants.hip launches both over a table of its own spans.
//
// Bytes (d): 0.25 read and 1 written per base, and 1/16 for e16.
// Every sum is an integer and every atomic commutes: the result depends on
// the input alone, whatever the schedule.
#include "pg_seqdec.h"

namespace pg {

#define RS_ACGT 0x54474341u        // "ACGT", A in the low byte
// ------------------------------------------------------------ b. arg-max
// d_max[label] = the largest length of its used rows (zeroed before)
__global__ void __launch_bounds__(RG_BLOCK) k_rs_max(const long long* __restrict__ rows, uint64_t n,
                                                     const int* __restrict__ rec_group, ull* d_max) {
  __shared__ long long lds[RG_TILE_WORDS(false)];
  const uint64_t ntiles = (n + RG_BLOCK - 1) / RG_BLOCK;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    RgRow r;
    const bool todo = rg_load_tile(rows, n, t, lds, r) && rs_used(r, rec_group);
    const ull lab = todo ? (ull)r.label : 0ull;
    const ull len = todo ? rg_len(r) : 0ull;
    // every lane of the wave runs the loop (its conditions are ballots)
    const bool own = rg_by_label(todo, lab, [&](ull lab0, bool mine, ull, bool leader) {
      const ull hi = rg_wave_max(mine ? len : 0ull);
      if (leader) RG_MAX(d_max + lab0, hi);
    });
    if (own) RG_MAX(d_max + lab, len);
  }
}
// d_row[label] = the first used row whose length is d_max[label] (RS_NONE before: no used row)
__global__ void __launch_bounds__(RG_BLOCK) k_rs_first(const long long* __restrict__ rows, uint64_t n,
                                                       const int* __restrict__ rec_group,
                                                       const ull* __restrict__ d_max, ull* d_row) {
  __shared__ long long lds[RG_TILE_WORDS(false)];
  const uint64_t ntiles = (n + RG_BLOCK - 1) / RG_BLOCK;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    RgRow r;
    bool todo = rg_load_tile(rows, n, t, lds, r) && rs_used(r, rec_group);
    const ull lab = todo ? (ull)r.label : 0ull;
    todo = todo && rg_len(r) == d_max[lab];
    const ull idx = t * RG_BLOCK + threadIdx.x;
    const bool own = rg_by_label(todo, lab, [&](ull lab0, bool mine, ull, bool leader) {
      const ull lo = rg_wave_min(mine ? idx : RS_NONE);
      if (leader) RG_MIN(d_row + lab0, lo);
    });
    if (own) RG_MIN(d_row + lab, idx);
  }
}

// ------------------------------------------------------------ c. compaction
__global__ void k_rs_seen(const ull* __restrict__ d_row, uint64_t L, uint8_t* __restrict__ flag) {
  RG_LOOP(l, L) flag[l] = d_row[l] != RS_NONE;
}
// T.label[i] is set; plen[i] = the entry's length rounded up to 16
__global__ void k_rs_gather(RsTab T, uint64_t n, const long long* __restrict__ rows, const ull* __restrict__ d_max,
                            const ull* __restrict__ d_row, ull* __restrict__ plen) {
  RG_LOOP(i, n) {
    const uint64_t l = (uint64_t)T.label[i];
    const ull r = d_row[l], len = d_max[l];
    const long long* q = rows + 5 * r;
    T.row[i] = (long long)r;
    T.rec[i] = q[0];
    T.start[i] = q[1];
    T.end[i] = q[2];
    T.strand[i] = q[3];
    T.len[i] = len;
    T.gc[i] = 0;
    T.amb[i] = 0;
    plen[i] = (len + 15ull) & ~15ull;
  }
}

// ------------------------------------------------------------ d. decoder
// the entry byte x of the blob belongs to: the last i in [lo, hi) with poff[i] <= x (poff[lo] <= x)
__device__ __forceinline__ uint64_t rs_entry_of(const ull* __restrict__ poff, uint64_t lo, uint64_t hi, ull x) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (poff[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}
// The entry of the block's chunk q = base + threadIdx.x, for every thread of the block (two barriers):
// thread 0 and thread 64 search all n entries for the block's first and last chunk, every thread then
// only between the two.  rng: 2 words of LDS.  Returns whether q < end (the block's chunks end there).
__device__ __forceinline__ bool rs_chunk_entry(const ull* __restrict__ poff, uint64_t n, uint64_t base,
                                               uint64_t end, ull* rng, uint64_t& q, uint64_t& entry) {
  const uint64_t last = (base + RG_BLOCK < end ? base + RG_BLOCK : end) - 1;
  __syncthreads();                                         // (the previous round's readers are done)
  if (threadIdx.x == 0) rng[0] = rs_entry_of(poff, 0, n, 16ull * base);
  if (threadIdx.x == 64) rng[1] = rs_entry_of(poff, 0, n, 16ull * last);
  __syncthreads();
  q = base + threadIdx.x;
  const bool have = q < end;
  entry = have ? rs_entry_of(poff, rng[0], rng[1] + 1, 16ull * q) : 0;
  return have;
}
// A block's chunks: the b-th of gridDim.x contiguous ranges of whole RG_BLOCK rounds.  Contiguous, so that
// a thread's successive chunks (RG_BLOCK apart) stay inside a long entry.
__device__ __forceinline__ void rs_block_range(uint64_t nchunks, uint64_t& b0, uint64_t& b1) {
  const uint64_t per = ((nchunks + gridDim.x - 1) / gridDim.x + RG_BLOCK - 1) / RG_BLOCK * RG_BLOCK;
  b0 = blockIdx.x * per < nchunks ? blockIdx.x * per : nchunks;
  b1 = b0 + per < nchunks ? b0 + per : nchunks;
}
// gc and amb added to entry i of the lanes with todo, aggregated in the wave; every lane of the wave calls it
__device__ __forceinline__ void rs_add_counts(bool todo, uint64_t i, ull gc, ull amb, const RsTab& T) {
  const bool own = rg_by_label(todo, (ull)i, [&](ull i0, bool mine, ull, bool leader) {
    const ull sg = rg_wave_sum(mine ? gc : 0ull), sa = rg_wave_sum(mine ? amb : 0ull);
    if (leader) {
      if (sg) RG_ADD(T.gc + i0, sg);
      if (sa) RG_ADD(T.amb + i0, sa);
    }
  });
  if (own) {
    if (gc) RG_ADD(T.gc + i, gc);
    if (amb) RG_ADD(T.amb + i, amb);
  }
}
// sixteen 2-bit groups -> 16 letters
__device__ __forceinline__ uint4 rs_ascii(uint32_t x) {
  return make_uint4(__builtin_amdgcn_perm(RS_ACGT, RS_ACGT, unpack4(x, 0)),
                    __builtin_amdgcn_perm(RS_ACGT, RS_ACGT, unpack4(x, 1)),
                    __builtin_amdgcn_perm(RS_ACGT, RS_ACGT, unpack4(x, 2)),
                    __builtin_amdgcn_perm(RS_ACGT, RS_ACGT, unpack4(x, 3)));
}
// the low m bytes of a chunk kept, the others zero (1 <= m <= 16)
__device__ __forceinline__ uint4 rs_keep(uint4 v, uint32_t m) {
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int k = (int)m - 4 * d;                          // bytes of word d that are real
    w[d] &= k >= 4 ? 0xFFFFFFFFu : k <= 0 ? 0u : (1u << (8 * k)) - 1u;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
// lastw: the index of the stream's last packed word (no word past it is read)
__global__ void __launch_bounds__(RG_BLOCK) k_rs_decode(PackedCls pc, const long long* __restrict__ rec_start,
                                                        ull lastw, RsTab T, uint64_t n, uint64_t nchunks,
                                                        uint4* __restrict__ blob) {
  __shared__ ull rng[2];
  uint64_t b0, b1;
  rs_block_range(nchunks, b0, b1);
  // the entry the thread is in, and its counts there: added to the table when the thread leaves the entry
  // (one atomic per wave and entry, not per chunk: a long entry's counter is one address)
  uint64_t cur = RS_NONE;
  ull poff = 0, len = 0, gc = 0, amb = 0;
  long long g0 = 0, h0 = 0;                                // stream indices of the entry's first and last base
  bool fw = true;
  // (whole blocks step together: every thread meets the barriers, every lane of a wave runs rg_by_label)
  for (uint64_t base = b0; base < b1; base += RG_BLOCK) {
    uint64_t q, i;
    const bool have = rs_chunk_entry(T.poff, n, base, b1, rng, q, i);
    const bool moved = have && i != cur;
    rs_add_counts(moved && (gc | amb), cur, gc, amb, T);
    if (moved) {
      const long long s = T.start[i], e = T.end[i], r0 = rec_start[T.rec[i]];
      cur = i;
      poff = T.poff[i];
      len = T.len[i];
      g0 = r0 + (s < e ? s : e);
      h0 = r0 + (s < e ? e : s) - 1;
      fw = T.strand[i] == 1;
      gc = amb = 0;
    }
    if (have) {
      const ull j = 16ull * q - poff;                                // the chunk is letters j .. j + m - 1 of the entry
      const uint32_t m = len - j < 16ull ? (uint32_t)(len - j) : 16u;
      // source bases: forward g, g + 1, ...; reverse h, h - 1, ... (all m of them inside the record)
      const long long g = g0 + (long long)j, h = h0 - (long long)j;
      const long long first = fw ? g : h - (long long)m + 1, lastb = fw ? g + (long long)m - 1 : h;
      uint4 v;
      if (!(pc.e16[first >> 4] | pc.e16[lastb >> 4])) {
        // the 16 bases a .. a + 15 as one word: a = g, or h - 15 (which may lie before the stream: those
        // bases are none of the m real ones, and the word index is clamped like the one past the end)
        const long long a = fw ? g : h - 15;
        const long long wa = a >> 4;
        const ull w0 = wa < 0 ? 0ull : (ull)wa, w1 = (ull)(wa + 1) > lastw ? lastw : (ull)(wa + 1);
        uint32_t x = __funnelshift_r(pc.p2[w0], pc.p2[w1], 2u * (uint32_t)(a & 15));
        if (!fw) {
          x = __brev(x);                                             // the groups reversed, their two bits too
          x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);   // ... and put back
          x = ~x;                                                    // the complement
        }
        v = rs_keep(rs_ascii(x), m);
        const uint32_t real = m < 16u ? (1u << (2u * m)) - 1u : 0xFFFFFFFFu;
        gc += (ull)__popc((x ^ (x >> 1)) & 0x55555555u & real);      // C = 01, G = 10
      } else {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t t = 0; t < 16; ++t) {
          if (t >= m) continue;
          uint32_t cl = pc[fw ? g + (long long)t : h - (long long)t];
          if (!fw) cl = comp_class(cl);
          const uint32_t ch = cl < 4u ? (RS_ACGT >> (8u * cl)) & 0xFFu : (uint32_t)'N';
          gc += cl == CLS_C || cl == CLS_G;
          amb += cl >= 4u;
          w[t >> 2] |= ch << (8u * (t & 3u));
        }
        v = make_uint4(w[0], w[1], w[2], w[3]);
      }
      blob[q] = v;                                                   // (the bytes past the entry's end: zero)
    }
  }
  rs_add_counts((gc | amb) != 0, cur, gc, amb, T);
}

// ------------------------------------------------------------ e. texts
// every entry's letters from the blob to dst + dst_off[entry] (RS_NONE: the entry is left out), a 16-byte
// piece per thread
struct __attribute__((packed)) RsPiece {
  uint32_t w[4];
};
__global__ void __launch_bounds__(RG_BLOCK) k_rs_copy(const uint4* __restrict__ blob, RsTab T, uint64_t n,
                                                      uint64_t nchunks, const ull* __restrict__ dst_off,
                                                      char* __restrict__ dst) {
  __shared__ ull rng[2];
  uint64_t b0, b1;
  rs_block_range(nchunks, b0, b1);
  for (uint64_t base = b0; base < b1; base += RG_BLOCK) {
    uint64_t q, i;
    if (!rs_chunk_entry(T.poff, n, base, b1, rng, q, i) || dst_off[i] == RS_NONE) continue;
    const ull j = 16ull * q - T.poff[i], len = T.len[i];
    const uint32_t m = len - j < 16ull ? (uint32_t)(len - j) : 16u;
    const uint4 v = blob[q];
    char* o = dst + dst_off[i] + j;
    if (m == 16u) {
      *reinterpret_cast<RsPiece*>(o) = RsPiece{{v.x, v.y, v.z, v.w}};   // (any alignment)
    } else {
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t t = 0; t < 15; ++t)
        if (t < m) o[t] = (char)((w[t >> 2] >> (8u * (t & 3u))) & 0xFFu);
    }
  }
}

// ><label> <name>:<lo>-<hi>:<+|-> len=<len>\n<sequence>\n; the line leaves a gap for the letters
// (sdst[i]: where entry i's gap starts in the text)
struct FastaLine {
  RsTab T;
  const char* names;
  const long long* name_off;
  ull* sdst;
  template <class S>
  __device__ __forceinline__ void operator()(S& s, uint64_t i) const {
    const long long r = T.rec[i], st = T.start[i], e = T.end[i];
    s.ch('>'); s.dec((ull)T.label[i]); s.ch(' ');
    s.bytes(names + name_off[r], (ull)(name_off[r + 1] - name_off[r]));
    s.ch(':'); s.sdec(st < e ? st : e); s.ch('-'); s.sdec(st < e ? e : st);
    s.ch(':'); s.ch(T.strand[i] == 1 ? '+' : '-');
    s.lit(" len="); s.dec(T.len[i]); s.ch('\n');
    const ull at = s.gap(T.len[i]);
    if constexpr (S::writes) sdst[i] = at;
    s.ch('\n');
  }
};
// mismatch += the entries whose label or length is not the node's
__global__ void k_rs_match(RsTab T, RgNodes N, uint64_t n, ull* __restrict__ mismatch) {
  RG_LOOP(i, n)
    if (T.label[i] != N.label[i] || T.len[i] != N.maxlen[i]) RG_ADD(mismatch, 1ull);
}

void region_seqs(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                 uint32_t G, uint64_t* n_regions, uint64_t* n_bases, uint64_t* n_skipped) {
  // ---- arguments (and a parse): everything refused here leaves the previous result in place
  if (rec_group && !c.parsed) throw Error(-22, "pg_region_seqs: no parse (the bases come from the context's parse)");
  const RowInput in = row_input(c, "pg_region_seqs", h_rows5, n_rows, rec_group, n_records, G, true);
  const uint64_t n = in.n;
  const unsigned grid_rows = in.grid_rows;
  const long long* rows = in.rows;
  const int* d_group = in.group;

  // ---- a. the dense size and the coordinates, checked before anything is allocated or replaced
  const RowScan sc = row_scan(c, "pg_region_seqs", in, nullptr, c.rec_len.as<long long>());
  const uint64_t L = sc.L;

  DevBuf dense, seen, labs, tab, plen, blob;
  uint64_t nr = 0, bases = 0, pad = 0;
  if (L) {
    // ---- b. dense per-label arrays: the largest length, the first row that has it
    dense.reserve(16 * (size_t)L);
    ull *d_max = dense.as<ull>(), *d_row = d_max + L;
    PG_HIP(hipMemsetAsync(d_max, 0, 8 * (size_t)L, c.stream));
    PG_HIP(hipMemsetAsync(d_row, 0xFF, 8 * (size_t)L, c.stream));
    RG_LAUNCH(k_rs_max, grid_rows, rows, n, d_group, d_max);
    RG_LAUNCH(k_rs_first, grid_rows, rows, n, d_group, d_max, d_row);
    // ---- c. the labels seen, their rows, the two offsets
    seen.reserve(L + 16);
    RG_LAUNCH(k_rs_seen, grid_for(L, RG_BLOCK, 8192), d_row, L, seen.as<uint8_t>());
    nr = labels_seen(c, seen.as<uint8_t>(), L, labs);
    tab.reserve(RsTab::bytes(nr));
    RsTab T(tab, nr);
    plen.reserve(8 * (nr + 1));
    PG_HIP(hipMemcpyAsync(T.label, labs.p, 8 * nr, hipMemcpyDeviceToDevice, c.stream));
    RG_LAUNCH(k_rs_gather, grid_for(nr, RG_BLOCK, 8192), T, nr, rows, d_max, d_row, plen.as<ull>());
    bases = excl_scan_total(c, T.len, T.off, nr);
    pad = excl_scan_total(c, plen.as<ull>(), T.poff, nr);
  } else {
    tab.reserve(RsTab::bytes(0));
  }
  // ---- d. the letters
  blob.reserve(pad + 16);
  if (pad) {
    RsTab T(tab, nr);
    const uint64_t nchunks = pad / 16;
    c.t_rs.init();
    c.t_rs.start(c.stream);
    RG_LAUNCH(k_rs_decode, grid_for(nchunks, RG_BLOCK, RS_DECODE_GRID), packed_cls(c), c.rec_start.as<long long>(),
              (ull)((c.n_cls - 1) >> 4), T, nr, nchunks, blob.as<uint4>());
    c.t_rs.stop(c.stream);
  }
  c.sync();
  c.ms_rs_decode = pad ? c.t_rs.ms() : 0.0;
  c.rs_chunks = pad / 16;
  // ---- the new result replaces the previous one
  c.rs_tab.swap(tab);
  c.rs_blob.swap(blob);
  c.rs_n = nr;
  c.rs_bases = bases;
  c.rs_pad = pad;
  c.rs_names = h_rows5 ? sc.names : c.n_records;
  c.rs_ready = true;
  if (n_regions) *n_regions = nr;
  if (n_bases) *n_bases = bases;
  if (n_skipped) *n_skipped = sc.skipped;
}

void region_seqs_table(Ctx& c, int64_t* label, int64_t* row, int64_t* record, int64_t* start, int64_t* end,
                       int64_t* strand, uint64_t* len, uint64_t* gc, uint64_t* amb, uint64_t* offset, uint64_t cap) {
  need(c.rs_ready, "pg_region_seqs_table", NEED_SEQS);
  const uint64_t n = c.rs_n;
  if (cap < n) throw Error(-34, "pg_region_seqs_table: buffer too small");
  if (!n) return;
  RsTab T(c.rs_tab, n);
  get(c, label, T.label, 8 * n);
  get(c, row, T.row, 8 * n);
  get(c, record, T.rec, 8 * n);
  get(c, start, T.start, 8 * n);
  get(c, end, T.end, 8 * n);
  get(c, strand, T.strand, 8 * n);
  get(c, len, T.len, 8 * n);
  get(c, gc, T.gc, 8 * n);
  get(c, amb, T.amb, 8 * n);
  get(c, offset, T.off, 8 * n);
  c.sync();
}

void region_seqs_copy(Ctx& c, const ull* d_dst_off, char* d_dst) {
  if (!c.rs_pad) return;
  const uint64_t nchunks = c.rs_pad / 16;
  RG_LAUNCH(k_rs_copy, grid_for(nchunks, RG_BLOCK, RS_DECODE_GRID), c.rs_blob.as<uint4>(), RsTab(c.rs_tab, c.rs_n),
            c.rs_n, nchunks, d_dst_off, d_dst);
}

const ull* region_seqs_len(Ctx& c) { return RsTab(c.rs_tab, c.rs_n).len; }

// the letters of the last region_seqs, the entries one after another: their number (out null), or copied into out
uint64_t region_seqs_bases(Ctx& c, uint8_t* out, uint64_t cap) {
  need(c.rs_ready, "pg_region_seqs_bases", NEED_SEQS);
  if (!out) return c.rs_bases;
  if (cap < c.rs_bases) throw Error(-34, "pg_region_seqs_bases: buffer too small");
  if (!c.rs_bases) return 0;
  DevBuf flat;
  flat.reserve(c.rs_bases + 16);
  region_seqs_copy(c, RsTab(c.rs_tab, c.rs_n).off, flat.as<char>());
  PG_HIP(hipMemcpyAsync(out, flat.p, c.rs_bases, hipMemcpyDeviceToHost, c.stream));
  c.sync();
  return c.rs_bases;
}

void region_seqs_match(Ctx& c, const char* what) {
  need(c.rs_ready, what, NEED_SEQS);
  need(c.rg_ready, what, NEED_GRAPH);
  ull bad = c.rs_n != c.rg_nn;
  if (!bad && c.rs_n) {
    DevBuf ctr;
    ctr.reserve(16);
    PG_HIP(hipMemsetAsync(ctr.p, 0, 8, c.stream));
    RG_LAUNCH(k_rs_match, grid_for(c.rs_n, RG_BLOCK, 8192), RsTab(c.rs_tab, c.rs_n), RgNodes(c.rg_nodes, c.rg_nn),
              c.rs_n, ctr.as<ull>());
    PG_HIP(hipMemcpyAsync(&bad, ctr.p, 8, hipMemcpyDeviceToHost, c.stream));
    c.sync();
  }
  if (bad)
    throw Error(-22, std::string(what) + ": the region sequences and the region graph are not of the same rows "
                                         "and groups (labels or lengths differ)");
}

// the FASTA text of the last region_seqs with this call's record names: its size (out null, fd < 0),
// copied into out, or written to fd
uint64_t format_region_fasta(Ctx& c, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                             uint64_t cap, int fd) {
  const char* what = fd >= 0 ? "pg_region_fasta_fd" : "pg_region_fasta";
  need(c.rs_ready, what, NEED_SEQS);
  const DevNames nm = names_upload(c, what, names, name_off, n_names, c.rs_names, "entries");
  const uint64_t n = c.rs_n;
  DevBuf toff, sdst, text;
  FastaLine line{RsTab(c.rs_tab, n), nm.bytes, nm.off, nullptr};
  const uint64_t total = text_measure(c, line, n, toff);
  if (!text_wanted(total, out, cap, fd, what) || !total) return total;
  text.reserve(total + 16);
  sdst.reserve(8 * (n + 1));
  line.sdst = sdst.as<ull>();
  text_write(c, line, n, toff, text.as<char>());
  region_seqs_copy(c, sdst.as<ull>(), text.as<char>());
  return text_out(c, text.p, total, out, cap, fd, what, what);
}

}  // namespace pg
