// pg_region.hip — the region graph of the region rows: which region follows
// which along a genome.  Nodes are the labels, links the ordered pairs of
// labels on adjacent rows of one walk, paths the walks themselves; the links
// table's text and the whole graph as GFA 1.
//
// Rows are (record, start, end, strand, label); rec_group maps a record to
// its genome (or -1).  A row is used iff label >= 0 and its record has a
// genome (pg_freq's rule).  A run is a maximal stretch of consecutive used
// rows of one record and strand; a link (a, b) is two adjacent rows of a run.
// Tables are dense in the label (L = 1 + the largest used label).
//
// Steps, each its own launch on c.stream (no hand-shake inside a kernel):
//   a. k_row_scan   per row a flag byte (used, run head); the largest used
//                   label and record, the used and the skipped rows.  The row
//                   before a tile's first one is loaded with the tile (one
//                   halo row), so a run that crosses a tile is not cut.
//      two scans of the flag bits: used rows / run heads before every row
//      (the step index and the run id of a row)
//   b. k_rg_emit    per used row its step (label, first / last of its run);
//                   run heads and tails fill the path table; every other used
//                   row emits the pair key a << lb | b and its genome
//   c. two stable radix sorts (by genome, then by key) give (key, genome)
//      order; k_rg_lflags marks where the key and where (key, genome) change,
//      two scans number the links and count the changes, k_rg_links /
//      k_rg_linkfin fill from, to, count and n_genomes
//   d. k_rg_accum   rows and max length per label, k_rg_degree the distinct
//                   links leaving and entering it, into dense arrays with
//                   integer atomics at agent scope; select + k_rg_gather the
//                   labels seen
//   e. LinkLine    the links text, kept on the device;
//      GfaLine     the GFA text, made by every call with its own names: one
//                   thread per S line, L line and path step (a path's header
//                   belongs to its first step, its trailer to its last: no
//                   thread walks a path).  Both go through pg_text.h, which
//                   counts and writes a line by one definition.
//
// Contention (d): at a low weight cut one label holds every other row (rows
// A b A c A d ..., see pg_freq.hip) and is an end of most links.  Each wave
// therefore aggregates first, as k_fr_accum does: it takes the label of its
// first unserved lane, ballots the lanes that share it, and one lane issues
// the atomics.  Links are sorted by (a, b), so the lanes of a wave share a.
//
// Every sum is an integer and every atomic commutes: the result depends on
// the input alone, whatever the schedule.
//
// The file begins with the host side of what pg_freq, pg_region_graph and
// pg_region_seqs share (declared in pg_internal.h; the device side is
// pg_region.h): row_input, k_row_scan / row_scan, labels_seen, text_out and
// names_upload.
#include <cstring>

#include "pg_region.h"

namespace pg {

#define RG_FIRST 1u               // flag byte of a step: first of its path
#define RG_LAST 2u                 //                      last of its path
#define RG_LINK 1u                 // flag byte of a sorted pair: its key differs from the pair before
#define RG_GCHG 2u                 //                             its (key, genome) differs

// ------------------------------------------------------------ the shared front end
// out[0] = 1 + the largest used label (0: none), out[1] = used rows, out[2] = skipped rows,
// out[3] = 1 + the largest record of a used row, out[4] = used rows with lo < 0 or hi > rec_len[record]
// (RECLEN only).  FLAGS: rf[i] = RG_USED | RG_HEAD of row i; the row before a tile's first one is loaded
// with the tile (one halo row), so a run that crosses a tile is not cut.
template <bool FLAGS, bool RECLEN>
__global__ void __launch_bounds__(RG_BLOCK) k_row_scan(const long long* __restrict__ rows, uint64_t n,
                                                       const int* __restrict__ rec_group, uint8_t* __restrict__ rf,
                                                       const long long* __restrict__ rec_len, ull* __restrict__ out) {
  __shared__ long long lds[RG_TILE_WORDS(FLAGS)];
  const uint64_t ntiles = (n + RG_BLOCK - 1) / RG_BLOCK;
  ull top = 0, used = 0, skipped = 0, toprec = 0, bad = 0;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    RgRow r, p;
    bool hp;
    if (rg_load_tile<FLAGS>(rows, n, t, lds, r, p, hp)) {
      const bool u = rs_used(r, rec_group);
      if (FLAGS) {
        // the row before continues into this one: used, same record and strand
        const bool cont = u && hp && p.rec == r.rec && p.strand == r.strand && rs_used(p, rec_group);
        rf[t * RG_BLOCK + threadIdx.x] = (uint8_t)((u ? RG_USED : 0u) | (u && !cont ? RG_HEAD : 0u));
      }
      used += u;
      skipped += !u;
      if (u) {
        if (RECLEN) {
          const long long lo = r.start < r.end ? r.start : r.end, hi = r.start < r.end ? r.end : r.start;
          bad += lo < 0 || hi > rec_len[r.rec];
        }
        if ((ull)r.label + 1 > top) top = (ull)r.label + 1;
        if ((ull)r.rec + 1 > toprec) toprec = (ull)r.rec + 1;
      }
    }
  }
  top = rg_wave_max(top);
  toprec = rg_wave_max(toprec);
  used = rg_wave_sum(used);
  skipped = rg_wave_sum(skipped);
  if (RECLEN) bad = rg_wave_sum(bad);
  // the block's waves meet in LDS: the five counters are single words that every wave of the grid would
  // otherwise queue on, so each takes one atomic per block
  __shared__ ull tot[5];
  if (threadIdx.x < 5) tot[threadIdx.x] = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&tot[0], top);
    atomicAdd(&tot[1], used);
    atomicAdd(&tot[2], skipped);
    atomicMax(&tot[3], toprec);
    atomicAdd(&tot[4], bad);
  }
  __syncthreads();
  if (threadIdx.x < 5 && tot[threadIdx.x]) {
    if (threadIdx.x == 0 || threadIdx.x == 3) RG_MAX(out + threadIdx.x, tot[threadIdx.x]);
    else RG_ADD(out + threadIdx.x, tot[threadIdx.x]);
  }
}

RowInput row_input(Ctx& c, const char* what, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group,
                   uint64_t n_records, uint32_t G, bool records_match_always) {
  const std::string w = std::string(what) + ": ";
  const auto records_match = [&] {
    if (n_records != c.n_records)
      throw Error(-22, w + std::to_string(n_records) + " records, the context has " + std::to_string(c.n_records));
  };
  if (!rec_group) throw Error(-22, w + "rec_group is NULL");
  if (records_match_always) records_match();
  if (!h_rows5) {
    if (!c.rows_ready) throw Error(-22, w + "no row pass (call pg_rows first, or pass rows)");
    if (!records_match_always) records_match();
    n_rows = c.n_rows;
  }
  for (uint64_t r = 0; r < n_records; ++r)
    if (rec_group[r] < -1 || (int64_t)rec_group[r] >= (int64_t)G)
      throw Error(-22, w + "rec_group[" + std::to_string(r) + "] = " + std::to_string(rec_group[r]) +
                           " is outside [-1, " + std::to_string(G) + ")");
  if (h_rows5)
    for (uint64_t i = 0; i < n_rows; ++i)
      if (h_rows5[5 * i] < 0 || (uint64_t)h_rows5[5 * i] >= n_records)
        throw Error(-22, w + "row " + std::to_string(i) + " names record " + std::to_string(h_rows5[5 * i]) +
                             " of " + std::to_string(n_records));
  if (G == 0 && n_rows) throw Error(-22, w + "n_groups is 0 with rows");

  RowInput in;
  in.n = n_rows;
  in.grid_rows = grid_for((n_rows + RG_BLOCK - 1) / RG_BLOCK, 1, 8u * (unsigned)std::max(1, c.n_cu));
  in.rows = c.rows_buf.as<long long>();
  if (h_rows5) {
    in.up.reserve(40 * (n_rows + 1));
    if (n_rows) PG_HIP(hipMemcpyAsync(in.up.p, h_rows5, 40 * n_rows, hipMemcpyHostToDevice, c.stream));
    in.rows = in.up.as<long long>();
  }
  in.grpmap.reserve(4 * (n_records + 1));
  if (n_records) PG_HIP(hipMemcpyAsync(in.grpmap.p, rec_group, 4 * n_records, hipMemcpyHostToDevice, c.stream));
  in.group = in.grpmap.as<int>();
  return in;
}

RowScan row_scan(Ctx& c, const char* what, const RowInput& in, uint8_t* rf, const long long* rec_len) {
  ull h[5] = {0, 0, 0, 0, 0};
  if (in.n) {
    DevBuf ctr;
    ctr.reserve(40);
    PG_HIP(hipMemsetAsync(ctr.p, 0, 40, c.stream));
    if (rf && rec_len) {
      PG_HIP(hipMemsetAsync(rf + in.n, 0, 1, c.stream));
      RG_LAUNCH((k_row_scan<true, true>), in.grid_rows, in.rows, in.n, in.group, rf, rec_len, ctr.as<ull>());
    } else if (rf) {
      PG_HIP(hipMemsetAsync(rf + in.n, 0, 1, c.stream));
      RG_LAUNCH((k_row_scan<true, false>), in.grid_rows, in.rows, in.n, in.group, rf, rec_len, ctr.as<ull>());
    } else if (rec_len) {
      RG_LAUNCH((k_row_scan<false, true>), in.grid_rows, in.rows, in.n, in.group, rf, rec_len, ctr.as<ull>());
    } else {
      RG_LAUNCH((k_row_scan<false, false>), in.grid_rows, in.rows, in.n, in.group, rf, rec_len, ctr.as<ull>());
    }
    PG_HIP(hipMemcpyAsync(h, ctr.p, 40, hipMemcpyDeviceToHost, c.stream));
    c.sync();
  }
  if (h[4]) throw Error(-22, std::string(what) + ": " + std::to_string(h[4]) + " used rows reach outside their record");
  if (h[0] > (1ull << 31))
    throw Error(-34, std::string(what) + ": the largest used label is " + std::to_string(h[0] - 1) +
                         ": the dense tables take labels below 2^31");
  return RowScan{h[0], h[1], h[2], h[3]};
}

uint64_t labels_seen(Ctx& c, const uint8_t* flag, uint64_t L, DevBuf& labs) {
  DevBuf cnt;
  labs.reserve(8 * (L + 1));
  return select_flagged(c, rocprim::counting_iterator<long long>(0), flag, labs.as<long long>(), L, cnt);
}

bool text_wanted(uint64_t total, const char* out, uint64_t cap, int fd, const char* what) {
  if (!out && fd < 0) return false;
  if (out && cap < total) throw Error(-34, std::string(what) + ": buffer too small");
  return true;
}
uint64_t text_out(Ctx& c, const void* d_text, uint64_t total, char* out, uint64_t cap, int fd, const char* what,
                  const char* what_fd) {
  if (!text_wanted(total, out, cap, fd, what) || !total) return total;
  if (out) PG_HIP(hipMemcpyAsync(out, d_text, total, hipMemcpyDeviceToHost, c.stream));
  c.sync();                                                // (text_to_fd reads on streams of its own)
  if (!out) text_to_fd(c, static_cast<const uint8_t*>(d_text), total, fd, what_fd);
  return total;
}

DevNames names_upload(Ctx& c, const char* what, const char* names, const int64_t* name_off, uint64_t n_names,
                      uint64_t n_needed, const char* noun) {
  if (!name_off) throw Error(-22, std::string(what) + ": name_off is NULL");
  if (n_names < n_needed)
    throw Error(-22, std::string(what) + ": " + std::to_string(n_names) + " names, the " + noun + " need " +
                         std::to_string(n_needed));
  for (uint64_t r = 0; r < n_names; ++r)
    if (name_off[r] < 0 || name_off[r + 1] < name_off[r])
      throw Error(-22, std::string(what) + ": name_off is not ascending from 0 up");
  const uint64_t nbytes = (uint64_t)name_off[n_names];
  if (nbytes && !names) throw Error(-22, std::string(what) + ": names is NULL");
  DevNames d;
  d.buf.reserve(8 * (n_names + 1) + nbytes + 16);
  long long* off = d.buf.as<long long>();
  char* bytes = reinterpret_cast<char*>(off + n_names + 1);
  PG_HIP(hipMemcpyAsync(off, name_off, 8 * (n_names + 1), hipMemcpyHostToDevice, c.stream));
  if (nbytes) PG_HIP(hipMemcpyAsync(bytes, names, nbytes, hipMemcpyHostToDevice, c.stream));
  d.off = off;
  d.bytes = bytes;
  return d;
}

// ------------------------------------------------------------ b. steps, paths, pairs
// the path table's columns (np entries); lo / hi / steps hold the head's start / end and the
// tail's step index until k_rg_pathfin
struct RgPaths {
  long long *rec, *strand, *lo, *hi;
  ull *steps, *first;
  static size_t bytes(uint64_t np) { return 48 * np + 64; }
  RgPaths(const DevBuf& b, uint64_t np) {
    rec = b.as<long long>();
    strand = rec + np;
    lo = strand + np;
    hi = lo + np;
    steps = reinterpret_cast<ull*>(hi + np);
    first = steps + np;
  }
};
// uoff[i] / hoff[i]: the used rows / run heads before row i; rf[n] = 0
__global__ void __launch_bounds__(RG_BLOCK) k_rg_emit(const long long* __restrict__ rows, uint64_t n,
                                                      const int* __restrict__ rec_group,
                                                      const uint8_t* __restrict__ rf, const ull* __restrict__ uoff,
                                                      const ull* __restrict__ hoff, int lb,
                                                      long long* __restrict__ step_label,
                                                      uint8_t* __restrict__ step_flag, RgPaths P,
                                                      long long* __restrict__ tail_start,
                                                      long long* __restrict__ tail_end, ull* __restrict__ pkey,
                                                      ull* __restrict__ pgen) {
  __shared__ long long lds[RG_TILE_WORDS(true)];
  const uint64_t ntiles = (n + RG_BLOCK - 1) / RG_BLOCK;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    RgRow r, p;
    bool hp;
    if (!rg_load_tile<true>(rows, n, t, lds, r, p, hp)) continue;
    const uint64_t i = t * RG_BLOCK + threadIdx.x;
    const uint32_t f = rf[i];
    if (!(f & RG_USED)) continue;
    const bool head = (f & RG_HEAD) != 0;
    const uint32_t fn = rf[i + 1];                         // (rf[n] = 0)
    const bool last = !((fn & RG_USED) && !(fn & RG_HEAD));
    const ull s = uoff[i];
    const ull pid = hoff[i] + (head ? 1 : 0) - 1;          // (a used row that is no head has a head before it)
    step_label[s] = r.label;
    step_flag[s] = (uint8_t)((head ? RG_FIRST : 0u) | (last ? RG_LAST : 0u));
    if (head) {
      P.rec[pid] = r.rec;
      P.strand[pid] = r.strand;
      P.lo[pid] = r.start;
      P.hi[pid] = r.end;
      P.first[pid] = s;
    } else {
      const ull j = s - hoff[i];                           // the used rows before i that are no heads
      pkey[j] = ((ull)p.label << lb) | (ull)r.label;
      pgen[j] = (ull)(uint32_t)rec_group[r.rec];
    }
    if (last) {
      tail_start[pid] = r.start;
      tail_end[pid] = r.end;
      P.steps[pid] = s;
    }
  }
}
__global__ void k_rg_pathfin(RgPaths P, const long long* __restrict__ tail_start,
                             const long long* __restrict__ tail_end, uint64_t np) {
  RG_LOOP(i, np) {
    if (tail_start[i] < P.lo[i]) P.lo[i] = tail_start[i];
    if (tail_end[i] > P.hi[i]) P.hi[i] = tail_end[i];
    P.steps[i] = P.steps[i] - P.first[i] + 1;
  }
}

// ------------------------------------------------------------ c. links
struct RgLinks {
  long long *from, *to;
  ull* count;
  uint32_t* ngen;
  static size_t bytes(uint64_t nl) { return 28 * nl + 64; }
  RgLinks(const DevBuf& b, uint64_t nl) {
    from = b.as<long long>();
    to = from + nl;
    count = reinterpret_cast<ull*>(to + nl);
    ngen = reinterpret_cast<uint32_t*>(count + nl);
  }
};
// key / gen: the pairs in (key, genome) order; lf[np] = 0
__global__ void k_rg_lflags(const ull* __restrict__ key, const ull* __restrict__ gen, uint64_t np,
                            uint8_t* __restrict__ lf) {
  RG_LOOP(j, np) {
    const bool link = j == 0 || key[j] != key[j - 1];
    const bool gchg = link || gen[j] != gen[j - 1];
    lf[j] = (uint8_t)((link ? RG_LINK : 0u) | (gchg ? RG_GCHG : 0u));
  }
}
// lnum[j] / gsum[j]: the links / (key, genome) changes before pair j
__global__ void k_rg_links(const ull* __restrict__ key, const uint8_t* __restrict__ lf, const ull* __restrict__ lnum,
                           const ull* __restrict__ gsum, uint64_t np, int lb, RgLinks T, ull* __restrict__ lpos,
                           ull* __restrict__ gpos) {
  RG_LOOP(j, np) {
    if (!(lf[j] & RG_LINK)) continue;
    const ull l = lnum[j];
    T.from[l] = (long long)(key[j] >> lb);
    T.to[l] = (long long)(key[j] & ((1ull << lb) - 1ull));
    lpos[l] = j;
    gpos[l] = gsum[j];
  }
}
__global__ void k_rg_linkfin(RgLinks T, const ull* __restrict__ lpos, const ull* __restrict__ gpos, uint64_t nl,
                             ull np, ull ng) {
  RG_LOOP(l, nl) {
    const bool more = l + 1 < nl;
    T.count[l] = (more ? lpos[l + 1] : np) - lpos[l];
    T.ngen[l] = (uint32_t)((more ? gpos[l + 1] : ng) - gpos[l]);
  }
}

// ------------------------------------------------------------ d. nodes
__global__ void __launch_bounds__(RG_BLOCK) k_rg_accum(const long long* __restrict__ rows, uint64_t n,
                                                       const uint8_t* __restrict__ rf, ull* d_rows, ull* d_max) {
  __shared__ long long lds[RG_TILE_WORDS(false)];
  const uint64_t ntiles = (n + RG_BLOCK - 1) / RG_BLOCK;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    RgRow r;
    const bool have = rg_load_tile(rows, n, t, lds, r);
    const bool todo = have && (rf[t * RG_BLOCK + threadIdx.x] & RG_USED);
    const ull lab = todo ? (ull)r.label : 0ull;
    const ull len = todo ? rg_len(r) : 0ull;
    // every lane of the wave runs the loop (its conditions are ballots)
    const bool own = rg_by_label(todo, lab, [&](ull lab0, bool mine, ull cnt, bool leader) {
      const ull hi = rg_wave_max(mine ? len : 0ull);
      if (leader) {
        RG_ADD(d_rows + lab0, cnt);
        RG_MAX(d_max + lab0, hi);
      }
    });
    if (own) {
      RG_ADD(d_rows + lab, 1ull);
      RG_MAX(d_max + lab, len);
    }
  }
}
// one count per link into its two ends: d_out[from], d_in[to]
__global__ void __launch_bounds__(RG_BLOCK) k_rg_degree(RgLinks T, uint64_t nl, uint32_t* d_out, uint32_t* d_in) {
  // (whole blocks step together: every lane of a wave runs rg_by_label)
  for (uint64_t base = blockIdx.x * (uint64_t)RG_BLOCK; base < nl; base += (uint64_t)gridDim.x * RG_BLOCK) {
    const uint64_t l = base + threadIdx.x;
    const bool todo = l < nl;
    const ull a = todo ? (ull)T.from[l] : 0ull, b = todo ? (ull)T.to[l] : 0ull;
    if (rg_by_label(todo, a, [&](ull lab0, bool, ull cnt, bool leader) {
          if (leader) RG_ADD(d_out + lab0, (uint32_t)cnt);
        }))
      RG_ADD(d_out + a, 1u);
    if (rg_by_label(todo, b, [&](ull lab0, bool, ull cnt, bool leader) {
          if (leader) RG_ADD(d_in + lab0, (uint32_t)cnt);
        }))
      RG_ADD(d_in + b, 1u);
  }
}
__global__ void k_rg_seen(const ull* __restrict__ d_rows, uint64_t L, uint8_t* __restrict__ flag) {
  RG_LOOP(l, L) flag[l] = d_rows[l] != 0;
}
__global__ void k_rg_gather(RgNodes T, uint64_t nn, const ull* __restrict__ d_rows, const ull* __restrict__ d_max,
                            const uint32_t* __restrict__ d_out, const uint32_t* __restrict__ d_in) {
  RG_LOOP(i, nn) {
    const uint64_t l = (uint64_t)T.label[i];
    T.rows[i] = d_rows[l];
    T.maxlen[i] = d_max[l];
    T.nout[i] = d_out[l];
    T.nin[i] = d_in[l];
  }
}

// ------------------------------------------------------------ e. text
#define RG_LINKS_HEADER "#from\tto\tcount\tgenomes\n"
#define RG_GFA_HEADER "H\tVN:Z:1.0\n"

// <from> <to> <count> <genomes>, tab separated
struct LinkLine {
  RgLinks T;
  template <class S>
  __device__ __forceinline__ void operator()(S& s, uint64_t i) const {
    s.dec((ull)T.from[i]); s.ch('\t');
    s.dec((ull)T.to[i]); s.ch('\t');
    s.dec(T.count[i]); s.ch('\t');
    s.dec(T.ngen[i]); s.ch('\n');
  }
};
// the path whose first step is s (there is one): the last p with first[p] <= s
__device__ __forceinline__ uint64_t rg_path_of(const ull* __restrict__ first, uint64_t np, ull s) {
  uint64_t lo = 0, hi = np;                                // first[lo] <= s < first[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= s) lo = mid; else hi = mid;
  }
  return lo;
}
// Item i of the GFA: nn S lines, then nl L lines, then nu path steps (a path's header belongs to its
// first step, its trailer to its last).  slen null: an S line carries `*`; otherwise node i's sequence
// of slen[i] letters, which the line leaves a gap for (sdst[i]: where the gap starts in the text)
struct GfaLine {
  RgNodes N;
  uint64_t nn;
  RgLinks T;
  uint64_t nl;
  const long long* step_label;
  const uint8_t* step_flag;
  RgPaths P;
  uint64_t np;
  const char* names;
  const long long* name_off;
  const ull* slen;
  ull* sdst;
  template <class S>
  __device__ __forceinline__ void operator()(S& s, uint64_t i) const {
    if (i < nn) {
      s.lit("S\t"); s.dec((ull)N.label[i]); s.ch('\t');
      if (slen) {
        const ull at = s.gap(slen[i]);
        if constexpr (S::writes) sdst[i] = at;
      } else {
        s.ch('*');
      }
      s.lit("\tLN:i:"); s.dec(N.maxlen[i]); s.ch('\n');
    } else if (i < nn + nl) {
      const uint64_t l = i - nn;
      s.lit("L\t"); s.dec((ull)T.from[l]);
      s.lit("\t+\t"); s.dec((ull)T.to[l]);
      s.lit("\t+\t0M\tRC:i:"); s.dec(T.count[l]);
      s.lit("\tgn:i:"); s.dec(T.ngen[l]); s.ch('\n');
    } else {
      const uint64_t st = i - nn - nl;
      const uint32_t f = step_flag[st];
      if (f & RG_FIRST) {
        const uint64_t p = rg_path_of(P.first, np, st);
        const long long r = P.rec[p];
        s.lit("P\t"); s.bytes(names + name_off[r], (ull)(name_off[r + 1] - name_off[r]));
        s.ch(':'); s.sdec(P.lo[p]); s.ch('-'); s.sdec(P.hi[p]);
        s.ch(':'); s.ch(P.strand[p] == 1 ? '+' : '-'); s.ch('\t');
      }
      s.dec((ull)step_label[st]); s.ch('+');
      if (f & RG_LAST) s.lit("\t*\n"); else s.ch(',');
    }
  }
};

void region_graph(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                  uint32_t G, uint64_t* n_nodes, uint64_t* n_links, uint64_t* n_paths, uint64_t* n_skipped) {
  // ---- arguments: everything refused here leaves the previous result in place
  const RowInput in = row_input(c, "pg_region_graph", h_rows5, n_rows, rec_group, n_records, G, false);
  const uint64_t n = in.n;
  const unsigned grid_rows = in.grid_rows;
  const long long* rows = in.rows;
  const int* d_group = in.group;

  // ---- a. the flags and the dense size, found before anything is allocated or replaced
  DevBuf rf;
  rf.reserve(n + 16);
  const RowScan sc = row_scan(c, "pg_region_graph", in, rf.as<uint8_t>(), nullptr);
  const uint64_t L = sc.L, nu = sc.used;
  const int lb = bits_for(L ? L - 1 : 0);                  // a pair key a << lb | b has at most 62 bits

  DevBuf uoff, hoff, steps, paths, tails, keyA, keyB, genA, genB, lf, lnum, gsum, lpos, links, dense, seen, labs,
      nodes, toff, text;
  uint64_t np = 0, npairs = 0, nl = 0, nn = 0;
  steps.reserve(9 * nu + 64);
  long long* step_label = steps.as<long long>();
  uint8_t* step_flag = reinterpret_cast<uint8_t*>(step_label + nu);
  if (nu) {
    // ---- the step index and the run id of every row
    uoff.reserve(8 * (n + 1));
    hoff.reserve(8 * (n + 1));
    const uint64_t used = scan_bit(c, rf.as<uint8_t>(), RG_USED, uoff.as<ull>(), n);
    np = scan_bit(c, rf.as<uint8_t>(), RG_HEAD, hoff.as<ull>(), n);
    if (used != nu || np == 0 || np > nu) throw Error(-5, "pg_region_graph: the scans disagree with the row pass");
    npairs = nu - np;
  }
  paths.reserve(RgPaths::bytes(np));
  RgPaths P(paths, np);
  if (nu) {
    // ---- b. steps, paths, pairs
    tails.reserve(16 * np + 16);
    keyA.reserve(8 * (npairs + 1));
    genA.reserve(8 * (npairs + 1));
    RG_LAUNCH(k_rg_emit, grid_rows, rows, n, d_group, rf.as<uint8_t>(), uoff.as<ull>(), hoff.as<ull>(), lb,
              step_label, step_flag, P, tails.as<long long>(), tails.as<long long>() + np, keyA.as<ull>(),
              genA.as<ull>());
    RG_LAUNCH(k_rg_pathfin, grid_for(np, RG_BLOCK, 8192), P, tails.as<long long>(), tails.as<long long>() + np, np);
  }
  if (npairs) {
    // ---- c. (key, genome) order: stable sorts by genome, then by key
    keyB.reserve(8 * (npairs + 1));
    genB.reserve(8 * (npairs + 1));
    sort_pairs(c, genA.as<ull>(), genB.as<ull>(), keyA.as<ull>(), keyB.as<ull>(), npairs, bits_for(G - 1));
    sort_pairs(c, keyB.as<ull>(), keyA.as<ull>(), genB.as<ull>(), genA.as<ull>(), npairs, 2 * lb);
    lf.reserve(npairs + 16);
    lnum.reserve(8 * (npairs + 1));
    gsum.reserve(8 * (npairs + 1));
    PG_HIP(hipMemsetAsync(lf.as<uint8_t>() + npairs, 0, 1, c.stream));
    RG_LAUNCH(k_rg_lflags, grid_for(npairs, RG_BLOCK, 8192), keyA.as<ull>(), genA.as<ull>(), npairs,
              lf.as<uint8_t>());
    nl = scan_bit(c, lf.as<uint8_t>(), RG_LINK, lnum.as<ull>(), npairs);
    const uint64_t ng = scan_bit(c, lf.as<uint8_t>(), RG_GCHG, gsum.as<ull>(), npairs);
    links.reserve(RgLinks::bytes(nl));
    lpos.reserve(16 * (nl + 1));
    RgLinks T(links, nl);
    RG_LAUNCH(k_rg_links, grid_for(npairs, RG_BLOCK, 8192), keyA.as<ull>(), lf.as<uint8_t>(), lnum.as<ull>(),
              gsum.as<ull>(), npairs, lb, T, lpos.as<ull>(), lpos.as<ull>() + nl);
    RG_LAUNCH(k_rg_linkfin, grid_for(nl, RG_BLOCK, 8192), T, lpos.as<ull>(), lpos.as<ull>() + nl, nl, (ull)npairs,
              (ull)ng);
  } else {
    links.reserve(RgLinks::bytes(0));
  }
  RgLinks T(links, nl);
  if (L) {
    // ---- d. dense per-label arrays: rows, max length (8 bytes), links out, links in (4 bytes)
    dense.reserve(24 * (size_t)L);
    ull *d_rows = dense.as<ull>(), *d_max = d_rows + L;
    uint32_t *d_out = reinterpret_cast<uint32_t*>(d_max + L), *d_in = d_out + L;
    PG_HIP(hipMemsetAsync(dense.p, 0, 24 * (size_t)L, c.stream));
    RG_LAUNCH(k_rg_accum, grid_rows, rows, n, rf.as<uint8_t>(), d_rows, d_max);
    if (nl) RG_LAUNCH(k_rg_degree, grid_for(nl, RG_BLOCK, 1024), T, nl, d_out, d_in);
    seen.reserve(L + 16);
    RG_LAUNCH(k_rg_seen, grid_for(L, RG_BLOCK, 8192), d_rows, L, seen.as<uint8_t>());
    nn = labels_seen(c, seen.as<uint8_t>(), L, labs);
    nodes.reserve(RgNodes::bytes(nn));
    RgNodes N(nodes, nn);
    PG_HIP(hipMemcpyAsync(N.label, labs.p, 8 * nn, hipMemcpyDeviceToDevice, c.stream));
    RG_LAUNCH(k_rg_gather, grid_for(nn, RG_BLOCK, 8192), N, nn, d_rows, d_max, d_out, d_in);
  } else {
    nodes.reserve(RgNodes::bytes(0));
  }
  // ---- e. the links text: the header, then one line per link
  const size_t hdr = sizeof(RG_LINKS_HEADER) - 1;
  const LinkLine line{T};
  const uint64_t body = text_measure(c, line, nl, toff);
  text.reserve(hdr + body + 16);
  PG_HIP(hipMemcpyAsync(text.p, RG_LINKS_HEADER, hdr, hipMemcpyHostToDevice, c.stream));
  text_write(c, line, nl, toff, text.as<char>() + hdr);
  c.sync();
  // ---- the new result replaces the previous one
  c.rg_nodes.swap(nodes);
  c.rg_links.swap(links);
  c.rg_paths.swap(paths);
  c.rg_steps.swap(steps);
  c.rg_text.swap(text);
  c.rg_nn = nn;
  c.rg_nl = nl;
  c.rg_np = np;
  c.rg_nu = nu;
  c.rg_total = hdr + body;
  c.rg_names = h_rows5 ? sc.names : c.n_records;
  c.rg_ready = true;
  if (n_nodes) *n_nodes = nn;
  if (n_links) *n_links = nl;
  if (n_paths) *n_paths = np;
  if (n_skipped) *n_skipped = sc.skipped;
}

void region_nodes(Ctx& c, int64_t* label, uint64_t* n_rows, uint64_t* max_len, uint32_t* n_out, uint32_t* n_in,
                  uint64_t cap) {
  need(c.rg_ready, "pg_region_nodes", NEED_GRAPH);
  const uint64_t nn = c.rg_nn;
  if (cap < nn) throw Error(-34, "pg_region_nodes: buffer too small");
  if (!nn) return;
  RgNodes N(c.rg_nodes, nn);
  get(c, label, N.label, 8 * nn);
  get(c, n_rows, N.rows, 8 * nn);
  get(c, max_len, N.maxlen, 8 * nn);
  get(c, n_out, N.nout, 4 * nn);
  get(c, n_in, N.nin, 4 * nn);
  c.sync();
}

void region_links(Ctx& c, int64_t* from, int64_t* to, uint64_t* count, uint32_t* n_genomes, uint64_t cap) {
  need(c.rg_ready, "pg_region_links", NEED_GRAPH);
  const uint64_t nl = c.rg_nl;
  if (cap < nl) throw Error(-34, "pg_region_links: buffer too small");
  if (!nl) return;
  RgLinks T(c.rg_links, nl);
  get(c, from, T.from, 8 * nl);
  get(c, to, T.to, 8 * nl);
  get(c, count, T.count, 8 * nl);
  get(c, n_genomes, T.ngen, 4 * nl);
  c.sync();
}

void region_paths(Ctx& c, int64_t* record, int64_t* strand, int64_t* lo, int64_t* hi, uint64_t* n_steps,
                  uint64_t cap) {
  need(c.rg_ready, "pg_region_paths", NEED_GRAPH);
  const uint64_t np = c.rg_np;
  if (cap < np) throw Error(-34, "pg_region_paths: buffer too small");
  if (!np) return;
  RgPaths P(c.rg_paths, np);
  get(c, record, P.rec, 8 * np);
  get(c, strand, P.strand, 8 * np);
  get(c, lo, P.lo, 8 * np);
  get(c, hi, P.hi, 8 * np);
  get(c, n_steps, P.steps, 8 * np);
  c.sync();
}

// the links text of the last region_graph: its size (out null, fd < 0), copied into out, or written to fd
uint64_t format_region_links(Ctx& c, char* out, uint64_t cap, int fd) {
  need(c.rg_ready, fd >= 0 ? "pg_region_links_format_fd" : "pg_region_links_format", NEED_GRAPH);
  return text_out(c, c.rg_text.p, c.rg_total, out, cap, fd, "pg_region_links_format", "pg_region_links_format_fd");
}

// the GFA text of the last region_graph with this call's record names (names[name_off[r] ..
// name_off[r+1]) is record r's): its size (out null, fd < 0), copied into out, or written to fd
// (seq: every S line carries its region's sequence, from the last region_seqs - pg_region_gfa_seq)
uint64_t format_region_gfa(Ctx& c, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                           uint64_t cap, int fd, bool seq) {
  const char* what = seq ? (fd >= 0 ? "pg_region_gfa_seq_fd" : "pg_region_gfa_seq")
                         : (fd >= 0 ? "pg_region_gfa_fd" : "pg_region_gfa");
  need(c.rg_ready, what, NEED_GRAPH);
  if (seq) region_seqs_match(c, what);
  const DevNames nm = names_upload(c, what, names, name_off, n_names, c.rg_names, "paths");
  const uint64_t nn = c.rg_nn, nl = c.rg_nl, nu = c.rg_nu, np = c.rg_np, items = nn + nl + nu;
  const size_t hdr = sizeof(RG_GFA_HEADER) - 1;
  DevBuf toff, text, sdst;
  const long long* step_label = c.rg_steps.as<long long>();
  GfaLine line{RgNodes(c.rg_nodes, nn), nn, RgLinks(c.rg_links, nl), nl, step_label,
               reinterpret_cast<const uint8_t*>(step_label + nu), RgPaths(c.rg_paths, np), np, nm.bytes, nm.off,
               seq ? region_seqs_len(c) : nullptr, nullptr};
  const uint64_t total = hdr + text_measure(c, line, items, toff);
  if (!text_wanted(total, out, cap, fd, what)) return total;
  text.reserve(total + 16);
  PG_HIP(hipMemcpyAsync(text.p, RG_GFA_HEADER, hdr, hipMemcpyHostToDevice, c.stream));
  if (seq) sdst.reserve(8 * (nn + 1));
  line.sdst = sdst.as<ull>();
  text_write(c, line, items, toff, text.as<char>() + hdr);
  if (seq) region_seqs_copy(c, sdst.as<ull>(), text.as<char>() + hdr);
  return text_out(c, text.p, total, out, cap, fd, what, what);
}

}  // namespace pg
