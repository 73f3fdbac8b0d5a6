// pg_freq.hip — the frequency table of the region rows (the reference README's
// purpose: "find the frequency across species"): per label the genomes it
// occurs in, its occurrences and its bases; the spectrum (labels and bases by
// number of genomes) and the core / shell / unique bases of every genome.
//
// Rows are (record, start, end, strand, label); rec_group maps a record to
// its genome (or -1).  A row is used iff label >= 0 and its record has a
// genome.  Tables are dense in the label (L = 1 + the largest used label).
//
// Steps, each its own launch on c.stream (no hand-shake inside a kernel):
//   a. k_row_scan   the largest used label, the used and the skipped rows
//                   (the front end of every row pass: pg_region.h, pg_region.hip)
//   b. k_fr_accum   one streaming pass over the rows into the dense per-label
//                   arrays with no-return 64-bit add / min / max / or atomics
//                   at agent scope
//   c. k_fr_dense   per label: seen flag and the popcount of its presence set
//   d. select + k_fr_gather   the labels seen, compacted into the table
//   e. k_fr_spectrum          labels and bases by number of genomes
//   f. k_fr_groups  a second pass over the rows: per genome rows / bases /
//                   core / unique bases; k_fr_shell the rest
//   g. FrLine through pg_text.h     the text, kept on the device
//
// Contention (b): at a low weight cut the rdBG is close to one component, so
// nearly every row carries one label and five atomics per row would all land
// on the same five words.  (A row ends where the label changes, so one label
// holds at most every other row of a record: a giant component between small
// ones gives rows A b A c A d ...)  Each wave therefore aggregates first: it
// takes the label of its first unserved lane, ballots the lanes that share it,
// reduces their values across those lanes, and one lane issues the atomics -
// five per wave and label instead of five per row.  Rows of one record are
// adjacent in print order, so the presence word is one OR per wave, label and
// genome.  Labels held by fewer than RG_AGG_MIN lanes of the wave are left to
// their lanes.  PG_TUNE_FREQ_FORM 1 keeps the plain form (every lane its own
// atomics) for comparison.
//
// Every sum is an integer and every atomic commutes: the result depends on
// the input alone, whatever the schedule.
#include <cstring>
#include <limits>

#include "pg_region.h"

namespace pg {

#define FR_LDS_GROUPS 1024u        // k_fr_groups: 4 counters per genome in LDS up to here (32 KiB)
#define FR_LDS_BINS 2048u          // k_fr_spectrum: 2 counters per bin in LDS up to here (32 KiB)

// ------------------------------------------------------------ b. accumulate
__global__ void k_fr_fill(ull* __restrict__ p, uint64_t n, ull v) {
  RG_LOOP(i, n) p[i] = v;
}

// a lane's own six atomics (the plain form, and the rows the aggregated form leaves to it)
__device__ __forceinline__ void fr_row_atomics(ull lab, ull len, bool plus, int g, uint32_t W, ull* d_rows,
                                               ull* d_plus, ull* d_bp, ull* d_min, ull* d_max, ull* d_bits) {
  RG_ADD(d_rows + lab, 1ull);
  if (plus) RG_ADD(d_plus + lab, 1ull);
  RG_ADD(d_bp + lab, len);
  RG_MIN(d_min + lab, len);
  RG_MAX(d_max + lab, len);
  RG_OR(d_bits + lab * W + ((uint32_t)g >> 6), 1ull << (g & 63));
}

// PLAIN: every lane issues its own atomics.  Otherwise the wave takes the
// label of its first unserved lane and ballots the lanes that share it
// (rg_by_label); a label held by RG_AGG_MIN lanes or more is reduced across
// them and one lane issues its atomics, a label held by fewer is left to its
// lanes, which issue theirs together once the wave has gone through its labels
// (one lane per atomic instruction costs more than it saves: a wave of 64
// labels would issue 384 instructions of one lane instead of 6 of 64).
template <bool PLAIN>
__global__ void __launch_bounds__(RG_BLOCK) k_fr_accum(const long long* __restrict__ rows, uint64_t n,
                                                       const int* __restrict__ rec_group, uint32_t W,
                                                       ull* d_rows, ull* d_plus, ull* d_bp, ull* d_min, ull* d_max,
                                                       ull* d_bits) {
  __shared__ long long lds[RG_TILE_WORDS(false)];
  const uint64_t ntiles = (n + RG_BLOCK - 1) / RG_BLOCK;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    RgRow r;
    const bool todo = rg_load_tile(rows, n, t, lds, r) && rs_used(r, rec_group);
    const int g = todo ? rec_group[r.rec] : -1;
    const ull lab = todo ? (ull)r.label : 0ull;
    const ull len = todo ? rg_len(r) : 0ull;
    const bool plus = todo && r.strand == 1;
    bool own = todo;                                       // this lane issues its own atomics
    if (!PLAIN) {
      // every lane of the wave runs the loop (its conditions are ballots) and calls the callback, so the
      // ballots and reductions inside the callback are whole-wave too
      const int lane = threadIdx.x & 63;
      own = rg_by_label(todo, lab, [&](ull lab0, bool mine, ull cnt, bool leader) {
        const ull mp = __ballot(mine && plus);
        const ull sum = rg_wave_sum(mine ? len : 0ull);
        const ull lo = rg_wave_min(mine ? len : ~0ull);
        const ull hi = rg_wave_max(mine ? len : 0ull);
        if (leader) {
          RG_ADD(d_rows + lab0, cnt);
          if (mp) RG_ADD(d_plus + lab0, (ull)__popcll(mp));
          RG_ADD(d_bp + lab0, sum);
          RG_MIN(d_min + lab0, lo);
          RG_MAX(d_max + lab0, hi);
        }
        // the presence set: one OR per genome among these lanes (rows of a record are adjacent)
        bool gtodo = mine;
        for (;;) {
          const ull gopen = __ballot(gtodo);
          if (!gopen) break;
          const int glead = __ffsll(gopen) - 1;
          const int g0 = __builtin_amdgcn_readlane(g, glead);
          if (lane == glead) RG_OR(d_bits + lab0 * W + ((uint32_t)g0 >> 6), 1ull << (g0 & 63));
          gtodo = gtodo && g != g0;
        }
      });
    }
    if (own) fr_row_atomics(lab, len, plus, g, W, d_rows, d_plus, d_bp, d_min, d_max, d_bits);
  }
}

// ------------------------------------------------------------ c, d. table
__global__ void k_fr_dense(const ull* __restrict__ d_rows, const ull* __restrict__ d_bits, uint64_t L, uint32_t W,
                           uint8_t* __restrict__ flag, uint32_t* __restrict__ ngen) {
  RG_LOOP(l, L) {
    uint32_t c = 0;
    for (uint32_t w = 0; w < W; ++w) c += __popcll(d_bits[l * W + w]);
    ngen[l] = c;
    flag[l] = d_rows[l] != 0;
  }
}
__global__ void k_fr_gather(const long long* __restrict__ labs, uint64_t nt, uint32_t W,
                            const ull* __restrict__ d_rows, const ull* __restrict__ d_plus,
                            const ull* __restrict__ d_bp, const ull* __restrict__ d_min,
                            const ull* __restrict__ d_max, const ull* __restrict__ d_bits,
                            const uint32_t* __restrict__ d_ngen, ull* __restrict__ t_rows, ull* __restrict__ t_plus,
                            ull* __restrict__ t_bp, ull* __restrict__ t_min, ull* __restrict__ t_max,
                            ull* __restrict__ t_bits, uint32_t* __restrict__ t_ngen) {
  RG_LOOP(i, nt) {
    const uint64_t l = (uint64_t)labs[i];
    t_rows[i] = d_rows[l];
    t_plus[i] = d_plus[l];
    t_bp[i] = d_bp[l];
    t_min[i] = d_min[l];
    t_max[i] = d_max[l];
    t_ngen[i] = d_ngen[l];
    for (uint32_t w = 0; w < W; ++w) t_bits[i * W + w] = d_bits[l * W + w];
  }
}

// ------------------------------------------------------------ e. spectrum
// spec[0..G] = labels by number of genomes, spec[G+1..2G+1] = their bases
template <bool LDS>
__global__ void __launch_bounds__(RG_BLOCK) k_fr_spectrum(const uint32_t* __restrict__ t_ngen,
                                                          const ull* __restrict__ t_bp, uint64_t nt, uint32_t G,
                                                          ull* __restrict__ spec) {
  __shared__ ull bins[LDS ? 2 * FR_LDS_BINS : 1];
  const uint32_t nb = G + 1;
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < 2 * nb; i += blockDim.x) bins[i] = 0;
    __syncthreads();
  }
  RG_LOOP(i, nt) {
    const uint32_t g = t_ngen[i];
    if (LDS) {
      atomicAdd(&bins[g], 1ull);
      atomicAdd(&bins[nb + g], t_bp[i]);
    } else {
      RG_ADD(spec + g, 1ull);
      RG_ADD(spec + nb + g, t_bp[i]);
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2 * nb; i += blockDim.x)
      if (bins[i]) RG_ADD(spec + i, bins[i]);
  }
}

// ------------------------------------------------------------ f. per genome
// grp: [5][G] = rows, bases, core, shell, unique (shell by k_fr_shell)
template <bool LDS>
__global__ void __launch_bounds__(RG_BLOCK) k_fr_groups(const long long* __restrict__ rows, uint64_t n,
                                                        const int* __restrict__ rec_group,
                                                        const uint32_t* __restrict__ d_ngen, uint32_t G,
                                                        ull* __restrict__ grp) {
  __shared__ long long lds[RG_TILE_WORDS(false)];
  __shared__ ull acc[LDS ? 4 * FR_LDS_GROUPS : 1];
  if (LDS)
    for (uint32_t i = threadIdx.x; i < 4 * G; i += blockDim.x) acc[i] = 0;   // (rg_load_tile's barrier orders this)
  const uint64_t ntiles = (n + RG_BLOCK - 1) / RG_BLOCK;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    RgRow r;
    if (!rg_load_tile(rows, n, t, lds, r) || !rs_used(r, rec_group)) continue;
    const int g = rec_group[r.rec];
    const ull len = rg_len(r);
    const uint32_t ng = d_ngen[r.label];
    const int cls = ng == G ? 2 : (ng == 1 ? 3 : -1);      // (one genome in all: everything is core)
    if (LDS) {
      atomicAdd(&acc[g], 1ull);
      atomicAdd(&acc[G + g], len);
      if (cls >= 0) atomicAdd(&acc[cls * G + g], len);
    } else {
      RG_ADD(grp + g, 1ull);
      RG_ADD(grp + G + g, len);
      if (cls >= 0) RG_ADD(grp + (uint64_t)(cls == 2 ? 2 : 4) * G + g, len);
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 4 * G; i += blockDim.x) {
      const uint32_t col = i / G, g = i - col * G;         // LDS columns: rows, bases, core, unique
      if (acc[i]) RG_ADD(grp + (uint64_t)(col == 3 ? 4 : col) * G + g, acc[i]);
    }
  }
}
__global__ void k_fr_shell(ull* __restrict__ grp, uint32_t G) {
  RG_LOOP(g, G) grp[3ull * G + g] = grp[1ull * G + g] - grp[2ull * G + g] - grp[4ull * G + g];
}

// ------------------------------------------------------------ g. text
#define FR_HEADER "#label\tgenomes\trows\tplus\tbp\tmin\tmax\n"
// the table's columns inside c.fr_tab (nt entries, W presence words each)
struct FrCols {
  long long* label;
  ull *rows, *plus, *bp, *mn, *mx, *bits;
  uint32_t* ngen;
  static size_t bytes(uint64_t nt, uint32_t W) { return 8 * (6 + (size_t)W) * nt + 4 * nt + 64; }
  FrCols(const DevBuf& b, uint64_t nt, uint32_t W) {
    label = b.as<long long>();
    rows = reinterpret_cast<ull*>(label + nt);
    plus = rows + nt;
    bp = plus + nt;
    mn = bp + nt;
    mx = mn + nt;
    bits = mx + nt;
    ngen = reinterpret_cast<uint32_t*>(bits + (size_t)W * nt);
  }
};

// <label> <genomes> <rows> <plus> <bp> <min> <max>, tab separated
struct FrLine {
  FrCols T;
  template <class S>
  __device__ __forceinline__ void operator()(S& s, uint64_t i) const {
    s.dec((ull)T.label[i]); s.ch('\t');
    s.dec(T.ngen[i]); s.ch('\t');
    s.dec(T.rows[i]); s.ch('\t');
    s.dec(T.plus[i]); s.ch('\t');
    s.dec(T.bp[i]); s.ch('\t');
    s.dec(T.mn[i]); s.ch('\t');
    s.dec(T.mx[i]); s.ch('\n');
  }
};

void freq(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
          uint32_t G, uint64_t* n_labels, uint64_t* n_used, uint64_t* n_skipped) {
  // ---- arguments: everything refused here leaves the previous result in place
  const RowInput in = row_input(c, "pg_freq", h_rows5, n_rows, rec_group, n_records, G, false);
  n_rows = in.n;
  const uint32_t W = (uint32_t)(((uint64_t)G + 63) / 64);
  const unsigned grid_rows = in.grid_rows;
  const long long* rows = in.rows;
  const int* d_group = in.group;

  // ---- a. the dense size, found before anything is allocated or replaced
  const RowScan sc = row_scan(c, "pg_freq", in, nullptr, nullptr);
  const uint64_t L = sc.L;

  // ---- b, c. dense per-label arrays: rows, plus, bases, min, max, [W] presence words
  DevBuf dense, dflag, dngen, labs, tab, spec, grp, toff, text;
  uint64_t nt = 0;
  spec.reserve(16 * ((size_t)G + 1));
  grp.reserve(40 * (size_t)G + 16);
  PG_HIP(hipMemsetAsync(spec.p, 0, 16 * ((size_t)G + 1), c.stream));
  PG_HIP(hipMemsetAsync(grp.p, 0, 40 * (size_t)G + 16, c.stream));
  if (L) {
    dense.reserve(8 * (5 + (size_t)W) * L);
    ull* d_rows = dense.as<ull>();
    ull *d_plus = d_rows + L, *d_bp = d_plus + L, *d_min = d_bp + L, *d_max = d_min + L, *d_bits = d_max + L;
    PG_HIP(hipMemsetAsync(dense.p, 0, 8 * (5 + (size_t)W) * L, c.stream));
    RG_LAUNCH(k_fr_fill, grid_for(L, RG_BLOCK, 8192), d_min, L, ~0ull);
    if (c.freq_form == 1)
      RG_LAUNCH(k_fr_accum<true>, grid_rows, rows, n_rows, d_group, W, d_rows, d_plus, d_bp, d_min, d_max, d_bits);
    else
      RG_LAUNCH(k_fr_accum<false>, grid_rows, rows, n_rows, d_group, W, d_rows, d_plus, d_bp, d_min, d_max, d_bits);
    dflag.reserve(L + 16);
    dngen.reserve(4 * L + 16);
    RG_LAUNCH(k_fr_dense, grid_for(L, RG_BLOCK, 8192), d_rows, d_bits, L, W, dflag.as<uint8_t>(), dngen.as<uint32_t>());
    // ---- d. the labels seen, ascending
    nt = labels_seen(c, dflag.as<uint8_t>(), L, labs);
    tab.reserve(FrCols::bytes(nt, W));
    FrCols T(tab, nt, W);
    PG_HIP(hipMemcpyAsync(T.label, labs.p, 8 * nt, hipMemcpyDeviceToDevice, c.stream));
    RG_LAUNCH(k_fr_gather, grid_for(nt, RG_BLOCK, 8192), T.label, nt, W, d_rows, d_plus, d_bp, d_min, d_max, d_bits,
              dngen.as<uint32_t>(), T.rows, T.plus, T.bp, T.mn, T.mx, T.bits, T.ngen);
    // ---- e. spectrum
    if ((uint64_t)G + 1 <= FR_LDS_BINS)
      RG_LAUNCH(k_fr_spectrum<true>, grid_for(nt, RG_BLOCK, 1024), T.ngen, T.bp, nt, G, spec.as<ull>());
    else
      RG_LAUNCH(k_fr_spectrum<false>, grid_for(nt, RG_BLOCK, 8192), T.ngen, T.bp, nt, G, spec.as<ull>());
    // ---- f. per genome
    if (G <= FR_LDS_GROUPS)
      RG_LAUNCH(k_fr_groups<true>, std::min(grid_rows, 2u * (unsigned)std::max(1, c.n_cu)), rows, n_rows, d_group,
                dngen.as<uint32_t>(), G, grp.as<ull>());
    else
      RG_LAUNCH(k_fr_groups<false>, grid_rows, rows, n_rows, d_group, dngen.as<uint32_t>(), G, grp.as<ull>());
    RG_LAUNCH(k_fr_shell, grid_for(G, RG_BLOCK, 8192), grp.as<ull>(), G);
  } else {
    tab.reserve(FrCols::bytes(0, W));
  }
  // ---- g. text: the header, then one line per entry
  const size_t hdr = sizeof(FR_HEADER) - 1;
  const FrLine line{FrCols(tab, nt, W)};
  const uint64_t body = text_measure(c, line, nt, toff);
  text.reserve(hdr + body + 16);
  PG_HIP(hipMemcpyAsync(text.p, FR_HEADER, hdr, hipMemcpyHostToDevice, c.stream));
  text_write(c, line, nt, toff, text.as<char>() + hdr);
  c.sync();
  // ---- the new result replaces the previous one
  c.fr_tab.swap(tab);
  c.fr_spec.swap(spec);
  c.fr_grp.swap(grp);
  c.fr_text.swap(text);
  c.fr_n = nt;
  c.fr_groups = G;
  c.fr_words = W;
  c.fr_total = hdr + body;
  c.fr_ready = true;
  c.cmp_ready = false;                                     // (a comparison described the old table)
  if (n_labels) *n_labels = nt;
  if (n_used) *n_used = sc.used;
  if (n_skipped) *n_skipped = sc.skipped;
}

void freq_export(Ctx& c, int64_t* label, uint32_t* n_genomes, uint64_t* n_rows, uint64_t* n_plus, uint64_t* total_bp,
                 uint64_t* min_len, uint64_t* max_len, uint64_t* bits, uint64_t cap) {
  need(c.fr_ready, "pg_freq_export", NEED_FREQ);
  const uint64_t nt = c.fr_n;
  if (cap < nt) throw Error(-34, "pg_freq_export: buffer too small");
  if (!nt) return;
  FrCols T(c.fr_tab, nt, c.fr_words);
  get(c, label, T.label, 8 * nt);
  get(c, n_genomes, T.ngen, 4 * nt);
  get(c, n_rows, T.rows, 8 * nt);
  get(c, n_plus, T.plus, 8 * nt);
  get(c, total_bp, T.bp, 8 * nt);
  get(c, min_len, T.mn, 8 * nt);
  get(c, max_len, T.mx, 8 * nt);
  get(c, bits, T.bits, 8 * (size_t)c.fr_words * nt);
  c.sync();
}

void freq_spectrum(Ctx& c, uint64_t* labels_by_g, uint64_t* bp_by_g, uint64_t cap) {
  need(c.fr_ready, "pg_freq_spectrum", NEED_FREQ);
  const uint64_t nb = (uint64_t)c.fr_groups + 1;
  if (cap < nb) throw Error(-34, "pg_freq_spectrum: buffer too small");
  if (labels_by_g) PG_HIP(hipMemcpyAsync(labels_by_g, c.fr_spec.p, 8 * nb, hipMemcpyDeviceToHost, c.stream));
  if (bp_by_g) PG_HIP(hipMemcpyAsync(bp_by_g, c.fr_spec.as<ull>() + nb, 8 * nb, hipMemcpyDeviceToHost, c.stream));
  c.sync();
}

void freq_groups(Ctx& c, uint64_t* rows, uint64_t* bp_total, uint64_t* bp_core, uint64_t* bp_shell,
                 uint64_t* bp_unique, uint64_t cap) {
  need(c.fr_ready, "pg_freq_groups", NEED_FREQ);
  const uint64_t G = c.fr_groups;
  if (cap < G) throw Error(-34, "pg_freq_groups: buffer too small");
  if (!G) return;
  uint64_t* dst[5] = {rows, bp_total, bp_core, bp_shell, bp_unique};
  for (int i = 0; i < 5; ++i)
    if (dst[i]) PG_HIP(hipMemcpyAsync(dst[i], c.fr_grp.as<ull>() + i * G, 8 * G, hipMemcpyDeviceToHost, c.stream));
  c.sync();
}

// the text of the last freq: its size (out null, fd < 0), copied into out, or written to descriptor fd
uint64_t format_freq(Ctx& c, char* out, uint64_t cap, int fd) {
  need(c.fr_ready, fd >= 0 ? "pg_freq_format_fd" : "pg_freq_format", NEED_FREQ);
  return text_out(c, c.fr_text.p, c.fr_total, out, cap, fd, "pg_freq_format", "pg_freq_format_fd");
}

}  // namespace pg
