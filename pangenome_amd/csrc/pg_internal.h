// pg_internal.h — host-side context shared by the pangenome HIP translation
// units.  Not part of the public ABI (include/pangenome.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <functional>
#include <vector>

#include "pg_common.h"

namespace pg {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define PG_HIP(x)                                                                       \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess)                                                               \
      throw ::pg::Error(-5, std::string(#x) + ": " + hipGetErrorString(e_));            \
  } while (0)

// Device bytes held by every DevBuf of the process, their peak, and an
// optional cap (pg_tune PG_TUNE_DEVICE_CAP: tests of the memory budget of a
// path at a scaled-down size; 0 = none).
struct DevBytes {
  static std::atomic<uint64_t>& cur() { static std::atomic<uint64_t> v{0}; return v; }
  static std::atomic<uint64_t>& peak() { static std::atomic<uint64_t> v{0}; return v; }
  static std::atomic<uint64_t>& cap() { static std::atomic<uint64_t> v{0}; return v; }
  static void add(uint64_t b) {
    const uint64_t now = cur().fetch_add(b) + b;
    uint64_t pk = peak().load();
    while (now > pk && !peak().compare_exchange_weak(pk, now)) {}
  }
  // pg_tune PG_TUNE_POISON (debug): every new allocation is filled with this
  // byte (-1 = off), so a read of memory no kernel wrote shows up as a
  // different result instead of inheriting an earlier run's bytes
  static std::atomic<int>& poison() { static std::atomic<int> v{-1}; return v; }
};

// A growable device buffer (never shrinks; reused across calls so the steady
// state does no hipMalloc).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept { swap(o); }  // (a function may return the buffers it filled)
  ~DevBuf() { release(); }                // (function-local scratch buffers free themselves)
  void reserve(size_t bytes) {
    if (bytes <= cap) return;
    release();
    size_t nb = bytes + bytes / 8 + 256;
    const uint64_t lim = DevBytes::cap().load();
    if (lim && DevBytes::cur().load() + nb > lim)
      throw Error(-12, "device memory cap: " + std::to_string(DevBytes::cur().load() + nb) + " > " +
                           std::to_string(lim) + " bytes");
    const hipError_t e = hipMalloc(&p, nb);
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      throw Error(e == hipErrorOutOfMemory ? -12 : -5,
                  std::string("hipMalloc of ") + std::to_string(nb) + " bytes (" +
                      std::to_string(DevBytes::cur().load()) + " held by the library): " + hipGetErrorString(e));
    }
    cap = nb;
    DevBytes::add(nb);
    const int pv = DevBytes::poison().load();
    if (pv >= 0) {
      PG_HIP(hipMemset(p, pv, nb));
      PG_HIP(hipDeviceSynchronize());
    }
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
  void release() {
    if (p) {
      (void)hipFree(p);
      DevBytes::cur().fetch_sub(cap);
    }
    p = nullptr;
    cap = 0;
  }
};

// A growable pinned host buffer: device-to-host copies into it are plain DMA
// on the stream (a pageable destination costs a staged, synchronous copy).
struct PinBuf {
  void* p = nullptr;
  void* dp = nullptr;             // device view (coherent buffers written by kernels)
  size_t cap = 0;
  unsigned flags = hipHostMallocDefault;
  void reserve(size_t bytes) {
    if (bytes <= cap) return;
    if (p) PG_HIP(hipHostFree(p));
    p = dp = nullptr;
    size_t nb = bytes + bytes / 8 + 256;
    PG_HIP(hipHostMalloc(&p, nb, flags));
    if (flags & hipHostMallocMapped) PG_HIP(hipHostGetDevicePointer(&dp, p, 0));
    cap = nb;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Per-kernel timing on the context's stream (HIP events), so callers can
// price the dominant kernel against the HBM roofline.
// (off: no event is recorded and ms() is 0 - PG_TUNE_TIMERS 0, to price the
// timing events themselves)
struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  bool off = false;
  void init() {
    if (!a) { PG_HIP(hipEventCreate(&a)); PG_HIP(hipEventCreate(&b)); }
  }
  void start(hipStream_t s) { if (!off) PG_HIP(hipEventRecord(a, s)); }
  void stop(hipStream_t s) { if (!off) PG_HIP(hipEventRecord(b, s)); }
  double ms() {
    if (off) return 0.0;
    float t = 0;
    PG_HIP(hipEventSynchronize(b));
    PG_HIP(hipEventElapsedTime(&t, a, b));
    return (double)t;
  }
  void destroy() {
    if (a) { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
    a = b = nullptr;
  }
};

struct HostPool;                  // pg_stage.hip: the pinned staging ring's threads

struct Ctx {
  int device = 0;
  int k = 27;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // side stream: K3 work passes overlap the next coverage pass
  hipStream_t stream3 = nullptr;  // copy stream: chunked host uploads (pg_parse_host, pg_build_host)
  hipStream_t stream_hi = nullptr; // high priority: K1's header pass and record table beside the emission
  hipEvent_t ev[16] = {};         // ordering events between the two streams
  hipEvent_t ext_ev = nullptr;    // pg_stream_wait: the caller's stream's queued work, waited on by ours
  hipEvent_t rec_ev = nullptr;    // the record table's copy to the host (K1)
  hipEvent_t cev[16] = {};        // chunk-landed events of the copy stream
  int n_cu = 256;                 // compute units (persistent-kernel grids)
  int k3_chunks = 0;              // pg_tune: K3 chunks (0 = by tile count)
  int k3_wblk = 0;                // pg_tune: work blocks per CU, low 4 bits; last chunk's, high 4 bits (0 = 2)
  int k3_emit = 0;                // pg_tune: work pass (0 = two halves per segment, 1 = one)
  int k1_form = 0;                // pg_tune: K1 form bits (PG_TUNE_K1; default: the per-step span pass)
  int k3_tail = 0;                // pg_tune: last K3 chunk in 16ths of the others (0 = 10)
  int k3_head = 0;                // pg_tune: first K3 chunk in 16ths of the others (0 = 16)
  int k3_cover = 0;               // pg_tune: coverage pass (0 = packed form, 1 = LDS-staged members, 2 = quad form)
  int k3_anchors = 0;             // pg_tune: packed coverage pass anchors per tile and reference (0 = 4)
  int early_split = 1;            // pg_tune: pg_build_host splits each landed chunk's records (stage B under the upload)
  uint64_t h2d_chunk = 64ull << 20;   // pg_tune: bytes per H2D chunk of pg_parse_host
  uint64_t h2d_tail = 0;              // pg_tune: bytes of pg_build_host's last H2D chunk (0: uniform chunks)
  int host_threads = 0;           // pg_tune: memcpy threads of the staging ring (0 = by CPU affinity)
  uint64_t stage_piece = 32ull << 20;  // pg_tune: bytes per staging-ring slot (one DMA)
  uint64_t stage_slots = 4;       // pg_tune: staging-ring slots (2..8)
  int host_register = 1;          // pg_tune: register pageable chunks and DMA them (0: staging ring only)
  HostPool* pool = nullptr;       // staging ring threads (created on the first pageable upload)
  PinBuf stage_pin;               // staging ring slots
  int bb_shift = 0;               // pg_tune: table bits below the sized ones (tests of the overflow paths)
  uint64_t region_cap_force = 0;  // pg_tune: first stage A region size (tests of the re-run path)

  // ---- input FASTA (device-resident; either owned or borrowed)
  DevBuf fasta_own;
  const uint8_t* d_fasta = nullptr;
  uint64_t n_bytes = 0;

  // ---- parse products (K1)
  DevBuf span_sum, span_start;    // per 16 KiB wave span: function / inclusive prefix (K1)
  DevBuf n_sel;                   // device counters
  DevBuf rec_start, rec_len;      // int64 per record: compacted offset / length
  DevBuf rec_hdr, rec_ptr;        // int64 per record: header byte span packed, `ptr` emulation
  DevBuf rec_flag;                // uint8 per record: take part in the current pass
  DevBuf cls;                     // uint8 per base: class code (records concatenated); K1 writes only
                                  // the 16-base chunks with an exception or shared by two spans
  DevBuf p2;                      // uint32 per 16 bases: 2-bit codes (class & 3), the packed base stream
  DevBuf e16;                     // uint8 per 16 bases: nonzero if any is not ACGT
  bool cls_full = false;          // every chunk of `cls` written (ensure_cls)
  // ---- routed exchange (pg_route_*): the last build's stage A records held
  // in their regions for their owners instead of stages B/C
  bool route_req = false;         // the next build_dbg stops after stage A
  bool route_ready = false;       // stage A records held (route_reg: per region, clipped)
  uint64_t route_total = 0, route_maxreg = 0, route_maxbin = 0;
  unsigned route_sentinel = 0;
  std::vector<uint64_t> route_reg;
  DevBuf route_buf;               // region offsets and owner sums of pg_route_scatter
  PinBuf route_pin;
  uint64_t n_cls = 0;             // length of the compacted stream (bases before the first header too)
  DevBuf scratch;                 // rocPRIM temp storage
  DevBuf rec_pack;                // the scan total + int64 [5][rec_cap]: the record table for one copy
  uint64_t rec_cap = 0;           // record arrays sized for the last parse's record count
  PinBuf h_pin;                   // pinned staging for small device-to-host reads
  uint64_t n_lines = 0, n_records = 0, n_bases = 0, n_nl = 0;
  std::vector<int64_t> h_rec_start, h_rec_len, h_rec_hdr_start, h_rec_hdr_len, h_rec_ptr;
  bool parsed = false;

  // ---- dBG table (K3 stage C) and rdBG (fused K5)
  DevBuf table;                   // primary buckets (2 x 64-bit words each)
  DevBuf ovf;                     // overflow slots (16 B)
  TableView tv{};                 // hash (fixed by k) and current geometry (pg_common.h)
  int kb = 0, cbits = 0, hash_k = 0, bb = 0;   // key bits, coarse bin bits, k of tv's hash, bucket bits
  uint64_t cap = 0;               // primary buckets (power of two)
  uint64_t ovf_cap = 0;           // overflow slots (power of two)
  PinBuf h_out{nullptr, nullptr, 0, hipHostMallocMapped | hipHostMallocCoherent};   // k_gather_out's target
  std::vector<uint8_t> dev_flag;  // the record flags last uploaded to rec_flag (at dev_flag_p)
  const void* dev_flag_p = nullptr;
  bool t1_open = false;           // stage A queued, its side stream not yet joined (finish_build joins)
  DevBuf flags;                   // [0] sentinel seen, [1] stage A bits, [4] stage B/C bits
  uint64_t n_dbg = 0, n_rdbg = 0, n_canon = 0, sentinel = 0;
  bool built = false, reduced = false;
  int rc0 = 1;
  uint64_t windows_fw = 0, windows_total = 0;

  // ---- partitioned build (pg_dbg.hip)
  DevBuf recA_key, recA_mw, ctrA;     // stage A: records per (coarse bin, XCD) region and cursors
  uint64_t capA = 0;                  // records per stage A region
  DevBuf recS_key[2], recS_mw[2];     // stage B outputs (ping-pong)
  DevBuf ctrS;                        // stage B cursors, all levels
  DevBuf snapA;                       // pg_build_host's early split: stage A cursors already split
  double w_ratio = 0;                 // last host build: forward windows per input byte
  bool early_split_used = false;      // the last pg_build_host's stage C read the early split's partitions
  int bc_attempts = 0;                // stages B/C runs of the last build (1: no re-run)
  int split_passes = 0;               // stage B k_split passes of the last build (0: split under the upload)
  // the largest partition of each split level that a build had to re-run
  // for (at table bits lv_keep_bb): later builds' plans start from them
  std::vector<uint64_t> lv_keep;
  int lv_keep_bb = -1;
  // rdBG keys.  By default a build only counts the members and export_rdbg
  // sweeps the table; the eager form keeps each stage C block's member keys
  int rdbg_keys = 0;                  // pg_tune: 0 = count in the range pass, keys from the table on export; 1 = eager
  bool rseg_built = false;            // the last build was eager: rseg / rseg_cnt hold its keys
  DevBuf rseg;                        // (eager) rdBG keys: one segment of rseg_cap per stage C block
  DevBuf k5_ctr;                      // per stage C block: key / dBG / member counts
  uint64_t rseg_cap = 0, rseg_nseg = 0;
  std::vector<uint64_t> rseg_cnt;     // (eager) members per segment
  uint64_t n_records_a = 0;           // stage A records of the last build
  double u_ratio = 0, r_ratio = 0;    // last build: records per forward window, rdBG keys per record

  // ---- K3 tiles
  DevBuf tile_sched;              // per-stripe tile offsets + record order (k_tiles input)
  PinBuf tile_pin;
  uint64_t n_tiles = 0;
  int tile_k = 0;
  int k3_ref = -1;                // k_cover's dedup reference record (the lead), -1: none
  int k3_ref2 = -1;               // k_cover's second reference record, -1: none
  DevBuf part_cnt;                // multi-GPU partition: owner counts and cursors
  uint64_t part_counts[64] = {};  // counts of the last count pass
  uint64_t part_sums[64] = {};    // row_check sums of the last scatter's runs
  uint64_t merge_sum = 0, merge_rows = 0;   // the last merge: row_check sum / non-empty records it read
  uint64_t work_items = 0;        // the last build's work-pass items (segments the coverage pass left)
  uint64_t part_total = 0;
  int part_nparts = 0;
  uint64_t part_gen = ~0ull;      // build_gen of the table the counts are for
  uint64_t build_gen = 0;         // bumped by every table build / merge
  DevBuf k3_hint;                 // int32 [8 XCDs][2 references][R]: last drift k_cover found
  DevBuf tile_desc;               // tile descriptors (record start / length / index / stripe)
  DevBuf tile_geo;                // one GroupGeo per coverage group: the packed coverage pass's geometry (k_tiles)
  DevBuf k3_queue;                // segments left with work after the coverage pass, + counters
  std::vector<int64_t> tile_sig_len;   // record lengths / flags the tile list was built for
  std::vector<uint8_t> tile_sig_flag;

  // ---- walk passes (edges / labels)
  DevBuf tile_cnt, tile_off;      // per tile x strand counts / offsets
  DevBuf occ;                     // member / hit occurrences, walk ordered
  DevBuf edge_tab, pair_tab;      // edge table and (edge, walk) dedup set
  DevBuf edge_out;                // compacted edge slots
  DevBuf edge_exp;                // edges in first-occurrence order: [n][4] tuple, [n] count, [n] first walk
  uint64_t edge_cap = 0, pair_cap = 0, n_edges = 0;
  bool edges_ready = false;       // an edge pass has run (edge_exp / n_edges are its result)
  DevBuf lab_tab;                 // label table (hash of (key, value) -> label)
  uint64_t lab_cap = 0;
  DevBuf lab_list;                // the labels in order: [n] key, [n] value, [n] label
  uint64_t n_labels = 0;
  DevBuf rows_buf;                // rows of the last row pass: [n][5] int64
  uint64_t n_rows = 0;
  bool rows_ready = false;        // a row pass has run (rows_buf / n_rows are its result)
  // the `.xyz` line offsets of the last edge pass and their total, kept from pg_edges_format's size
  // call for its fill call (xyz_sized; walk_edges clears it); no other text touches them
  DevBuf xyz_off;
  uint64_t xyz_total = 0;
  bool xyz_sized = false;
  DevBuf text_buf;                // reusable storage of the `.xyz` and the rows text
  // ---- built-in clustering (pg_cluster.hip, pg_markov.hip): the `.mcl` text of the last pg_cluster_cc or
  // pg_cluster_markov
  DevBuf clu_text;
  uint64_t clu_total = 0, n_clusters = 0, n_clu_nodes = 0;
  bool clu_ready = false;
  // the last pg_cluster_markov's final matrix: uint32 [U] col_len, [U x select] rows, [U x select] vals
  // (released by the next clustering call), and the columns each size class ran, summed over the iterations
  DevBuf mk_mat;
  uint64_t mk_nodes = 0, mk_cols_wave = 0, mk_cols_mid = 0, mk_cols_block = 0;
  uint32_t mk_select = 0;
  bool mk_ready = false;
  // ---- frequency table (pg_freq.hip): the result of the last pg_freq
  DevBuf fr_tab;                  // [n] label, rows, plus, bases, min, max; [n][W] presence words; uint32 [n] genomes
  DevBuf fr_spec;                 // [2][G + 1]: labels / bases by number of genomes
  DevBuf fr_grp;                  // [5][G]: rows, bases, core, shell, unique per genome
  DevBuf fr_text;                 // the table's text
  uint64_t fr_n = 0, fr_total = 0;
  uint32_t fr_groups = 0, fr_words = 0;
  bool fr_ready = false;
  int freq_form = 0;              // pg_tune: accumulate pass (0 = aggregated in the wave, 1 = every lane its atomics)
  // ---- genome comparison (pg_compare.hip): the result of the last pg_freq_compare
  DevBuf cmp_shared;              // uint64 [G][G]: labels shared by every pair of genomes
  DevBuf cmp_curve;               // uint64 [2][P][G]: pan / core counts per order and number of genomes
  uint32_t cmp_groups = 0, cmp_orders = 0;
  bool cmp_ready = false;         // (a successful pg_freq clears it: the result described the old table)
  uint64_t cmp_chunk = 0;         // pg_tune: label-axis words per k_cmp_shared block (0 = by size)
  int cmp_form = 0;               // pg_tune: curves (0 = LDS counters up to CMP_LDS_GROUPS genomes, 1 = global atomics)
  // ---- genome tree (pg_tree.hip): the result of the last pg_tree_nj (no other pass reads or drops it)
  DevBuf nj_dist;                 // uint64 [n][n]: the distances the tree was built from
  std::vector<uint32_t> nj_join;  // [2][J]: left, right node of every join (the tables are a few bytes per leaf: host)
  std::vector<uint64_t> nj_len;   // [2][J]: their lengths, 16 fractional bits
  std::vector<uint32_t> nj_root;  // n_children, child [3]
  std::vector<uint64_t> nj_rlen;  // [3]
  uint32_t nj_n = 0;
  bool nj_ready = false;
  Timer t_nj;                     // the joins of the last pg_tree_nj
  double ms_nj = 0;
  uint64_t nj_cells = 0;          // the sum of m^2 over its joins
  int nj_blocks = 0;              // pg_tune: blocks of the arg-min pass (0 = by size)
  // ---- tree support (pg_boot.hip): the result of the last pg_tree_bootstrap (a successful pg_tree_nj drops it)
  std::vector<uint32_t> bt_support;  // [J]: the replicates whose tree has the rated tree's join t's split
  std::vector<uint32_t> bt_join;     // [2][R][J]: left, right node of every replicate's joins
  uint32_t bt_reps = 0, bt_form = 0, bt_batches = 0;   // (form: which NJ ran, 1 LDS, 2 global scratch, 3 per-join launches)
  bool bt_ready = false;
  Timer t_bt[3];                  // distances, joins, clades and matching of a batch
  double ms_bt[3] = {0, 0, 0};    // their sums over the batches of the last pg_tree_bootstrap
  uint64_t bt_cells = 0;          // R x the sum of m^2 over a tree's joins
  uint64_t bt_scratch = 0;        // pg_tune: device bytes of a batch of replicates (0 = default)
  int bt_form_tune = 0;           // pg_tune: 0 = by size, 1 = LDS where legal, 2 = global scratch, 3 = per-join launches
  // ---- k-mer colours (pg_colors.hip): the result of the last pg_kmer_colors, valid while kc_gen == build_gen
  // (no other pass reads or drops it)
  DevBuf kc_keys;                 // uint64 [n]: the table's plain keys, ascending
  DevBuf kc_bits;                 // uint64 [n][W]: the genomes of every key
  DevBuf kc_stat;                 // uint64 [G + 1] keys by number of genomes, then [2][G]: non-core keys, unique keys per genome
  uint64_t kc_n = 0, kc_gen = 0, kc_windows = 0, kc_missing = 0;
  uint32_t kc_groups = 0, kc_words = 0;
  bool kc_ready = false;
  DevBuf kc_shared, kc_curve;     // the last pg_kmer_compare: uint64 [G][G], [2][P][G] (a successful pg_kmer_colors drops it)
  uint32_t kc_cmp_orders = 0;
  bool kc_cmp_ready = false;
  Timer t_kc[4];                  // the index, the colouring pass, the tables after it, the comparison
  double ms_kc_index = 0, ms_kc_colour = 0, ms_kc_compare = 0;
  // ---- region graph (pg_region.hip): the result of the last pg_region_graph
  DevBuf rg_nodes;                // [n] label, rows, max length; uint32 [n] links out, links in
  DevBuf rg_links;                // [n] from, to, count; uint32 [n] genomes
  DevBuf rg_paths;                // [n] record, strand, lo, hi, steps, first step
  DevBuf rg_steps;                // the used rows in list order: [n] label; uint8 [n] first / last of its path
  DevBuf rg_text;                 // the links table's text
  uint64_t rg_nn = 0, rg_nl = 0, rg_np = 0, rg_nu = 0, rg_total = 0;
  uint64_t rg_names = 0;          // record names a GFA text needs
  bool rg_ready = false;
  // ---- region sequences (pg_regionseq.hip): the result of the last pg_region_seqs
  DevBuf rs_tab;                  // [n + 1] label, row, record, start, end, strand, len, gc, amb, offset, padded offset
  DevBuf rs_blob;                 // the sequences, every entry's start padded to 16 bytes
  uint64_t rs_n = 0, rs_bases = 0, rs_pad = 0;   // entries, letters, bytes of the padded blob
  uint64_t rs_names = 0;          // record names a FASTA text needs
  bool rs_ready = false;
  Timer t_rs;                     // the decoder kernel of the last pg_region_seqs (HIP events on `stream`)
  double ms_rs_decode = 0;
  uint64_t rs_chunks = 0;         // its 16-letter chunks
  // ---- variable sites (pg_sites.hip): the result of the last pg_region_sites
  DevBuf vs_sites;                // [n] from, to, first, count; uint32 [n] alleles, genomes
  DevBuf vs_alleles;              // [n] site, via, count, min, max; uint32 [n] genomes
  DevBuf vs_bits;                 // [alleles][W] presence words
  DevBuf vs_grp;                  // [3][G]: sites, alleles, private per genome
  DevBuf vs_text;                 // the alleles' text
  uint64_t vs_ns = 0, vs_na = 0, vs_total = 0;
  uint32_t vs_groups = 0, vs_words = 0;
  bool vs_ready = false;
  // ---- variable sites between anchors (pg_bubbles.hip): the result of the last pg_region_bubbles
  DevBuf bb_sites;                // [n] from, to, first, count; uint32 [n] alleles, genomes
  DevBuf bb_alleles;              // [n + 1] site, regions, first row, count, min, max, inner offset; uint32 [n] genomes
  DevBuf bb_bits;                 // [alleles][W] presence words
  DevBuf bb_inner;                // the alleles' inner paths one after another
  DevBuf bb_grp;                  // [3][G]: sites, alleles, private per genome
  DevBuf bb_anchors;              // [n] label; uint32 [n] genomes
  DevBuf bb_text;                 // the alleles' text
  uint64_t bb_ns = 0, bb_na = 0, bb_nin = 0, bb_nanc = 0, bb_total = 0;
  uint32_t bb_groups = 0, bb_words = 0;
  bool bb_ready = false;
  int bb_hash_bits = 0;           // pg_tune: low bits kept of the inner path's hash (0 = all of it)
  // ---- allele sequences and reference placement (pg_variants.hip): the result of the last pg_region_variants
  // (a successful pg_region_bubbles clears vr_ready: the texts read the bubbles tables)
  DevBuf vr_tab;                  // pg_seqdec.h's table: [na] the alleles, then [np] the placed sites' pad + REF
  DevBuf vr_blob;                 // their letters, every entry's start padded to 16 bytes
  DevBuf vr_place;                // [np] site, record, pos0, ref row, ref length; uint32 [np] ref allele
  uint64_t vr_na = 0, vr_np = 0, vr_unplaced = 0, vr_bases = 0;
  uint64_t vr_pad_al = 0, vr_pad = 0;   // bytes of the padded blob: the alleles' part, all of it
  bool vr_ready = false;
  Timer t_vr;                     // the decoder kernel of the last pg_region_variants
  double ms_vr_decode = 0;
  uint64_t vr_chunks = 0;         // its 16-letter chunks
  // ---- allele alignments (pg_align.hip): the result of the last pg_region_align (a successful
  // pg_region_variants or pg_region_bubbles clears al_ready: it describes their tables)
  DevBuf al_pairs;                // [n + 1] x 19 columns (AlPairs)
  DevBuf al_ops;                  // [n] len; uint8 [n] op
  DevBuf al_prims;                // [n + 1] pair, tpos, qpos, tlen, qlen; uint8 [n] type
  DevBuf al_lines;                // [n + 1] x 10 columns (AlLines); uint32 [n] genomes; uint8 [n] type
  DevBuf al_bits;                 // [lines][W] carrier words
  DevBuf al_memb;                 // the alleles that carry the lines, a line's one after another
  uint64_t al_np = 0, al_aligned = 0, al_nops = 0, al_nprims = 0, al_nl = 0, al_cells = 0;
  double ms_al_fill = 0;
  bool al_ready = false;
  Timer t_al;                     // the fill kernels of the last pg_region_align, batch by batch
  uint64_t al_cells_cap = 0;      // pg_tune: cells above which a pair is not aligned (0 = 2^24)
  uint64_t al_scratch = 0;        // pg_tune: bytes of direction bits per batch (0 = 256 MiB)
  int al_hash_bits = 0;           // pg_tune: low bits kept of a primitive's letters' hash (0 = all of it)
  int al_band = 0;                // pg_tune: 1 = pairs above the cells cap are aligned in a band
  uint64_t al_band_cap = 0;       // pg_tune: band cells above which a pair is given up (0 = 2^26)
  uint64_t al_band_t0 = 0;        // pg_tune: the band's first threshold (0 = 64)
  // the band form's part of the last pg_region_align (pg_region_align_band)
  uint64_t al_nover = 0, al_nbanded = 0, al_nattempts = 0, al_bandcells = 0;
  double ms_al_band = 0;

  // ---- npz persistence (pg_persist.hip)
  DevBuf preload;                 // staged PreEnt pairs, OR-merged by every build
  uint64_t n_preload = 0;
  std::vector<uint8_t> last_flag; // record flags / extra empties / strands of the last build
  int last_extra = 0;
  DevBuf dump_cnt;                // uint32 occurrence count per (entry, orientation) of the last build
  std::vector<PinBuf> dump_pin;   // pg_dbg_dump_fd: one pinned piece buffer per writer thread
  bool dump_ready = false;
  uint64_t dump_size = 0, dump_sentinel = 0;

  // timings of the last calls (ms, HIP events on `stream`)
  Timer t0, t1, t6;
  double ms_parse = 0, ms_clear = 0, ms_insert = 0, ms_short = 0, ms_scan = 0, ms_split = 0, ms_range = 0;
  double ms_total_build = 0;

  // Wait for the stream by polling it: the blocking wait's wake-up costs
  // ~20-30 us per host round trip on the build's critical path (two per
  // build).  After 50 ms of polling it blocks (long waits, and errors come
  // back through the blocking call).
  void sync() {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = hipStreamQuery(stream);
      if (e == hipSuccess) return;
      if (e != hipErrorNotReady) break;
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
    }
    PG_HIP(hipStreamSynchronize(stream));
  }
};

// pg_stage.hip
// One chunked upload of n host bytes to dst on c.stream3: chunk i's copy is
// marked by c.cev[i & 15] on stream3 once wait_queued(i) returns.  A
// pageable source goes through the pinned staging ring (a stager thread and
// its memcpy pool); a pinned one is DMA'd directly, up to 8 chunks ahead.
// The source is read until finish() (or the destructor) returns.
class Upload {
 public:
  Upload(Ctx& c, uint8_t* dst, const uint8_t* src, uint64_t n, uint64_t chunk);
  // chunk i = bytes [bounds[i], bounds[i+1]) (bounds[0] = 0, back() = n)
  Upload(Ctx& c, uint8_t* dst, const uint8_t* src, uint64_t n, std::vector<uint64_t> bounds);
  uint64_t off(uint64_t i) const { return bounds_[i]; }
  uint64_t len(uint64_t i) const { return bounds_[i + 1] - bounds_[i]; }
  ~Upload();
  Upload(const Upload&) = delete;
  Upload& operator=(const Upload&) = delete;
  uint64_t chunks() const { return nch_; }
  void wait_queued(uint64_t i);   // chunk i's copy is queued and c.cev[i & 15] recorded
  void consumed(uint64_t i);      // the caller has queued its wait on c.cev[i & 15]
  void finish();                  // every chunk queued; rethrows a stager error
  bool staged = false;            // through the pinned ring

 private:
  Ctx& c_;
  uint8_t* dst_;
  const uint8_t* src_;
  uint64_t nch_;
  std::vector<uint64_t> bounds_;
  HostPool* P_ = nullptr;
  uint64_t issued_ = 0;
  bool done_ = false;
};
void pool_destroy(Ctx& c);

// pg_parse.hip
// h_src: host bytes, uploaded in chunks pipelined with K1.  on_chunk (host
// input only): called after each chunk with the number of records complete
// so far (their lengths in c.h_rec_len, c.n_records = that count), and once
// at the end with all of them; it may enqueue work on c.stream.
void parse_fasta(Ctx& c, const uint8_t* h_src = nullptr, const std::function<void(uint64_t)>* on_chunk = nullptr);
// the class bytes of every chunk K1 left packed (e16 == 0), once per parse,
// on c.stream: for the passes that read `cls` directly (walks, checkpoints)
void ensure_cls(Ctx& c);
inline PackedCls packed_cls(Ctx& c) { return PackedCls{c.cls.as<uint8_t>(), c.p2.as<uint32_t>(), c.e16.as<uint8_t>()}; }
// pg_build_host: parse of host bytes with stage A of the build streamed under
// the upload (every record, no -n / checkpoint plan), then stages B and C
void build_host(Ctx& c, const uint8_t* h_src, uint64_t n, int rc0);
// pg_dbg.hip
void build_dbg(Ctx& c, const uint8_t* h_rec_flag, int extra_empty, int rc0);
void build_rdbg(Ctx& c);
uint64_t export_dbg(Ctx& c, uint64_t* h_keys, uint16_t* h_masks, uint64_t cap);
uint64_t export_rdbg(Ctx& c, uint64_t* h_keys, uint64_t cap);
uint64_t partition_dbg(Ctx& c, int nparts, void* d_out, uint64_t out_cap, uint64_t* h_counts);
void merge_dbg(Ctx& c, const void* d_pairs, uint64_t n, uint64_t cap_hint, int sentinel, int rot = -1);
void merge_dbg_segs(Ctx& c, const void* const* segs, const uint64_t* ns, int nseg, int sentinel, int rot);
// routed exchange: owners of the held stage A records (2^lg owners)
void route_counts(Ctx& c, int lg, uint64_t* counts);
void route_scatter(Ctx& c, int lg, void* d_out, uint64_t out_cap, uint64_t* sums);
void route_finish(Ctx& c);
void rows_checksum(Ctx& c, const void* d_rows, const uint64_t* off, uint64_t nseg, uint64_t* sums, bool row12 = false);
// pg_persist.hip
struct PreEnt {                   // one staged oakht slot: oriented key, 12-bit mask, count
  unsigned long long key;
  uint32_t mask, count;
};
void dbg_load(Ctx& c, const uint64_t* keys, const uint16_t* masks, const uint8_t* counts, uint64_t n);
uint64_t dbg_dump(Ctx& c, uint64_t& capacity, uint64_t* keys, uint16_t* values, uint8_t* counts);
uint64_t dbg_dump_fd(Ctx& c, uint64_t& capacity, int fd, const uint64_t* off, uint32_t* crc);
// n device bytes to descriptor fd at its position (pg_edges_format_fd, pg_rows_format_fd)
void text_to_fd(Ctx& c, const uint8_t* src, uint64_t n, int fd, const char* what);
uint64_t oakht_capacity(uint64_t size);
// pg_walk.hip
uint64_t walk_edges(Ctx& c, const uint8_t* h_rec_flag, int rc1);
void export_edges(Ctx& c, uint64_t* tuples, int64_t* counts, int64_t* first_walk, uint64_t cap);
void set_labels(Ctx& c, const int64_t* key, const int64_t* val, const int64_t* id, uint64_t n);
uint64_t walk_rows(Ctx& c, const uint8_t* h_rec_flag, int rc1);
void export_rows(Ctx& c, int64_t* rows5, uint64_t cap);
uint64_t format_edges(Ctx& c, char* out, uint64_t cap, int fd = -1);
uint64_t labels_from_edges(Ctx& c, const uint64_t* h_tuples, uint64_t n_edges, const int64_t* mk, const int64_t* mv,
                           const int64_t* mi, uint64_t n_mcl, int64_t next_id);
void export_labels(Ctx& c, int64_t* key, int64_t* val, int64_t* id, uint64_t cap);
// the label hash table of n (key, value, label) device entries (c.lab_tab), on c.stream
void lab_build(Ctx& c, const long long* d_key, const long long* d_val, const long long* d_id, uint64_t n);
uint64_t format_rows_text(Ctx& c, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                          uint64_t cap, int fd = -1);

// pg_cluster.hip
// Weight cut + connected components of the `.xyz` graph; h_tuples NULL: the
// last edge pass (c.edge_exp).  Replaces the label table; keeps the `.mcl`
// text on the device for format_clusters.
void cluster_cc(Ctx& c, const uint64_t* h_tuples, const int64_t* h_counts, uint64_t n_edges, int64_t min_weight);
uint64_t format_clusters(Ctx& c, char* out, uint64_t cap, int fd = -1);
// pg_markov.hip
// Markov clustering of the same graph (include/pangenome.h has the definition); the result takes cluster_cc's
// slot and the final matrix stays in c.mk_mat.  markov_drop releases that matrix.
void cluster_markov(Ctx& c, const uint64_t* h_tuples, const int64_t* h_counts, uint64_t n_edges, int64_t min_weight,
                    uint32_t inflation2, uint32_t select, uint32_t max_iter, uint32_t* n_iter, uint64_t* chaos);
void markov_matrix(Ctx& c, uint32_t* col_len, uint32_t* rows, uint32_t* vals);
void markov_drop(Ctx& c);
// The cluster curve: row i describes the components cluster_cc would form at min_weight = thr[i] (thr
// strictly ascending, nt <= SW_MAX_LEVELS, checked by the caller); nt == 0: the node count and the
// largest count alone.  Every output may be null.  Reads and replaces no result of the context.
#define SW_MAX_LEVELS 4096
void cluster_sweep(Ctx& c, const uint64_t* h_tuples, const int64_t* h_counts, uint64_t n_edges, const int64_t* thr,
                   uint64_t nt, uint64_t* n_nodes, int64_t* max_weight, uint64_t* edges, uint64_t* clusters,
                   uint64_t* largest, uint64_t* singletons);

// pg_freq.hip
// The frequency table of rows (h_rows5 NULL: the last row pass) grouped by
// rec_group; replaces the context's previous table only when it succeeds.
void freq(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
          uint32_t n_groups, uint64_t* n_labels, uint64_t* n_used, uint64_t* n_skipped);
void freq_export(Ctx& c, int64_t* label, uint32_t* n_genomes, uint64_t* n_rows, uint64_t* n_plus, uint64_t* total_bp,
                 uint64_t* min_len, uint64_t* max_len, uint64_t* bits, uint64_t cap);
void freq_spectrum(Ctx& c, uint64_t* labels_by_g, uint64_t* bp_by_g, uint64_t cap);
void freq_groups(Ctx& c, uint64_t* rows, uint64_t* bp_total, uint64_t* bp_core, uint64_t* bp_shell,
                 uint64_t* bp_unique, uint64_t cap);
uint64_t format_freq(Ctx& c, char* out, uint64_t cap, int fd = -1);

// pg_compare.hip
// Shared-label matrix and pan / core curves over presence bits [n][W] (h_bits
// NULL: the last freq's table on the device); replaces the context's previous
// comparison only when it succeeds.
void freq_compare(Ctx& c, const uint64_t* h_bits, uint64_t n_labels, uint32_t n_groups, const int32_t* orders,
                  uint32_t n_orders);
void freq_shared(Ctx& c, uint64_t* shared, uint64_t cap);
void freq_curve(Ctx& c, uint64_t* pan, uint64_t* core, uint64_t cap);

// the comparison of any device bit table bits [n][W] (pg_freq_compare's and pg_kmer_compare's work): the orders
// checked (-22 in `what`'s name), then shared [G][G] and curve [2][P][G] filled; nothing of the context is replaced
void compare_bits(Ctx& c, const char* what, const unsigned long long* d_bits, uint64_t n, uint32_t G,
                  const int32_t* orders, uint32_t P, DevBuf& shared, DevBuf& curve);
void compare_check(const char* what, uint64_t n, uint32_t G, const int32_t* orders, uint32_t P);

// pg_colors.hip
// The k-mer colours: which genomes hold every key of the dBG table (include/pangenome.h, "k-mer colours");
// replaces the context's previous colours only when it succeeds.
void kmer_colors(Ctx& c, const int32_t* rec_group, const uint8_t* rec_flags, uint64_t n_records, uint32_t n_groups,
                 int rc0, uint64_t* n_keys, uint64_t* n_windows, uint64_t* n_missing, uint64_t* n_uncoloured);
void kmer_colors_export(Ctx& c, uint64_t* keys, uint64_t* bits, uint64_t cap, uint64_t* n);
void kmer_colors_spectrum(Ctx& c, uint64_t* kmers_by_g, uint64_t* g_kmers, uint64_t* g_core, uint64_t* g_shell,
                          uint64_t* g_unique);
void kmer_compare(Ctx& c, const int32_t* orders, uint32_t n_orders);
void kmer_compare_export(Ctx& c, uint64_t* shared, uint64_t shared_cap, uint64_t* pan, uint64_t* core,
                         uint64_t curve_cap);
void kmer_colors_time(Ctx& c, double* ms_index, double* ms_colour, double* ms_compare, uint64_t* n_windows);
void kmer_colors_drop(Ctx& c);

// pg_tree.hip
// The neighbour-joining tree of a distance matrix (h_dist NULL: formed from the
// last freq_compare's shared matrix on the device); replaces the context's
// previous tree only when it succeeds.
void tree_nj(Ctx& c, const uint64_t* h_dist, uint32_t n, uint64_t* n_joins);
void tree_dist(Ctx& c, uint64_t* dist, uint64_t cap);
void tree_joins(Ctx& c, uint32_t* left, uint32_t* right, uint64_t* left_len, uint64_t* right_len, uint64_t cap);
void tree_root(Ctx& c, uint32_t* n_children, uint32_t* child, uint64_t* len);
void tree_time(Ctx& c, double* ms, uint64_t* cells);
void tree_bootstrap(Ctx& c, const uint64_t* h_bits, uint64_t n_labels, uint32_t n_groups, uint32_t n_reps, uint64_t seed,
                    uint64_t* rep_dist, uint64_t rep_dist_cap);
void tree_support(Ctx& c, uint32_t* support, uint64_t cap, uint32_t* n_reps);
void tree_bootstrap_joins(Ctx& c, uint32_t* left, uint32_t* right, uint64_t cap);
void tree_bootstrap_time(Ctx& c, double* ms_dist, double* ms_nj, double* ms_support, uint64_t* cells);
void tree_bootstrap_form(Ctx& c, uint32_t* form, uint32_t* n_batches);

// pg_region.hip: the front end the passes over the region rows share (pg_freq, pg_region_graph,
// pg_region_seqs; device side in pg_region.h)
// The arguments of a row pass checked (`what`, the pass's pg_ name, begins every message: -22) and its
// input on the device: the rows (h_rows5 NULL: the last row pass's, where they lie) and rec_group.
// records_match_always: n_records must be the context's record count even with host rows (pg_region_seqs,
// whose bases are the context's); otherwise only with the device rows, and host rows may come with
// any n_records that covers them (pg_freq, pg_region_graph).  The difference is kept as it was found.
struct RowInput {
  DevBuf up, grpmap;              // own the uploads
  const long long* rows;          // [n][5]
  const int* group;               // [n_records]
  uint64_t n;                     // rows
  unsigned grid_rows;             // blocks of a pass over the row tiles
};
RowInput row_input(Ctx& c, const char* what, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group,
                   uint64_t n_records, uint32_t n_groups, bool records_match_always);
// One pass over the rows (k_row_scan): L = 1 + the largest used label (0: none), the used and the skipped
// rows, names = 1 + the largest record of a used row.  rf (n + 1 bytes) non-null: the USED / HEAD flag byte
// of every row, rf[n] = 0.  rec_len non-null: -22 if a used row reaches outside its record (with or without
// rf).  -34 if L > 2^31.
struct RowScan {
  uint64_t L, used, skipped, names;
};
RowScan row_scan(Ctx& c, const char* what, const RowInput& in, uint8_t* rf, const long long* rec_len);
// the labels l < L with flag[l] set, ascending, into labs; returns their number
uint64_t labels_seen(Ctx& c, const uint8_t* flag, uint64_t L, DevBuf& labs);
// The end of a text call over `total` device bytes: their number alone (out null, fd < 0), or the text
// copied into out (cap: its room; -34 in `what`'s name if too small) or written to descriptor fd.
// text_wanted: the first two steps alone, for a text that is only made when it is wanted.
bool text_wanted(uint64_t total, const char* out, uint64_t cap, int fd, const char* what);
uint64_t text_out(Ctx& c, const void* d_text, uint64_t total, char* out, uint64_t cap, int fd, const char* what,
                  const char* what_fd);
// The record names of a text call checked (-22: fewer than the n_needed that `noun` need, offsets not
// ascending, NULL) and uploaded: off [n_names + 1], then the bytes.
struct DevNames {
  DevBuf buf;
  const long long* off;
  const char* bytes;
};
DevNames names_upload(Ctx& c, const char* what, const char* names, const int64_t* name_off, uint64_t n_names,
                      uint64_t n_needed, const char* noun);
// the result a call reads is there, or -22 "<what>: <hint>"
#define NEED_FREQ "no frequency table (call pg_freq first)"
#define NEED_COMPARE "no comparison (call pg_freq_compare first)"
#define NEED_GRAPH "no region graph (call pg_region_graph first)"
#define NEED_SEQS "no region sequences (call pg_region_seqs first)"
#define NEED_SITES "no variable sites (call pg_region_sites first)"
inline void need(bool ready, const char* what, const char* hint) {
  if (!ready) throw Error(-22, std::string(what) + ": " + hint);
}
// an optional column of a result to the host, on c.stream
inline void get(Ctx& c, void* dst, const void* src, size_t bytes) {
  if (dst && bytes) PG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c.stream));
}

// The region graph of rows (h_rows5 NULL: the last row pass) grouped by
// rec_group: nodes, links and paths; replaces the context's previous graph
// only when it succeeds.
void region_graph(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                  uint32_t n_groups, uint64_t* n_nodes, uint64_t* n_links, uint64_t* n_paths, uint64_t* n_skipped);
void region_nodes(Ctx& c, int64_t* label, uint64_t* n_rows, uint64_t* max_len, uint32_t* n_out, uint32_t* n_in,
                  uint64_t cap);
void region_links(Ctx& c, int64_t* from, int64_t* to, uint64_t* count, uint32_t* n_genomes, uint64_t cap);
void region_paths(Ctx& c, int64_t* record, int64_t* strand, int64_t* lo, int64_t* hi, uint64_t* n_steps,
                  uint64_t cap);
uint64_t format_region_links(Ctx& c, char* out, uint64_t cap, int fd = -1);
uint64_t format_region_gfa(Ctx& c, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                           uint64_t cap, int fd = -1, bool seq = false);

// pg_regionseq.hip
// One representative sequence per label of rows (h_rows5 NULL: the last row
// pass), decoded from the parse's packed class stream; replaces the context's
// previous sequences only when it succeeds.
void region_seqs(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                 uint32_t n_groups, uint64_t* n_regions, uint64_t* n_bases, uint64_t* n_skipped);
void region_seqs_table(Ctx& c, int64_t* label, int64_t* row, int64_t* record, int64_t* start, int64_t* end,
                       int64_t* strand, uint64_t* len, uint64_t* gc, uint64_t* amb, uint64_t* offset, uint64_t cap);
uint64_t region_seqs_bases(Ctx& c, uint8_t* out, uint64_t cap);
uint64_t format_region_fasta(Ctx& c, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                             uint64_t cap, int fd = -1);
// for format_region_gfa's S lines: -22 unless the sequences are those of the graph's nodes (same labels,
// len == max_len; checked on the device); the device column of their lengths; every sequence copied to
// d_dst + d_dst_off[entry] on c.stream
void region_seqs_match(Ctx& c, const char* what);
const unsigned long long* region_seqs_len(Ctx& c);
void region_seqs_copy(Ctx& c, const unsigned long long* d_dst_off, char* d_dst);

// pg_sites.hip
// The variable sites of rows (h_rows5 NULL: the last row pass) grouped by
// rec_group: the flank pairs (a, c) that two or more alleles join; replaces the
// context's previous sites only when it succeeds.
void region_sites(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                  uint32_t n_groups, uint64_t* n_sites, uint64_t* n_alleles, uint64_t* n_records_emitted,
                  uint64_t* n_skipped);
void region_sites_table(Ctx& c, int64_t* from, int64_t* to, uint32_t* n_alleles, uint64_t* first, uint64_t* count,
                        uint32_t* n_genomes, uint64_t cap);
void region_sites_alleles(Ctx& c, uint64_t* site, int64_t* via, uint64_t* count, uint32_t* n_genomes,
                          uint64_t* min_len, uint64_t* max_len, uint64_t* bits, uint64_t cap);
void region_sites_groups(Ctx& c, uint64_t* sites, uint64_t* alleles, uint64_t* private_, uint64_t cap);
uint64_t format_region_sites(Ctx& c, char* out, uint64_t cap, int fd = -1);

// pg_bubbles.hip
// The variable sites between anchor regions of rows (h_rows5 NULL: the last
// row pass) grouped by rec_group: the pairs of anchors - labels carried by
// min_genomes genomes or more - that two or more inner paths join; replaces
// the context's previous bubbles only when it succeeds.
#define NEED_BUBBLES "no bubbles (call pg_region_bubbles first)"
void region_bubbles(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                    uint32_t n_groups, uint32_t min_genomes, uint64_t* n_anchors, uint64_t* n_segments,
                    uint64_t* n_sites, uint64_t* n_alleles, uint64_t* n_skipped);
void region_bubbles_table(Ctx& c, int64_t* from, int64_t* to, uint32_t* n_alleles, uint64_t* first, uint64_t* count,
                          uint32_t* n_genomes, uint64_t cap);
void region_bubbles_alleles(Ctx& c, uint64_t* site, uint64_t* regions, uint64_t* first_row, uint64_t* count,
                            uint32_t* n_genomes, uint64_t* min_bp, uint64_t* max_bp, uint64_t* inner_off,
                            uint64_t* bits, uint64_t cap);
uint64_t region_bubbles_inner(Ctx& c, int64_t* inner, uint64_t cap);
void region_bubbles_groups(Ctx& c, uint64_t* sites, uint64_t* alleles, uint64_t* private_, uint64_t cap);
void region_bubbles_anchors(Ctx& c, int64_t* label, uint32_t* n_genomes, uint64_t cap);
uint64_t format_region_bubbles(Ctx& c, char* out, uint64_t cap, int fd = -1);

// pg_variants.hip
// The bases of every allele of the last region_bubbles and the sites placed on
// the walks of genome ref_group (UINT32_MAX: none); the rows must be the ones
// the bubbles were made of.  Replaces the context's previous variants only
// when it succeeds.
#define NEED_VARIANTS "no variants (call pg_region_variants first, after the last pg_region_bubbles)"
void region_variants(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                     uint32_t n_groups, uint32_t ref_group, uint64_t* n_alleles, uint64_t* n_bases, uint64_t* n_placed,
                     uint64_t* n_unplaced);
void region_variants_alleles(Ctx& c, int64_t* record, int64_t* lo, int64_t* hi, int64_t* strand, uint64_t* len,
                             uint64_t* gc, uint64_t* amb, uint64_t* offset, uint64_t cap);
uint64_t region_variants_bases(Ctx& c, uint8_t* out, uint64_t cap);
void region_variants_placed(Ctx& c, uint64_t* site, int64_t* record, int64_t* pos0, uint64_t* ref_row,
                            uint32_t* ref_allele, uint64_t* ref_len, uint64_t cap);
uint64_t format_region_alleles_fasta(Ctx& c, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                                     uint64_t cap, int fd = -1);
uint64_t format_region_vcf(Ctx& c, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                           uint64_t cap, int fd = -1);

// pg_align.hip
// Every allele of the last region_variants aligned against its site's
// reference (the placed site's REF, else allele 0): CIGARs, primitives and
// the merged lines of the placed sites.  Replaces the context's previous
// alignments only when it succeeds.
#define NEED_ALIGN "no alignments (call pg_region_align first, after the last pg_region_variants)"
void region_align(Ctx& c, uint64_t* n_pairs, uint64_t* n_aligned, uint64_t* n_ops, uint64_t* n_prims,
                  uint64_t* n_lines);
void region_align_pairs(Ctx& c, uint64_t* const cols[17], uint64_t cap);
void region_align_ops(Ctx& c, uint8_t* op, uint64_t* len, uint64_t cap);
void region_align_prims(Ctx& c, uint64_t* pair, uint8_t* type, uint64_t* tpos, uint64_t* qpos, uint64_t* tlen,
                        uint64_t* qlen, uint64_t cap);
void region_align_lines(Ctx& c, uint64_t* site, int64_t* pos, uint8_t* type, uint64_t* tpos, uint64_t* tlen,
                        uint64_t* qlen, uint64_t* first_prim, uint64_t* ac, uint32_t* n_genomes, uint64_t* bits,
                        uint64_t cap);
uint64_t format_region_align(Ctx& c, char* out, uint64_t cap, int fd = -1);
uint64_t format_region_primitives_vcf(Ctx& c, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                                      uint64_t cap, int fd = -1);

// helpers
inline uint64_t next_pow2(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}
inline int log2u(uint64_t p) {
  int b = 0;
  while ((1ull << b) < p) ++b;
  return b;
}

// Bits of a k-mer key: keys < 5^k <= 2^kb.
inline int key_bits(int k) {
  uint64_t maxkey = 1;
  for (int i = 0; i < k; ++i) maxkey *= 5;
  return std::max(1, log2u(maxkey));
}

// The hash of a table for k-mers of length k (a bijection of kb-bit keys,
// fixed by k: records carry h = perm(c) before the table is sized) and the
// reverse-complement constants; the bucket geometry comes from set_geometry.
inline TableView make_hash(int k, int& kb) {
  kb = key_bits(k);
  TableView t{};
  t.kmask = kb >= 64 ? ~0ull : ((1ull << kb) - 1ull);
  t.sh1 = std::max(1, kb / 2);
  t.sh2 = std::max(1, kb / 3);
  auto inv = [](uint64_t m) {                                 // inverse of odd m mod 2^64
    uint64_t x = m;
    for (int i = 0; i < 6; ++i) x *= 2 - m * x;
    return x;
  };
  t.m1 = (0x9E3779B97F4A7C15ull & t.kmask) | 1ull;
  t.m2 = (0xC2B2AE3D27D4EB4Full & t.kmask) | 1ull;
  t.m1i = inv(t.m1) & t.kmask;
  t.m2i = inv(t.m2) & t.kmask;
  rc_constants(k, t.rc_pad, t.rc_inv);
  return t;
}
// 2^bb buckets (kb - 38 <= bb <= kb: the quotient kb - bb plus the 26 mask
// bits fit one 64-bit word) and `ovf_slots` (a power of two) overflow slots.
inline void set_geometry(TableView& t, int kb, int bb, uint64_t ovf_slots) {
  t.bmask = (1ull << bb) - 1ull;
  t.qbits = (uint32_t)(kb - bb);
  t.omask = ovf_slots - 1;
}
inline unsigned grid_for(uint64_t n, unsigned block, unsigned cap = 65536u) {
  uint64_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

}  // namespace pg
