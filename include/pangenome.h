/*
 * pangenome.h — C ABI of libpangenome_hip.so, the MI355X (gfx950) build of
 * Rinoahu/pangenome's k-mer -> dBG -> rdBG -> region-table hot path.
 *
 * The reference (kmer_numba.py) has no FFI: its seams are Python functions.
 * Each entry point below replaces one of them; the Python host
 * (pangenome_amd/kmer.py) binds this header through ctypes and keeps the
 * reference's CLI, file contracts and printing.  INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every int-returning call returns PG_OK (0) or a negative error code and
 *     records a message for pg_last_error() (thread-local); no exception or
 *     abort crosses the ABI;
 *   - calls are synchronous: results are on the host (or in the caller's
 *     device buffer) when they return;
 *   - a pg_ctx owns all device working memory (one HIP stream on one device);
 *     it is not re-entrant — use one per thread / per GPU;
 *   - host arrays are caller-owned; `*_cap` arguments give their capacity in
 *     elements and the call fails with PG_ERANGE if it is too small (query
 *     sizes first with a NULL pointer where documented).
 */
#ifndef PANGENOME_H
#define PANGENOME_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_OK 0
#define PG_EINVAL (-22)
#define PG_ENOMEM (-12)
#define PG_ERANGE (-34)
#define PG_EDEVICE (-5)

typedef struct pg_ctx pg_ctx;

/* What one build did, for throughput and roofline accounting.  Kernel times
 * are HIP-event durations on the context's stream. */
typedef struct pg_stats {
  uint64_t n_bytes;        /* FASTA bytes parsed                                  */
  uint64_t n_records;      /* records (header lines)                              */
  uint64_t n_bases;        /* sequence bases over all records (forward strand)     */
  uint64_t n_windows;      /* k-mer windows inserted (both strands when rc)        */
  uint64_t n_dbg;          /* dBG keys (reference's non-canonical count)           */
  uint64_t n_rdbg;         /* rdBG keys                                            */
  uint64_t n_slots;        /* occupied canonical slots                             */
  uint64_t table_capacity; /* slots in the device hash table                       */
  double ms_parse;         /* K1 wall (host-timed, includes its small D2H syncs)  */
  double ms_clear;         /* (0: the table is written whole, never cleared)      */
  double ms_insert;        /* K3 stage A: coverage + work passes (record emission)*/
  double ms_scan;          /* K3 stages B + C: partition merge with the fused K5  */
  uint64_t sentinel;       /* 1 if the n<k key (2^64-1) is in the dBG              */
  uint64_t n_records_a;    /* K3 stage A records (windows the coverage pass kept)  */
  double ms_split;         /* K3 stage B: k_split pass(es)                         */
  double ms_range;         /* K3 stage C: k_build_range (table + fused K5)         */
  uint64_t build_flags;    /* bit 0: the last pg_build_host split its records into
                              the table's partitions chunk by chunk under the upload
                              (PG_TUNE_EARLY_SPLIT) and stage C read them; bits
                              8..15: stages B/C re-runs of the last build (a plan
                              or a capacity that did not hold); bits 16..23: the
                              k_split passes of stage B (0 when split under the
                              upload)                                             */
  uint64_t n_work_items;   /* K3 stage A work-pass items: 16-window segments the
                              coverage pass left, 64 class bytes read each        */
} pg_stats;

/* Context on HIP device `device` for k-mer length k (clamped to [1, 27] as
 * seq2rdbg does, kmer_numba.py:1236). */
int pg_create(pg_ctx** out, int device, int k);
void pg_destroy(pg_ctx* ctx);
const char* pg_last_error(void);
int pg_get_k(const pg_ctx* ctx);
/* Order this context after a caller's stream: every stream of the context
 * waits (on the device, hipStreamWaitEvent; the host does not block) for
 * the work queued on `stream` (a hipStream_t; NULL = the null stream) when
 * the call is made.  For callers whose allocator hands out memory that
 * work still queued on their stream may touch (a torch caching-allocator
 * block freed behind a queued copy or collective) before they pass it to
 * an entry point that writes or reads it.  Every entry point returns with
 * its own device work complete, so the other direction needs nothing. */
int pg_stream_wait(pg_ctx* ctx, void* stream);

/* ---- input: the mmapped FASTA the reference reads with seq2bytes
 *      (kmer_numba.py:117-119).  Host bytes are copied to HBM; device bytes
 *      (16-byte aligned) are used in place and must outlive the parse. */
int pg_set_fasta(pg_ctx* ctx, const uint8_t* host_bytes, uint64_t nbytes);
int pg_set_fasta_device(pg_ctx* ctx, const uint8_t* device_bytes, uint64_t nbytes);

/* K1: readline_jit_ + seqio_jit_ (kmer_numba.py:122-172) on the device. */
int pg_parse(pg_ctx* ctx, uint64_t* n_records, uint64_t* n_bases);
/* pg_set_fasta + pg_parse for host bytes in one call (seq2bytes + seqio_jit_,
 * :117-172): the copy to HBM goes in chunks (PG_TUNE_H2D_CHUNK, 64 MiB) on a
 * side stream and K1 runs on each chunk once it has landed, so the parse of
 * all but the last chunk hides under the PCIe transfer.  Pinned host memory
 * is DMA'd directly; pageable memory (the np.memmap the reference reads) is
 * copied by a few host threads into a ring of pinned slots that the DMA
 * drains (PG_TUNE_HOST_THREADS).  The bytes are read until the call returns. */
int pg_parse_host(pg_ctx* ctx, const uint8_t* host_bytes, uint64_t nbytes, uint64_t* n_records,
                  uint64_t* n_bases);
/* pg_parse_host + pg_build of every record (seq2rdbg + dbg2rdbg,
 * kmer_numba.py:1234-1321, for an input no -n limit or 2^33-base checkpoint
 * touches) with the build's first stage streamed under the upload: the
 * records a chunk completes go through the coverage / emission pass while
 * the next chunk is copied.  Results equal pg_parse + pg_build(NULL, 0, rc0);
 * the record table is available afterwards (pg_records). */
int pg_build_host(pg_ctx* ctx, const uint8_t* host_bytes, uint64_t nbytes, int rc0, uint64_t* n_rdbg,
                  pg_stats* stats);
/* pg_set_fasta_device + pg_parse + pg_build(NULL, 0, rc0) in one call, for a
 * FASTA already in HBM (seq2rdbg + dbg2rdbg, kmer_numba.py:1234-1321, no -n
 * limit or checkpoint): the host step between the parse and the build runs
 * in C++ with no return to the caller.  The bytes must outlive the call;
 * the record table is available afterwards (pg_records). */
int pg_build_device(pg_ctx* ctx, const uint8_t* device_bytes, uint64_t nbytes, int rc0, uint64_t* n_rdbg,
                    pg_stats* stats);
/* Per-record table (arrays of n_records): compacted sequence length, header
 * byte span (qid = bytes[hdr_start : hdr_start+hdr_len], '>' included,
 * :160) and seqio's resume pointer (:153). Any pointer may be NULL. */
int pg_records(const pg_ctx* ctx, int64_t* seq_len, int64_t* hdr_start, int64_t* hdr_len, int64_t* ptr);

/* K3: seq2rdbg's dBG pass (kmer_numba.py:1234-1268 -> seq2dbg_jit_ :1202-1230
 * -> build_dbg :1052-1090 -> add_kmer :1036-1047).  rec_flags (NULL = all)
 * holds one byte per record: bit0 = record is part of the pass (the host
 * applies -n and the checkpoint/resume rules); extra_empty = number of extra
 * empty records the reference's resume yields (each adds the n<k sentinel).
 * rc0 != 0 inserts the reverse strand too (-c bit 1, :2110). */
int pg_build_dbg(pg_ctx* ctx, const uint8_t* rec_flags, int extra_empty, int rc0, pg_stats* stats);

/* K5: dbg2rdbg (kmer_numba.py:1313-1321 -> build_rdbg_jit_ :1292-1309).
 * The degree scan runs inside pg_build_dbg (every key's masks are final when
 * its table partition is merged; the rdBG members are counted there), so
 * this only reports it. */
int pg_build_rdbg(pg_ctx* ctx, uint64_t* n_rdbg, pg_stats* stats);

/* seq2rdbg then dbg2rdbg (kmer_numba.py:1234-1268, :1313-1321) in one call:
 * pg_build_dbg + pg_build_rdbg. */
int pg_build(pg_ctx* ctx, const uint8_t* rec_flags, int extra_empty, int rc0, uint64_t* n_rdbg, pg_stats* stats);

/* dump()'s keys/values (kmer_numba.py:243-261) of the dBG, sorted by key
 * (on the device).  keys == NULL: only *n is set. */
int pg_dbg_export(pg_ctx* ctx, uint64_t* keys, uint16_t* masks, uint64_t cap, uint64_t* n);
/* rdBG keys, sorted. keys == NULL: only *n is set (the build's count: no
 * device work).  With keys, the call reads the whole table once (16 bytes per
 * bucket plus the overflow slots: 0.5 GB for a 2^25-bucket table, whatever the
 * number of keys), sorts the member keys on the device and copies them back;
 * it fails with PG_EDEVICE if the table does not hold exactly the members
 * the build counted.  After a build in the eager form (PG_TUNE_RDBG_KEYS 1)
 * it gathers the keys that build wrote instead of reading the table. */
int pg_rdbg_export(pg_ctx* ctx, uint64_t* keys, uint64_t cap, uint64_t* n);

/* ---- npz persistence: dump() / load_on_disk() (kmer_numba.py:243-335).
 * pg_dbg_dump writes the last build's dBG as an oakht slot layout that
 * load_on_disk (:289-335) and oakht.pointer (:521-538) accept: FNV-1a over the
 * key's low 4 bytes mod a prime capacity, probes j, j, j+1, j+4, j+9, ...;
 * keys[capacity] uint64, values[capacity] uint16 (12-bit mask), counts
 * [capacity] uint8 = occurrences of the oriented key, saturating at 255
 * (__setitem__ :556; counted by an extra window pass over the build).
 * *capacity == 0 picks the reference's growth chain (find_prime(2^20), then
 * find_prime(cap * 1.62) while size > 0.75 * cap, :423-474).  keys == NULL
 * only sets *capacity and *size (call again with arrays of *capacity). */
int pg_dbg_dump(pg_ctx* ctx, uint64_t* capacity, uint64_t* keys, uint16_t* values, uint8_t* counts, uint64_t* size);
/* pg_dbg_dump straight into an open file (dump() :243-261 without a host
 * copy of the slot arrays): the keys / values / counts arrays (8, 2 and 1 B
 * per slot) are written at file offsets offsets[0..2] of descriptor fd
 * (pwrite, in 16 MiB pieces streamed from the device through pinned buffers
 * by up to 16 host threads) and crcs[0..2] receive each array's CRC-32.  The
 * .npy headers and the zip framing around them are the caller's
 * (host.write_db_npz).  fd < 0 only sets *capacity and *size. */
int pg_dbg_dump_fd(pg_ctx* ctx, uint64_t* capacity, int fd, const uint64_t* offsets, uint32_t* crcs,
                   uint64_t* size);
/* Stage (oriented key, 12-bit mask, count) pairs — the counts > 0 slots of a
 * loaded npz — to be OR-merged into every following pg_build_dbg (-d: a dBG
 * with no records inserted; -D: rdBG keys with mask 0, members by the rdBG
 * rule; -r: a checkpoint the build resumes onto).  Key 2^64-1 is the n<k
 * sentinel.  counts may be NULL (1 each); n == 0 clears the stage. */
int pg_dbg_load(pg_ctx* ctx, const uint64_t* keys, const uint16_t* masks, const uint8_t* counts, uint64_t n);
/* The reference's final oakht capacity for `size` keys (host only). */
uint64_t pg_oakht_capacity(uint64_t size);

/* ---- multi-GPU exchange (one process per GPU; the caller moves the bytes
 *      with RCCL).  Replaces nothing in the reference, which is single-core.
 *      Device pointers the caller passes (d_out, d_records, d_rows) must be
 *      ready when the call is made: the library's streams do not wait on the
 *      caller's (synchronise the caller's streams first). */
/* Owner-partition this rank's local dBG into `nparts` contiguous runs of
 * 16-byte records (d_out device buffer, capacity out_cap records).
 * counts[nparts] receives run lengths; d_out == NULL only counts. */
int pg_dbg_partition(pg_ctx* ctx, int nparts, void* d_out, uint64_t out_cap, uint64_t* counts);
/* Integrity sums of the last pg_dbg_partition scatter: sums[i] = the sum
 * mod 2^64 of a 64-bit hash of each 16-byte record of run i (the hash is
 * row_check in pangenome_amd/csrc/pg_common.h; order-free, so the
 * receiver's pg_rows_checksum of the same records must equal it). */
int pg_dbg_partition_sums(pg_ctx* ctx, int nparts, uint64_t* sums);
/* The same sums over nseg segments of 16-byte records at device address
 * d_rows: segment s = records [seg_off[s], seg_off[s+1]). */
int pg_rows_checksum(pg_ctx* ctx, const void* d_rows, const uint64_t* seg_off, uint64_t nseg, uint64_t* sums);
/* OR-merge received 16-byte records (device pointer) into a fresh owner
 * table (the rdBG of the owner's keys is built with it); sentinel != 0 adds
 * the n<k key.  capacity_hint is ignored (the table is sized exactly). */
int pg_dbg_merge(pg_ctx* ctx, const void* d_records, uint64_t n, uint64_t capacity_hint, int sentinel);
/* What the last pg_dbg_merge read: non-empty records and the sum of their
 * hashes (pg_dbg_partition_sums' hash over all n records). */
int pg_dbg_merge_check(const pg_ctx* ctx, uint64_t* rows, uint64_t* sum);
/* Routed exchange: the owners build once.  Instead of a local dBG that is
 * partitioned and merged again, a rank's stage A records (h = the table
 * hash of the canonical key, the 26-bit mask word) go to their owners, and
 * only the owners run stages B and C.  The owner of a record is the top
 * log2(nparts) bits of h (nparts a power of two, at most 64 and at most one
 * owner per coarse bin of k's keys: 8 at k = 1, 32 at k = 2; every routed
 * call refuses more with PG_EINVAL before anything runs), so a rank's
 * records for one owner are whole stage A regions.
 * pg_route_stage_a: after pg_parse / pg_set_fasta(_device) + pg_parse, stage
 * A of the build pg_build_dbg would run (same arguments), held for routing;
 * counts[nparts] = records per owner, *sentinel = the n<k sentinel seen. */
int pg_route_stage_a(pg_ctx* ctx, const uint8_t* rec_flags, int extra_empty, int rc0, int nparts, uint64_t* counts,
                     int* sentinel);
/* The held records as 12-byte rows {h as two little-endian 32-bit words,
 * mask word} grouped by owner into d_out (device, 4-byte aligned, capacity
 * out_cap rows; owner o's run after owner o-1's); sums[nparts] = each run's
 * integrity sum: the hash of the 16-byte {h, mask word, 0} form, as
 * pg_dbg_partition_sums (round 6: 16-byte rows before, a quarter more bytes
 * on the wire). */
int pg_route_scatter(pg_ctx* ctx, int nparts, void* d_out, uint64_t out_cap, uint64_t* sums);
/* pg_rows_checksum over 12-byte routed rows (the receiver's check of what
 * pg_route_scatter's sums say was sent). */
int pg_route_rows_checksum(pg_ctx* ctx, const void* d_rows, const uint64_t* seg_off, uint64_t nseg, uint64_t* sums);
/* World 1: stages B and C on the held records where they lie (this rank
 * owns them all) - the dBG and rdBG of pg_build_dbg, no copy. */
int pg_route_finish(pg_ctx* ctx, uint64_t* n_rdbg, pg_stats* stats);
/* Owner `part` of `nparts`: a fresh table from the n received 12-byte rows (every
 * rank's run for this owner, device pointer), stages A (re-binning), B and
 * C; sentinel != 0 adds the n<k key.  pg_dbg_merge_check reports what it
 * read.  The table's hash domain is h rotated left by log2(nparts) bits:
 * pg_dbg_export / pg_rdbg_export return plain keys. */
int pg_route_merge(pg_ctx* ctx, const void* d_rows, uint64_t n, int nparts, int sentinel, uint64_t* n_rdbg,
                   pg_stats* stats);
/* pg_route_merge over nseg segments of rows (segment s: n[s] rows at the
 * device pointer d_segs[s]) as one owner table: a sub-log received as one
 * run per round and source, merged without concatenating it first.
 * pg_dbg_merge_check reports the rows of every segment together. */
int pg_route_merge_segs(pg_ctx* ctx, const void* const* d_segs, const uint64_t* n, int nseg, int nparts, int sentinel,
                        uint64_t* n_rdbg, pg_stats* stats);

/* ---- edge pass: rdbg_edge_weight_jit_ (kmer_numba.py:1808-1827) ->
 *      rdbg_edge_weight (:1446-1518).  rec_flags as above (walked records);
 *      rc1 != 0 also walks the reverse strand (-c bit 0, :2141). */
int pg_edges(pg_ctx* ctx, const uint8_t* rec_flags, int rc1, uint64_t* n_edges);
/* Edges ordered by first occurrence: 4 x uint64 (n0, v0, n1, v1) per edge,
 * the number of walks containing it, and the walk of its first occurrence
 * (2 * record + strand) — what the host needs to emulate the order reversal
 * of the reference's dump/reload checkpoints (kmer_numba.py:1881-1887). */
int pg_edges_export(pg_ctx* ctx, uint64_t* tuples, int64_t* counts, int64_t* first_walk, uint64_t cap);

/* The `.xyz` text of the last pg_edges, "%d_%d\t%d_%d\t%d\n" per edge in
 * first-occurrence order (seq2graph :1893-1904), formatted on the device.
 * out == NULL: only *n_bytes (the size) is set; otherwise cap >= that size. */
int pg_edges_format(pg_ctx* ctx, char* out, uint64_t cap, uint64_t* n_bytes);
/* The same text written to descriptor fd at its position, which then follows
 * it (the reference writes it to `<qry>_rdbg_weight.xyz`, :1893-1904): a
 * regular file opened without O_APPEND takes 16 MiB pieces in parallel
 * (pwrite from per-thread pinned buffers), anything else in order (write).
 * *n_bytes = the bytes written.  Host-side buffered writers on fd must be
 * flushed first. */
int pg_edges_format_fd(pg_ctx* ctx, int fd, uint64_t* n_bytes);

/* seq2graph's label dictionary (kmer_numba.py:1918-1944) built on the device:
 * the `.mcl` entries (key, value) -> line index as the host's dict holds them
 * (a later line wins), then every `.xyz` node - n0_v0, then n1_v1 of each
 * edge in file order - the .mcl did not label, numbered next_label,
 * next_label + 1, ... in order of first appearance (next_label = the number
 * of .mcl lines).  tuples: the edges as the .xyz lists them (n_edges x 4
 * uint64), or NULL for the last pg_edges in first-occurrence order.  The
 * table replaces any pg_set_labels table for the following pg_rows.
 * PG_EINVAL (before any device work, the context's labels unchanged): a node
 * value above 2^32 - 1. */
int pg_labels_from_edges(pg_ctx* ctx, const uint64_t* tuples, uint64_t n_edges, const int64_t* mcl_key,
                         const int64_t* mcl_value, const int64_t* mcl_label, uint64_t n_mcl, int64_t next_label,
                         uint64_t* n_labels);
/* The label table in insertion order: the .mcl entries, then the new ones
 * by label (cap >= n_labels); after the last pg_cluster_cc or
 * pg_cluster_markov, the nodes in file order with their line indices. */
int pg_labels_export(pg_ctx* ctx, int64_t* key, int64_t* value, int64_t* label, uint64_t cap);

/* ---- built-in clustering of the `.xyz` graph (reference README step 4:
 *      "remove weak edges in rdBG and index the connect components"), for runs
 *      without the external `mcl` program.  Added after round 6 together with
 *      pg_clusters_format and pg_clusters_format_fd.
 * Input: the edges as the .xyz lists them (n_edges x 4 uint64 tuples and their
 * int64 counts), or tuples == NULL for the last pg_edges in first-occurrence
 * order (counts and n_edges are then ignored), and min_weight >= 1.
 * Nodes: every distinct (key, value) among (n0, v0) and (n1, v1); the same key
 * with two values is two nodes.  A node's id is its rank of first appearance,
 * reading n0_v0 then n1_v1 of each edge in list order (pg_labels_from_edges'
 * order).  Values fit 32 bits; 2^32 nodes or more is PG_ERANGE.
 * Components: two nodes are joined iff a path of edges with count >=
 * min_weight connects them.  Lighter edges and self-loops join nothing, but
 * their endpoints are nodes: a node without a surviving edge is a cluster of 1.
 * Order: clusters by size descending (mcl's convention), ties by the smallest
 * node id ascending; the position of a cluster is its label.  Members inside a
 * cluster by node id ascending.  The result depends on the input alone.
 * Text (`.mcl` format): one line per cluster, members "<key>_<value>" as
 * unsigned decimals (as pg_edges_format writes them) separated by '\t', the
 * line ended by '\n'; no edges give an empty text.
 * Label table: replaced, as by pg_labels_from_edges, with (key, value) ->
 * line index for every node in file order (pg_labels_export returns that
 * order): the table the written file gives through the `.mcl` reuse path.
 * *n_clusters, *n_nodes (each may be NULL): lines and tokens of the text.
 * PG_EINVAL (before any device work): NULL ctx, min_weight < 1, tuples without
 * counts, a node value above 2^32 - 1. */
int pg_cluster_cc(pg_ctx* ctx, const uint64_t* tuples, const int64_t* counts, uint64_t n_edges, int64_t min_weight,
                  uint64_t* n_clusters, uint64_t* n_nodes);
/* The cluster curve of the `.xyz` graph: what pg_cluster_cc would form at
 * every weight cut of a list, from one union-find that survives from the
 * highest threshold down (the components at a threshold are those at the next
 * higher one plus the unions of the edges whose count lies between the two).
 * Input: edges, nodes and node ids exactly as pg_cluster_cc (tuples == NULL:
 * the last pg_edges where it lies on the device); thresholds[n_thr] strictly
 * ascending, each >= 1, n_thr <= 4096.
 * Row i, T = thresholds[i]: edges[i] = the edges with count >= T (self-loops
 * included); clusters[i], largest[i], singletons[i] = the number of components
 * pg_cluster_cc(min_weight = T) forms (its *n_clusters), the size of the
 * biggest (0 with no nodes) and how many have exactly one node.  The result
 * depends on the input alone.  Integer only.
 * *n_nodes = the nodes, *max_weight = the largest count (0 with no edges).
 * n_thr == 0 is the query form: these two alone.  Every output pointer may be
 * NULL; the four arrays take n_thr entries each.
 * A pure query: the label table, the text of the last pg_cluster_cc and every
 * other result of the context are neither read nor replaced.
 * PG_EINVAL (before any device work): NULL ctx, tuples without counts, tuples
 * == NULL before any pg_edges, a threshold below 1 or not above the one before
 * it, n_thr > 4096, thresholds == NULL with n_thr > 0, a node value above
 * 2^32 - 1.  PG_ERANGE: 2^32 nodes or more. */
int pg_cluster_sweep(pg_ctx* ctx, const uint64_t* tuples, const int64_t* counts, uint64_t n_edges,
                     const int64_t* thresholds, uint64_t n_thr, uint64_t* n_nodes, int64_t* max_weight,
                     uint64_t* edges, uint64_t* clusters, uint64_t* largest, uint64_t* singletons);
/* ---- Markov clustering (MCL) of the `.xyz` graph: the clusters come from flow
 *      instead of a threshold.  Our own MCL in 31-bit fixed point: integer only,
 *      the result depends on the input alone.  It is not bit-identical to the
 *      external `mcl` program, whose pruning scheme and loop weights differ.
 * Constants: ONE = 2^31, CUT = ONE / 10000, STOP = ONE / 1000; every value is
 * an unsigned integer, >> and / are floor operations.
 * Parameters: min_weight >= 1; inflation2 in [3, 40], the inflation being
 * r = inflation2 / 2 (3: mcl's -I 1.5); select in [1, 64]; max_iter in
 * [0, 10000].
 * Nodes: exactly pg_cluster_cc's (ids by first appearance, the same limits).
 * Weights: for nodes i != j, w(i, j) = the summed counts of all listed edges
 * between them, in either direction, whose count is >= min_weight (symmetric).
 * Self-loops in the list and lighter edges add nothing, but their ends are
 * nodes.  A summed weight >= 2^32 is PG_ERANGE.  Every node j gets a loop
 * w(j, j) = the largest w(i, j) of its column, or 1 without an edge.
 * prune(f, select) of a column's positive values f[i]: n[i] = (f[i] << 31) /
 * sum f; the entries ordered by n descending, then by row ascending; the first
 * is kept always, of the rest in that order those with n >= CUT, at most
 * select - 1 of them; the stored value is (n[i] << 31) / sum n[kept], in
 * [1, ONE]; entries are stored by row ascending.
 * Initial matrix: column j = prune of its weights.
 * One iteration, for every column j of the previous matrix M:
 *   expansion  acc[i] = sum over the stored k of column j of M[i,k] * M[k,j]
 *              (exact 64-bit products, the sum below 2^62); e[i] = acc[i] >> 31
 *   scaling    x[i] = (e[i] << 31) / max e (the largest becomes ONE, so the
 *              inflation never empties a column)
 *   inflation  y = ONE; y = (y * x) >> 31, inflation2 / 2 times; inflation2
 *              odd: y = (y * isqrt(x << 31)) >> 31 with the exact integer
 *              root; entries with y == 0 are dropped
 *   new column prune(y, select)
 *   chaos_j    max v - ((sum v^2) >> 31) over the new column's values v
 * Stopping: chaos = the largest chaos_j; the iteration stops when chaos <=
 * STOP or after max_iter iterations.  max_iter == 0 gives the initial matrix
 * with its chaos computed the same way.  No edges: 0 iterations, chaos 0.
 * Clusters: nodes i and j are joined for every stored entry M[i, j] of the last
 * matrix; the clusters are the components.  Their order, the member order, the
 * `.mcl` text and the label table are exactly pg_cluster_cc's, in the same
 * slot: pg_clusters_format[_fd] and pg_labels_export serve either clusterer.
 * tuples == NULL: the last pg_edges where it lies on the device.
 * *n_clusters, *n_nodes, *n_iter (the iterations run), *chaos (the last
 * matrix's): each may be NULL.
 * PG_EINVAL before any device work, the previous clustering, text and label
 * table kept: pg_cluster_cc's list, or a parameter outside its range.
 * PG_ERANGE (2^32 nodes or more, a weight sum) and PG_ENOMEM on an allocation
 * failure of the matrices keep the previous result too.
 * Device memory: two matrices of (8 x select + 4) x U bytes while the call
 * runs (U nodes); the final one is kept, see pg_cluster_markov_matrix. */
int pg_cluster_markov(pg_ctx* ctx, const uint64_t* tuples, const int64_t* counts, uint64_t n_edges,
                      int64_t min_weight, uint32_t inflation2, uint32_t select, uint32_t max_iter,
                      uint64_t* n_clusters, uint64_t* n_nodes, uint32_t* n_iter, uint64_t* chaos);
/* The final matrix of the last pg_cluster_markov, for tests (max_iter = 0, 1,
 * 2 pin the weights, the expansion, the inflation and the pruning apart):
 * col_len[U] the column lengths, rows and vals [U x select] with each column's
 * entries by row ascending and 0 behind them, *select (may be NULL) the stride.
 * The context keeps that matrix, 8 x U x select + 4 x U device bytes, until the
 * next clustering call (pg_cluster_cc or pg_cluster_markov) or pg_destroy.
 * PG_EINVAL before any pg_cluster_markov (or after a later pg_cluster_cc);
 * PG_ERANGE if cap_nodes < U. */
int pg_cluster_markov_matrix(pg_ctx* ctx, uint32_t* col_len, uint32_t* rows, uint32_t* vals, uint64_t cap_nodes,
                             uint32_t* select);
/* Sizes of the last pg_cluster_markov (each pointer may be NULL): U, the
 * stride, and the columns its iterations ran in each size class, summed over
 * the iterations: a wave with a small table (a bound of at most 128
 * candidates), a block with a middle one (at most 1024) and a block with the
 * table for select^2.  PG_EINVAL as pg_cluster_markov_matrix. */
int pg_cluster_markov_stats(pg_ctx* ctx, uint64_t* n_nodes, uint32_t* select, uint64_t* cols_wave,
                            uint64_t* cols_mid, uint64_t* cols_block);
/* The `.mcl` text of the last pg_cluster_cc or pg_cluster_markov (kept on the
 * device).  out == NULL: only *n_bytes (the size) is set; otherwise cap >=
 * that size, else PG_ERANGE.  PG_EINVAL before any of the two. */
int pg_clusters_format(pg_ctx* ctx, char* out, uint64_t cap, uint64_t* n_bytes);
/* The same text written to descriptor fd, as pg_edges_format_fd writes. */
int pg_clusters_format_fd(pg_ctx* ctx, int fd, uint64_t* n_bytes);

/* ---- region rows: seqs2path_jit_ (kmer_numba.py:1830-1849) -> seq2path_jit_
 *      (:1523-1573).  Labels are the host-built label_dct (:1918-1944):
 *      (key, value) -> label, distinct (key, value) pairs.  Label -1 is the
 *      merge's label before a walk's first hit (:1529-1531): as in the
 *      reference, leading hits labelled -1 open no row and only move the
 *      next row's start. */
int pg_set_labels(pg_ctx* ctx, const int64_t* key, const int64_t* value, const int64_t* label, uint64_t n);
int pg_rows(pg_ctx* ctx, const uint8_t* rec_flags, int rc1, uint64_t* n_rows);
/* rows: 5 x int64 per row (record index, start, end, strand +1/-1, label),
 * in print order. */
int pg_rows_export(pg_ctx* ctx, int64_t* rows5, uint64_t cap);
/* The text of the last pg_rows, "qid\tstart\tend\t+|-\tlabel\n" per row in
 * print order (:1946-1949), formatted on the device; qid of record r is
 * names[name_off[r] .. name_off[r+1]) (n_names >= records, n_names + 1
 * offsets); every call formats with its own names.  out == NULL: only
 * *n_bytes is set. */
int pg_rows_format(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, char* out, uint64_t cap,
                   uint64_t* n_bytes);
/* The same text written to descriptor fd (the reference prints it to
 * stdout, :1946-1949), as pg_edges_format_fd writes. */
int pg_rows_format_fd(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                      uint64_t* n_bytes);

/* ---- frequency table: what the region rows are made for (the reference
 *      README: "a graph-based method to find the frequency across species";
 *      its only helper, other/fr_stat.py, reduces a row file to the count,
 *      max and mean of abs(end - start)).  Per label the genomes it occurs
 *      in, its occurrences and bases; the spectrum; per genome the core /
 *      shell / unique bases.  Integer only; the result depends on the input
 *      alone, whatever the schedule.
 * Input: rows (record, start, end, strand, label) - the last pg_rows where
 * they lie on the device (rows5 == NULL; n_rows is then ignored) or n_rows
 * host rows of 5 x int64 as pg_rows_export returns them - and rec_group
 * [n_records] int32: the genome of each record, in [0, n_groups), or -1 for
 * "no genome".  n_groups >= 1; n_groups == 0 only with no rows.
 * A row is used iff label >= 0 and rec_group[record] >= 0; the others are
 * skipped and counted in *n_skipped (*n_used: the used ones; *n_labels: the
 * table's entries; each may be NULL).
 * PG_EINVAL, before any device work, the previous frequency result kept: a
 * NULL context; rec_group == NULL; a rec_group entry outside [-1, n_groups);
 * n_records different from the context's record count when rows5 == NULL; a
 * host row whose record is outside [0, n_records); rows5 == NULL before any
 * pg_rows.
 * The tables are dense in the label: L = 1 + the largest used label, and
 * L > 2^31 is PG_ERANGE (found by a device reduction before anything is
 * allocated or replaced).  The pipeline's labels are line and first-appearance
 * indices, so they are dense.  The dense arrays take (5 + W) x 8 x L device
 * bytes while the call runs; an allocation failure is PG_ENOMEM with the
 * previous result kept.
 * Table: one entry per label with at least one used row, labels ascending:
 *   n_rows; n_plus, the used rows with strand +1; total_bp = sum of
 *   |end - start| (unsigned 64-bit; the absolute value as fr_stat.py:14);
 *   min_len, max_len; the presence set, W = ceil(n_groups / 64) uint64 words
 *   per entry, genome g being bit g % 64 of word g / 64; n_genomes, its
 *   popcount.
 * Spectrum, g in 0..n_groups: labels_by_g[g] = the labels with n_genomes ==
 * g, bp_by_g[g] = the sum of their total_bp; index 0 is always 0.
 * Per genome: rows (used rows), bp_total, bp_core (rows whose label has
 * n_genomes == n_groups), bp_unique (n_genomes == 1 when n_groups > 1: with
 * one genome everything is core), bp_shell (the rest); bp_core + bp_shell +
 * bp_unique == bp_total. */
int pg_freq(pg_ctx* ctx, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
            uint32_t n_groups, uint64_t* n_labels, uint64_t* n_used, uint64_t* n_skipped);
/* The table of the last pg_freq in label order; any output pointer may be
 * NULL; bits takes W words per entry.  cap (entries) below *n_labels is
 * PG_ERANGE.  This and the four calls below: PG_EINVAL before any pg_freq. */
int pg_freq_export(pg_ctx* ctx, int64_t* label, uint32_t* n_genomes, uint64_t* n_rows, uint64_t* n_plus,
                   uint64_t* total_bp, uint64_t* min_len, uint64_t* max_len, uint64_t* bits, uint64_t cap);
int pg_freq_spectrum(pg_ctx* ctx, uint64_t* labels_by_g, uint64_t* bp_by_g, uint64_t cap);      /* cap >= n_groups + 1 */
int pg_freq_groups(pg_ctx* ctx, uint64_t* rows, uint64_t* bp_total, uint64_t* bp_core, uint64_t* bp_shell,
                   uint64_t* bp_unique, uint64_t cap);                                      /* cap >= n_groups     */
/* The table's text, formatted on the device and kept there like the `.mcl`
 * text: the header "#label\tgenomes\trows\tplus\tbp\tmin\tmax\n", then one
 * line of unsigned decimals per entry in table order, '\t'-separated and
 * '\n'-ended (no entries: the header alone).  out == NULL: only *n_bytes (the
 * size) is set; otherwise cap >= that size, else PG_ERANGE. */
int pg_freq_format(pg_ctx* ctx, char* out, uint64_t cap, uint64_t* n_bytes);
/* The same text written to descriptor fd, as pg_clusters_format_fd writes. */
int pg_freq_format_fd(pg_ctx* ctx, int fd, uint64_t* n_bytes);

/* ---- genome comparison: the two results a pangenome study draws from the
 *      frequency table's presence sets - how much every pair of genomes
 *      shares, and how the pan and the core genome change as genomes are
 *      added (the accumulation or "growth" curves) over several genome
 *      orders.  Integer only; the result depends on the input alone, whatever
 *      the schedule.
 * Input: a presence table bits, uint64 [n_labels][W], W = ceil(n_groups / 64),
 * genome g being bit g % 64 of word g / 64 as pg_freq_export returns it -
 * the table of the last pg_freq where it lies on the device (bits == NULL;
 * n_labels is then ignored and n_groups must equal that table's) or n_labels
 * host rows of W words.  Label l "is in" genome g iff that bit is set; a row
 * of zeros is allowed and is in no genome.  orders: int32 [n_orders][n_groups],
 * every row a permutation of 0 .. n_groups - 1; n_orders >= 0.
 * Shared: shared[g][h] = the labels in both g and h, uint64 [G][G]; the
 * diagonal is the number of labels in g; the matrix is symmetric.
 * Curves, uint64 [P][G] each: for order p and n = 1 .. G let S = the first n
 * genomes of orders[p]; pan[p][n-1] = the labels in at least one genome of S,
 * core[p][n-1] = the labels in every genome of S.  So pan[p][G-1] = the
 * labels with at least one genome, core[p][G-1] = the labels in all G, and
 * pan[p][0] = core[p][0] = shared[o][o] with o = orders[p][0].
 * Computed as: the bits transposed to genome-major rows; shared = the
 * popcount of the AND of two rows; pan / core = the popcounts of the running
 * OR / AND of the rows taken in the order.
 * The results stay on the device until the next successful pg_freq_compare;
 * a successful pg_freq drops them (they described the old table: the two
 * exports then return PG_EINVAL).
 * PG_EINVAL, before any device work, the previous result kept: a NULL
 * context; bits == NULL before any pg_freq or with another n_groups than its
 * table's; n_groups == 0 with n_labels > 0; orders == NULL with n_orders > 0;
 * an order row that is not a permutation of 0 .. n_groups - 1; a host row
 * with a bit at or above n_groups set.  n_groups > 32768 is PG_ERANGE (the
 * matrix is dense).  An allocation failure is PG_ENOMEM with the previous
 * result kept.  n_labels == 0 gives all zeros, n_groups == 0 empty results. */
int pg_freq_compare(pg_ctx* ctx, const uint64_t* bits, uint64_t n_labels, uint32_t n_groups,
                    const int32_t* orders, uint32_t n_orders);
/* The results of the last pg_freq_compare: PG_EINVAL before any, PG_ERANGE
 * for a short cap (in cells).  shared, pan or core may be NULL; with
 * n_orders == 0 pg_freq_curve succeeds and writes nothing. */
int pg_freq_shared(pg_ctx* ctx, uint64_t* shared, uint64_t cap);              /* cap >= G * G      */
int pg_freq_curve(pg_ctx* ctx, uint64_t* pan, uint64_t* core, uint64_t cap);  /* cap >= P * G each */

/* ---- k-mer colours: the coloured de Bruijn graph - which genomes hold every
 *      k-mer of the dBG.  Unlike the region labels it depends on no clustering
 *      (-a, -w, -I): the exact k-mer spectrum (core, shell, unique), exact
 *      k-mer distances between genomes and the k-mer pan / core growth curves
 *      follow from it.  Integer only; OR is commutative, so the result depends
 *      on the input alone, whatever the schedule.
 * Input: a context with a parse and the dBG table of a build or load over
 * that parse (whatever pg_dbg_export would return); rec_group [n_records]
 * int32, the genome of each record in [0, n_groups) or -1 for "no genome";
 * rec_flags [n_records] uint8 as pg_build_dbg takes it (NULL: all); rc0.
 * Walked record: rec_flags[r] != 0 and rec_group[r] >= 0.  Its windows are
 * exactly the ones pg_build_dbg inserts for that record under that rc0: the
 * forward strand, and the reverse strand if rc0, the short-record rules for
 * n <= k + 1 included.  The n < k sentinel window is left out: the table never
 * holds it (pg_dbg_export appends the key 2^64 - 1 from a flag), so it is no
 * key here either.  Only keys matter; the masks are not read.
 * Keys and colours: K[0 .. n) = the table's plain keys in ascending order,
 * exactly pg_dbg_export's without that sentinel; colour[i] = W =
 * ceil(n_groups / 64) uint64 words, genome g being bit g % 64 of word g / 64
 * as in pg_freq.  The bit is set iff some window of a walked record of genome
 * g has the key K[i] - put differently, iff K[i] is in the dBG built from
 * genome g's records alone.  A bit at or above n_groups is never set.
 * Counts (each pointer may be NULL): *n_keys = n; *n_windows = the windows
 * looked up; *n_missing = those whose key is not in the table - they colour
 * nothing, which is no error and can only happen when the table was built
 * from fewer records than are walked; *n_uncoloured = the keys with no bit.
 * Spectrum: kmers_by_g[0 .. G] = the keys in exactly g genomes; index 0 equals
 * *n_uncoloured.  Per genome: kmers = its keys; core = its keys found in all G
 * genomes; unique = its keys found in it alone when G > 1 (with one genome
 * everything is core, as in pg_freq); shell = the rest; core + shell + unique
 * == kmers.
 * Comparison (pg_kmer_compare): shared[g][h], pan[p][n] and core[p][n] exactly
 * as pg_freq_compare defines them with "label" read as "key", over orders
 * int32 [n_orders][G]; its result is its own: pg_freq, pg_freq_compare,
 * pg_tree_nj and every region pass neither read nor drop it, nor it theirs.
 * Lifetime: the colours stay on the device - 8 (W + 1) n bytes; twice that
 * and 4 bytes per table slot while the call runs - until the next successful
 * pg_kmer_colors, pg_kmer_colors_drop, or any call that replaces the dBG
 * table (a parse, build, load or merge), after which the calls below return
 * PG_EINVAL.  A successful pg_kmer_colors drops the previous comparison.
 * PG_EINVAL, before any device work, the previous result kept: a NULL
 * context; no parse or no table; rec_group == NULL; an entry outside
 * [-1, n_groups); n_records different from the context's record count;
 * n_groups == 0 with records.  n_groups > 32768 is PG_ERANGE, as in the
 * comparison, and so is a table of 2^32 keys or more.  An allocation failure
 * is PG_ENOMEM with the previous result kept. */
int pg_kmer_colors(pg_ctx* ctx, const int32_t* rec_group, const uint8_t* rec_flags, uint64_t n_records,
                   uint32_t n_groups, int rc0, uint64_t* n_keys, uint64_t* n_windows, uint64_t* n_missing,
                   uint64_t* n_uncoloured);
/* The keys and colours of the last pg_kmer_colors, bits [n][W] key-major;
 * either pointer may be NULL (both: only *n is set, which may be NULL too);
 * cap (keys) below n is PG_ERANGE. */
int pg_kmer_colors_export(pg_ctx* ctx, uint64_t* keys, uint64_t* bits, uint64_t cap, uint64_t* n);
/* kmers_by_g [G + 1] and the per-genome columns [G]; each may be NULL. */
int pg_kmer_colors_spectrum(pg_ctx* ctx, uint64_t* kmers_by_g, uint64_t* g_kmers, uint64_t* g_core, uint64_t* g_shell,
                            uint64_t* g_unique);
/* The comparison of the colours where they lie; orders as pg_freq_compare
 * takes them (PG_EINVAL for a row that is no permutation, or NULL with
 * n_orders > 0; the previous comparison is kept).  Export: shared [G][G]
 * (shared_cap >= G * G), pan and core [P][G] (curve_cap >= P * G each); each
 * pointer may be NULL; a short cap is PG_ERANGE; PG_EINVAL before any
 * pg_kmer_compare over the current colours. */
int pg_kmer_compare(pg_ctx* ctx, const int32_t* orders, uint32_t n_orders);
int pg_kmer_compare_export(pg_ctx* ctx, uint64_t* shared, uint64_t shared_cap, uint64_t* pan, uint64_t* core,
                           uint64_t curve_cap);
/* HIP events on the context's stream over the last pg_kmer_colors: ms_index =
 * the key index before the colouring pass and the tables after it (rows
 * brought into key order, spectrum), ms_colour = the colouring pass alone,
 * ms_compare = the last pg_kmer_compare over these colours (0 before any);
 * n_windows as pg_kmer_colors returned it. */
int pg_kmer_colors_time(pg_ctx* ctx, double* ms_index, double* ms_colour, double* ms_compare, uint64_t* n_windows);
/* Releases the colours and their comparison (no error when there are none). */
int pg_kmer_colors_drop(pg_ctx* ctx);

/* ---- genome tree: the third thing a pangenome study draws from the
 *      comparison - a tree of the genomes, by neighbour joining over a
 *      distance matrix.  Integer only (fixed point); the result depends on
 *      the input alone, whatever the schedule.
 * Input: a distance matrix dist, uint64 [n][n], n <= 16384, in one of two forms.
 * From the host: symmetric, with a zero diagonal and no entry above 2^31.
 * dist == NULL: formed on the device from the `shared` matrix of the last
 * successful pg_freq_compare where it lies; n must equal its G, and
 *   d(g, h) = shared[g][g] + shared[h][h] - 2 shared[g][h],
 * the labels in exactly one of the two genomes: a Hamming distance, so a
 * metric, and at most 2^31 because pg_freq caps L at 2^31.
 * Fixed point: S = 16 fractional bits, D = d << S.  Every value is a signed
 * 64-bit integer; `>>` is an arithmetic shift and `/` is floor division, both
 * rounding towards minus infinity (as Python's >> and // do).
 * Slots: slot i holds leaf i at first.  Leaves have the node ids 0 .. n - 1,
 * internal nodes are numbered n, n + 1, .. in join order.  A live slot keeps
 * its position for the whole run.
 * One join, while more than 3 slots are live (m = the number of live slots):
 *   r_i = the sum over the live k of D[i][k];
 *   Q(i, j) = (m - 2) D[i][j] - r_i - r_j for the live i < j;
 *   the pair with the smallest Q is joined - among equal Q the smallest i,
 *   then the smallest j;
 *   len_i = clamp((D[i][j] + (r_i - r_j) / (m - 2)) >> 1, 0, D[i][j]),
 *   len_j = D[i][j] - len_i; the join record is (node[i], node[j], len_i, len_j);
 *   for every other live k, D[i][k] = D[k][i] = max(0, (D[i][k] + D[j][k] - D[i][j]) >> 1);
 *   slot i now holds the new internal node and slot j is dead.
 * The end: three live slots a < b < c are the three children of the root,
 * each length on its own: x_a = max(0, (D_ab + D_ac - D_bc) >> 1), x_b and x_c
 * likewise.  n = 2: two children, x_a = D_ab >> 1 and x_b = D_ab - x_a.  n = 1:
 * one child of length 0.  n = 0: an empty result (no join, no child).
 * There are max(n - 3, 0) joins.
 * Why 64 bits hold it: D < 2^47 at the start (d <= 2^31, S = 16), and the
 * clamped update never exceeds max(D[i][k], D[j][k]) (D[i][j] >= 0), so the
 * bound holds throughout.  With m <= 2^14, r and (m - 2) D stay below 2^61, so
 * |Q| < 2^63.
 * Exactness: on an additive matrix - the path lengths of a tree with integer
 * edge lengths - every division above is exact (every D is a multiple of
 * 2^S, and the sums that are halved or divided are the even / divisible ones
 * of the textbook method), so the tree and its lengths come back exactly:
 * every length is a multiple of 2^S and they sum to the tree's length.
 * (Checked on the host specification on 200 random trees of 4 to 40 leaves.)
 * Device memory: 8 n^2 + O(n) bytes while the call runs (one matrix holds the
 * working D in its upper triangle and the d that came in below it); the
 * 8 n^2 of d stay until the next successful pg_tree_nj.  Three plain launches
 * per join on the context's stream.
 * Lifetime: the tree is a copy and stays until the next successful
 * pg_tree_nj; pg_freq, pg_freq_compare and every region pass neither read nor
 * drop it, nor it theirs.
 * PG_EINVAL, the previous tree kept: a NULL context; dist == NULL before any
 * pg_freq_compare or with another n than its G; a host matrix that is not
 * symmetric, has a non-zero diagonal or an entry above 2^31 (found by a device
 * reduction before anything is replaced).  n > 16384 is PG_ERANGE, decided
 * before the matrix is read.  An allocation failure is PG_ENOMEM with the
 * previous tree kept.  n_joins may be NULL. */
int pg_tree_nj(pg_ctx* ctx, const uint64_t* dist, uint32_t n, uint64_t* n_joins);
/* The results of the last pg_tree_nj: PG_EINVAL before any, PG_ERANGE for a
 * short cap (entries).  Every output may be NULL.  pg_tree_dist: the d the
 * tree was built from, [n][n], cap >= n * n.  pg_tree_joins: per join the two
 * nodes joined (the left is slot i's, the right slot j's) and their lengths
 * with S fractional bits, cap >= max(n - 3, 0).  pg_tree_root: the number of
 * the root's children (min(n, 3)), their nodes and lengths, the unused
 * entries 0.  pg_tree_time: HIP events over the joins, and cells = the sum of
 * m^2 over them. */
int pg_tree_dist(pg_ctx* ctx, uint64_t* dist, uint64_t cap);
int pg_tree_joins(pg_ctx* ctx, uint32_t* left, uint32_t* right, uint64_t* left_len, uint64_t* right_len, uint64_t cap);
int pg_tree_root(pg_ctx* ctx, uint32_t* n_children, uint32_t child[3], uint64_t len[3]);
int pg_tree_time(pg_ctx* ctx, double* ms, uint64_t* cells);

/* ---- tree support: how far every branch of the genome tree can be trusted,
 *      by the bootstrap - the characters (the presence rows) are resampled
 *      with replacement, the tree is rebuilt for every resample, and every
 *      join of the real tree is rated by the number of replicate trees that
 *      split the genomes the same way.  Integer only; the draws are
 *      counter-based, so the result depends on (bits, seed, n_reps) and the
 *      rated tree alone, whatever the schedule, the batch size or the form.
 * Input: a presence table bits, uint64 [n_labels][W], exactly as
 * pg_freq_compare takes it (bits == NULL: the last pg_freq's table where it
 * lies; n_labels is then ignored and n_groups must equal that table's);
 * n_reps = R in [1, 4096]; a 64-bit seed; and the context's last pg_tree_nj
 * tree, whose joins are rated and whose n must equal n_groups.  L = n_labels.
 * Draws: for replicate b in 0 .. R - 1 and draw t in 0 .. L - 1, x = output t
 * of splitmix64 started at seed ^ ((b + 1) * 0xD1B54A32D192ED03) (synth.py's
 * splitmix64(seed, b + 1, L): z = state + (t + 1) * 0x9E3779B97F4A7C15, then
 * z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) *
 * 0x94D049BB133111EB, x = z ^ z >> 31) - a pure function of (seed, b, t) -
 * and idx(b, t) = ((x >> 32) * L) >> 32 in unsigned 64 bits (no wrap:
 * L <= 2^31).  The replicate's characters are the rows bits[idx(b, 0)], ..,
 * bits[idx(b, L - 1)].  L > 2^31 is PG_ERANGE.
 * Replicate distance: d_b(g, h) = the draws t whose row has exactly one of
 * the bits g, h set: a Hamming distance over the drawn rows, at most L <=
 * 2^31, pg_tree_nj's input bound.  With L == 0 every d_b is 0 (the star's
 * tie rule decides the tree).
 * Replicate tree: the method of "genome tree" above applied to d_b, unchanged
 * (16 fractional bits, floor shifts, the total order (Q, i, j), slots that
 * keep their position).  Only the joins' (left, right) are kept.
 * Splits: the clade of leaf i is {i}, that of node n + t the union of its two
 * children's.  The split of join t is its clade if leaf 0 is not in it,
 * otherwise the complement within 0 .. n - 1, held as W words.  A tree of
 * n > 3 leaves has n - 3 joins and as many distinct, non-trivial splits.
 * Support: support[t], uint32, t < J = max(n - 3, 0) = the replicates b whose
 * tree has a join with the same split as join t of the rated tree (a hash
 * pre-filters; a match counts only after all W words are equal).
 * Guard: before any replicate runs, the un-resampled Hamming matrix of bits is
 * formed by the same distance kernels (idx = the identity) and compared on the
 * device with the rated tree's pg_tree_dist; a difference is PG_EINVAL ("the
 * tree was not built from this table"), the previous support kept.
 * PG_EINVAL, before any device work, the previous result kept: a NULL
 * context; no tree; n_groups different from the tree's n; bits == NULL before
 * any pg_freq or with another n_groups than its table's; R outside [1, 4096];
 * a host row with a bit at or above n_groups.  An allocation failure is
 * PG_ENOMEM with the previous result kept.
 * rep_dist (for tests; NULL: not wanted): the full symmetric replicate
 * matrices with zero diagonal, uint64 [R][n][n]; rep_dist_cap (cells) below
 * R * n * n is PG_ERANGE, decided before any device work.  Nothing of size
 * R x n^2 is kept after the call.
 * Device work, in batches of replicates that fit PG_TUNE_BOOT_SCRATCH bytes:
 * draw + gather + transpose in one pass, a batched Hamming "popcount GEMM",
 * every replicate's whole neighbour joining by one workgroup (the matrix in
 * LDS up to n = 128, in global scratch above it while enough replicates run
 * side by side, pg_tree_nj's per-join launches otherwise; PG_TUNE_BOOT_FORM),
 * then clades and matching.
 * Lifetime: the support and the replicate joins are small host-side copies
 * and stay until the next successful pg_tree_bootstrap; a successful
 * pg_tree_nj drops them (they described the old tree: the exports below then
 * return PG_EINVAL). */
int pg_tree_bootstrap(pg_ctx* ctx, const uint64_t* bits, uint64_t n_labels, uint32_t n_groups, uint32_t n_reps,
                      uint64_t seed, uint64_t* rep_dist /* NULL or [R][n][n] */, uint64_t rep_dist_cap);
/* The results of the last pg_tree_bootstrap: PG_EINVAL before any (or after a
 * later pg_tree_nj), PG_ERANGE for a short cap (entries).  Every output may be
 * NULL.  pg_tree_support: support [J], cap >= J, and R.
 * pg_tree_bootstrap_joins: every replicate's joins, uint32 [R][J] each, cap >=
 * R * J.  pg_tree_bootstrap_time: HIP events over the batches' distance
 * passes, joins, and clade / matching passes, and cells = R x the sum of m^2
 * over a tree's joins.  pg_tree_bootstrap_form: which form of the neighbour
 * joining ran (1, 2 or 3 as PG_TUNE_BOOT_FORM numbers them; 0: n <= 3, there
 * was no join) and the number of batches. */
int pg_tree_support(pg_ctx* ctx, uint32_t* support, uint64_t cap, uint32_t* n_reps);
int pg_tree_bootstrap_joins(pg_ctx* ctx, uint32_t* left, uint32_t* right, uint64_t cap);
int pg_tree_bootstrap_time(pg_ctx* ctx, double* ms_dist, double* ms_nj, double* ms_support, uint64_t* cells);
int pg_tree_bootstrap_form(pg_ctx* ctx, uint32_t* form, uint32_t* n_batches);

/* ---- region graph: which region follows which along a genome - the other
 *      half of a pangenome result next to the frequency table.  Nodes are the
 *      labels, links the ordered pairs of labels on adjacent rows of one walk,
 *      paths the walks; the links table's text, and the whole graph as GFA 1.
 *      Integer only; the result depends on the input alone, whatever the
 *      schedule.
 * Input: exactly pg_freq's - rows (record, start, end, strand, label), the
 * last pg_rows where they lie on the device (rows5 == NULL; n_rows is then
 * ignored) or n_rows host rows of 5 x int64, and rec_group [n_records] int32
 * in [-1, n_groups).  A row is used iff label >= 0 and rec_group[record] >= 0;
 * the others are counted in *n_skipped (every count pointer may be NULL).
 * Run (one path): a maximal stretch of rows that are consecutive in the list,
 * all used, and equal in record and in strand (equal values); an unused row,
 * a new record or a new strand ends it; one row is a path of one step.  For
 * the rows of pg_rows a run is one walk of one record on one strand.
 * Link (a, b): two rows adjacent in a run, a the earlier row's label and b the
 * later one's - walk order; no orientation is inferred and a == b is a legal
 * link.  count = the adjacent pairs over all runs, n_genomes = the distinct
 * rec_group[record] among them.
 * Node: every label with a used row: n_rows, its used rows; max_len, the
 * largest |end - start| of them (unsigned 64-bit, as pg_freq); n_out / n_in,
 * the distinct links leaving / entering it.
 * Order: nodes by label ascending, links by (a, b) ascending, paths in list
 * order.
 * PG_EINVAL, before any device work, the previous region graph kept: pg_freq's
 * list - a NULL context; rec_group == NULL; a rec_group entry outside
 * [-1, n_groups); n_records different from the context's record count when
 * rows5 == NULL; a host row whose record is outside [0, n_records);
 * rows5 == NULL before any pg_rows; n_groups == 0 with rows.
 * The tables are dense in the label: L = 1 + the largest used label, and
 * L > 2^31 is PG_ERANGE (found by a device reduction before anything is
 * allocated or replaced).  The dense arrays take 24 x L device bytes while the
 * call runs, the link pass 32 bytes per adjacent pair; an allocation failure
 * is PG_ENOMEM with the previous graph kept.
 * The graph stays on the device until the next successful pg_region_graph;
 * pg_freq and pg_freq_compare neither read nor drop it, nor it theirs. */
int pg_region_graph(pg_ctx* ctx, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group,
                    uint64_t n_records, uint32_t n_groups, uint64_t* n_nodes, uint64_t* n_links, uint64_t* n_paths,
                    uint64_t* n_skipped);
/* The three tables of the last pg_region_graph; any output pointer may be
 * NULL; cap (entries) below the table's size is PG_ERANGE.  These and the
 * four text calls below: PG_EINVAL before any pg_region_graph.
 * Paths: for the run's first row f and last row z, lo = min(f.start, z.start)
 * and hi = max(f.end, z.end) (the run's span for the rows of pg_rows, on
 * either strand); n_steps, its rows; strand, the value the rows carry. */
int pg_region_nodes(pg_ctx* ctx, int64_t* label, uint64_t* n_rows, uint64_t* max_len, uint32_t* n_out,
                    uint32_t* n_in, uint64_t cap);
int pg_region_links(pg_ctx* ctx, int64_t* from, int64_t* to, uint64_t* count, uint32_t* n_genomes, uint64_t cap);
int pg_region_paths(pg_ctx* ctx, int64_t* record, int64_t* strand, int64_t* lo, int64_t* hi, uint64_t* n_steps,
                    uint64_t cap);
/* The links table's text, formatted on the device and kept there like
 * pg_freq_format's: the header "#from\tto\tcount\tgenomes\n", then one
 * "%d\t%d\t%d\t%d\n" line per link in table order (no links: the header
 * alone).  out == NULL: only *n_bytes (the size) is set; otherwise cap >= that
 * size, else PG_ERANGE.  The _fd form writes as pg_freq_format_fd does. */
int pg_region_links_format(pg_ctx* ctx, char* out, uint64_t cap, uint64_t* n_bytes);
int pg_region_links_format_fd(pg_ctx* ctx, int fd, uint64_t* n_bytes);
/* The graph as GFA 1, formatted on the device by every call with its own
 * names (names[name_off[r] .. name_off[r+1]) is record r's, copied verbatim,
 * as pg_rows_format takes them), in this order:
 *   H\tVN:Z:1.0\n
 *   S\t<label>\t*\tLN:i:<max_len>\n                              per node
 *   L\t<a>\t+\t<b>\t+\t0M\tRC:i:<count>\tgn:i:<n_genomes>\n      per link
 *   P\t<name>:<lo>-<hi>:<+|->\t<label>+,<label>+,...\t*\n        per path
 * the sign being + iff the strand equals 1, as pg_rows_format prints it.  No
 * segment sequences: `*` plus LN is valid GFA 1.  With no rows the text is the
 * H line alone.  n_names below the context's record count - with host rows:
 * below 1 + the largest record of a used row - is PG_EINVAL, as is a NULL or
 * descending name_off.  out == NULL: only *n_bytes is set; otherwise cap >=
 * that size, else PG_ERANGE.  The _fd form writes as pg_rows_format_fd does. */
int pg_region_gfa(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                  uint64_t cap, uint64_t* n_bytes);
int pg_region_gfa_fd(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                     uint64_t* n_bytes);

/* ---- region sequences: what a region is - one representative sequence per
 *      label, decoded on the device from the parse's packed base stream (the
 *      reference's `recover(path, dbg)` is a stub, kmer_numba.py:1953-1955).
 *      The result depends on the input alone, whatever the schedule.
 * Input: exactly pg_region_graph's rows, rec_group and rule for a used row;
 * the others are counted in *n_skipped (every count pointer may be NULL).  In
 * both forms n_records must equal the context's record count: the bases come
 * from the context's parse.
 * Representative of a label: its used row with the largest |end - start| (the
 * max_len of pg_region_nodes); among equals the first in list order.
 * Sequence: with lo = min(start, end) and hi = max(start, end), F is bases
 * [lo, hi) of the record's compacted sequence (the coordinates the rows are
 * printed in), one letter per base by its class: A, C, G, T; N, '$' and every
 * other byte give N (the parse has already folded case and the IUPAC codes:
 * no lower case and no code but N comes back).  strand == 1: F; otherwise the
 * reverse complement of F (A<->T, C<->G, N->N) - the walk's orientation, so a
 * GFA step <label>+ is consistent on both strands.
 * Table: one entry per label with a used row, labels ascending: label; row,
 * the representative's index in the list; record, start, end, strand as the
 * row carries them; len = hi - lo; gc, its C or G letters; amb, its N letters;
 * offset, the exclusive prefix sum of len.  The bases are the sequences one
 * after another in table order with no separators, n_bases = the sum of len.
 * PG_EINVAL, before any result is replaced: pg_region_graph's whole list; a
 * context without a parse; a used row with lo < 0 or hi > the record's length
 * (found by a device reduction before anything is allocated).  L = 1 + the
 * largest used label > 2^31 is PG_ERANGE (the dense arrays take 16 x L device
 * bytes while the call runs); an allocation failure is PG_ENOMEM.  In every
 * refusal the previous result stays.
 * The result is a copy: it stays until the next successful pg_region_seqs; a
 * later parse or build does not touch it; pg_freq, pg_freq_compare and
 * pg_region_graph neither read nor drop it, nor it theirs. */
int pg_region_seqs(pg_ctx* ctx, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group,
                   uint64_t n_records, uint32_t n_groups, uint64_t* n_regions, uint64_t* n_bases,
                   uint64_t* n_skipped);
/* The table and the bases of the last pg_region_seqs; any output pointer may
 * be NULL; cap (entries, bytes) below the size is PG_ERANGE.  out == NULL:
 * only *n_bytes is set.  These and the four text calls below: PG_EINVAL
 * before any pg_region_seqs. */
int pg_region_seqs_table(pg_ctx* ctx, int64_t* label, int64_t* row, int64_t* record, int64_t* start, int64_t* end,
                         int64_t* strand, uint64_t* len, uint64_t* gc, uint64_t* amb, uint64_t* offset,
                         uint64_t cap);
int pg_region_seqs_bases(pg_ctx* ctx, uint8_t* out, uint64_t cap, uint64_t* n_bytes);
/* The decoder kernel of the last pg_region_seqs: its time in ms (HIP events on
 * the context's stream; 0 with no bases) and the 16-letter chunks it wrote
 * (every sequence's length rounded up to 16, over 16).  Either may be NULL. */
int pg_region_seqs_time(pg_ctx* ctx, double* ms_decode, uint64_t* n_chunks);
/* The sequences as FASTA, formatted on the device by every call with its own
 * names (as pg_region_gfa takes them, copied verbatim), per entry
 *   ><label> <name>:<lo>-<hi>:<+|-> len=<len>\n<sequence>\n
 * the sign being + iff the strand equals 1 and the sequence on one line; no
 * entries: an empty text.  n_names, name_off, out, cap and the _fd form: as
 * pg_region_gfa and pg_region_gfa_fd. */
int pg_region_fasta(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                    uint64_t cap, uint64_t* n_bytes);
int pg_region_fasta_fd(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                       uint64_t* n_bytes);
/* pg_region_gfa's text and arguments, except that every S line carries its
 * sequence: S\t<label>\t<sequence>\tLN:i:<max_len>\n.  It needs both a region
 * graph and region sequences, of the same rows and groups: PG_EINVAL unless
 * the two tables have the same labels and len == max_len for every one
 * (checked on the device). */
int pg_region_gfa_seq(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                      uint64_t cap, uint64_t* n_bytes);
int pg_region_gfa_seq_fd(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                         uint64_t* n_bytes);

/* ---- variable sites: where the genomes differ - the simple bubbles of the
 *      region graph.  A site is a pair of flanking labels (a, c) that the
 *      genomes join in two or more ways: directly, or through one region x.
 *      Integer only; the result depends on the input alone, whatever the
 *      schedule.
 * Input: exactly pg_region_graph's - rows, rec_group, the rule for a used
 * row, the run, and the count of the others in *n_skipped (every count
 * pointer may be NULL).
 * Record: two consecutive rows of a run with labels (a, c) give a direct
 * record - site (a, c), via = -1, length 0; three consecutive rows with labels
 * (a, x, c) give a via record - site (a, c), via = x, length |end - start| of
 * the middle row (unsigned 64-bit, as pg_freq).  Walk order, as the links: no
 * orientation is inferred, the reverse walk's labels are other labels and its
 * bubbles other sites.  a == c, x == a and x == c are legal.  The genome of a
 * record is rec_group[record].  *n_records_emitted: the records, direct and
 * via.
 * Allele of a flank pair: a distinct via.  Site: a flank pair with two
 * alleles or more; a pair with one allele - the conserved chain - is dropped.
 * LIMIT: only bubbles with at most one region inside are found.  An insertion
 * of two regions against a direct join is a pair (a, c) with the direct
 * allele alone and is not reported, nor is it pieced together from shorter
 * sites; pg_region_bubbles, below, walks from anchor to anchor instead.
 * Alleles table, by (a, c, via) ascending - the direct allele first in its
 * site: site, the index of its site; via; count, its records; n_genomes, the
 * distinct genomes among them; min_len and max_len over their lengths; the
 * presence set, W = ceil(n_groups / 64) uint64 words with genome g at bit
 * g % 64 of word g / 64 (as pg_freq_export).
 * Sites table, by (a, c) ascending: from = a, to = c; n_alleles; first, the
 * index of its first allele; count, the sum over its alleles; n_genomes, the
 * popcount of the OR of their presence sets.
 * Per genome (n_groups entries): sites, the sites where it carries any
 * allele; alleles, the allele entries with its bit set; private, the allele
 * entries whose only genome it is.
 * PG_EINVAL, before any device work: pg_region_graph's whole list.  L = 1 +
 * the largest used label > 2^31 is PG_ERANGE (found by a device reduction
 * before anything is allocated).  Nothing is dense in the label: the call
 * takes device memory by the rows and the records (a run of r rows gives
 * 2 r - 3 of them) - 9 bytes per row, 37 per used row for the steps, 64 per
 * record while they are sorted, then 49 per record and at most 58 more per
 * allele of any pair for the flags, their scans and the heads - and the tables
 * 44 + 8 W bytes per allele and 40 + 8 W per site.  An allocation failure is PG_ENOMEM.  In every refusal
 * the previous result stays: the new one is built aside and swapped in last.
 * The result stays until the next successful pg_region_sites; pg_freq,
 * pg_freq_compare, pg_region_graph and pg_region_seqs neither read nor drop
 * it, nor it theirs. */
int pg_region_sites(pg_ctx* ctx, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group,
                    uint64_t n_records, uint32_t n_groups, uint64_t* n_sites, uint64_t* n_alleles,
                    uint64_t* n_records_emitted, uint64_t* n_skipped);
/* The three tables of the last pg_region_sites; any output pointer may be
 * NULL; cap (entries; bits takes W words per entry) below the table's size is
 * PG_ERANGE.  These and the two text calls below: PG_EINVAL before any
 * pg_region_sites. */
int pg_region_sites_table(pg_ctx* ctx, int64_t* from, int64_t* to, uint32_t* n_alleles, uint64_t* first,
                          uint64_t* count, uint32_t* n_genomes, uint64_t cap);
int pg_region_sites_alleles(pg_ctx* ctx, uint64_t* site, int64_t* via, uint64_t* count, uint32_t* n_genomes,
                            uint64_t* min_len, uint64_t* max_len, uint64_t* bits, uint64_t cap);
int pg_region_sites_groups(pg_ctx* ctx, uint64_t* sites, uint64_t* alleles, uint64_t* private_alleles,
                           uint64_t cap);                                    /* cap >= n_groups */
/* The alleles table's text, formatted on the device and kept there like
 * pg_region_links_format's: the header
 * "#from\tto\tvia\tcount\tgenomes\tmin\tmax\n", then one line of decimals per
 * allele in table order, `*` for the direct allele's via (no sites: the
 * header alone).  out, cap, n_bytes and the _fd form: as
 * pg_region_links_format and pg_region_links_format_fd. */
int pg_region_sites_format(pg_ctx* ctx, char* out, uint64_t cap, uint64_t* n_bytes);
int pg_region_sites_format_fd(pg_ctx* ctx, int fd, uint64_t* n_bytes);

/* ---- variable sites between anchor regions: the bubbles of the region
 *      graph, however many regions they span.  pg_region_sites looks through
 *      a window of two or three rows between any two flanks; this pass walks
 *      from one anchor to the next.  Integer only; the result depends on the
 *      input alone, whatever the schedule.
 * Input: exactly pg_region_sites' - rows (rows5 NULL: the last pg_rows where
 * they lie on the device), rec_group[n_records] in [-1, n_groups), the rule
 * for a used row, the run, and the count of the others in *n_skipped - and
 * min_genomes, 1 <= min_genomes <= n_groups (no rows and n_groups == 0: any
 * value >= 1, and the result is empty).
 * Anchor: a label whose used rows lie in min_genomes distinct genomes or
 * more (pg_freq's n_genomes of the same rows and groups; the call counts
 * them itself and reads no pg_freq result).
 * Segment: inside one run, two anchor steps with no anchor step between
 * them: a, the earlier label, c, the later; the inner path, the labels of the
 * steps strictly between them in walk order; regions, their number (0: c
 * follows a directly); bp, the sum of |end - start| of those rows (unsigned
 * 64-bit, as pg_freq); its genome, rec_group[record].  The steps before a
 * run's first anchor and after its last are in no segment.  Walk order, as
 * everywhere: no orientation is inferred.  a == c is legal.
 * Allele of a flank pair (a, c): a distinct inner path - equal length and
 * equal labels position by position.  Site: a flank pair with two alleles or
 * more; a pair with one allele is dropped.
 * Sites table, by (a, c) ascending: from = a, to = c; n_alleles; first, the
 * index of its first allele; count, the segments over its alleles;
 * n_genomes, the popcount of the OR of their presence sets.
 * Alleles table, by site and inside a site by first_row ascending: site;
 * regions; first_row, the index in the row list of the a row of the allele's
 * earliest segment (an anchor row opens at most one segment: no ties, and
 * the order depends on no hash); count, its segments; n_genomes; min_bp and
 * max_bp over them; inner_off, the exclusive prefix sum of regions in table
 * order; the presence set, W = ceil(n_groups / 64) uint64 words laid out as
 * pg_freq_export's.
 * Inner: int64 [sum of regions], the alleles' inner paths one after another
 * in table order.  Per genome: sites, alleles, private, as
 * pg_region_sites_groups defines them.  Anchors: their labels ascending, with
 * n_genomes.
 * Counts (each pointer may be NULL): *n_anchors, *n_segments, *n_sites,
 * *n_alleles, *n_skipped.
 * Exactness: the segments are grouped by (a, c), regions and a hash of the
 * inner path - two polynomial hashes mod 2^61 - 1, one fixed function of the
 * labels with no seed.  regions is compared before the hash, and every
 * segment is then compared label by label, on the device, with the first
 * segment of its group: a mismatch is PG_EDEVICE with the previous result
 * kept, and there is no retry.  The hash only groups; identity comes from
 * the comparison and order from first_row.
 * PG_EINVAL, before any device work: pg_region_graph's whole list, and
 * min_genomes out of range.  L = 1 + the largest used label > 2^31 is
 * PG_ERANGE (found by a device reduction before anything is allocated).
 * Nothing is dense in the label: the call takes device memory by the rows,
 * the segments and the alleles - 9 bytes per row; per used row 29 for the
 * steps, 33 more while the anchors are found, then 65 for the scans and the
 * hash; per segment 168 while they are sorted, then 89, and at most 99 more
 * per distinct (a, c, inner path) - and the tables 40 + 8 W bytes per site,
 * 60 + 8 W per allele, 8 per inner label and 12 per label for the anchors.
 * An allocation failure is PG_ENOMEM.  In every refusal the previous result
 * stays: the new one is built aside and swapped in last.  The result stays
 * until the next successful pg_region_bubbles; pg_freq, pg_freq_compare,
 * pg_region_graph, pg_region_seqs and pg_region_sites neither read nor drop
 * it, nor it theirs.  (pg_region_variants, below, reads it; a successful
 * pg_region_bubbles drops the variants.) */
int pg_region_bubbles(pg_ctx* ctx, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group,
                      uint64_t n_records, uint32_t n_groups, uint32_t min_genomes, uint64_t* n_anchors,
                      uint64_t* n_segments, uint64_t* n_sites, uint64_t* n_alleles, uint64_t* n_skipped);
/* The tables of the last pg_region_bubbles; any output pointer may be NULL;
 * cap (entries; bits takes W words per entry) below the table's size is
 * PG_ERANGE.  pg_region_bubbles_inner: *n_inner is the sum of regions; inner
 * == NULL: only *n_inner is set, otherwise cap >= that, else PG_ERANGE.
 * These and the two text calls below: PG_EINVAL before any
 * pg_region_bubbles. */
int pg_region_bubbles_table(pg_ctx* ctx, int64_t* from, int64_t* to, uint32_t* n_alleles, uint64_t* first,
                            uint64_t* count, uint32_t* n_genomes, uint64_t cap);
int pg_region_bubbles_alleles(pg_ctx* ctx, uint64_t* site, uint64_t* regions, uint64_t* first_row, uint64_t* count,
                              uint32_t* n_genomes, uint64_t* min_bp, uint64_t* max_bp, uint64_t* inner_off,
                              uint64_t* bits, uint64_t cap);
int pg_region_bubbles_inner(pg_ctx* ctx, int64_t* inner, uint64_t cap, uint64_t* n_inner);
int pg_region_bubbles_groups(pg_ctx* ctx, uint64_t* sites, uint64_t* alleles, uint64_t* private_alleles,
                             uint64_t cap);                                  /* cap >= n_groups */
int pg_region_bubbles_anchors(pg_ctx* ctx, int64_t* label, uint32_t* n_genomes, uint64_t cap);
/* The alleles table's text, formatted on the device and kept there like
 * pg_region_sites_format's: the header
 * "#from\tto\tinner\tregions\tcount\tgenomes\tmin\tmax\n", then one line of
 * decimals per allele in table order; inner is the labels joined by `,`, or
 * `*` for the direct join (no sites: the header alone).  out, cap, n_bytes
 * and the _fd form: as pg_region_sites_format and pg_region_sites_format_fd. */
int pg_region_bubbles_format(pg_ctx* ctx, char* out, uint64_t cap, uint64_t* n_bytes);
int pg_region_bubbles_format_fd(pg_ctx* ctx, int fd, uint64_t* n_bytes);

/* ---- the bubbles' alleles as sequences, and the sites placed on a reference
 *      genome: the tables, an allele FASTA and the body of a VCF.  Integer
 *      only; the result depends on the input alone, whatever the schedule.
 * Input: exactly pg_region_bubbles' rows (rows5 NULL: the last pg_rows where
 * they lie on the device), rec_group, the rule for a used row and the run;
 * n_records is the context's record count in both forms, because the bases
 * come from the context's parse; and the context's last pg_region_bubbles
 * result, which must describe these rows and groups.  lo(r) = min(start,
 * end), hi(r) = max(start, end).
 * Segment at row i, a used row whose label is an anchor: j > i is the next row
 * of i's run whose label is an anchor; flanks (label[i], label[j]), inner
 * path the labels of rows i + 1 .. j - 1.  Its span: bases [hi(i), lo(j)) of
 * the record's compacted sequence if strand == 1, otherwise [hi(j), lo(i));
 * its sequence: those bases, one letter per base class as pg_region_seqs (A C
 * G T, everything else N), as they stand if strand == 1 and reverse
 * complemented otherwise, so that every allele reads in walk direction.
 * Allele t's sequence is that of the segment at row first_row[t] (its c row
 * is first_row + regions + 1); a direct join may have length 0.  Two alleles
 * of a site may read the same - different label paths can have the same bases
 * - and they are not merged.
 * Allele table, in the bubbles alleles' order: record; lo, hi, the span;
 * strand; len; gc and amb as pg_region_seqs; offset, the exclusive prefix sum
 * of len.  The bases are the sequences one after another without separators;
 * *n_bases is the sum of len.
 * Reference placement: ref_group in [0, n_groups), or PG_NO_REF, which places
 * nothing.  The reference segment of site s is the segment with s's flank
 * pair in a record of genome ref_group on strand == 1 with the smallest row
 * index i.  Its inner path equals exactly one allele of s: ref_allele, an
 * index inside the site.  pos0 = hi(row i), ref_len its span's length.  A site
 * is placed iff it has a reference segment and pos0 >= 1, so that a padding
 * base exists; the others are unplaced.
 * Placed table, by (record, pos0, site index) ascending: site, record, pos0,
 * ref_row, ref_allele, ref_len.
 * Counts (each pointer may be NULL): *n_alleles, *n_bases, *n_placed,
 * *n_unplaced.
 * PG_EINVAL, before anything is replaced: pg_region_bubbles' whole list; no
 * bubbles result; n_groups other than the bubbles result's; ref_group >=
 * n_groups and not PG_NO_REF; a context without a parse, or another record
 * count; a used row with lo < 0 or hi past its record; an allele whose rows
 * first_row .. first_row + regions + 1 do not match the bubbles result (inside
 * the list, all used, one record and strand, labels equal to from, the inner
 * path and to: checked on the device, one thread per step); a representative
 * or reference segment whose flank rows overlap or are out of order (span
 * start > end); a reference segment that matches no allele.  An allocation
 * failure is PG_ENOMEM.  In every refusal the previous result stays.
 * Device memory while the call runs: 1 byte per row (and 40 for rows from the
 * host), 97 per allele, 45 per site and 32 more per placed site; the result
 * holds 88 per allele, 132 per placed site and 1 per base, every sequence
 * (and every placed site's padding base + REF) starting at a multiple of 16.
 * Lifetime: the texts read the bubbles tables when they are formatted, so a
 * later successful pg_region_bubbles drops the result (as pg_freq drops the
 * comparison) and the exports below return PG_EINVAL again; no other pass
 * reads or drops it. */
#define PG_NO_REF UINT32_MAX
int pg_region_variants(pg_ctx* ctx, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group,
                       uint64_t n_records, uint32_t n_groups, uint32_t ref_group, uint64_t* n_alleles,
                       uint64_t* n_bases, uint64_t* n_placed, uint64_t* n_unplaced);
/* The tables of the last pg_region_variants; any output pointer may be NULL;
 * cap (entries) below the table's size is PG_ERANGE.
 * pg_region_variants_bases: *n_bytes = n_bases; out == NULL: only that,
 * otherwise cap >= n_bases, else PG_ERANGE.  pg_region_variants_time: the
 * decoder kernel's time (HIP events) and its 16-letter chunks, the placed
 * sites' padding base + REF included.  All of these and the text calls below:
 * PG_EINVAL before any pg_region_variants. */
int pg_region_variants_alleles(pg_ctx* ctx, int64_t* record, int64_t* lo, int64_t* hi, int64_t* strand,
                               uint64_t* len, uint64_t* gc, uint64_t* amb, uint64_t* offset, uint64_t cap);
int pg_region_variants_bases(pg_ctx* ctx, uint8_t* out, uint64_t cap, uint64_t* n_bytes);
int pg_region_variants_placed(pg_ctx* ctx, uint64_t* site, int64_t* record, int64_t* pos0, uint64_t* ref_row,
                              uint32_t* ref_allele, uint64_t* ref_len, uint64_t cap);
int pg_region_variants_time(pg_ctx* ctx, double* ms_decode, uint64_t* n_chunks);
/* The allele FASTA, formatted on the device by every call with its own record
 * names: per allele in table order, k its index inside its site,
 *   ><from>_<to>_<k> <name>:<lo>-<hi>:<+|-> regions=<r> genomes=<g> len=<len>\n<sequence>\n
 * (a direct join of length 0 gives an empty sequence line).  names, out, cap,
 * n_bytes and the _fd form: as pg_region_gfa and pg_region_gfa_fd; n_names
 * must cover the context's records. */
int pg_region_alleles_fasta(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                            uint64_t cap, uint64_t* n_bytes);
int pg_region_alleles_fasta_fd(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                               uint64_t* n_bytes);
/* The VCF body: one line per placed site in the placed table's order,
 * tab separated and newline ended (no placed site: empty):
 *   <names[record]> <pos0> <from>_<to> <REF> <ALT> . . NS=<site n_genomes> GT <cell g = 0> ... <cell g = G - 1>
 * pad is the letter of reference base pos0 - 1, and POS = pos0 its 1-based
 * coordinate.  REF = pad + the reference record's own letters [pos0, pos0 +
 * ref_len) - the reference's bases, not the ref allele's representative.  ALT:
 * one entry pad + sequence for every other allele of the site in table order,
 * joined by `,`.  The ref allele is number 0, the others 1, 2, ... in table
 * order; the cell of genome g lists the numbers of the alleles whose presence
 * bit g is set, ascending, joined by `/`, or `.` if there are none.  Equal
 * allele strings are not merged.  The caller writes the header lines.  The
 * arguments: as pg_region_alleles_fasta. */
int pg_region_vcf(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, char* out, uint64_t cap,
                  uint64_t* n_bytes);
int pg_region_vcf_fd(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                     uint64_t* n_bytes);

/* ---- the alleles aligned against their site's reference: CIGARs, the
 *      primitive differences (SNVs, deletions, insertions) and, for the placed
 *      sites, the primitives merged into the lines of a VCF.  Integer only; the
 *      result depends on the input alone, whatever the schedule.
 * Input: the last successful pg_region_variants and the bubbles result it
 * belongs to; the pass takes no rows.
 * Pairs: every site s has a target T.  A placed site's T is the reference
 * record's own letters [pos0, pos0 + ref_len) - the placed entry's REF without
 * the padding base - and its skipped allele is ref_allele; every other site's
 * (PG_NO_REF: every site's) T is the sequence of its allele 0, and 0 is
 * skipped.  Every other allele of the site is a query Q, in table order; pairs
 * come by site index, then allele index: n_pairs = n_alleles - n_sites.
 * Letters compare as bytes (N equals N and nothing else).
 * Trimming, n = |T|, m = |Q|, the suffix first: q is the largest value <=
 * min(n, m) for which the last q letters of T and Q are equal, then p the
 * largest value <= min(n, m) - q for which the first p letters are.  The cores:
 * t = T[p : n - q] of length a, u = Q[p : m - q] of length b.
 * Distance: D[i][0] = i, D[0][j] = j, otherwise D[i][j] = min(D[i-1][j-1] +
 * (t[i-1] != u[j-1]), D[i-1][j] + 1, D[i][j-1] + 1); the distance is D[a][b].
 * Path, walked from (a, b) to (0, 0).  At (i, j): if i > 0, j > 0 and D[i][j]
 * == D[i-1][j-1] + (t[i-1] != u[j-1]) the step is diagonal, `=` for equal
 * letters and `X` otherwise; else if i > 0 and D[i][j] == D[i-1][j] + 1 it is
 * `D`, a target base with no query base; else `I`.  Going backwards the
 * diagonal comes first, so a gap sits at the leftmost of its co-optimal
 * places: AAA against AA deletes the first A.  The choice depends on its cell
 * alone (the fill stores it in 2 bits; the traceback follows the bits).
 * CIGAR: the run-length list over all of T and Q: p `=`, the core's runs, q
 * `=`, runs of length 0 left out; ops `=` `X` `D` `I`; the empty list (n = m =
 * 0) prints as `*`.  The core's first and last ops are never `=`, and a `D`
 * run never touches an `I` run.
 * Size cap: a pair with (a + 1) x (b + 1) above cells_cap (2^24, or
 * PG_TUNE_ALIGN_CELLS) is not aligned: status 1, CIGAR p `=`, a `D`, b `I`, q
 * `=`, distance UINT64_MAX (printed `.`), n_del = a, n_ins = b, and one
 * primitive of type REPL.  Every other pair has status 0.
 * Band form (PG_TUNE_ALIGN_BAND 1; nothing of this at 0): only the pairs above
 * cells_cap change, and no table or text marks them.  One with a == 0 or b ==
 * 0 is aligned without a fill: status 0, b `I` or a `D`, distance a + b, one
 * INS or DEL.  Any other is tried at the thresholds t_k = t0 2^k (t0 = 64, or
 * PG_TUNE_ALIGN_BAND_T0), a band of band_cells(t) = a x min(b, 2 t + 1) cells.
 * k_lo is the smallest k with t_k >= |a - b|, k* the smallest with t_k >=
 * D[a][b], k_hi the largest with band_cells(t_k) <= band_cap (2^26, or
 * PG_TUNE_ALIGN_BAND_CELLS), -1 if there is none.  The pair is aligned iff k*
 * <= k_hi: status 0, and every column, run and primitive is what the
 * definition above gives over the full D, as at an unlimited cells_cap;
 * otherwise it keeps status 1 as above.  Its attempts: max(0, min(k*, k_hi) -
 * k_lo + 1).  A pair with a + b >= 2^30 is never tried (the fill counts in 32
 * bits).
 * Why a band is exact: the band fill takes only the cells with |j - i| <= t and
 * counts every other neighbour as infinity; its values B are >= D.  A cheapest
 * path to a cell with D[i][j] <= t passes only cells (i', j') with |j' - i'|
 * <= D[i'][j'] <= t, all in the band, so B = D there: B[a][b] <= t iff D[a][b]
 * <= t.  Then every cell of the path has D <= t, and each test of the path
 * rule gives with B what it gives with D: if D[i][j] == D[i-1][j-1] + ne, that
 * neighbour has D <= t and is exact in B; if it holds in B, D[i-1][j-1] + ne
 * <= B[i-1][j-1] + ne = D[i][j], and the recurrence says >=.  The same for
 * the other two neighbours.
 * Pair table, every column uint64: site; allele, the index inside its site;
 * placed, 0 or 1; t_len, q_len, prefix, suffix; status; distance; n_eq, with
 * p + q; n_sub, n_ins, n_del, in bases; op_off, n_ops: its runs in the run
 * arrays - op, one of '=' 'X' 'D' 'I', and len; prim_off, n_prims.
 * Primitives, per pair in target order: pair, type, tpos, qpos, tlen, qlen,
 * the offsets into T and Q.  SNV (0): every X column on its own, 1 and 1.  DEL
 * (1): every maximal D run of length L, L and 0.  INS (2): every maximal I run,
 * 0 and L; tpos is the target base before which the insertion lies.  REPL (3):
 * a status 1 pair, tpos = qpos = p, a and b.
 * Lines: the merged primitives of the placed sites.  Two primitives of one
 * site are the same line iff (tpos, type, tlen, qlen) are equal and Q[qpos :
 * qpos + qlen] is, letter by letter.  A line has site; pos, the 1-based VCF
 * POS: pos0 + tpos + 1 for an SNV, and pos0 + tpos, the anchor base (the
 * padding base when tpos = 0), for the others; type, tpos, tlen, qlen;
 * first_prim, the smallest primitive index of the group (its Q gives the ALT
 * letters); ac, the allele entries that carry it; its carrier set, W =
 * ceil(n_groups / 64) words, the OR of those alleles' presence bits, and
 * n_genomes, its popcount.  Lines come by (record, pos, site, type, tlen, qlen,
 * first_prim) ascending.
 * Counts (each pointer may be NULL): *n_pairs; *n_aligned, the status 0 pairs;
 * *n_ops; *n_prims; *n_lines.
 * PG_EINVAL before any successful pg_region_variants; PG_ENOMEM on an
 * allocation failure; PG_EDEVICE if two primitives with unequal letters share
 * every key and their letters' hash (PG_TUNE_ALIGN_HASH_BITS).  In every
 * refusal the previous result stays.
 * Device memory while the call runs: per batch of pairs (a + 1) words of 16
 * choices per core row and b + 1 row values, within PG_TUNE_ALIGN_SCRATCH (256
 * MiB; one pair if a pair needs more) - in the band form at threshold t, a
 * pair takes a ceil(min(b, 2 min(t, max(a, b)) + 79) / 16) + b + 1 words, every
 * 64-row strip's choices from its first column less one, rounded down to a
 * multiple of 16; 5 bytes per run bound, min(a + b, 2 min(a, b) + 1), of every
 * aligned pair and every pair the band form tries; 56 per primitive of a placed site
 * while the lines are made.  The result: 152 per pair, 9 per run, 41 per
 * primitive, 85 + 8 W per line and 8 per carrying allele of a line.
 * Lifetime: a successful pg_region_variants or pg_region_bubbles drops the
 * result, because it describes theirs; no other pass reads or drops it. */
int pg_region_align(pg_ctx* ctx, uint64_t* n_pairs, uint64_t* n_aligned, uint64_t* n_ops, uint64_t* n_prims,
                    uint64_t* n_lines);
/* The tables of the last pg_region_align; any output pointer may be NULL; cap
 * (entries) below the table's size is PG_ERANGE.  bits: [n_lines][W].
 * pg_region_align_time: the fill kernels' time (HIP events, summed over the
 * batches) and the a x b cells they computed.  All of these and the text
 * calls below: PG_EINVAL before any pg_region_align. */
int pg_region_align_pairs(pg_ctx* ctx, uint64_t* site, uint64_t* allele, uint64_t* placed, uint64_t* t_len,
                          uint64_t* q_len, uint64_t* prefix, uint64_t* suffix, uint64_t* status, uint64_t* distance,
                          uint64_t* n_eq, uint64_t* n_sub, uint64_t* n_ins, uint64_t* n_del, uint64_t* op_off,
                          uint64_t* n_ops, uint64_t* prim_off, uint64_t* n_prims, uint64_t cap);
int pg_region_align_ops(pg_ctx* ctx, uint8_t* op, uint64_t* len, uint64_t cap);
int pg_region_align_prims(pg_ctx* ctx, uint64_t* pair, uint8_t* type, uint64_t* tpos, uint64_t* qpos, uint64_t* tlen,
                          uint64_t* qlen, uint64_t cap);
int pg_region_align_lines(pg_ctx* ctx, uint64_t* site, int64_t* pos, uint8_t* type, uint64_t* tpos, uint64_t* tlen,
                          uint64_t* qlen, uint64_t* first_prim, uint64_t* ac, uint32_t* n_genomes, uint64_t* bits,
                          uint64_t cap);
int pg_region_align_time(pg_ctx* ctx, double* ms_fill, uint64_t* cells);
/* The band form's part of the last pg_region_align (every pointer may be
 * NULL; all 0 with PG_TUNE_ALIGN_BAND 0): *n_over, the pairs above cells_cap;
 * *n_banded, those of them that came out aligned (the ones with an empty core
 * side included); *n_attempts, the attempts summed; *band_cells, band_cells(t_k)
 * summed over the attempts; *ms_band, the band fills' time (HIP events), which
 * pg_region_align_time leaves out.  PG_EINVAL before any pg_region_align. */
int pg_region_align_band(pg_ctx* ctx, uint64_t* n_over, uint64_t* n_banded, uint64_t* n_attempts, uint64_t* band_cells,
                         double* ms_band);
/* The pair table's text, formatted on the device: the header
 * "#from\tto\tallele\ttarget\ttlen\tqlen\tprefix\tsuffix\tdist\teq\tsub\tins\tdel\tcigar\n",
 * then one line per pair; target is `ref` for a placed site, else `0`; dist is
 * `.` for a status 1 pair; cigar is <len><op> per run, or `*`.  out, cap,
 * n_bytes and the _fd form: as pg_region_sites_format and its _fd form. */
int pg_region_align_format(pg_ctx* ctx, char* out, uint64_t cap, uint64_t* n_bytes);
int pg_region_align_format_fd(pg_ctx* ctx, int fd, uint64_t* n_bytes);
/* The primitives' VCF body: one line per line entry, tab separated and newline
 * ended (no line: empty):
 *   <names[record]> <pos> <from>_<to> <REF> <ALT> . . NS=<site n_genomes>;AC=<ac> GT <cell g = 0> ... <cell g = G - 1>
 * SNV: REF is T[tpos] and ALT is Q[qpos].  The others: the anchor letter
 * (reference base pos - 1, 0-based) followed by T[tpos : tpos + tlen] for REF
 * and by Q[qpos : qpos + qlen] for ALT.  The cell of genome g: `1` if an allele
 * of the site with presence bit g carries the line, `0` if an allele of the
 * site with bit g does not (the reference allele never does), `0/1` if both
 * hold, `.` if neither does.  The caller writes the header lines.  The
 * arguments: as pg_region_vcf and pg_region_vcf_fd. */
int pg_region_primitives_vcf(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                             uint64_t cap, uint64_t* n_bytes);
int pg_region_primitives_vcf_fd(pg_ctx* ctx, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                                uint64_t* n_bytes);

/* ---- text output (host only; no context).  The reference formats these in
 *      Python loops (kmer_numba.py:1893-1904, :1946-1949).
 * pg_format_xyz: "%d_%d\t%d_%d\t%d\n" per edge (tuples as unsigned).
 * pg_format_rows: "qid\tstart\tend\t+|-\tlabel\n" per row; qid of record r
 * is names[name_off[r] .. name_off[r+1]).  With out == NULL both return the
 * buffer size they need; otherwise the bytes written, 0 if cap is short. */
uint64_t pg_format_xyz(const uint64_t* tuples, const int64_t* counts, uint64_t n, char* out, uint64_t cap);
uint64_t pg_format_rows(const int64_t* rows5, uint64_t n, const char* names, const int64_t* name_off, char* out,
                        uint64_t cap);

/* Tuning (tests and experiments; the defaults are the product setting).
 * PG_TUNE_K3_CHUNKS: chunks of the K3 tile list whose work pass overlaps the
 * next chunk's coverage pass, 1..6, or 0 = by tile count (3 when the list
 * has >= 3072 coverage groups, else 1). */
#define PG_TUNE_K3_CHUNKS 1
/* PG_TUNE_K3_COVER: form of the K3 coverage pass, 0 (default) = K1's packed
 * 2-bit base stream compared word by word, exact per base (round 4); 1 =
 * class bytes staged in LDS (round 2); 2 = class bytes compared 16 at a time
 * from registers, per dword (round 3).  The results are the same, only the
 * records left to the work pass differ. */
#define PG_TUNE_K3_COVER 10
/* PG_TUNE_K3_WBLK: blocks per CU of the K3 work passes when the tile list
 * runs in chunks: low 4 bits for every chunk but the last, high 4 bits for
 * the last (0 = 2 and the same as the others). */
#define PG_TUNE_K3_WBLK 11
/* PG_TUNE_K3_EMIT: form of the K3 work pass, 0 (default) = each queued
 * segment's records computed and emitted in two halves, 1 = at once. */
#define PG_TUNE_K3_EMIT 12
/* PG_TUNE_K3_TAIL: size of the last K3 chunk in 16ths of the others (1..64,
 * 0 = 10: the work pass left behind the last coverage pass is smaller). */
#define PG_TUNE_K3_TAIL 13
/* PG_TUNE_EARLY_SPLIT: pg_build_host's stage B under the upload, 1 (default)
 * = the records of each landed chunk split into the table's fine partitions
 * as soon as its stage A share is done (geometry from the last build; a
 * mismatch at the end re-splits everything), 0 = after the last chunk. */
#define PG_TUNE_EARLY_SPLIT 14
/* PG_TUNE_K3_HEAD: size of the first K3 chunk in 16ths of the middle ones
 * (1..64, 0 = 16: the coverage pass that runs before any work pass). */
#define PG_TUNE_K3_HEAD 15
/* PG_TUNE_H2D_TAIL: bytes of pg_build_host's last H2D chunk (0, the default:
 * every chunk PG_TUNE_H2D_CHUNK bytes).  A small last chunk puts two chunks'
 * K1, record round trip and stage A share behind the last copy (C3: 9.91 ms
 * at 8 MiB, 9.86 at 16, 9.80 uniform). */
#define PG_TUNE_H2D_TAIL 16
/* PG_TUNE_BUCKET_SHIFT: size the table 2^value times smaller than the record
 * count asks (0..8): exercises the overflow set, its spill and the re-run
 * with more buckets (results are unchanged). */
#define PG_TUNE_BUCKET_SHIFT 2
/* PG_TUNE_REGION_CAP: first stage A region size in records (0 = estimated):
 * a small value exercises the stage A re-run (results are unchanged). */
#define PG_TUNE_REGION_CAP 3
/* PG_TUNE_H2D_CHUNK: bytes per pg_parse_host chunk, rounded down to whole
 * 16 KiB K1 spans (0 = 64 MiB): small values exercise the pipeline. */
#define PG_TUNE_H2D_CHUNK 4
/* PG_TUNE_HOST_THREADS: host threads that copy a pageable input (an mmap)
 * into the pinned staging ring of pg_parse_host / pg_build_host / pg_set_fasta
 * (1..64, 0 = half the CPUs the process may run on, at most 8). */
#define PG_TUNE_HOST_THREADS 5
/* PG_TUNE_STAGE_PIECE / PG_TUNE_STAGE_SLOTS: bytes per slot of that ring (one
 * DMA each; 0 = 32 MiB) and its slot count (2..8, 0 = 4); the first pieces
 * of an upload are smaller (2, 4, 8 ... MiB). */
#define PG_TUNE_STAGE_PIECE 6
#define PG_TUNE_STAGE_SLOTS 7
/* PG_TUNE_HOST_REGISTER: 1 (default) = a pageable input's page-aligned
 * chunks are registered (hipHostRegister, read-only) for the duration of the
 * upload and DMA'd directly, falling back to the staging ring for the rest
 * when a chunk cannot be; 0 = staging ring only. */
#define PG_TUNE_HOST_REGISTER 8
/* PG_TUNE_DEVICE_CAP: the most device bytes the library's buffers may hold
 * in this process, over all contexts (0 = no cap): an allocation past it
 * fails with PG_ENOMEM.  Setting it also restarts pg_device_bytes' peak.
 * PROCESS-WIDE: although it is set through one context's pg_tune, the cap
 * and the peak it restarts are shared by every context of the process (and
 * every device).  For tests of a path's memory budget at a scaled-down size. */
#define PG_TUNE_DEVICE_CAP 9
/* PG_TUNE_POISON (debug, PROCESS-WIDE like PG_TUNE_DEVICE_CAP): every device
 * buffer the library allocates from now on is filled with this byte value
 * (0..255; -1, the default, = off), so that a kernel reading memory nothing
 * wrote gives a different result instead of inheriting an earlier run's. */
#define PG_TUNE_POISON 17
/* PG_TUNE_K1: K1 form bits.  Bit 0: the span pass, 0 = per-step form (fast
 * or general 1 KiB step), 1 = whole-span form (a 16 KiB span without '>' and
 * below the last byte counted in one pass of SWAR sums, its newline positions
 * found afterwards; the spans left over by a step-parallel per-step pass).
 * Bit 1: the emission keeps two wave steps of loads in flight (else one).
 * Bit 2: the record table (header pass, k_records, its copy to the host) on
 * the context's stream ahead of the emission, instead of beside it on the
 * high-priority stream. */
#define PG_TUNE_K1 18
/* PG_TUNE_TIMERS: which stage spans of pg_stats are timed with HIP events on
 * the stream (each timing event costs the stream a few us): bit 0 K1
 * (ms_parse), bit 1 stage A (ms_insert), bit 2 stages B/C (ms_split,
 * ms_range); 7 (default) = all, 0 = none (the spans read 0). */
#define PG_TUNE_TIMERS 19
/* PG_TUNE_K3_ANCHORS: anchors per tile and reference of the packed coverage
 * pass (3, 4, 5, 6 or 8; 0 = 4).  More anchors find the drift of more of the
 * short runs between two indels, so fewer windows go to the work pass as
 * records (C3: 27.6 M stage A records with 3, 24.2 M with 4, 21.8 M with 8),
 * at a dearer drift search (C3 step: 4 is the fastest). */
#define PG_TUNE_K3_ANCHORS 20
/* PG_TUNE_FREQ_FORM: pg_freq's accumulate pass, 0 (default) = rows of one
 * label aggregated inside each wave before one lane issues the atomics, 1 =
 * every lane issues its own (the same results; for comparison). */
#define PG_TUNE_FREQ_FORM 21
/* PG_TUNE_CMP_CHUNK: pg_freq_compare's shared pass, words (64 labels each) of
 * the label axis per block, 1 .. 2^25 (a block sums in 32 bits); 0 (default)
 * = what gives about four blocks per compute unit over the upper triangle of
 * 64 x 64 genome tiles, in multiples of 32 words and at least 256.  A small
 * value makes a small input take many chunks and the atomic flush (the same
 * results). */
#define PG_TUNE_CMP_CHUNK 22
/* PG_TUNE_CMP_FORM: pg_freq_compare's curve pass, 0 (default) = per-block LDS
 * counters flushed once, up to 2048 genomes, and every wave's sums straight
 * to global atomics above; 1 = the global form at every size (the same
 * results; for comparison). */
#define PG_TUNE_CMP_FORM 23
/* PG_TUNE_RDBG_KEYS: where the rdBG keys come from.  0 (default) = the
 * build's range pass only counts the rdBG members, and pg_rdbg_export sweeps
 * the table for their keys when asked; 1 = the eager form: the range pass
 * also writes every member's key (about a fifth of its time on a 100-genome
 * batch, and 8 bytes per key of device memory), and pg_rdbg_export gathers
 * them without reading the table.  For a caller that exports after every
 * build of a table too large to sweep each time (the streamed merge's 2^30
 * bucket tables).  It takes effect at the next build; pg_rdbg_export follows
 * the form of the last build.  The same keys either way. */
#define PG_TUNE_RDBG_KEYS 24
/* PG_TUNE_BUBBLE_HASH_BITS: pg_region_bubbles groups the segments of a flank
 * pair by a hash of their inner paths before it compares them label by
 * label.  0 (default) = the full hash; 1..32 = only that many low bits of one
 * hash word, so that equal hashes of unequal paths - PG_EDEVICE from the
 * comparison - can be tested.  The results that are returned are the same. */
#define PG_TUNE_BUBBLE_HASH_BITS 25
/* PG_TUNE_ALIGN_CELLS: pg_region_align's cells_cap: a pair whose (a + 1) x
 * (b + 1) is above it is not aligned (status 1).  1 .. 2^30 (the fill counts
 * in 32 bits); 0 (default) = 2^24. */
#define PG_TUNE_ALIGN_CELLS 26
/* PG_TUNE_ALIGN_SCRATCH: bytes of direction bits and row values one batch of
 * pg_region_align's pairs may take.  0 (default) = 256 MiB; a value below one
 * pair's need gives one pair per batch.  The same results at any value. */
#define PG_TUNE_ALIGN_SCRATCH 27
/* PG_TUNE_ALIGN_HASH_BITS: pg_region_align groups the primitives of a site by
 * a hash of their query letters before it compares them letter by letter.  0
 * (default) = the full hash; 1..64 = only that many low bits, so that equal
 * hashes of unequal letters - PG_EDEVICE from the comparison - can be tested.
 * The results that are returned are the same. */
#define PG_TUNE_ALIGN_HASH_BITS 28
/* PG_TUNE_ALIGN_BAND: 0 (default) = pg_region_align gives up every pair above
 * cells_cap; 1 = it aligns them in a band of diagonals (pg_region_align's
 * "Band form").  Nothing else changes. */
#define PG_TUNE_ALIGN_BAND 29
/* PG_TUNE_ALIGN_BAND_CELLS: the band form's band_cap: a pair is given up
 * before a band of more cells.  1 .. 2^34; 0 (default) = 2^26. */
#define PG_TUNE_ALIGN_BAND_CELLS 30
/* PG_TUNE_ALIGN_BAND_T0: the band form's first threshold t0.  1 .. 2^20; 0
 * (default) = 64.  For tests: at 1 the band's edges and the doubling show on
 * cores of a few dozen letters. */
#define PG_TUNE_ALIGN_BAND_T0 31
/* PG_TUNE_NJ_BLOCKS: blocks of pg_tree_nj's arg-min pass.  0 (default) = by
 * size: a wave per row, up to four blocks per compute unit; 1 .. 4096 = that
 * many, so that a small input runs the reduction across blocks.  The result
 * is the same at any value. */
#define PG_TUNE_NJ_BLOCKS 32
/* PG_TUNE_BOOT_SCRATCH: device bytes of one batch of pg_tree_bootstrap's
 * replicates (their bit rows, matrices and clades).  0 (default) = 256 MiB;
 * a batch always holds at least one replicate.  For tests: a small value
 * forces batches of one, or a ragged last batch.  The result is the same at
 * any value. */
#define PG_TUNE_BOOT_SCRATCH 33
/* PG_TUNE_BOOT_FORM: how pg_tree_bootstrap runs a replicate's neighbour
 * joining.  0 (default) = by size, as measured: form 1 up to 128 leaves,
 * form 2 up to 256 leaves with 4 or more replicates and up to 512 with 16 or
 * more, form 3 otherwise; 1 = one workgroup with the matrix in LDS (n <= 128;
 * above it as 0); 2 = one workgroup with the matrix in global scratch (n <=
 * 1024; above it as 3); 3 = pg_tree_nj's per-join launches, one replicate
 * after another.  The result is the same at any value. */
#define PG_TUNE_BOOT_FORM 34
int pg_tune(pg_ctx* ctx, int what, int64_t value);

/* Device bytes the library's buffers hold in this process now (peak == 0)
 * or at most since the last PG_TUNE_DEVICE_CAP (peak != 0). */
uint64_t pg_device_bytes(int peak);

/* Timings and counters of the last build (see pg_stats). */
int pg_get_stats(const pg_ctx* ctx, pg_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* PANGENOME_H */
